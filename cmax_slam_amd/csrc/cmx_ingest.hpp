// cmx_ingest.hpp -- the host side of every hand-over of events (set_packet, set_window, recon_add, events_push and their
// _aos / _from / group forms): where the events are, how they are cut into batches, the one packing pass and the one batch-time
// pass.  Pure host code: no HIP, no context -- tests/ingest_host.cpp builds it alone with a plain C++ compiler.
#pragma once
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/cmax_hip.h"
#include "cmx_hostpool.hpp"

namespace cmx {

// ---- event views: element i of a range of events, whatever the host keeps them in
// (p / op: the polarity of event i, read by the _pol hand-overs alone -- everything else never looks at it)
struct EvSoa {
  const uint16_t *x = nullptr, *y = nullptr;
  const int64_t *t = nullptr;
  const uint8_t *p = nullptr;
  unsigned X(int64_t i) const { return x[i]; }
  unsigned Y(int64_t i) const { return y[i]; }
  int64_t T(int64_t i) const { return t[i]; }
  unsigned P(int64_t i) const { return p[i] != 0; }
  EvSoa from(int64_t first) const { return EvSoa{x + first, y + first, t + first, p ? p + first : nullptr}; }
};
// an array of records (cmx_aos_layout, e.g. dvs_msgs::Event)
struct EvAos {
  const unsigned char *base = nullptr;
  size_t stride = 0, ox = 0, oy = 0, os = 0, on = 0, op = 0;
  unsigned X(int64_t i) const { uint16_t v; memcpy(&v, base + (size_t)i * stride + ox, 2); return v; }
  unsigned Y(int64_t i) const { uint16_t v; memcpy(&v, base + (size_t)i * stride + oy, 2); return v; }
  int64_t T(int64_t i) const {
    uint32_t sec, nsec;
    memcpy(&sec, base + (size_t)i * stride + os, 4);
    memcpy(&nsec, base + (size_t)i * stride + on, 4);
    return (int64_t)sec * 1000000000LL + (int64_t)nsec;
  }
  unsigned P(int64_t i) const { return base[(size_t)i * stride + op] != 0; }
  EvAos from(int64_t first) const { EvAos r = *this; r.base = base + (size_t)first * stride; return r; }
};
// the one layout check (`layout` is not null); the callers report a failure in their own words
inline bool aos_view(const void *events, const cmx_aos_layout *layout, EvAos *out) {
  const size_t st = layout->stride;
  if (st < 12 || layout->off_x + 2 > st || layout->off_y + 2 > st || layout->off_sec + 4 > st || layout->off_nsec + 4 > st) return false;
  out->base = static_cast<const unsigned char *>(events);
  out->stride = st; out->ox = layout->off_x; out->oy = layout->off_y; out->os = layout->off_sec; out->on = layout->off_nsec;
  return true;
}
// ... with the byte offset of a polarity field (one byte, nonzero = ON) inside the record: the _pol hand-overs
inline bool aos_view_pol(const void *events, const cmx_aos_layout *layout, size_t off_polarity, EvAos *out) {
  if (!aos_view(events, layout, out) || off_polarity >= layout->stride) return false;
  out->op = off_polarity;
  return true;
}

// ---- where the n events of a hand-over are
struct EventSource {
  enum Kind { SOA, AOS, DEVICE } kind = SOA;
  int64_t n = 0;
  EvSoa soa;  // SOA; DEVICE: soa.t is the store's host mirror of the timestamps
  EvAos aos;  // AOS
  // DEVICE: the store and the global index of the first event; once a consumer's device is known (store_source, cmx_events.cpp)
  // the packed events and timestamps of the replica on that device
  const cmx_events *store = nullptr;
  int64_t first = 0;
  const uint32_t *d_xy = nullptr;
  const int64_t *d_t = nullptr;
  const uint8_t *d_pol = nullptr;  // DEVICE: the replica's polarity bytes (0 / 1), null when the store holds none

  static EventSource arrays(int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t) { return EventSource{SOA, n, EvSoa{x, y, t}}; }
  bool on_device() const { return kind == DEVICE; }
  EventSource from(int64_t beg, int64_t count) const {  // events [beg, beg + count) of this source
    EventSource r = *this;
    r.n = count;
    if (kind == SOA) r.soa = soa.from(beg);
    if (kind == AOS) r.aos = aos.from(beg);
    r.first = first + beg;
    if (d_xy) { r.soa.t = soa.t + beg; r.d_xy = d_xy + beg; r.d_t = d_t + beg; }
    if (d_pol) r.d_pol = d_pol + beg;
    return r;
  }
  template <typename F>
  auto view(F f) const { return kind == AOS ? f(aos) : f(soa); }  // f(view) on the host-readable view (DEVICE: timestamps only)
};

// ---- everything of a back-end window that is not its events
struct KnotSupport {
  int order = 0, K = 0;
  long long start_ns = 0, dt_ns = 0;
};
struct WindowSpec {
  KnotSupport sup;
  const double *knots;
  int num_fixed;
  int64_t t_next_win_beg_ns;
  int batch, rate;
  double sigma;
  int measure;
  const float *IG;
};

// ---- ros::Time arithmetic (roscpp noetic semantics), needed to reproduce the per-batch pose time:
//   time_batch = time_first + (time_last - time_first) * 0.5         [Duration*double -> fromSec: floor + round]
//   reference: local_image_warped_events.cpp:68-75, event_pano_warper.cpp:239-242
inline long long time_batch_ns(long long t_first, long long t_last) {
  const long long d = t_last - t_first;
  long long ds = d / 1000000000LL, dn = d % 1000000000LL;
  if (dn < 0) { dn += 1000000000LL; ds -= 1; }
  const double half = ((double)ds + 1e-9 * (double)dn) * 0.5;
  const long long hs = (long long)floor(half);
  const long long hn = (long long)round((half - (double)hs) * 1e9);
  return t_first + hs * 1000000000LL + hn;
}
inline double time_to_sec(long long t_ns) {  // ros::Time::toSec
  return (double)(t_ns / 1000000000LL) + 1e-9 * (double)(t_ns % 1000000000LL);
}

// ---- the back end's batches: for (beg = 0; beg < n-1; beg += B) { end = (n-beg > B) ? beg+B : n; } -- a trailing batch holding
// exactly the last single event is never opened (event_pano_warper.cpp:188-196); inside a batch events are taken with stride `rate`
// restarting at the batch start (:262)
struct BatchPlan {
  int B = 1, rate = 1, per_batch = 1, nb = 0;
  int64_t last_len = 0;  // events of the last batch
  int64_t n_packed = 0;  // events the sampling selects
  int64_t packed(int b_lo, int b_hi) const {  // ... in the batches [b_lo, b_hi)
    const int64_t nbs = b_hi - b_lo;
    if (nbs <= 0) return 0;
    return b_hi == nb ? (nbs - 1) * per_batch + (last_len + rate - 1) / rate : nbs * per_batch;
  }
};
inline bool plan_batches(int64_t n, int B, int rate, BatchPlan *p) {  // false: more batches than an int counts
  *p = BatchPlan{};
  p->B = B; p->rate = rate; p->per_batch = (B + rate - 1) / rate;
  const int64_t nb64 = (n > 1) ? (n - 1 + B - 1) / B : 0;
  if (nb64 > 0x7fffffffLL) return false;
  p->nb = (int)nb64;
  if (p->nb > 0) {
    const int64_t last_beg = (int64_t)(p->nb - 1) * B;
    p->last_len = (n - last_beg > B) ? B : (n - last_beg);
    p->n_packed = p->packed(0, p->nb);
  }
  return true;
}
// ---- the chunk table of a tile sort (window path: do_binning; bound whole-trajectory events: bound_build): the sizes that follow
// from counts alone.  chunk_events: events of a full chunk -- hot tiles are split so that the chunks fill the chip in ONE resident
// round; big chunks amortise the window zeroing and flush.  So n / div, at least 1536 (floor swept on MI355X, 1M events:
// 1536 -> 11.8 us, 1024 -> 15.3) and at most 32768, a multiple of 256.  The divisor is the caller's:
//   back end (kBackEndChunkDiv): 135 VGPRs = 3 workgroups of 256 threads per CU (swept at 5M events, splat us: 512 -> 50, 640 -> 51,
//     768 -> 44, 1152 -> 50, 1536 -> 48, 3072 -> 53: anything that needs a second round loses more than it gains in latency hiding;
//     128 VGPRs + 4 per CU and one event per thread + 4 per CU: no gain, 72 vs 81 us per cost evaluation);
//   front end (CMX_FE_CHUNK_DIV, cmx_pipeline.cpp; 50 VGPRs, LDS-bound): with 256-thread workgroups n / 512 (1M events, splat us:
//     256 -> 10.0, 384 -> 8.4, 512 -> 8.2, 640 -> 8.5, 768 -> 8.8); round 5: 512-thread workgroups x chunks of n / 256
//     (profiles/r05_fe_shape.txt: 7.9 us; 1024 x n / 256: 7.7 but no better as an evaluation).
// max_chunks: an upper bound of the table's length, known on the host, for ANY distribution of the n events over `keys` sort
// tiles and the no-window tile, whose events go in chunks of 256 (the bound for 'all events rejected'): every tile adds
// floor(len / M) full chunks and at most one remainder.
constexpr int kBackEndChunkDiv = 768;
struct ChunkPlan {
  int chunk_events = 0;
  int64_t max_chunks = 0;
};
inline ChunkPlan plan_chunks(int64_t n, int64_t keys, int div) {
  ChunkPlan p;
  int64_t M = n / div;
  M = M < 1536 ? 1536 : (M > 32768 ? 32768 : M);
  p.chunk_events = (int)((M + 255) / 256 * 256);
  p.max_chunks = n / p.chunk_events + keys + 2 + n / 256;
  return p;
}
// ---- a pass over events in slices of whole batches (every recon_add*, the bound gather pass): batches per slice, and the slice
// that starts at batch b_lo of the plan of n_events events
inline int slice_batches_of(int64_t slice_events, int B) {
  const int64_t sb = slice_events / B;
  return (int)(sb < 1 ? 1 : sb);
}
struct Slice {
  int b_hi = 0;          // its batches are [b_lo, b_hi)
  int64_t ev_first = 0;  // its first event as handed in ...
  int64_t ev_n = 0;      // ... and how many of those it spans (the last slice: up to the end, a never-opened single-event tail included)
  int64_t first = 0;     // its first packed event
  int64_t n = 0;         // its packed events
};
inline Slice slice_at(const BatchPlan &p, int64_t n_events, int b_lo, int slice_batches) {
  Slice s;
  s.b_hi = (p.nb - b_lo > slice_batches) ? b_lo + slice_batches : p.nb;
  s.ev_first = (int64_t)b_lo * p.B;
  s.ev_n = s.b_hi == p.nb ? n_events - s.ev_first : (int64_t)(s.b_hi - b_lo) * p.B;
  s.first = (int64_t)b_lo * p.per_batch;
  s.n = p.packed(b_lo, s.b_hi);
  return s;
}
// ... and the walk over a whole hand-over of n_events events (recon_add*, recon_grad_add*, recon_warp*): slice k of it, false
// behind the last.  every_event (the per-event export): the trailing event no batch holds (n_events = nb B + 1) rides on the last
// slice, and n_events == 1 -- no batch at all -- is one slice of that event alone; a sampling pass has nothing to do there.
struct FeedSlice : Slice {
  int b_lo = 0;
  bool lone = false;  // every_event: the lone trailing event is element ev_n - 1 of this slice
};
inline bool feed_slice_at(const BatchPlan &p, int64_t n_events, int slice_batches, bool every_event, int64_t k, FeedSlice *f) {
  *f = FeedSlice{};
  if (p.nb == 0) {
    if (!(every_event && n_events == 1 && k == 0)) return false;
    f->ev_n = 1;
    f->lone = true;
    return true;
  }
  const int64_t b_lo = k * slice_batches;
  if (b_lo >= p.nb) return false;
  static_cast<Slice &>(*f) = slice_at(p, n_events, (int)b_lo, slice_batches);
  f->b_lo = (int)b_lo;
  f->lone = every_event && f->b_hi == p.nb && (int64_t)p.nb * p.B < n_events;
  return true;
}

// ---- the frozen head of a bound whole-trajectory evaluation (cmx_backend_recon_freeze_head): the batches whose pose no free knot
// can move.  A batch at pose time t lies in segment s = (t - start) / dt, clamped to [0, K - order] as the kernels clamp it
// (recon_pose, recon_segment), and its pose reads the knots s .. s + order - 1: it is frozen when all of them are among the first
// num_fixed, s + order - 1 < num_fixed.  Returns b_act, the number of LEADING frozen batches: the frozen head is [0, b_act), the
// active batches are [b_act, nb).  Batch times of a time-ordered recording do not decrease, so no batch behind b_act is frozen;
// were one out of order, it would merely be evaluated again every time, which is exact too.  The order is sup.order.
inline bool batch_is_frozen(const KnotSupport &sup, int num_fixed, long long t_ns) {
  long long s = (t_ns - sup.start_ns) / sup.dt_ns;
  const long long s_max = (long long)sup.K - sup.order;
  s = s < 0 ? 0 : (s > s_max ? s_max : s);
  return s + sup.order - 1 < (long long)num_fixed;
}
inline int frozen_prefix(const KnotSupport &sup, int num_fixed, const long long *batch_t, int nb) {
  if (num_fixed <= 0 || !batch_t) return 0;
  int b = 0;
  while (b < nb && batch_is_frozen(sup, num_fixed, batch_t[b])) b++;
  return b;
}

// ---- appending to a binding (cmx_backend_recon_bind_append_from): `count` events behind n_old bound ones.  A batch that holds B
// events is closed: plan_batches over any longer stream cuts it the same.  Everything behind the closed batches is OPEN -- a last
// batch of fewer than B events, or the lone trailing event no batch has opened (with B = 1: always) -- and is cut again together
// with the new events: the scratch stream is "the open tail ++ the new range", its own plan_batches is the plan of the batches
// [b_recut, nb), and its packed events land at packed_at.  The plan of the whole is plan_batches(n_old + count), nothing else.
struct AppendPlan {
  int b_recut = 0;         // first batch that is cut (again): every batch in front of it stays as it is
  int64_t keep_from = 0;   // its first event, b_recut * B: the events [keep_from, n_old) are the open tail
  int64_t tail_n = 0;      // n_old - keep_from, at most B
  int64_t packed_at = 0;   // packed index of the scratch plan's first event, b_recut * per_batch
  BatchPlan scratch;       // plan_batches(tail_n + count)
  BatchPlan plan;          // plan_batches(n_old + count)
};
inline int64_t open_tail_from(int64_t n, const BatchPlan &p) {  // first event behind the closed batches of n events
  const int64_t full = n / p.B;
  return (full < p.nb ? full : (int64_t)p.nb) * p.B;
}
inline bool plan_append(int64_t n_old, int64_t count, int B, int rate, AppendPlan *a) {  // false: more batches than an int counts
  *a = AppendPlan{};
  BatchPlan old;
  if (!plan_batches(n_old, B, rate, &old)) return false;
  a->keep_from = open_tail_from(n_old, old);
  a->b_recut = (int)(a->keep_from / B);
  a->tail_n = n_old - a->keep_from;
  a->packed_at = (int64_t)a->b_recut * old.per_batch;
  return plan_batches(a->tail_n + count, B, rate, &a->scratch) && plan_batches(n_old + count, B, rate, &a->plan);
}

// the contiguous range of whole batches a group hands member `rank` (cmax_slam_amd/dist.py: batch_range)
inline void batch_range(int64_t n, int B, int rank, int world, int64_t *beg, int64_t *end) {
  const int64_t nb = (n + B - 1) / B, per = (nb + world - 1) / world;
  const int64_t b0 = (int64_t)rank * per < nb ? (int64_t)rank * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
  *beg = b0 * B < n ? b0 * B : n;
  *end = b1 * B < n ? b1 * B : n;
}
// ... and the events the member is handed: one event more than its batches hold.  With the extra event the member's last batch
// is a whole one (n - beg = B + 1 > B) and the event itself is in no batch of this member -- the next member owns it.  The last
// member holding events sees the true tail, the never-opened single-event batch included.
inline void member_range(int64_t n, int B, int rank, int world, int64_t *beg, int64_t *end) {
  batch_range(n, B, rank, world, beg, end);
  if (*end > *beg && *end < n) *end += 1;
}

// ---- the packing pass.  Batch j of the n events of `v` is [j B, min(j B + B, n)); of the batches [0, nb) every rate-th event
// from its batch's start becomes the word x | y << 16 [| (t < t_old) << 31] at out[j per_batch ...] (and its timestamp at
// t_out, when given).  Returns non-zero when a packed event lies outside the W x H sensor.
// kPol (the polarity votes of a reconstruction, host paths): bit 31 carries the event's polarity instead, 1 = ON -- the
// reconstruction kernels mask the bit off before they read the coordinates, so the word serves them as it is.
template <bool kOldFlag, bool kPol = false, typename View>
inline uint32_t pack_word(const View &v, int64_t i, unsigned W, unsigned H, int64_t t_old, unsigned &outside) {
  static_assert(!(kOldFlag && kPol), "bit 31 holds one flag");
  const unsigned ex = v.X(i), ey = v.Y(i);
  outside |= (unsigned)(ex >= W) | (unsigned)(ey >= H);
  uint32_t w = ex | (ey << 16);
  if (kOldFlag) w |= (uint32_t)(v.T(i) < t_old) << 31;
  if (kPol) w |= (uint32_t)v.P(i) << 31;
  return w;
}
template <bool kOldFlag, bool kPol = false, typename View>
unsigned pack_events(const View &v, int64_t n, int64_t nb, int64_t B, int rate, unsigned W, unsigned H, int64_t t_old, uint32_t *out,
                     int64_t *t_out = nullptr) {
  std::atomic<unsigned> outside(0);
  if (rate == 1) {  // flat and vectorisable: packed index == event index
    const int64_t count = nb * B < n ? nb * B : n;
    // (the loop's scalars and pointers by value: captured by reference they may alias the words it stores, and the loop loses its shape)
    parallel_ranges(count, [&, W, H, t_old, out, t_out](int64_t a0, int64_t a1) {
      unsigned acc = 0;
      for (int64_t i = a0; i < a1; i++) {
        out[i] = pack_word<kOldFlag, kPol>(v, i, W, H, t_old, acc);
        if (t_out) t_out[i] = v.T(i);
      }
      if (acc) outside = 1;
    });
  } else {
    const int64_t per_batch = (B + rate - 1) / rate;
    parallel_ranges(nb, [&](int64_t j0, int64_t j1) {
      unsigned acc = 0;
      for (int64_t j = j0; j < j1; j++) {
        const int64_t beg = j * B, end = (n - beg > B) ? beg + B : n;
        int64_t k = j * per_batch;
        for (int64_t i = beg; i < end; i += rate, k++) {
          out[k] = pack_word<kOldFlag, kPol>(v, i, W, H, t_old, acc);
          if (t_out) t_out[k] = v.T(i);
        }
      }
      if (acc) outside = 1;
    });
  }
  return outside.load();
}

// the polarity bytes of an event store: out[i] = 1 for an ON event (any nonzero input), else 0
template <typename View>
void pack_polarity(const View &v, int64_t n, uint8_t *out) {
  parallel_ranges(n, [&, out](int64_t a0, int64_t a1) {
    for (int64_t i = a0; i < a1; i++) out[i] = (uint8_t)v.P(i);
  });
}

// index of the first event outside the W x H sensor, -1 when there is none
template <typename View>
int64_t first_outside(const View &v, int64_t n, unsigned W, unsigned H) {
  std::atomic<int64_t> bad(-1);
  parallel_ranges(n, [&](int64_t a, int64_t b) {
    unsigned acc = 0;
    for (int64_t i = a; i < b; i++) acc |= (unsigned)(v.X(i) >= W) | (unsigned)(v.Y(i) >= H);
    if (acc)
      for (int64_t i = a; i < b; i++)
        if (v.X(i) >= W || v.Y(i) >= H) {
          int64_t cur = bad.load();
          while ((cur < 0 || i < cur) && !bad.compare_exchange_weak(cur, i)) {}
          break;
        }
  });
  return bad.load();
}

// ---- the batch-time pass: emit(b, t_b) with t_b the midpoint (time_batch_ns) of the first and last timestamp of batch b, for b in
// [b_lo, b_hi) of the n events of `v`.  Reports the first batch that spans a negative interval (CMX_ERR_TIME_ORDER, at = its first
// event) or, with a knot support, whose time lies outside it (CMX_ERR_SPLINE_RANGE, at = the batch time); emits nothing for it.
struct BatchTimeError {
  int kind = CMX_OK;
  long long at = -1;
};
template <typename View, typename Emit>
BatchTimeError batch_times(const View &v, int64_t n, int64_t B, int64_t b_lo, int64_t b_hi, const KnotSupport *sup, Emit emit,
                           int64_t serial_below = 262144) {
  auto one = [&](int64_t b, long long *tb) {
    const int64_t beg = b * B, end = (n - beg > B) ? beg + B : n;
    const int64_t t_first = v.T(beg), t_last = v.T(end - 1);
    if (t_last < t_first) return BatchTimeError{CMX_ERR_TIME_ORDER, (long long)beg};
    *tb = time_batch_ns(t_first, t_last);
    const long long st = sup ? *tb - sup->start_ns : 0;
    if (sup && (st < 0 || st / sup->dt_ns + sup->order > sup->K)) return BatchTimeError{CMX_ERR_SPLINE_RANGE, *tb};
    return BatchTimeError{};
  };
  std::atomic<int64_t> bad(-1);
  parallel_ranges(b_hi - b_lo, [&](int64_t j0, int64_t j1) {
    for (int64_t b = b_lo + j0; b < b_lo + j1; b++) {
      long long tb = 0;
      if (one(b, &tb).kind) {
        int64_t cur = bad.load();
        while ((cur < 0 || b < cur) && !bad.compare_exchange_weak(cur, b)) {}
        return;
      }
      emit(b, tb);
    }
  }, serial_below);
  long long tb = 0;
  return bad.load() < 0 ? BatchTimeError{} : one(bad.load(), &tb);
}

}  // namespace cmx

// ingest_host.cpp -- the host ingest layer (cmax_slam_amd/csrc/cmx_ingest.hpp) on its own: no HIP, no context, no GPU.
//   g++ -O2 -std=c++17 -pthread tests/ingest_host.cpp -o ingest_host        (also the program the sanitizer builds use)
//   ingest_host CASE_IN CASE_OUT
// CASE_IN : 16 int64 {n, B, rate, W, H, t_old, order, K, start_ns, dt_ns, stride, off_x, off_y, off_sec, off_nsec, slice_batches},
//           then x[n], y[n] (uint16), t[n] (int64) and the same events as n records of `stride` bytes.
// CASE_OUT: int64 arrays, each behind its length, in the order main() writes them (tests/test_ingest_cpu.py reads them back).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cmax_slam_amd/csrc/cmx_hostpool.hpp"
#include "../cmax_slam_amd/csrc/cmx_ingest.hpp"
#include "../include/cmax_hip.h"

using namespace cmx;

static FILE *g_out = nullptr;
template <typename T>
static void put(const std::vector<T> &v) {
  const int64_t n = (int64_t)v.size();
  fwrite(&n, sizeof(n), 1, g_out);
  for (const T &e : v) {
    const int64_t w = (int64_t)e;
    fwrite(&w, sizeof(w), 1, g_out);
  }
}
static void put(std::initializer_list<int64_t> v) { put(std::vector<int64_t>(v)); }
template <typename T>
static bool get(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <typename View>
static void batch_time_outputs(const View &v, int64_t n, int B, int nb, const KnotSupport *sup) {
  std::vector<long long> bt((size_t)nb, 0);
  const BatchTimeError e = batch_times(v, n, B, 0, nb, sup, [&](int64_t b, long long tb) { bt[(size_t)b] = tb; });
  put({e.kind, e.at});
  put(bt);
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s CASE_IN CASE_OUT\n", argv[0]); return 2; }
  FILE *in = fopen(argv[1], "rb");
  std::vector<int64_t> h, t;
  std::vector<uint16_t> x, y;
  std::vector<unsigned char> rec;
  if (!in || !get(in, h, 16)) { fprintf(stderr, "cannot read the header of %s\n", argv[1]); return 2; }
  const int64_t n = h[0], t_old = h[5];
  const int B = (int)h[1], rate = (int)h[2], slice_batches = (int)h[15];
  const unsigned W = (unsigned)h[3], H = (unsigned)h[4];
  const KnotSupport sup{(int)h[6], (int)h[7], (long long)h[8], (long long)h[9]};
  const cmx_aos_layout layout{(size_t)h[10], (size_t)h[11], (size_t)h[12], (size_t)h[13], (size_t)h[14]};
  if (!get(in, x, (size_t)n) || !get(in, y, (size_t)n) || !get(in, t, (size_t)n) || !get(in, rec, (size_t)n * layout.stride)) {
    fprintf(stderr, "%s is shorter than its header says\n", argv[1]);
    return 2;
  }
  fclose(in);
  g_out = fopen(argv[2], "wb");
  if (!g_out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }

  const EvSoa soa{x.data(), y.data(), t.data()};
  EvAos aos;
  const bool layout_ok = aos_view(rec.data(), &layout, &aos);
  put({layout_ok});
  if (!layout_ok) { fclose(g_out); return 0; }

  // the plan
  BatchPlan p;
  if (!plan_batches(n, B, rate, &p)) return 3;
  put({p.B, p.rate, p.per_batch, p.nb, p.last_len, p.n_packed});

  // the packed words: SoA and AoS view, without and with the old flag, then slice by slice as the reconstruction packs them
  for (int flag = 0; flag < 2; flag++) {
    std::vector<uint32_t> ws((size_t)p.n_packed, 0xdeadbeefu), wa((size_t)p.n_packed, 0xdeadbeefu);
    const unsigned os = flag ? pack_events<true>(soa, n, p.nb, B, rate, W, H, t_old, ws.data())
                             : pack_events<false>(soa, n, p.nb, B, rate, W, H, t_old, ws.data());
    const unsigned oa = flag ? pack_events<true>(aos, n, p.nb, B, rate, W, H, t_old, wa.data())
                             : pack_events<false>(aos, n, p.nb, B, rate, W, H, t_old, wa.data());
    put({os != 0, oa != 0});
    put(ws);
    put(wa);
  }
  {
    std::vector<uint32_t> w((size_t)p.n_packed, 0xdeadbeefu);
    int64_t at = 0;
    for (int b_lo = 0; b_lo < p.nb; b_lo += slice_batches) {
      const int b_hi = (p.nb - b_lo > slice_batches) ? b_lo + slice_batches : p.nb;
      const int64_t ev_off = (int64_t)b_lo * B;
      pack_events<true>(aos.from(ev_off), n - ev_off, b_hi - b_lo, B, rate, W, H, t_old, w.data() + at);
      at += p.packed(b_lo, b_hi);
    }
    put({at});
    put(w);
  }
  // every event with its timestamp, as the event store packs a push
  {
    std::vector<uint32_t> w((size_t)n, 0xdeadbeefu);
    std::vector<int64_t> ts((size_t)n, -1);
    const unsigned o = n ? pack_events<false>(aos, n, 1, n, 1, W, H, 0, w.data(), ts.data()) : 0u;
    put({o != 0, first_outside(soa, n, W, H), first_outside(aos, n, W, H)});
    put(w);
    put(ts);
  }
  // batch times and (error kind, at): back end (knot support) through both views, front end (every event in a batch, no support)
  batch_time_outputs(soa, n, B, p.nb, &sup);
  batch_time_outputs(aos, n, B, p.nb, &sup);
  batch_time_outputs(aos, n, B, (int)((n + B - 1) / B), nullptr);

  // a group's cut: per world size and rank {batch_range, member_range, the member's own plan}
  for (int world : {1, 2, 3, 8}) {
    std::vector<int64_t> rows;
    for (int r = 0; r < world; r++) {
      int64_t b0, b1, m0, m1;
      batch_range(n, B, r, world, &b0, &b1);
      member_range(n, B, r, world, &m0, &m1);
      BatchPlan mp;
      if (!plan_batches(m1 - m0, B, rate, &mp)) return 3;
      for (int64_t v : {b0, b1, m0, m1, (int64_t)mp.nb, mp.n_packed}) rows.push_back(v);
    }
    put(rows);
  }
  return fclose(g_out) == 0 ? 0 : 2;
}

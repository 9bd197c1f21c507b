// cmx_events.cpp -- cmx_events_*: the device-resident event store and the packets /
// windows cut from it (AngVelEstimator::pushEvent / getEventSubset, PoseGraphOptimizer::getEventSubset).
#include "cmx_context.hpp"

// ---- device-resident event store -------------------------------------------------------------------------------
static int efail(cmx_events *e, int code, const char *msg) {
  if (e) e->err = msg;
  return code;
}
static int events_create(cmx_events **out, const int *devices, int n_devices, int W, int H, size_t capacity) {
  if (!out) return CMX_ERR_INVALID_ARG;
  *out = nullptr;
  if (!devices || n_devices < 1 || W <= 0 || H <= 0 || W > 32767 || H > 32767 || capacity == 0 || capacity > (size_t)kMaxEvents)
    return CMX_ERR_INVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CMX_ERR_HIP;
  for (int k = 0; k < n_devices; k++)
    if (devices[k] < 0 || devices[k] >= ndev) return CMX_ERR_INVALID_ARG;
  cmx_events *e = new cmx_events();
  e->device = devices[0]; e->W = W; e->H = H; e->capacity = capacity;
  *out = e;
  for (int k = 0; k < n_devices; k++) {
    if (e->on(devices[k])) continue;  // members that share a device share its replica
    cmx_events::Replica r;
    r.device = devices[k];
    if (hipSetDevice(r.device) != hipSuccess) return efail(e, CMX_ERR_HIP, "hipSetDevice failed");
    e->rep.push_back(r);  // (pushed first: cmx_events_destroy frees whatever a failed allocation left behind)
    cmx_events::Replica &q = e->rep.back();
    if (hipStreamCreateWithFlags(&q.stream, hipStreamNonBlocking) != hipSuccess) return efail(e, CMX_ERR_HIP, "hipStreamCreate failed");
    for (int b = 0; b < 2; b++) {
      if (hipMalloc((void **)&q.d_xy[b], capacity * sizeof(uint32_t)) != hipSuccess) return efail(e, CMX_ERR_HIP, "hipMalloc failed");
      if (hipMalloc((void **)&q.d_t[b], capacity * sizeof(int64_t)) != hipSuccess) return efail(e, CMX_ERR_HIP, "hipMalloc failed");
    }
  }
  e->h_t.reserve(capacity);
  (void)hipSetDevice(e->device);
  return CMX_OK;
}
int cmx_events_create(cmx_events **out, int device, int W, int H, size_t capacity) {
  return events_create(out, &device, 1, W, H, capacity);
}
int cmx_events_create_group(cmx_events **out, const int *devices, int n_devices, int W, int H, size_t capacity) {
  return events_create(out, devices, n_devices, W, H, capacity);
}
void cmx_events_destroy(cmx_events *e) {
  if (!e) return;
  for (cmx_events::Replica &r : e->rep) {
    (void)hipSetDevice(r.device);
    if (r.stream) { (void)hipStreamSynchronize(r.stream); (void)hipStreamDestroy(r.stream); }
    for (int k = 0; k < 2; k++) { (void)hipFree(r.d_xy[k]); (void)hipFree(r.d_t[k]); (void)hipFree(r.d_pol[k]); }
  }
  if (!e->rep.empty()) (void)hipSetDevice(e->rep[0].device);  // the scratch of cmx_events_select*
  (void)hipFree(e->d_sel_ballot); (void)hipFree(e->d_sel_counts); (void)hipFree(e->d_sel_offsets); (void)hipFree(e->d_sel_in);
  if (e->h_sel_total) (void)hipHostFree(e->h_sel_total);
  if (e->h_xy) (void)hipHostFree(e->h_xy);
  if (e->h_tp) (void)hipHostFree(e->h_tp);
  if (e->h_pol) (void)hipHostFree(e->h_pol);
  delete e;
}
const char *cmx_events_last_error(const cmx_events *e) { return e ? e->err.c_str() : "null event store"; }
int64_t cmx_events_begin(const cmx_events *e) { return e ? e->first_index : 0; }
int64_t cmx_events_end(const cmx_events *e) { return e ? e->first_index + (int64_t)e->size : 0; }
int cmx_events_devices(const cmx_events *e, int *devices, int max_devices) {
  if (!e) return 0;
  for (size_t k = 0; k < e->rep.size() && (int)k < max_devices && devices; k++) devices[k] = e->rep[k].device;
  return (int)e->rep.size();
}

// append a chunk of the (time-ordered) stream: AngVelEstimator::pushEvent's events_.push_back (ang_vel_estimator.cpp:68-78).
// One packing pass on the host into pinned staging, then one asynchronous upload per replica (the devices copy side by side).
// with_pol (the _pol forms): the events' polarity goes into a byte array of its own beside d_xy / d_t -- never into bit 31 of the
// packed word, which cmx_backend_set_window_from uses for the old / new flag -- so every consumer that does not ask for polarity
// reads the bytes it always read.  A store holds polarity for all of its events or for none: the first push into an EMPTY store
// decides, and the other form is CMX_ERR_STATE until the store is empty again.
static int events_push_impl(cmx_events *e, const EventSource &src, bool with_pol = false);
int cmx_events_has_polarity(const cmx_events *e) { return e && e->has_pol && e->size > 0 ? 1 : 0; }
int cmx_events_push_pol(cmx_events *e, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns, const uint8_t *pol) {
  if (!e || n < 0 || (n > 0 && (!x || !y || !t_ns || !pol))) return efail(e, CMX_ERR_INVALID_ARG, "bad arguments");
  EventSource src = EventSource::arrays(n, x, y, t_ns);
  src.soa.p = pol;
  return events_push_impl(e, src, true);
}
int cmx_events_push_aos_pol(cmx_events *e, int64_t n, const void *events, const cmx_aos_layout *layout, size_t off_polarity) {
  if (!e || n < 0 || !layout || (n > 0 && !events)) return efail(e, CMX_ERR_INVALID_ARG, "bad arguments");
  EventSource src{EventSource::AOS, n};
  if (!aos_view_pol(events, layout, off_polarity, &src.aos)) return efail(e, CMX_ERR_INVALID_ARG, "record layout: fields outside the record");
  return events_push_impl(e, src, true);
}
int cmx_events_push(cmx_events *e, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns) {
  if (!e || n < 0 || (n > 0 && (!x || !y || !t_ns))) return efail(e, CMX_ERR_INVALID_ARG, "bad arguments");
  return events_push_impl(e, EventSource::arrays(n, x, y, t_ns));
}
// the same from the host's own records (dvs_msgs::Event, cmx_aos_layout): pushEvent's loop over msg->events
// (ang_vel_estimator.cpp:68-78) as ONE call -- x | y << 16 and sec * 1e9 + nsec are formed in the packing pass
int cmx_events_push_aos(cmx_events *e, int64_t n, const void *events, const cmx_aos_layout *layout) {
  if (!e || n < 0 || !layout || (n > 0 && !events)) return efail(e, CMX_ERR_INVALID_ARG, "bad arguments");
  EventSource src{EventSource::AOS, n};
  if (!aos_view(events, layout, &src.aos)) return efail(e, CMX_ERR_INVALID_ARG, "record layout: fields outside the record");
  return events_push_impl(e, src);
}
// pinned staging of at least n events (packed words and timestamps); what it held is gone when it grows
static bool stage_reserve(cmx_events *e, size_t n) {
  if (n <= e->stage_cap) return true;
  if (e->h_xy) (void)hipHostFree(e->h_xy);
  if (e->h_tp) (void)hipHostFree(e->h_tp);
  e->h_xy = nullptr; e->h_tp = nullptr; e->stage_cap = 0;
  const size_t cap = std::max<size_t>(n, 1u << 16);
  if (hipHostMalloc((void **)&e->h_xy, cap * sizeof(uint32_t), hipHostMallocPortable) != hipSuccess ||
      hipHostMalloc((void **)&e->h_tp, cap * sizeof(int64_t), hipHostMallocPortable) != hipSuccess)
    return false;
  e->stage_cap = cap;
  return true;
}
static int events_push_impl(cmx_events *e, const EventSource &src, bool with_pol) {
  const int64_t n = src.n;
  if (e->size > 0 && with_pol != e->has_pol)
    return efail(e, CMX_ERR_STATE, e->has_pol ? "the store's events carry polarity: push with polarity" : "the store's events carry no polarity");
  if (e->size + (size_t)n > e->capacity) return efail(e, CMX_ERR_INVALID_ARG, "event store full: drop old events first");
  if (n == 0) return CMX_OK;
  if (with_pol) {  // the byte arrays, at the first _pol push; the staging, as the other two
    for (cmx_events::Replica &r : e->rep)
      for (int b = 0; b < 2; b++)
        if (!r.d_pol[b] && (hipSetDevice(r.device) != hipSuccess || hipMalloc((void **)&r.d_pol[b], e->capacity) != hipSuccess))
          return efail(e, CMX_ERR_HIP, "hipMalloc failed");
    if ((size_t)n > e->pol_stage_cap) {
      if (e->h_pol) (void)hipHostFree(e->h_pol);
      e->h_pol = nullptr; e->pol_stage_cap = 0;
      const size_t cap = std::max<size_t>((size_t)n, 1u << 16);
      if (hipHostMalloc((void **)&e->h_pol, cap, hipHostMallocPortable) != hipSuccess) return efail(e, CMX_ERR_HIP, "pinned staging allocation failed");
      e->pol_stage_cap = cap;
    }
  }
  if (!stage_reserve(e, (size_t)n)) return efail(e, CMX_ERR_HIP, "pinned staging allocation failed");
  uint32_t *xy = e->h_xy;
  int64_t *tp = e->h_tp;
  const unsigned outside = src.view([&](const auto &v) {  // every event, as one batch
    return pack_events<false>(v, n, 1, n, 1, (unsigned)e->W, (unsigned)e->H, 0, xy, tp);
  });
  if (outside) return efail(e, CMX_ERR_EVENT_RANGE, "event coordinates outside the sensor");
  if (with_pol) src.view([&](const auto &v) { pack_polarity(v, n, e->h_pol); return 0; });
  for (cmx_events::Replica &r : e->rep) {
    if (hipSetDevice(r.device) != hipSuccess) return efail(e, CMX_ERR_HIP, "hipSetDevice failed");
    if (hipMemcpyAsync(r.d_xy[e->cur] + e->size, xy, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, r.stream) != hipSuccess ||
        hipMemcpyAsync(r.d_t[e->cur] + e->size, tp, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, r.stream) != hipSuccess)
      return efail(e, CMX_ERR_HIP, "upload failed");
    if (with_pol && hipMemcpyAsync(r.d_pol[e->cur] + e->size, e->h_pol, (size_t)n, hipMemcpyHostToDevice, r.stream) != hipSuccess)
      return efail(e, CMX_ERR_HIP, "upload failed");
  }
  for (cmx_events::Replica &r : e->rep) {
    if (hipSetDevice(r.device) != hipSuccess || hipStreamSynchronize(r.stream) != hipSuccess) return efail(e, CMX_ERR_HIP, "upload failed");
  }
  (void)hipSetDevice(e->device);
  e->h_t.insert(e->h_t.end(), tp, tp + n);  // (the packed timestamps: the AoS form has no t_ns[] of its own)
  e->size += (size_t)n;
  e->has_pol = with_pol;
  return CMX_OK;
}

// AngVelEstimator::deleteOldEvents (ang_vel_estimator.cpp:149-173): forget everything before a global index
int cmx_events_drop_before(cmx_events *e, int64_t global_index) {
  if (!e) return CMX_ERR_INVALID_ARG;
  if (global_index <= e->first_index) return CMX_OK;
  if (global_index > e->first_index + (int64_t)e->size) return efail(e, CMX_ERR_INVALID_ARG, "index beyond the stored events");
  const size_t k = (size_t)(global_index - e->first_index), keep = e->size - k;
  const int other = 1 - e->cur;
  if (keep) {
    for (cmx_events::Replica &r : e->rep) {
      if (hipSetDevice(r.device) != hipSuccess) return efail(e, CMX_ERR_HIP, "hipSetDevice failed");
      if (hipMemcpyAsync(r.d_xy[other], r.d_xy[e->cur] + k, keep * sizeof(uint32_t), hipMemcpyDeviceToDevice, r.stream) != hipSuccess ||
          hipMemcpyAsync(r.d_t[other], r.d_t[e->cur] + k, keep * sizeof(int64_t), hipMemcpyDeviceToDevice, r.stream) != hipSuccess)
        return efail(e, CMX_ERR_HIP, "compaction failed");
      if (e->has_pol && hipMemcpyAsync(r.d_pol[other], r.d_pol[e->cur] + k, keep, hipMemcpyDeviceToDevice, r.stream) != hipSuccess)
        return efail(e, CMX_ERR_HIP, "compaction failed");
    }
    // the contexts that cut packets / windows from the store use their own non-blocking streams: the compaction is complete
    // on every replica before the buffers are flipped
    //  device-wide: cmx_*_set_*_from leaves an asynchronous copy OUT of the current buffer pending on the consumer's own
    // stream -- after two drops without an evaluation in between the second compaction would write the buffer that copy still reads
    for (cmx_events::Replica &r : e->rep)
      if (hipSetDevice(r.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return efail(e, CMX_ERR_HIP, "compaction failed");
    (void)hipSetDevice(e->device);
  }
  e->h_t.erase(e->h_t.begin(), e->h_t.begin() + (ptrdiff_t)k);
  e->cur = other;
  e->size = keep;
  e->first_index = global_index;
  return CMX_OK;
}

// ---- selection, histogram, read-back (kernels: cmx_select.hip) -------------------------------------------------
// events one slice of a read-back through the pinned staging holds at most: what the staging holds, or
// CMX_DIAG_EVENTS_STAGE_SLICE when set (tests: small stores through the multi-slice loops)
static std::atomic<int> g_events_stage_slice{0};
int events_diag_stage_slice(int n) {
  if (n < 0) return CMX_ERR_INVALID_ARG;
  g_events_stage_slice.store(n, std::memory_order_relaxed);
  return CMX_OK;
}
static size_t stage_slice(const cmx_events *e, size_t left) {
  const int lim = g_events_stage_slice.load(std::memory_order_relaxed);
  return std::min(left, lim > 0 ? std::min(e->stage_cap, (size_t)lim) : e->stage_cap);
}
static bool range_held(const cmx_events *e, int64_t first, int64_t count) {
  return count >= 0 && first >= e->first_index && first + count <= e->first_index + (int64_t)e->size;
}
// everything of cmx_events_select* that can be refused before any work: CMX_OK, or the status with dst's error text set
static int select_check(cmx_events *dst, const cmx_events *src, int64_t first, int64_t count, const cmx_select *sel) {
  if (!dst || !src) return efail(dst, CMX_ERR_INVALID_ARG, "null event store");
  if (dst == src) return efail(dst, CMX_ERR_INVALID_ARG, "select: source and destination are the same store (no selection in place)");
  if (!sel || sel->size != sizeof(cmx_select)) return efail(dst, CMX_ERR_INVALID_ARG, "select: null cmx_select or a size that is not this library's");
  if (dst->W != src->W || dst->H != src->H) return efail(dst, CMX_ERR_INVALID_ARG, "select: the stores belong to different sensors");
  if (dst->rep.size() != 1 || src->rep.size() != 1)
    return efail(dst, CMX_ERR_INVALID_ARG, "select: group stores (more than one replica) are out of scope");
  if (dst->rep[0].device != src->rep[0].device) return efail(dst, CMX_ERR_INVALID_ARG, "select: the stores are on different devices");
  if (!range_held(src, first, count)) return efail(dst, CMX_ERR_INVALID_ARG, "select: range not held by the source store");
  if (src->size > 0 && dst->size > 0 && dst->has_pol != src->has_pol)
    return efail(dst, CMX_ERR_STATE, dst->has_pol ? "the store's events carry polarity: the source's do not" : "the store's events carry no polarity: the source's do");
  return CMX_OK;
}
int cmx_events_select_device(cmx_events *dst, const cmx_events *src, int64_t first, int64_t count, const cmx_select *sel, int64_t *n_kept) {
  const int rc = select_check(dst, src, first, count, sel);
  if (rc) return rc;
  if (n_kept) *n_kept = 0;
  if (count == 0) return CMX_OK;
  cmx_events::Replica &r = dst->rep[0];
  const cmx_events::Replica &q = src->rep[0];
  const bool with_pol = src->has_pol;
  if (hipSetDevice(r.device) != hipSuccess) return efail(dst, CMX_ERR_HIP, "hipSetDevice failed");
  if (with_pol)
    for (int b = 0; b < 2; b++)
      if (!r.d_pol[b] && hipMalloc((void **)&r.d_pol[b], dst->capacity) != hipSuccess) return efail(dst, CMX_ERR_HIP, "hipMalloc failed");
  const size_t ntiles = (size_t)sel_tiles(count);
  if (ntiles > dst->sel_tiles_cap) {
    (void)hipFree(dst->d_sel_ballot); (void)hipFree(dst->d_sel_counts); (void)hipFree(dst->d_sel_offsets);
    dst->d_sel_ballot = nullptr; dst->d_sel_counts = nullptr; dst->d_sel_offsets = nullptr; dst->sel_tiles_cap = 0;
    if (hipMalloc((void **)&dst->d_sel_ballot, ntiles * 64 * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc((void **)&dst->d_sel_counts, ntiles * sizeof(unsigned)) != hipSuccess ||
        hipMalloc((void **)&dst->d_sel_offsets, (ntiles + 1) * sizeof(long long)) != hipSuccess)
      return efail(dst, CMX_ERR_HIP, "hipMalloc failed");
    dst->sel_tiles_cap = ntiles;
  }
  if (!dst->h_sel_total && hipHostMalloc((void **)&dst->h_sel_total, sizeof(int64_t), hipHostMallocPortable) != hipSuccess)
    return efail(dst, CMX_ERR_HIP, "pinned allocation failed");
  const size_t off = (size_t)(first - src->first_index);
  SelectArgs a{};
  a.n = count; a.W = src->W;
  a.src_xy = q.d_xy[src->cur] + off;
  a.src_t = reinterpret_cast<const long long *>(q.d_t[src->cur] + off);
  a.src_pol = with_pol ? q.d_pol[src->cur] + off : nullptr;
  a.keep = sel->keep; a.score = sel->score; a.min_score = sel->min_score;
  a.flags = sel->flags; a.flags_mask = sel->flags_mask; a.flags_value = sel->flags_value;
  a.pixel_keep = sel->pixel_keep;
  a.ballot = dst->d_sel_ballot; a.counts = dst->d_sel_counts; a.offsets = dst->d_sel_offsets;
  a.dst_xy = r.d_xy[dst->cur] + dst->size;
  a.dst_t = reinterpret_cast<long long *>(r.d_t[dst->cur] + dst->size);
  a.dst_pol = with_pol ? r.d_pol[dst->cur] + dst->size : nullptr;
  launch_select_mark(a, r.stream);
  launch_select_scan(a.counts, (long long)ntiles, a.offsets, r.stream);
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(dst->h_sel_total, a.offsets + ntiles, sizeof(int64_t), hipMemcpyDeviceToHost, r.stream) != hipSuccess ||
      hipStreamSynchronize(r.stream) != hipSuccess)
    return efail(dst, CMX_ERR_HIP, "select: the count pass failed");
  const int64_t kept = *dst->h_sel_total;
  if (kept < 0 || kept > count) return efail(dst, CMX_ERR_HIP, "select: the count pass returned an impossible total");
  if (dst->size + (size_t)kept > dst->capacity) return efail(dst, CMX_ERR_INVALID_ARG, "event store full: drop old events first");
  if (kept == 0) return CMX_OK;
  // the slots behind dst->size belong to nobody until size is committed: an error from here on leaves the store as it was
  launch_select_scatter(a, r.stream);
  if (hipGetLastError() != hipSuccess) return efail(dst, CMX_ERR_HIP, "select: the scatter launch failed");
  // the host mirror: the kept timestamps back from dst's own buffer through the pinned staging, slice by slice (a staging that has
  // to grow grows to at most 2^22 events, 48 MB pinned: the slices of cmx_backend_recon_add*)
  if (!stage_reserve(dst, (size_t)std::min<int64_t>(kept, (int64_t)1 << 22))) return efail(dst, CMX_ERR_HIP, "pinned staging allocation failed");
  const size_t size0 = dst->size;
  for (size_t done = 0; done < (size_t)kept;) {
    const size_t m = stage_slice(dst, (size_t)kept - done);
    if (hipMemcpyAsync(dst->h_tp, r.d_t[dst->cur] + size0 + done, m * sizeof(int64_t), hipMemcpyDeviceToHost, r.stream) != hipSuccess ||
        hipStreamSynchronize(r.stream) != hipSuccess) {
      dst->h_t.resize(size0);
      return efail(dst, CMX_ERR_HIP, "select: the scatter or the timestamps' read-back failed");
    }
    if (done == 0 && size0 > 0 && dst->h_tp[0] < dst->h_t[size0 - 1])
      return efail(dst, CMX_ERR_TIME_ORDER, "select: the first kept event is earlier than the store's last event");
    dst->h_t.insert(dst->h_t.end(), dst->h_tp, dst->h_tp + m);
    done += m;
  }
  dst->size = size0 + (size_t)kept;
  dst->has_pol = with_pol;
  if (n_kept) *n_kept = kept;
  return CMX_OK;
}
// host arrays: uploaded into scratch of dst (floats first: 4-byte alignment), then the device form
int cmx_events_select(cmx_events *dst, const cmx_events *src, int64_t first, int64_t count, const cmx_select *sel, int64_t *n_kept) {
  const int rc = select_check(dst, src, first, count, sel);
  if (rc) return rc;
  if (count == 0) return cmx_events_select_device(dst, src, first, count, sel, n_kept);  // (nothing is read)
  const size_t n = (size_t)count, npix = (size_t)src->W * (size_t)src->H, n4 = (n + 3) & ~(size_t)3;
  const size_t need = (sel->score ? n * sizeof(float) : 0) + (sel->keep ? n4 : 0) + (sel->flags ? n4 : 0) + (sel->pixel_keep ? npix : 0);
  cmx_events::Replica &r = dst->rep[0];
  if (hipSetDevice(r.device) != hipSuccess) return efail(dst, CMX_ERR_HIP, "hipSetDevice failed");
  if (need > dst->sel_in_cap) {
    (void)hipFree(dst->d_sel_in);
    dst->d_sel_in = nullptr; dst->sel_in_cap = 0;
    if (hipMalloc((void **)&dst->d_sel_in, need) != hipSuccess) return efail(dst, CMX_ERR_HIP, "hipMalloc failed");
    dst->sel_in_cap = need;
  }
  cmx_select dev = *sel;
  unsigned char *p = dst->d_sel_in;
  auto upload = [&](const void *h, size_t bytes, size_t step) -> const void * {
    if (!h) return nullptr;
    const void *d = p;
    if (hipMemcpyAsync(p, h, bytes, hipMemcpyHostToDevice, r.stream) != hipSuccess) return nullptr;
    p += step;
    return d;
  };
  dev.score = (const float *)upload(sel->score, n * sizeof(float), n * sizeof(float));
  dev.keep = (const unsigned char *)upload(sel->keep, n, n4);
  dev.flags = (const unsigned char *)upload(sel->flags, n, n4);
  dev.pixel_keep = (const unsigned char *)upload(sel->pixel_keep, npix, npix);
  if ((sel->score && !dev.score) || (sel->keep && !dev.keep) || (sel->flags && !dev.flags) || (sel->pixel_keep && !dev.pixel_keep))
    return efail(dst, CMX_ERR_HIP, "select: upload of the criteria failed");
  if (hipStreamSynchronize(r.stream) != hipSuccess) return efail(dst, CMX_ERR_HIP, "select: upload of the criteria failed");  // (the caller's arrays are free again)
  return cmx_events_select_device(dst, src, first, count, &dev, n_kept);
}

// counts[y * W + x] = events of the range at that pixel: written, not accumulated.  A group store: its first replica.
int cmx_events_pixel_counts_device(const cmx_events *ev, int64_t first, int64_t count, uint32_t *d_counts) {
  cmx_events *e = const_cast<cmx_events *>(ev);  // (the error text only)
  if (!ev || !d_counts) return efail(e, CMX_ERR_INVALID_ARG, "bad arguments");
  if (!range_held(ev, first, count)) return efail(e, CMX_ERR_INVALID_ARG, "pixel_counts: range not held by the event store");
  const cmx_events::Replica &r = ev->rep[0];
  if (hipSetDevice(r.device) != hipSuccess) return efail(e, CMX_ERR_HIP, "hipSetDevice failed");
  if (hipMemsetAsync(d_counts, 0, (size_t)ev->W * (size_t)ev->H * sizeof(uint32_t), r.stream) != hipSuccess)
    return efail(e, CMX_ERR_HIP, "pixel_counts: hipMemsetAsync failed");
  launch_pixel_counts(r.d_xy[ev->cur] + (size_t)(first - ev->first_index), count, ev->W, d_counts, r.stream);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(r.stream) != hipSuccess) return efail(e, CMX_ERR_HIP, "pixel_counts: the kernel failed");
  return CMX_OK;
}
int cmx_events_pixel_counts(const cmx_events *ev, int64_t first, int64_t count, uint32_t *counts) {
  cmx_events *e = const_cast<cmx_events *>(ev);
  if (!ev || !counts) return efail(e, CMX_ERR_INVALID_ARG, "bad arguments");
  if (!range_held(ev, first, count)) return efail(e, CMX_ERR_INVALID_ARG, "pixel_counts: range not held by the event store");
  const size_t bytes = (size_t)ev->W * (size_t)ev->H * sizeof(uint32_t);
  uint32_t *d = nullptr;
  if (hipSetDevice(ev->rep[0].device) != hipSuccess || hipMalloc((void **)&d, bytes) != hipSuccess) return efail(e, CMX_ERR_HIP, "hipMalloc failed");
  int rc = cmx_events_pixel_counts_device(ev, first, count, d);
  if (rc == CMX_OK && hipMemcpy(counts, d, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = efail(e, CMX_ERR_HIP, "pixel_counts: read-back failed");
  (void)hipFree(d);
  return rc;
}

// the inverse of cmx_events_push_pol: a test and export call, through the pinned staging in slices (a group store: its first replica)
int cmx_events_read(const cmx_events *ev, int64_t first, int64_t count, uint16_t *x, uint16_t *y, int64_t *t_ns, unsigned char *pol) {
  cmx_events *e = const_cast<cmx_events *>(ev);  // (the staging and the error text: scratch, not state)
  if (!ev) return CMX_ERR_INVALID_ARG;
  if (!range_held(ev, first, count)) return efail(e, CMX_ERR_INVALID_ARG, "read: range not held by the event store");
  if (pol && !(ev->has_pol && ev->size > 0)) return efail(e, CMX_ERR_STATE, "the store's events carry no polarity");
  if (count == 0) return CMX_OK;
  const cmx_events::Replica &r = ev->rep[0];
  if (hipSetDevice(r.device) != hipSuccess) return efail(e, CMX_ERR_HIP, "hipSetDevice failed");
  if (!stage_reserve(e, 1)) return efail(e, CMX_ERR_HIP, "pinned staging allocation failed");
  const size_t off = (size_t)(first - ev->first_index), n = (size_t)count;
  for (size_t done = 0; done < n;) {
    const size_t m = stage_slice(e, n - done);
    if (((x || y) && hipMemcpyAsync(e->h_xy, r.d_xy[ev->cur] + off + done, m * sizeof(uint32_t), hipMemcpyDeviceToHost, r.stream) != hipSuccess) ||
        (t_ns && hipMemcpyAsync(e->h_tp, r.d_t[ev->cur] + off + done, m * sizeof(int64_t), hipMemcpyDeviceToHost, r.stream) != hipSuccess) ||
        hipStreamSynchronize(r.stream) != hipSuccess)
      return efail(e, CMX_ERR_HIP, "read: copy failed");
    for (size_t i = 0; i < m && (x || y); i++) {
      if (x) x[done + i] = (uint16_t)(e->h_xy[i] & 0xffffu);
      if (y) y[done + i] = (uint16_t)((e->h_xy[i] >> 16) & 0x7fffu);
    }
    if (t_ns) memcpy(t_ns + done, e->h_tp, m * sizeof(int64_t));
    done += m;
  }
  if (pol && hipMemcpy(pol, r.d_pol[ev->cur] + off, n, hipMemcpyDeviceToHost) != hipSuccess) return efail(e, CMX_ERR_HIP, "read: copy failed");
  return CMX_OK;
}

// events_[first, first + count) of the store, as the replica on c's device holds them
int store_source(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count, EventSource *out) {
  if (!e) return fail(c, CMX_ERR_INVALID_ARG, "null event store");
  if (!c) return CMX_ERR_INVALID_ARG;
  const cmx_events::Replica *rep = e->on(c->device);
  if (!rep || e->W != c->W || e->H != c->H)
    return fail(c, CMX_ERR_INVALID_ARG, "event store belongs to another device / sensor");
  if (count < 0 || first < e->first_index || first + count > e->first_index + (int64_t)e->size)
    return fail(c, CMX_ERR_INVALID_ARG, "range [%lld, %lld) is not held by the event store [%lld, %lld)", (long long)first,
                (long long)(first + count), (long long)e->first_index, (long long)(e->first_index + (int64_t)e->size));
  const size_t off = (size_t)(first - e->first_index);
  *out = EventSource{EventSource::DEVICE, count, EvSoa{nullptr, nullptr, e->h_t.data() + off}, EvAos{}, e, first,
                     rep->d_xy[e->cur] + off, rep->d_t[e->cur] + off, e->has_pol && e->size > 0 ? rep->d_pol[e->cur] + off : nullptr};
  return CMX_OK;
}

// packets / windows cut from the store: events_[first, first+count), exactly what getEventSubset copies
// (ang_vel_estimator.cpp:137-147, pose_graph_optimizer.cpp:131-165), without leaving the device
int cmx_frontend_set_packet_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count, int64_t t_ref_ns, double fx,
                                 double fy, double cx, double cy, int event_batch_size, double blur_sigma,
                                 int contrast_measure) {
  EventSource src;
  const int rc = store_source(c, e, first, count, &src);
  if (rc) return rc;
  return fe_set_packet_impl(c, src, t_ref_ns, fx, fy, cx, cy, event_batch_size, blur_sigma, contrast_measure);
}
int cmx_backend_set_window_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count, int order, int K,
                                const double *knots_xyzw, int64_t start_ns, int64_t dt_ns, int num_fixed,
                                int64_t t_next_win_beg_ns, int event_batch_size, int event_sample_rate, double blur_sigma,
                                int contrast_measure, const float *IG) {
  const WindowSpec w{{order, K, start_ns, dt_ns}, knots_xyzw, num_fixed, t_next_win_beg_ns, event_batch_size, event_sample_rate, blur_sigma,
                     contrast_measure, IG};
  // (a group: every member cuts its range from the replica on its own device, group_member_window_from)
  if (is_group(c)) return group_set_window(c, EventSource{EventSource::DEVICE, count, EvSoa{}, EvAos{}, e, first}, w);
  EventSource src;
  const int rc = store_source(c, e, first, count, &src);
  if (rc) return rc;
  return be_set_window_impl(c, src, w);
}

// A window cut from a replicated store on a GROUP: member r cuts ITS batch range (the range group_set_window hands it, the
// one-event rule included) from the replica on its own device -- no event crosses the host or a link at hand-over
// (pose_graph_optimizer.cpp:131-165 is the copy this replaces; event_pano_warper.cpp:188-196 the loop being sharded).
int group_member_window_from(cmx_ctx *m, const EventSource &src, const WindowSpec &w) {
  EventSource mine;
  const int rc = store_source(m, src.store, src.first, src.n, &mine);
  if (rc) return rc;
  return be_set_window_impl(m, mine, w);
}

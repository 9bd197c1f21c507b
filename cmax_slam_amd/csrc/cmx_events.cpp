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
  if ((size_t)n > e->stage_cap) {
    if (e->h_xy) (void)hipHostFree(e->h_xy);
    if (e->h_tp) (void)hipHostFree(e->h_tp);
    e->h_xy = nullptr; e->h_tp = nullptr; e->stage_cap = 0;
    const size_t cap = std::max<size_t>((size_t)n, 1u << 16);
    if (hipHostMalloc((void **)&e->h_xy, cap * sizeof(uint32_t), hipHostMallocPortable) != hipSuccess ||
        hipHostMalloc((void **)&e->h_tp, cap * sizeof(int64_t), hipHostMallocPortable) != hipSuccess)
      return efail(e, CMX_ERR_HIP, "pinned staging allocation failed");
    e->stage_cap = cap;
  }
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

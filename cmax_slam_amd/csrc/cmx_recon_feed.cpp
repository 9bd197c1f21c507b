// cmx_recon_feed.cpp -- every cmx_backend_recon_* call that is handed events: ONE walk over them (feed) in slices of whole batches
// (feed_slice_at, cmx_ingest.hpp), and what each call does with a slice on the device.
//   add*       the vote loop of EventWarper::computeImageOfWarpedEvents (event_pano_warper.cpp:188-196, :233-311) over the sampled
//              events, into the reconstruction's plane
//   grad_add*  the second pass over the same events, their share of the gradient sums
//   warp*      the per-event export: where EVERY event handed in lands under the knots the reconstruction holds now
//   score*     the export's walk with another sink: the support plane of the open score pass read at every event
//   pol_add*   add*'s vote loop into the ON / OFF planes of the signed polarity map
//   view_add*  add*'s vote loop into the planes of the pinhole views
//   voxel_add* add*'s vote loop into the bins of the voxel grids, by every event's own timestamp and polarity
//   surface_add*  add*'s vote loop into the cells of the time surfaces: the latest timestamp per pixel and polarity
// Host arrays (SoA, or the host's own records) are packed slice by slice into two slots of pinned memory and uploaded on the copy
// stream while the slice before runs; a range of an event store is read in place, its batch times formed on the device.
#include "cmx_recon_state.hpp"

int queue_gather(cmx_ctx *c, ReconState *r, ReconGatherArgs &g) {
  const int blocks = recon_gather_blocks(g.ev);
  if (blocks <= 0) return CMX_OK;
  if (r->deterministic) {
    if ((size_t)blocks > r->rows_cap) HIP_TRY(c, hipStreamSynchronize(c->stream));  // (an earlier slice may still be reading the rows)
    const int rc = ensure_pair(c, r->d_rows, r->d_row_win, r->rows_cap, (size_t)blocks);
    if (rc) return rc;
    g.rows = r->d_rows[0];
    g.row_win = r->d_row_win;
  }
  launch_recon_gather(g, c->stream);
  launch_recon_gather_rows(g, blocks, c->stream);
  return CMX_OK;
}

int validate_store_times(cmx_ctx *c, ReconState *r, const int64_t *d_t, int64_t n, const BatchPlan &p, int slice_batches, long long *d_bt) {
  int rc = CMX_OK;
  FeedSlice f;
  for (int64_t k = 0; !rc && feed_slice_at(p, n, slice_batches, false, k, &f); k++)
    rc = queue_batch_times(c, d_t + f.ev_first, f.ev_n, p.B, f.b_hi - f.b_lo, r->sup, d_bt, r->d_err, k == 0);
  if (rc) return rc;
  HIP_TRY(c, hipGetLastError());
  BatchTimeError bad;
  rc = read_batch_errors(c, r->d_err, &bad);
  if (rc) return rc;
  if (bad.kind) return fail_batch_time(c, bad, r->sup, /*with_event=*/false);  // (its index would be relative to a slice)
  return CMX_OK;
}

static int slot_ensure(cmx_ctx *c, ReconSlot &s, size_t n_xy, size_t n_bt, bool with_time) {
  int rc = ensure_pinned(c, s.h_xy, s.h_xy_cap, n_xy);
  if (!rc) rc = ensure(c, s.d_xy, s.xy_cap, n_xy);
  if (!rc) rc = ensure_pinned(c, s.h_bt, s.h_bt_cap, n_bt);
  if (!rc) rc = ensure(c, s.d_bt, s.bt_cap, n_bt);
  if (!rc && with_time) rc = ensure_pinned(c, s.h_t, s.h_t_cap, n_xy);
  if (!rc && with_time) rc = ensure(c, s.d_t, s.t_cap, n_xy);
  return rc;
}

// ---- the feeder
// argument checks of a hand-over, and for host sources EVERY coordinate inside the sensor, those the sampling or the one-event rule
// skip included: what cmx_backend_set_window checks when it sub-samples, here at every rate (cmax_hip.h).  First thing of every
// call, in front of feed (the export has a check of its own between the two).
static int feed_checks(cmx_ctx *c, const EventSource &src) {
  if (!src.on_device()) return check_events(c, src);
  if (src.n < 0 || src.n > kMaxEvents) return fail(c, CMX_ERR_INVALID_ARG, "bad event count %lld", (long long)src.n);
  return CMX_OK;
}

// a slice as its consumer finds it on the device
struct FedSlice : FeedSlice {
  int64_t k = 0;
  const uint32_t *d_xy = nullptr;     // its events: packed (host sources; every_event: all ev_n of them, else the n sampled ones), or the
                                      // store's own from ev_first on, to be read in place
  const long long *d_bt = nullptr;    // its batch times
  long long lone_t = 0;               // every_event: the time of the call's lone trailing event
  const long long *d_t = nullptr;     // with_time: its events' own timestamps, indexed as d_xy is
};

// The batch plan of the n events of src, then validation of EVERYTHING -- a call that fails adds nothing: every batch time (host:
// batch_times; store: validate_store_times) and, every_event, the lone trailing event's own time -- and only then slice by slice:
// stage it, on_slice(slice), mark the staging in use.  Host sources: slice k+1 is packed (at the call's rate, or every event) and
// uploaded while the kernels of slice k run.  Store sources: the batch times of the slice into slot[0]'s table; a single slice finds
// there what the validation pass has just written.  From the first slice on only a runtime error (CMX_ERR_HIP) can end the call,
// and slices queued before it have run.  Returns after the context's stream has run dry, the slots idle either way.
// with_pol (pol_add*, signed voxel_add*, by-polarity surface_add*; host sources): the packed words carry the events' polarity in bit 31.
// with_time (voxel_add*, surface_add*; never with every_event): the slice also carries its events' own timestamps -- host sources: one int64 per
// packed event, written by the packing pass beside the word into the same slot and uploaded with it; store: its own array in place.
template <typename OnSlice>
static int feed(cmx_ctx *c, ReconState *r, const EventSource &src, bool every_event, bool with_pol, bool with_time, BatchPlan *plan,
                OnSlice on_slice) {
  const bool store = src.on_device();
  const int64_t n = src.n;
  const int B = r->B;
  BatchPlan &p = *plan;
  int slice_batches = 1;
  int rc = recon_plan(c, r, n, &p, &slice_batches);
  if (rc) return rc;
  FedSlice f;
  if (!feed_slice_at(p, n, slice_batches, every_event, 0, &f)) return CMX_OK;
  const bool lone = every_event && (int64_t)p.nb * B < n;  // the trailing event no batch holds (n = nb B + 1)
  f.lone_t = lone ? (long long)src.view([&](const auto &v) { return v.T(n - 1); }) : 0;  // (store: its host mirror)
  ReconSlot &s0 = r->slot[0];
  if (store && p.nb > 0) {
    rc = ensure(c, s0.d_bt, s0.bt_cap, (size_t)(p.nb < slice_batches ? p.nb : slice_batches));
    if (!rc) rc = validate_store_times(c, r, src.d_t, n, p, slice_batches, s0.d_bt);
    if (rc) return rc;
  } else if (p.nb > 0) {
    const BatchTimeError bad = src.view([&](const auto &v) { return batch_times(v, n, B, 0, p.nb, &r->sup, [](int64_t, long long) {}); });
    if (bad.kind) return fail_batch_time(c, bad, r->sup);
  }
  if (lone) {  // its own time is its pose time: inside the spline like a batch time
    const long long st = f.lone_t - r->sup.start_ns;
    if (st < 0 || st / r->sup.dt_ns + r->sup.order > r->sup.K) return fail_batch_time(c, BatchTimeError{CMX_ERR_SPLINE_RANGE, f.lone_t}, r->sup);
  }
  const bool one_slice = p.nb <= slice_batches;
  auto slices = [&]() -> int {
    for (f.k = 0; feed_slice_at(p, n, slice_batches, every_event, f.k, &f); f.k++) {
      const int nbs = f.b_hi - f.b_lo;
      ReconSlot &s = r->slot[f.k & 1];
      if (store) {
        if (!one_slice) {
          rc = queue_batch_times(c, src.d_t + f.ev_first, f.ev_n, B, nbs, r->sup, s0.d_bt, r->d_err, false);
          if (rc) return rc;
        }
        f.d_xy = src.d_xy + f.ev_first;
        f.d_bt = s0.d_bt;
        f.d_t = reinterpret_cast<const long long *>(src.d_t + f.ev_first);
      } else {
        const int64_t n_xy = every_event ? f.ev_n : f.n;
        if (s.busy) { HIP_TRY(c, hipEventSynchronize(s.done)); s.busy = false; }  // its previous slice has been consumed
        rc = slot_ensure(c, s, (size_t)n_xy, (size_t)nbs, with_time);
        if (rc) return rc;
        uint32_t *xy = s.h_xy;
        long long *bt = s.h_bt;
        int64_t *ts = with_time ? s.h_t : nullptr;
        src.view([&](const auto &v) {  // (validated above: neither pass finds anything)
          if (nbs > 0) batch_times(v, n, B, f.b_lo, f.b_hi, nullptr, [&](int64_t b, long long tb) { bt[b - f.b_lo] = tb; });
          const auto vs = v.from(f.ev_first);
          const int rate = every_event ? 1 : r->rate;
          unsigned outside = with_pol ? pack_events<false, true>(vs, n - f.ev_first, nbs, B, rate, (unsigned)c->W, (unsigned)c->H, 0, xy, ts)
                                      : pack_events<false>(vs, n - f.ev_first, nbs, B, rate, (unsigned)c->W, (unsigned)c->H, 0, xy, ts);
          if (f.lone) xy[f.ev_n - 1] = pack_word<false>(vs, f.ev_n - 1, (unsigned)c->W, (unsigned)c->H, 0, outside);
          return outside;
        });
        HIP_TRY(c, hipMemcpyAsync(s.d_xy, xy, (size_t)n_xy * sizeof(uint32_t), hipMemcpyHostToDevice, r->copy_stream));
        if (nbs > 0) HIP_TRY(c, hipMemcpyAsync(s.d_bt, bt, (size_t)nbs * sizeof(long long), hipMemcpyHostToDevice, r->copy_stream));
        if (ts) HIP_TRY(c, hipMemcpyAsync(s.d_t, ts, (size_t)n_xy * sizeof(int64_t), hipMemcpyHostToDevice, r->copy_stream));
        HIP_TRY(c, hipEventRecord(s.up, r->copy_stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, s.up, 0));
        f.d_xy = s.d_xy;
        f.d_bt = s.d_bt;
        f.d_t = reinterpret_cast<const long long *>(s.d_t);
      }
      rc = on_slice(f);
      if (rc) return rc;
      HIP_TRY(c, hipGetLastError());
      if (!store) {
        HIP_TRY(c, hipEventRecord(s.done, c->stream));
        s.busy = true;
      }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CMX_OK;
  };
  rc = slices();
  if (rc) { (void)hipStreamSynchronize(r->copy_stream); (void)hipStreamSynchronize(c->stream); }
  r->slot[0].busy = r->slot[1].busy = false;
  return rc;
}

// ---- add*, grad_add*: the vote pass or the gradient pass over the events handed in
int recon_add_source(cmx_ctx *c, const EventSource &src, bool grad) {
  ReconState *r = c->recon;
  if (int rc0 = recon_pass_enter(c, r, grad)) return rc0;
  int rc = feed_checks(c, src);
  if (rc) return rc;
  ReconGatherArgs ga = recon_gather_args(c, r);
  ReconArgs &a = ga.ev;
  BatchPlan p;
  rc = feed(c, r, src, false, false, false, &p, [&](const FedSlice &s) {
    a.xy = s.d_xy; a.stride = src.on_device() ? r->rate : 0;  // (the store's events in place: the sampling is an index map)
    a.batch_t = s.d_bt; a.nb = s.b_hi - s.b_lo;
    a.n = (int)s.n;
    if (grad) return queue_gather(c, r, ga);
    launch_recon_votes(a, c->stream);
    return (int)CMX_OK;
  });
  if (rc) return rc;
  (grad ? r->g_sampled : r->n_sampled) += p.n_packed;
  return CMX_OK;
}

// the six entry points: the front door, the call's own way to its source (host arrays, the host's records, a range of an event
// store -- with that form's argument checks), then the pass over it
template <typename MakeSource>
static int recon_add_entry(cmx_ctx *c, bool grad, MakeSource make) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  EventSource src;
  rc = make(&src);
  if (rc) return rc;
  return recon_add_source(c, src, grad);
}
int cmx_backend_recon_add(cmx_ctx *c, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns) {
  return recon_add_entry(c, false, [&](EventSource *src) { *src = EventSource::arrays(n, x, y, t_ns); return (int)CMX_OK; });
}
int cmx_backend_recon_grad_add(cmx_ctx *c, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns) {
  return recon_add_entry(c, true, [&](EventSource *src) { *src = EventSource::arrays(n, x, y, t_ns); return (int)CMX_OK; });
}
int cmx_backend_recon_add_aos(cmx_ctx *c, int64_t n, const void *events, const cmx_aos_layout *layout) {
  return recon_add_entry(c, false, [&](EventSource *src) { return make_aos(c, n, events, layout, src); });
}
int cmx_backend_recon_grad_add_aos(cmx_ctx *c, int64_t n, const void *events, const cmx_aos_layout *layout) {
  return recon_add_entry(c, true, [&](EventSource *src) { return make_aos(c, n, events, layout, src); });
}
int cmx_backend_recon_add_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count) {
  return recon_add_entry(c, false, [&](EventSource *src) { return store_source(c, e, first, count, src); });
}
int cmx_backend_recon_grad_add_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count) {
  return recon_add_entry(c, true, [&](EventSource *src) { return store_source(c, e, first, count, src); });
}

// ---- pol_add*: add*'s vote pass with the ON / OFF planes as its target.  Nothing of the reconstruction but the knots is read, and
// nothing but those two planes and their counters is written: no recon_pass_enter (an open gradient pass stays open), no n_sampled.
// Host sources carry the polarity in bit 31 of the packed word, a store in its byte array at the index of the word.
static int recon_pol_add_source(cmx_ctx *c, const EventSource &src) {
  ReconState *r = c->recon;
  int rc = feed_checks(c, src);
  if (rc) return rc;
  rc = recon_pol_ensure(c, r);
  if (rc) return rc;
  ReconArgs a = recon_args(c, r);
  a.plane = r->d_pol;
  a.fixed = r->d_pol_fixed;
  a.n_inside = r->d_pol_inside;
  BatchPlan p;
  return feed(c, r, src, false, !src.on_device(), false, &p, [&](const FedSlice &s) {
    a.xy = s.d_xy; a.stride = src.on_device() ? r->rate : 0;
    a.pol = src.on_device() ? src.d_pol + s.ev_first : nullptr;
    a.batch_t = s.d_bt; a.nb = s.b_hi - s.b_lo;
    a.n = (int)s.n;
    launch_recon_votes_pol(a, c->stream);
    return (int)CMX_OK;
  });
}
template <typename MakeSource>
static int recon_pol_add_entry(cmx_ctx *c, MakeSource make) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  EventSource src;
  rc = make(&src);
  if (rc) return rc;
  return recon_pol_add_source(c, src);
}
int cmx_backend_recon_pol_add(cmx_ctx *c, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns, const uint8_t *pol) {
  return recon_pol_add_entry(c, [&](EventSource *src) {
    if (n > 0 && !pol) return fail(c, CMX_ERR_INVALID_ARG, "null polarity array");
    *src = EventSource::arrays(n, x, y, t_ns);
    src->soa.p = pol;
    return (int)CMX_OK;
  });
}
int cmx_backend_recon_pol_add_aos(cmx_ctx *c, int64_t n, const void *events, const cmx_aos_layout *layout, size_t off_polarity) {
  return recon_pol_add_entry(c, [&](EventSource *src) {
    const int rc = make_aos(c, n, events, layout, src);
    if (rc) return rc;
    if (off_polarity >= layout->stride) return fail(c, CMX_ERR_INVALID_ARG, "record layout: polarity outside the %zu-byte record", layout->stride);
    src->aos.op = off_polarity;
    return (int)CMX_OK;
  });
}
int cmx_backend_recon_pol_add_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count) {
  return recon_pol_add_entry(c, [&](EventSource *src) {
    const int rc = store_source(c, e, first, count, src);
    if (rc) return rc;
    if (e->size > 0 && !e->has_pol) return fail(c, CMX_ERR_STATE, "the event store holds no polarity (cmx_events_push_pol)");
    return (int)CMX_OK;
  });
}

// ---- view_add*, voxel_add*, surface_add*: add*'s vote pass with the targets of a set as its targets.  As pol_add*:
// nothing of the reconstruction but the knots is read, nothing but the set's planes or cells and its counters is written, an open
// gradient pass stays open.  The packed words are those of add*; for the sets that vote by the event's OWN timestamp (voxel grids,
// surfaces) every sampled event brings it beside the word (feed: with_time), and a set that reads polarity (a signed voxel set, a
// by-polarity surface set) reads it as pol_add* does -- bit 31 of the word on the host paths, the store's byte array -- while any
// other set reads none and packs none.
static int recon_set_add_source(cmx_ctx *c, const EventSource &src, ReconTargetSet ReconState::*which) {
  ReconState *r = c->recon;
  const ReconTargetSet &t = r->*which;
  int rc = feed_checks(c, src);
  if (rc) return rc;
  ReconSetArgs g{};
  g.ev = recon_args(c, r);
  g.ev.plane = nullptr; g.ev.fixed = nullptr; g.ev.n_inside = nullptr;
  g.entries = t.d_entries; g.ranges = t.d_ranges;
  g.n = t.n; g.Wv = t.W; g.Hv = t.H;
  g.n_voted = t.d_voted;
  ReconArgs &a = g.ev;
  const bool with_time = &t != &r->views;
  BatchPlan p;
  return feed(c, r, src, false, t.polarity && !src.on_device(), with_time, &p, [&](const FedSlice &s) {
    a.xy = s.d_xy; a.stride = src.on_device() ? r->rate : 0;
    a.pol = t.polarity && src.on_device() ? src.d_pol + s.ev_first : nullptr;
    a.batch_t = s.d_bt; a.nb = s.b_hi - s.b_lo;
    a.n = (int)s.n;
    g.ev_t = with_time ? s.d_t : nullptr;
    if (&t == &r->views) launch_recon_view_votes(ReconViewArgs{g, t.d_planes, t.d_fixed}, c->stream);
    else if (&t == &r->voxels) launch_recon_voxel_votes(ReconVoxelArgs{g, t.d_planes, t.d_fixed, t.per, t.polarity ? 1 : 0}, c->stream);
    else launch_recon_surface_votes(ReconSurfaceArgs{g, t.d_cells, t.polarity ? 1 : 0}, c->stream);
    return (int)CMX_OK;
  });
}
// the front door of the nine entry points: the set, the call's own way to its source -- told whether the set reads polarity, and
// so whether the source must bring it -- then the pass
template <typename MakeSource>
static int recon_set_add_entry(cmx_ctx *c, ReconTargetSet ReconState::*which, MakeSource make) {
  int rc = recon_set_enter(c, which);
  if (rc) return rc;
  EventSource src;
  rc = make(&src, (c->recon->*which).polarity);
  if (rc) return rc;
  return recon_set_add_source(c, src, which);
}
// the three forms of a source and the polarity that comes with each; kind / why: a set that reads polarity, as the message about a
// source without it puts it ("signed voxel", "voxel set is signed")
static int recon_set_add(cmx_ctx *c, ReconTargetSet ReconState::*which, const char *kind, int64_t n, const uint16_t *x, const uint16_t *y,
                         const int64_t *t_ns, const uint8_t *pol) {
  return recon_set_add_entry(c, which, [&](EventSource *src, bool reads_pol) {
    if (reads_pol && !pol) return fail(c, CMX_ERR_INVALID_ARG, "null polarity array for a %s set", kind);
    *src = EventSource::arrays(n, x, y, t_ns);
    src->soa.p = pol;
    return (int)CMX_OK;
  });
}
static int recon_set_add_aos(cmx_ctx *c, ReconTargetSet ReconState::*which, int64_t n, const void *events, const cmx_aos_layout *layout,
                             size_t off_polarity) {
  return recon_set_add_entry(c, which, [&](EventSource *src, bool reads_pol) {
    const int rc = make_aos(c, n, events, layout, src);
    if (rc) return rc;
    if (!reads_pol) return (int)CMX_OK;  // (polarity is neither needed nor read)
    if (off_polarity >= layout->stride) return fail(c, CMX_ERR_INVALID_ARG, "record layout: polarity outside the %zu-byte record", layout->stride);
    src->aos.op = off_polarity;
    return (int)CMX_OK;
  });
}
static int recon_set_add_from(cmx_ctx *c, ReconTargetSet ReconState::*which, const char *why, const cmx_events *e, int64_t first, int64_t count) {
  return recon_set_add_entry(c, which, [&](EventSource *src, bool reads_pol) {
    const int rc = store_source(c, e, first, count, src);
    if (rc) return rc;
    if (reads_pol && e->size > 0 && !e->has_pol)
      return fail(c, CMX_ERR_STATE, "the %s and the event store holds no polarity (cmx_events_push_pol)", why);
    return (int)CMX_OK;
  });
}
int cmx_backend_recon_view_add(cmx_ctx *c, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns) {
  return recon_set_add(c, &ReconState::views, "", n, x, y, t_ns, nullptr);
}
int cmx_backend_recon_view_add_aos(cmx_ctx *c, int64_t n, const void *events, const cmx_aos_layout *layout) {
  return recon_set_add_aos(c, &ReconState::views, n, events, layout, 0);
}
int cmx_backend_recon_view_add_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count) {
  return recon_set_add_from(c, &ReconState::views, "", e, first, count);
}
int cmx_backend_recon_voxel_add(cmx_ctx *c, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns, const uint8_t *pol) {
  return recon_set_add(c, &ReconState::voxels, "signed voxel", n, x, y, t_ns, pol);
}
int cmx_backend_recon_voxel_add_aos(cmx_ctx *c, int64_t n, const void *events, const cmx_aos_layout *layout, size_t off_polarity) {
  return recon_set_add_aos(c, &ReconState::voxels, n, events, layout, off_polarity);
}
int cmx_backend_recon_voxel_add_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count) {
  return recon_set_add_from(c, &ReconState::voxels, "voxel set is signed", e, first, count);
}
int cmx_backend_recon_surface_add(cmx_ctx *c, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns, const uint8_t *pol) {
  return recon_set_add(c, &ReconState::surfaces, "by-polarity surface", n, x, y, t_ns, pol);
}
int cmx_backend_recon_surface_add_aos(cmx_ctx *c, int64_t n, const void *events, const cmx_aos_layout *layout, size_t off_polarity) {
  return recon_set_add_aos(c, &ReconState::surfaces, n, events, layout, off_polarity);
}
int cmx_backend_recon_surface_add_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count) {
  return recon_set_add_from(c, &ReconState::surfaces, "surface set is by polarity", e, first, count);
}

// ---- warp*: ALL events of a slice reach the kernel (the host paths pack at rate 1, the store is read in place), the true rate only
// decides the SAMPLED bit.  Nothing of the reconstruction but the knots is read and nothing of it is written: no recon_pass_enter,
// no counter, no plane.  The output staging (host output) is the export's own.
static int warp_slot_ensure(cmx_ctx *c, ReconState *r, ReconWarpSlot &s, size_t n) {
  if (!r->down_stream) HIP_TRY(c, hipStreamCreateWithFlags(&r->down_stream, hipStreamNonBlocking));
  if (!s.kdone) HIP_TRY(c, hipEventCreateWithFlags(&s.kdone, hipEventDisableTiming));
  if (!s.down) HIP_TRY(c, hipEventCreateWithFlags(&s.down, hipEventDisableTiming));
  int rc = ensure_pinned(c, s.h_xy, s.h_xy_cap, 2 * n);
  if (!rc) rc = ensure_pinned(c, s.h_fl, s.h_fl_cap, n);
  if (!rc) rc = ensure(c, s.d_xy, s.d_xy_cap, 2 * n);
  if (!rc) rc = ensure(c, s.d_fl, s.d_fl_cap, n);
  return rc;
}

// The walk of warp* and score*: one kernel per slice (launch(slice, d_out, d_flags): the sink's own), `elem` bytes of output per event
// and one flag byte.  dev_out: straight into the caller's device pointers.  Host output: slice k into the staging of wslot[k & 1],
// a copy on the download stream into its pinned twin, and from there into the caller's arrays by the host pool while slice k + 1 runs.
template <typename Launch>
static int recon_export_walk(cmx_ctx *c, const EventSource &src, size_t elem, void *out, unsigned char *flags_out, bool dev_out, Launch launch) {
  ReconState *r = c->recon;
  struct Pending { ReconWarpSlot *o = nullptr; int64_t first = 0, count = 0; } pend;
  auto finish = [&](Pending &q) -> int {  // the download of a slice is complete: into the caller's arrays
    if (!q.o) return CMX_OK;
    HIP_TRY(c, hipEventSynchronize(q.o->down));
    const char *hx = reinterpret_cast<const char *>(q.o->h_xy);
    const unsigned char *hf = q.o->h_fl;
    char *ox = static_cast<char *>(out) + (size_t)q.first * elem;
    unsigned char *of = flags_out ? flags_out + q.first : nullptr;
    parallel_ranges(q.count, [=](int64_t a0, int64_t a1) {
      memcpy(ox + (size_t)a0 * elem, hx + (size_t)a0 * elem, (size_t)(a1 - a0) * elem);
      if (of) memcpy(of + a0, hf + a0, (size_t)(a1 - a0));
    });
    q.o = nullptr;
    return CMX_OK;
  };
  BatchPlan p;
  int rc = feed(c, r, src, true, false, false, &p, [&](const FedSlice &s) -> int {
    ReconWarpSlot *o = nullptr;
    void *d_out = static_cast<char *>(out) + (size_t)s.ev_first * elem;
    unsigned char *d_fl = flags_out ? flags_out + s.ev_first : nullptr;
    if (!dev_out) {
      o = &r->wslot[s.k & 1];  // (free: the slice before the last was finished while the last one ran)
      const int rc2 = warp_slot_ensure(c, r, *o, (size_t)s.ev_n);
      if (rc2) return rc2;
      d_out = o->d_xy;
      d_fl = flags_out ? o->d_fl : nullptr;
    }
    launch(s, d_out, d_fl);
    if (!o) return CMX_OK;
    HIP_TRY(c, hipEventRecord(o->kdone, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(r->down_stream, o->kdone, 0));
    HIP_TRY(c, hipMemcpyAsync(o->h_xy, o->d_xy, (size_t)s.ev_n * elem, hipMemcpyDeviceToHost, r->down_stream));
    if (flags_out) HIP_TRY(c, hipMemcpyAsync(o->h_fl, o->d_fl, (size_t)s.ev_n, hipMemcpyDeviceToHost, r->down_stream));
    HIP_TRY(c, hipEventRecord(o->down, r->down_stream));
    const int rc2 = finish(pend);  // the slice before this one, while this one runs
    if (rc2) return rc2;
    pend.o = o; pend.first = s.ev_first; pend.count = s.ev_n;
    return CMX_OK;
  });
  if (!rc) rc = finish(pend);
  if (rc && r->down_stream) (void)hipStreamSynchronize(r->down_stream);
  return rc;
}
// what both sinks' kernels read of a slice: ALL its raw events, one run of recon_run(B) of them per workgroup
static ReconWarpArgs warp_args(const cmx_ctx *c, const ReconState *r) {
  ReconWarpArgs g{};
  g.ev = recon_args(c, r);
  g.ev.per_batch = r->B; g.ev.stride = 0;
  g.ev.run = recon_run(r->B);
  g.rate = r->rate;
  return g;
}
static void warp_slice(ReconWarpArgs &g, const FedSlice &s, unsigned char *d_flags) {
  g.ev.xy = s.d_xy;
  g.ev.batch_t = s.d_bt; g.ev.nb = s.b_hi - s.b_lo;
  g.ev.n = (int)s.ev_n;
  g.lone = s.lone ? 1 : 0;
  g.lone_t = s.lone_t;
  g.flags_out = d_flags;
}

static int recon_warp_source(cmx_ctx *c, const EventSource &src, int format, void *xy_out, unsigned char *flags_out, bool dev_out) {
  ReconState *r = c->recon;
  int rc = feed_checks(c, src);
  if (rc) return rc;
  if (src.n > 0 && !xy_out) return fail(c, CMX_ERR_INVALID_ARG, "null coordinate output");
  const bool f32 = format == CMX_WARP_F32;
  ReconWarpArgs g = warp_args(c, r);
  g.f32 = f32 ? 1 : 0;
  return recon_export_walk(c, src, f32 ? 2 * sizeof(float) : 2 * sizeof(double), xy_out, flags_out, dev_out,
                           [&](const FedSlice &s, void *d_out, unsigned char *d_flags) {
                             warp_slice(g, s, d_flags);
                             g.xy_out = d_out;
                             g.vec = (uintptr_t)g.xy_out % (f32 ? 8 : 16) == 0 ? 1 : 0;
                             launch_recon_warp(g, c->stream);
                           });
}

template <typename MakeSource>
static int recon_warp_entry(cmx_ctx *c, int format, void *xy_out, unsigned char *flags_out, bool dev_out, MakeSource make) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  if (format != CMX_WARP_F64 && format != CMX_WARP_F32) return fail(c, CMX_ERR_INVALID_ARG, "unknown output format %d", format);
  EventSource src;
  rc = make(&src);
  if (rc) return rc;
  return recon_warp_source(c, src, format, xy_out, flags_out, dev_out);
}
int cmx_backend_recon_warp(cmx_ctx *c, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns, int format, void *xy_out,
                           unsigned char *flags_out) {
  return recon_warp_entry(c, format, xy_out, flags_out, false,
                          [&](EventSource *src) { *src = EventSource::arrays(n, x, y, t_ns); return (int)CMX_OK; });
}
int cmx_backend_recon_warp_aos(cmx_ctx *c, int64_t n, const void *events, const cmx_aos_layout *layout, int format, void *xy_out,
                               unsigned char *flags_out) {
  return recon_warp_entry(c, format, xy_out, flags_out, false, [&](EventSource *src) { return make_aos(c, n, events, layout, src); });
}
int cmx_backend_recon_warp_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count, int format, void *xy_out,
                                unsigned char *flags_out) {
  return recon_warp_entry(c, format, xy_out, flags_out, false, [&](EventSource *src) { return store_source(c, e, first, count, src); });
}
int cmx_backend_recon_warp_from_device(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count, int format, void *d_xy_out,
                                       unsigned char *d_flags_out) {
  return recon_warp_entry(c, format, d_xy_out, d_flags_out, true, [&](EventSource *src) { return store_source(c, e, first, count, src); });
}

// ---- score*: the export's walk with the support plane of the open score pass read at every event's vote cell -- one float per
// event, the export's flag byte.  Read-only on everything but the output staging: no recon_pass_enter, no counter, no plane.
static int recon_score_source(cmx_ctx *c, const EventSource &src, int loo, float *score_out, unsigned char *flags_out, bool dev_out) {
  ReconState *r = c->recon;
  int rc = feed_checks(c, src);
  if (rc) return rc;
  if (src.n > 0 && !score_out) return fail(c, CMX_ERR_INVALID_ARG, "null score output");
  ReconScoreArgs g{};
  g.w = warp_args(c, r);
  g.S = r->score_radius > 0 ? r->d_support : r->d_plane;
  g.loo = loo ? 1 : 0;
  g.r = r->score_radius;
  memcpy(g.taps, r->score_taps, sizeof(g.taps));
  return recon_export_walk(c, src, sizeof(float), score_out, flags_out, dev_out, [&](const FedSlice &s, void *d_out, unsigned char *d_flags) {
    warp_slice(g.w, s, d_flags);
    g.score_out = static_cast<float *>(d_out);
    launch_recon_score(g, c->stream);
  });
}
template <typename MakeSource>
static int recon_score_entry(cmx_ctx *c, int loo, float *score_out, unsigned char *flags_out, bool dev_out, MakeSource make) {
  int rc = recon_score_enter(c);
  if (rc) return rc;
  EventSource src;
  rc = make(&src);
  if (rc) return rc;
  return recon_score_source(c, src, loo, score_out, flags_out, dev_out);
}
int cmx_backend_recon_score(cmx_ctx *c, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns, int loo, float *score_out,
                            unsigned char *flags_out) {
  return recon_score_entry(c, loo, score_out, flags_out, false,
                           [&](EventSource *src) { *src = EventSource::arrays(n, x, y, t_ns); return (int)CMX_OK; });
}
int cmx_backend_recon_score_aos(cmx_ctx *c, int64_t n, const void *events, const cmx_aos_layout *layout, int loo, float *score_out,
                                unsigned char *flags_out) {
  return recon_score_entry(c, loo, score_out, flags_out, false, [&](EventSource *src) { return make_aos(c, n, events, layout, src); });
}
int cmx_backend_recon_score_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count, int loo, float *score_out,
                                 unsigned char *flags_out) {
  return recon_score_entry(c, loo, score_out, flags_out, false, [&](EventSource *src) { return store_source(c, e, first, count, src); });
}
int cmx_backend_recon_score_from_device(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count, int loo, float *d_score_out,
                                        unsigned char *d_flags_out) {
  return recon_score_entry(c, loo, d_score_out, d_flags_out, true, [&](EventSource *src) { return store_source(c, e, first, count, src); });
}

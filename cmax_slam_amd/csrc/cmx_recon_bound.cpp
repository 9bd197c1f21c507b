// cmx_recon_bound.cpp -- cmx_backend_recon_* for an optimiser that evaluates the SAME events many times: events bound once
// (recon_bind_from), evaluated through a batch-pose table, a tile sort of the reconstruction's own and LDS votes (recon_eval_bound;
// DESIGN 4.13).  For the online case -- a settled head, a free tail: the batches under fixed knots voted once into a base plane
// (recon_freeze_head), and the evaluation side of the native bundle adjustment (recon_solve_*, driven by cmx_solver.cpp's FR-CG
// machine).  And for a recording that grows: events appended to the binding (recon_bind_append_from), the freeze line
// moved forward (recon_advance_head) and the settled events' memory given back (recon_release_head) -- book-keeping around the same
// kernels over sub-ranges.
// Kernels: cmx_recon.hip.
#include <limits>

#include "cmx_recon_state.hpp"

// ---- bound events: hand the events over ONCE, evaluate them many times (an optimiser's trial points) with the votes made through LDS
// bind_from   validation of recon_add_from, then the sampled events of the range, packed in time order, and their batch times into
//             memory of the reconstruction's own, with a TileSort reserved for them; everything is built beside an earlier binding,
//             which is replaced only once nothing can fail any more
// eval_bound  restart + eval_from over the bound events: batch-pose table behind recon_delta, tile sort at the first evaluation and
//             again after one whose votes left their windows (kRebinFallbackFrac), recon_votes_lds, the image pass, and the gather
//             pass over the time-ordered copy in the slices of every add (slice_at)
constexpr int64_t kMaxBoundSampled = 1LL << 30;  // (sorted positions, chunk bounds and keys are 32-bit)

// the open tail of a binding for its next append: the last n raw events, as a store replica or the append's scratch holds them, into
// buffers of the binding's own (queued; large enough, or new ones -- the caller has made sure nothing queued reads the old ones)
static int tail_keep(cmx_ctx *c, ReconBound *b, const uint32_t *d_xy, const int64_t *d_t, int64_t n) {
  if ((size_t)n > b->tail_cap) {
    const int rc = ensure_pair(c, b->d_tail_xy, b->d_tail_t, b->tail_cap, (size_t)n);
    if (rc) return rc;
  }
  if (n > 0) {
    HIP_TRY(c, hipMemcpyAsync(b->d_tail_xy, d_xy, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(b->d_tail_t, d_t, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, c->stream));
  }
  b->tail_n = n;
  return CMX_OK;
}

static int bound_build(cmx_ctx *c, ReconState *r, const EventSource &src, const BatchPlan &p, ReconBound *b) {
  b->n_events = src.n;
  b->plan = p;
  HIP_TRY(c, hipHostMalloc((void **)&b->h_stat, 2 * sizeof(unsigned long long), hipHostMallocDefault));
  b->h_stat[0] = b->h_stat[1] = 0ull;
  const int64_t tail_from = open_tail_from(src.n, p);
  if (src.n > 0) b->t_last = (long long)src.soa.t[src.n - 1];
  if (p.nb == 0) {  // (0 or 1 events: nothing to vote)
    const int rc0 = tail_keep(c, b, src.d_xy, src.d_t, src.n);
    if (rc0) return rc0;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CMX_OK;
  }
  HIP_TRY(c, hipMalloc((void **)&b->d_bt, (size_t)p.nb * sizeof(long long)));
  b->bt_cap = (size_t)p.nb;
  int rc = validate_store_times(c, r, src.d_t, src.n, p, p.nb, b->d_bt);  // (all batches at once: the table is the binding's)
  if (rc) return rc;
  // ---- valid: the copy, the pose table, and the sort's buffers with the chunk table at the back end's chunk size
  const size_t n = (size_t)p.n_packed;
  const int ntiles = 2 * recon_sort_tiles(c);  // (the back end's sort keys carry the old / new bit: no bound event sets it, half of the bins stay empty)
  HIP_TRY(c, hipMalloc((void **)&b->d_xy, n * sizeof(uint32_t)));
  b->xy_cap = n;
  HIP_TRY(c, hipMalloc((void **)&b->d_poseR, (size_t)p.nb * sizeof(PoseR)));
  rc = tail_keep(c, b, src.d_xy + tail_from, src.d_t + tail_from, src.n - tail_from);
  if (rc) return rc;
  const ChunkPlan cp = plan_chunks(p.n_packed, ntiles, kBackEndChunkDiv);
  b->chunk_events = cp.chunk_events;
  b->max_chunks = (int)cp.max_chunks;  // (n <= 2^30, at most 2^20 tiles: below 2^23)
  rc = b->ts.reserve(c, p.n_packed, ntiles, cp.max_chunks);
  if (rc) return rc;
  // (t_next = the smallest time: no event carries the old flag)
  launch_be_pack_from_store(src.d_xy, reinterpret_cast<const long long *>(src.d_t), (long long)src.n, r->B, r->rate, p.per_batch, (int)n,
                            std::numeric_limits<long long>::min(), b->d_xy, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the store may be pushed to, compacted or closed from here on
  return CMX_OK;
}

int cmx_backend_recon_bind_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  EventSource src;
  rc = store_source(c, e, first, count, &src);
  if (rc) return rc;
  ReconState *r = c->recon;
  (void)recon_pass_enter(c, r, false);  // as every add: an open gradient pass is closed
  if (src.n < 0 || src.n > kMaxEvents) return fail(c, CMX_ERR_INVALID_ARG, "bad event count %lld", (long long)src.n);
  BatchPlan p;
  int slice_batches = 1;
  rc = recon_plan(c, r, src.n, &p, &slice_batches);
  if (rc) return rc;
  if (p.n_packed > kMaxBoundSampled)
    return fail(c, CMX_ERR_INVALID_ARG, "%lld sampled events above the limit of a binding (2^30)", (long long)p.n_packed);
  ReconBound b;
  rc = bound_build(c, r, src, p, &b);
  if (rc) {  // (an earlier binding is intact: nothing of it was touched)
    (void)hipStreamSynchronize(c->stream);
    b.release();
    return rc;
  }
  frozen_drop(c, r);  // (a frozen head is a property of the binding it was cut from)
  r->bnd.release();
  r->bnd = b;
  r->bound = true;
  return CMX_OK;
}

int cmx_backend_recon_unbind(cmx_ctx *c) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return CMX_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  frozen_drop(c, r);
  r->bnd.release();
  r->bound = false;
  return CMX_OK;
}

int cmx_backend_recon_bound_info(cmx_ctx *c, int64_t *n_events, int64_t *n_sampled, int64_t *sorts, double *fallback_frac) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  const ReconState *r = c->recon;  // (without a binding: all zero)
  if (n_events) *n_events = r->bound ? r->bnd.n_events : 0;
  if (n_sampled) *n_sampled = r->bound ? r->bnd.plan.n_packed : 0;
  if (sorts) *sorts = r->bound ? r->bnd.sorts : 0;
  if (fallback_frac) *fallback_frac = r->bound ? r->bnd.fallback_frac : 0.0;
  return CMX_OK;
}

// the bound events by the destination tile of their vote under the pose table as it stands, and the chunk table
// (be.xy / be.n / be.poseR: all bound events, or with a frozen head the active ones and the pose table from their first batch on --
//  the sort numbers batches from the first event it is given)
static int bound_sort(cmx_ctx *c, ReconBound &b, const BeSplatArgs &be, int chunk_events) {
  TileSortJob job;
  job.be = &be;
  job.tiles_x = (c->Wp + kBinTile - 1) / kBinTile;
  job.tiles = recon_sort_tiles(c);
  job.planes_per_tile = 2;
  job.xy = be.xy; job.per_batch = b.plan.per_batch; job.n = be.n;
  job.chunk_events = chunk_events;
  const int rc = b.ts.run(c, job);
  if (rc) return rc;
  b.sorted = true;
  b.sorts++;
  return CMX_OK;
}

// One vote pass over the batches [b_lo, b_hi) of the binding at the knots the reconstruction holds: their pose table; with `sort`
// THOSE events into the binding's TileSort, in chunks of cp.chunk_events (the sort numbers batches from the first event it is
// given); the fallback word cleared; LDS votes ON TOP of what `plane` / `fixed` (deterministic mode) and the counter hold, the launch
// sized by cp.max_chunks.  Where the events lie in the resident arrays is xy_at's business.  Queued; spans: timed as an evaluation's.
static int bound_vote(cmx_ctx *c, ReconState *r, int b_lo, int b_hi, float *plane, unsigned long long *fixed, unsigned long long *n_inside,
                      const ChunkPlan &cp, bool sort, bool spans) {
  ReconBound &b = r->bnd;
  ReconArgs a = recon_args(c, r);
  a.batch_t = b.bt_at(b_lo); a.nb = b_hi - b_lo;
  {
    Span sp(c, CMX_T_POSE, /*exact=*/true, spans);
    launch_recon_pose_table(a, b.pose_at(b_lo), c->stream, sp.t0(), sp.t1());
  }
  ReconLdsArgs g{};
  g.cam = a.cam;
  g.cam.poseR = b.pose_at(b_lo);
  g.cam.xy = b.xy_at(b.plan.packed(0, b_lo));
  g.cam.per_batch = b.plan.per_batch;
  g.cam.n = (int)b.plan.packed(b_lo, b_hi);
  g.cam.order = r->sup.order;
  if (sort) {
    Span sp(c, CMX_T_BATCH, /*exact=*/false, spans);
    const int rc = bound_sort(c, b, g.cam, cp.chunk_events);
    if (rc) return rc;
  }
  g.ev.sxy = b.ts.d_sxy; g.ev.sbatch = b.ts.d_sbatch;
  g.ev.chunks = b.ts.d_chunks; g.ev.nchunks = (int)cp.max_chunks; g.ev.nchunks_dev = b.ts.d_nchunks;
  g.ev.fallback = b.ts.d_fallback;
  g.ev.fixed = fixed;
  g.plane = plane;
  g.n_inside = n_inside;
  HIP_TRY(c, hipMemsetAsync(b.ts.d_fallback, 0, sizeof(unsigned), c->stream));
  {
    Span sp(c, CMX_T_SPLAT, /*exact=*/true, spans);
    launch_recon_votes_lds(g, c->stream, sp.t0(), sp.t1());
  }
  HIP_TRY(c, hipGetLastError());
  return CMX_OK;
}

// the gradient pass over the bound time-ordered copy: the slices, runs and launches of recon_grad_add_from, with stride 0
// From batch b_first on (0, or a frozen head's first active batch: the slices then start there, so with b_first = 0 they are
// the unbound pass's).  wait = false: queued only, the caller waits.
static int bound_gather(cmx_ctx *c, ReconState *r, int b_first, bool wait) {
  if (int rc0 = recon_pass_enter(c, r, true)) return rc0;
  const ReconBound &b = r->bnd;
  const BatchPlan &p = b.plan;
  const int slice_batches = recon_slice_batches(r);
  ReconGatherArgs ga = recon_gather_args(c, r);
  ReconArgs &a = ga.ev;
  for (int b_lo = b_first; b_lo < p.nb; b_lo += slice_batches) {
    const Slice sl = slice_at(p, b.n_events, b_lo, slice_batches);
    a.xy = b.xy_at(sl.first); a.stride = 0;  // (resident addresses: b_first is never in front of what release_head gave back)
    a.batch_t = b.bt_at(b_lo); a.nb = sl.b_hi - b_lo;
    a.n = (int)sl.n;
    Span sp(c, CMX_T_GATHER);
    const int rc = queue_gather(c, r, ga);
    if (rc) return rc;
  }
  HIP_TRY(c, hipGetLastError());
  if (wait) HIP_TRY(c, recon_wait(c, r));
  r->g_sampled += p.packed(b_first, p.nb);
  return CMX_OK;
}

// One evaluation of the binding: cmx_backend_recon_eval_bound's body, and -- with sv set -- a trial point of
// cmx_backend_recon_solve: the same launches in the same order, but the knots come from pinned staging, nothing waits in between,
// the free gradient entries are formed on the device (recon_grad_finalize) and ONE wait at the end delivers contrast, mean, both
// counters and that slice.  With a frozen head the plane starts from the base and every pass walks the active batches alone.
static int bound_eval(cmx_ctx *c, ReconState *r, const double *knots_xyzw, double blur_sigma, int contrast_measure, double *contrast,
                      double *grad, ReconSolve *sv) {
  ReconBound &b = r->bnd;
  const ReconFrozen &fz = r->frozen;
  const bool frozen = fz.num_fixed > 0;
  if (frozen && knots_xyzw && memcmp(knots_xyzw, fz.knots.data(), (size_t)fz.num_fixed * sizeof(Quat)) != 0)
    return fail(c, CMX_ERR_INVALID_ARG, "the first %d knots differ from those the head was frozen at (cmx_backend_recon_freeze_head)",
                fz.num_fixed);
  int rc = recon_start_over(c, r, knots_xyzw, /*from_base=*/true, /*staged=*/sv != nullptr);
  if (rc) return rc;
  const int b0 = frozen ? fz.b_act : 0;
  const int64_t n_act = b.plan.packed(b0, b.plan.nb);
  if (n_act > 0) {  // (sorted at the first evaluation, and again after one whose votes left their windows)
    const ChunkPlan cp{frozen ? fz.chunk_events : b.chunk_events, frozen ? fz.max_chunks : b.max_chunks};
    rc = bound_vote(c, r, b0, b.plan.nb, r->d_plane, r->deterministic ? r->d_fixed : nullptr, r->d_inside, cp,
                    /*sort=*/!b.sorted || b.fallback_frac > kRebinFallbackFrac, /*spans=*/true);
    if (rc) return rc;
    // (into pinned memory of the binding's own; complete once the image pass below has waited for the stream)
    b.h_stat[1] = 0ull;
    HIP_TRY(c, hipMemcpyAsync(&b.h_stat[0], r->d_inside, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&b.h_stat[1], b.ts.d_fallback, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    r->n_sampled += n_act;
  }
  // the share of the ACTIVE events' votes that left their windows: the frozen head's votes are in the counter, not in the sort
  auto note_fallback = [&]() {
    if (n_act <= 0) { if (frozen) b.fallback_frac = 0.0; return; }
    const unsigned long long act = b.h_stat[0] - (frozen ? fz.inside : 0ull);
    b.fallback_frac = act ? (double)(unsigned)b.h_stat[1] / (double)act : 0.0;
  };
  // a frozen evaluation's gradient pass: both of its counts start from the frozen head's, so that grad_get's test -- sampled and
  // voted counts against the plane's -- holds for base plus active, and the fixed entries are zero by definition
  auto open_frozen_pass = [&]() -> int {
    if (!frozen) return CMX_OK;
    r->g_sampled = fz.sampled;
    r->g_num_fixed = fz.num_fixed;
    HIP_TRY(c, hipMemcpyAsync(r->d_voted, fz.d_inside, sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
    return CMX_OK;
  };
  if (!sv) {
    rc = cmx_backend_recon_contrast(c, blur_sigma, contrast_measure, grad != nullptr, contrast);
    if (rc && hipStreamSynchronize(c->stream) != hipSuccess) return rc;  // (the two words below are not known to have arrived)
    note_fallback();
    if (!rc && grad) rc = open_frozen_pass();
    if (!rc && grad) rc = bound_gather(c, r, b0, /*wait=*/true);
    if (!rc && grad) rc = cmx_backend_recon_grad_get(c, grad);
    return rc;
  }
  rc = recon_contrast_queue(c, r, blur_sigma, contrast_measure, grad != nullptr, sv->h_cm);
  const size_t P = 3 * (size_t)r->sup.K, p0 = 3 * (size_t)sv->num_fixed;
  if (!rc && grad) rc = open_frozen_pass();
  if (!rc && grad) rc = bound_gather(c, r, b0, /*wait=*/false);
  if (!rc && grad) {
    launch_recon_grad_finalize(r->d_gsum, r->d_cm, (long long)P, (long long)p0, (double)c->Wp * (double)c->Hp,
                               contrast_measure == CMX_MEAN_SQUARE, sv->d_grad, c->stream);
    rc = hipGetLastError() == hipSuccess ? CMX_OK : fail(c, CMX_ERR_HIP, "the gradient finalize could not be queued");
    if (!rc) {
      HIP_TRY(c, hipMemcpyAsync(&sv->h_cnt[0], r->d_inside, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(&sv->h_cnt[1], r->d_voted, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    }
  }
  const hipError_t waited = recon_wait(c, r);  // the evaluation's one wait (a queueing error above: so that nothing is left in flight)
  if (!rc && waited != hipSuccess) rc = fail(c, CMX_ERR_HIP, "the evaluation failed: %s", hipGetErrorString(waited));
  if (rc) return rc;
  note_fallback();
  *contrast = sv->h_cm[0];
  if (grad) {
    r->mu = sv->h_cm[1];
    if (r->g_sampled != r->n_sampled || sv->h_cnt[0] != sv->h_cnt[1])  // (grad_get's test)
      return fail(c, CMX_ERR_STATE, "the gradient pass saw %lld sampled / %llu voting events, the plane holds %lld / %llu",
                  (long long)r->g_sampled, sv->h_cnt[1], (long long)r->n_sampled, sv->h_cnt[0]);
    memcpy(grad, sv->h_grad, (P - p0) * sizeof(double));
  }
  return CMX_OK;
}

int cmx_backend_recon_eval_bound(cmx_ctx *c, const double *knots_xyzw, double blur_sigma, int contrast_measure, double *contrast,
                                 double *grad) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return fail(c, CMX_ERR_STATE, "no events are bound (cmx_backend_recon_bind_from)");
  if (!contrast) return fail(c, CMX_ERR_INVALID_ARG, "null output");
  if (grad) {  // (before anything is changed, as in eval_from)
    rc = recon_grad_precheck(c, r, blur_sigma);
    if (rc) return rc;
  }
  return bound_eval(c, r, knots_xyzw, blur_sigma, contrast_measure, contrast, grad, nullptr);
}

// ---- frozen head
// eval_bound's own vote pass over the batches [b_lo, b_hi) of the binding, at the knots the reconstruction holds, into a base plane
// and its counter ON TOP of what they hold: pose table, the binding's TileSort filled with THOSE events (the next evaluation sorts
// the active ones into it, as it would anyway), LDS votes.  freeze_head: [0, b_act) into a cleared base; advance_head: the batches
// the moved line newly names.  Queued; the caller waits.
static int frozen_vote(cmx_ctx *c, ReconState *r, void *d_base, unsigned long long *d_inside, int b_lo, int b_hi) {
  ReconBound &b = r->bnd;
  const int64_t n = b.plan.packed(b_lo, b_hi);
  if (n <= 0) return CMX_OK;
  const int keys = 2 * recon_sort_tiles(c);
  const ChunkPlan cp = plan_chunks(n, keys, kBackEndChunkDiv);  // the chunk rule at the sub-range's count
  int rc = b.ts.reserve(c, n, keys, cp.max_chunks);
  if (!rc) rc = bound_vote(c, r, b_lo, b_hi, r->deterministic ? nullptr : static_cast<float *>(d_base),
                           r->deterministic ? static_cast<unsigned long long *>(d_base) : nullptr, d_inside, cp, /*sort=*/true, /*spans=*/false);
  b.sorted = false;
  return rc;
}
// the active part's chunk table: the chunk rule at ITS count (the table may be longer than the one the bind reserved)
static int frozen_plan_active(cmx_ctx *c, ReconState *r, ReconFrozen *fz) {
  const int64_t n_act = r->bnd.plan.n_packed - fz->sampled;
  if (n_act <= 0) return CMX_OK;
  const int tiles = recon_sort_tiles(c);
  const ChunkPlan cp = plan_chunks(n_act, 2 * tiles, kBackEndChunkDiv);
  fz->chunk_events = cp.chunk_events;
  fz->max_chunks = (int)cp.max_chunks;
  return r->bnd.ts.reserve(c, n_act, 2 * tiles, cp.max_chunks);
}

int cmx_backend_recon_freeze_head(cmx_ctx *c, int num_fixed) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return fail(c, CMX_ERR_STATE, "no events are bound (cmx_backend_recon_bind_from)");
  if (num_fixed < 0 || num_fixed >= r->sup.K) return fail(c, CMX_ERR_INVALID_ARG, "num_fixed=%d outside [0, %d)", num_fixed, r->sup.K);
  rc = recon_refuse_released(c, r, "freeze_head");
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  (void)recon_pass_enter(c, r, false);  // as a bind: an open gradient pass is closed
  frozen_drop(c, r);
  if (num_fixed == 0) return CMX_OK;
  ReconBound &b = r->bnd;
  const BatchPlan &p = b.plan;
  ReconFrozen fz;
  auto build = [&]() -> int {
    // the prefix rule on the host, over the binding's batch times read back once
    std::vector<long long> bt((size_t)p.nb);
    if (p.nb > 0) HIP_TRY(c, hipMemcpy(bt.data(), b.d_bt, (size_t)p.nb * sizeof(long long), hipMemcpyDeviceToHost));
    fz.b_act = frozen_prefix(r->sup, num_fixed, bt.data(), p.nb);
    fz.sampled = p.packed(0, fz.b_act);
    fz.knots.resize(4 * (size_t)num_fixed);
    HIP_TRY(c, hipMemcpy(fz.knots.data(), r->d_knots, (size_t)num_fixed * sizeof(Quat), hipMemcpyDeviceToHost));
    // the base: the frozen batches' votes at the current knots
    const size_t np = (size_t)c->Wp * c->Hp, cell = r->deterministic ? sizeof(unsigned long long) : sizeof(float);
    HIP_TRY(c, hipMalloc(&fz.d_base, np * cell));
    HIP_TRY(c, hipMalloc((void **)&fz.d_inside, sizeof(unsigned long long)));
    HIP_TRY(c, hipMemsetAsync(fz.d_base, 0, np * cell, c->stream));
    HIP_TRY(c, hipMemsetAsync(fz.d_inside, 0, sizeof(unsigned long long), c->stream));
    int rc2 = frozen_vote(c, r, fz.d_base, fz.d_inside, 0, fz.b_act);
    if (rc2) return rc2;
    HIP_TRY(c, hipMemcpyAsync(&fz.inside, fz.d_inside, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rc2 = frozen_plan_active(c, r, &fz);
    if (rc2) return rc2;
    fz.num_fixed = num_fixed;
    return CMX_OK;
  };
  rc = build();
  if (rc) {
    (void)hipStreamSynchronize(c->stream);
    fz.release();
    return rc;
  }
  r->frozen = fz;
  r->bnd.sorted = false;  // (the sort holds the active events alone from the next evaluation on)
  return CMX_OK;
}

int cmx_backend_recon_frozen_info(cmx_ctx *c, int *num_fixed, int64_t *frozen_batches, int64_t *frozen_sampled) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  const ReconFrozen &fz = c->recon->frozen;  // (without a frozen head: all zero)
  if (num_fixed) *num_fixed = fz.num_fixed;
  if (frozen_batches) *frozen_batches = fz.num_fixed ? fz.b_act : 0;
  if (frozen_sampled) *frozen_sampled = fz.num_fixed ? fz.sampled : 0;
  return CMX_OK;
}

// ---- a binding that grows
// The freeze line moves forward: the batches [b_act, b_act') the prefix rule newly names under num_fixed_new fixed knots vote once, at
// the knots the reconstruction holds, into the base as it stands.  Frozen batches read fixed knots alone, and those are bytewise the
// same at every evaluation and extend since the freeze, so the base is what one freeze of [0, b_act') would have voted.
int cmx_backend_recon_advance_head(cmx_ctx *c, int num_fixed_new) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return fail(c, CMX_ERR_STATE, "no events are bound (cmx_backend_recon_bind_from)");
  ReconFrozen &fz = r->frozen;
  if (num_fixed_new < fz.num_fixed || num_fixed_new >= r->sup.K)
    return fail(c, CMX_ERR_INVALID_ARG, "num_fixed_new=%d outside [%d, %d)", num_fixed_new, fz.num_fixed, r->sup.K);
  if (fz.num_fixed == 0) return cmx_backend_recon_freeze_head(c, num_fixed_new);
  ReconBound &b = r->bnd;
  const BatchPlan &p = b.plan;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // the prefix rule from the line on, over the active batches' times
  const int n_act_b = p.nb - fz.b_act;
  std::vector<long long> bt((size_t)n_act_b);
  if (n_act_b > 0) HIP_TRY(c, hipMemcpy(bt.data(), b.bt_at(fz.b_act), (size_t)n_act_b * sizeof(long long), hipMemcpyDeviceToHost));
  const int b_new = fz.b_act + frozen_prefix(r->sup, num_fixed_new, bt.data(), n_act_b);
  std::vector<double> knots(4 * (size_t)num_fixed_new);
  HIP_TRY(c, hipMemcpy(knots.data(), r->d_knots, (size_t)num_fixed_new * sizeof(Quat), hipMemcpyDeviceToHost));
  // from here on only a runtime error can end the call
  (void)recon_pass_enter(c, r, false);  // as freeze_head: an open gradient pass is closed
  rc = frozen_vote(c, r, fz.d_base, fz.d_inside, fz.b_act, b_new);
  if (!rc) {
    const hipError_t e = hipMemcpyAsync(&fz.inside, fz.d_inside, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) rc = fail(c, CMX_ERR_HIP, "reading the base's counter: %s", hipGetErrorString(e));
  }
  const hipError_t waited = hipStreamSynchronize(c->stream);
  if (!rc && waited != hipSuccess) rc = fail(c, CMX_ERR_HIP, "the votes of the newly frozen batches failed: %s", hipGetErrorString(waited));
  if (rc) return rc;
  fz.b_act = b_new;
  fz.sampled = p.packed(0, b_new);
  fz.knots = knots;
  fz.num_fixed = num_fixed_new;
  b.sorted = false;  // (the sort holds the newly frozen events, or the old active ones)
  return frozen_plan_active(c, r, &fz);
}

// The frozen batches' resident entries go: the active tail moves into buffers of its own size and the old ones are freed, so the
// binding holds (and its capacity follows) the active tail, not the recording.  The open tail's raw events stay.
int cmx_backend_recon_release_head(cmx_ctx *c) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return fail(c, CMX_ERR_STATE, "no events are bound (cmx_backend_recon_bind_from)");
  ReconBound &b = r->bnd;
  const ReconFrozen &fz = r->frozen;
  const BatchPlan &p = b.plan;
  if (fz.num_fixed == 0 || fz.b_act <= b.rel_batches) return CMX_OK;  // nothing (new) to give back
  // The released entries are dead space in front of the live ones.  Once there is more dead than live the live tail moves into
  // buffers of twice its size and the old ones are freed (a copy of `live` entries per more than `live` released: amortised, and
  // the capacity stays within twice the active tail); until then -- and an append that runs out of room does the same -- the
  // release is book-keeping alone.
  const size_t n_xy = (size_t)(p.n_packed - fz.sampled), n_bt = (size_t)(p.nb - fz.b_act);
  if ((size_t)(fz.sampled - b.base_sampled) > n_xy) {
    const size_t cap_xy = n_xy ? 2 * n_xy : 1, cap_bt = n_bt ? 2 * n_bt : 1;
    uint32_t *xy = nullptr;
    long long *bt = nullptr;
    PoseR *pose = nullptr;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMalloc((void **)&xy, cap_xy * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&bt, cap_bt * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc((void **)&pose, cap_bt * sizeof(PoseR));
    if (e == hipSuccess && n_xy) e = hipMemcpyAsync(xy, b.xy_at(fz.sampled), n_xy * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess && n_bt) e = hipMemcpyAsync(bt, b.bt_at(fz.b_act), n_bt * sizeof(long long), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {  // (the binding is as it was)
      (void)hipStreamSynchronize(c->stream);
      (void)hipFree(xy); (void)hipFree(bt); (void)hipFree(pose);
      return fail(c, CMX_ERR_HIP, "moving the active tail: %s", hipGetErrorString(e));
    }
    (void)hipFree(b.d_xy); (void)hipFree(b.d_bt); (void)hipFree(b.d_poseR);
    b.d_xy = xy; b.d_bt = bt; b.d_poseR = pose;
    b.xy_cap = cap_xy;
    b.bt_cap = cap_bt;
    b.base_sampled = fz.sampled;
    b.base_batches = fz.b_act;
  }
  b.rel_batches = fz.b_act;
  b.rel_sampled = fz.sampled;
  // (whole batches in front of an active one; all of them: every event a batch holds -- a lone trailing event is in none)
  b.rel_events = fz.b_act < p.nb ? (int64_t)fz.b_act * p.B : (int64_t)(p.nb - 1) * p.B + p.last_len;
  return CMX_OK;
}

int cmx_backend_recon_online_info(cmx_ctx *c, int64_t *released_batches, int64_t *released_events, int64_t *released_sampled,
                                  int64_t *resident_sampled) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  const ReconState *r = c->recon;  // (without a binding: all zero)
  if (released_batches) *released_batches = r->bound ? r->bnd.rel_batches : 0;
  if (released_events) *released_events = r->bound ? r->bnd.rel_events : 0;
  if (released_sampled) *released_sampled = r->bound ? r->bnd.rel_sampled : 0;
  if (resident_sampled) *resident_sampled = r->bound ? r->bnd.resident_sampled() : 0;
  return CMX_OK;
}

// `count` events behind the bound ones: the binding afterwards is bind_from's over the concatenation.  plan_append (cmx_ingest.hpp)
// names the batch that is cut again; "the kept open tail ++ the new range" is assembled in a scratch of count + B events at most, and
// the batch-time and packing kernels of bind_from run over that scratch alone.
int cmx_backend_recon_bind_append_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return fail(c, CMX_ERR_STATE, "no events are bound (cmx_backend_recon_bind_from)");
  EventSource src;
  rc = store_source(c, e, first, count, &src);
  if (rc) return rc;
  (void)recon_pass_enter(c, r, false);  // as every add: an open gradient pass is closed
  if (src.n > kMaxEvents) return fail(c, CMX_ERR_INVALID_ARG, "bad event count %lld", (long long)src.n);
  if (src.n == 0) return CMX_OK;
  ReconBound &b = r->bnd;
  ReconFrozen &fz = r->frozen;
  if (b.n_events > 0 && (long long)src.soa.t[0] < b.t_last)
    return fail(c, CMX_ERR_TIME_ORDER, "the first new event (%lld ns) is earlier than the last bound one (%lld ns)", (long long)src.soa.t[0],
                b.t_last);
  AppendPlan ap;
  if (!plan_append(b.n_events, src.n, r->B, r->rate, &ap)) return fail(c, CMX_ERR_INVALID_ARG, "too many batches");
  if (fz.num_fixed > 0 && ap.b_recut < fz.b_act)
    return fail(c, CMX_ERR_STATE, "batch %d, which the new events cut again, is part of the frozen head (%d batches)", ap.b_recut, fz.b_act);
  if (ap.plan.n_packed - b.rel_sampled > kMaxBoundSampled)
    return fail(c, CMX_ERR_INVALID_ARG, "%lld resident sampled events above the limit of a binding (2^30)",
                (long long)(ap.plan.n_packed - b.rel_sampled));
  if (ap.tail_n != b.tail_n) return fail(c, CMX_ERR_STATE, "the binding's open tail holds %lld events, its plan says %lld", (long long)b.tail_n,
                                         (long long)ap.tail_n);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // ---- the scratch stream and its batch times (staging: nothing of the binding is touched)
  const int64_t m = ap.tail_n + src.n;
  if ((size_t)m > r->app_cap) {
    rc = ensure_pair(c, r->d_app_xy, r->d_app_t, r->app_cap, (size_t)m + (size_t)m / 2);
    if (rc) return rc;
  }
  if (ap.tail_n > 0) {
    HIP_TRY(c, hipMemcpyAsync(r->d_app_xy, b.d_tail_xy, (size_t)ap.tail_n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(r->d_app_t, b.d_tail_t, (size_t)ap.tail_n * sizeof(int64_t), hipMemcpyDeviceToDevice, c->stream));
  }
  HIP_TRY(c, hipMemcpyAsync(r->d_app_xy + ap.tail_n, src.d_xy, (size_t)src.n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(r->d_app_t + ap.tail_n, src.d_t, (size_t)src.n * sizeof(int64_t), hipMemcpyDeviceToDevice, c->stream));
  const BatchPlan &sp = ap.scratch;
  ReconSlot &s = r->slot[0];
  if (sp.nb > 0) {
    rc = ensure(c, s.d_bt, s.bt_cap, (size_t)sp.nb);
    if (!rc) rc = validate_store_times(c, r, r->d_app_t, m, sp, sp.nb, s.d_bt);
    if (rc) return rc;
  }
  // ---- valid.  Room for the longer binding, beside the buffers in use, when the arrays' end is reached: twice the LIVE entries (so
  // dead space in front, left by release_head, is dropped on the way and the capacity follows the active tail), the live part
  // copied across; a failure frees the new buffers alone
  const int tiles = recon_sort_tiles(c);
  const int64_t n_act = ap.plan.n_packed - (fz.num_fixed > 0 ? fz.sampled : 0);
  const ChunkPlan cp = plan_chunks(n_act > 0 ? n_act : 1, 2 * tiles, kBackEndChunkDiv);
  const size_t need_xy = (size_t)(ap.plan.n_packed - b.rel_sampled), need_bt = (size_t)(ap.plan.nb - b.rel_batches);
  const size_t keep_xy = (size_t)(ap.packed_at - b.rel_sampled), keep_bt = (size_t)(ap.b_recut - b.rel_batches);
  const int64_t tail_from = open_tail_from(b.n_events + src.n, ap.plan), tail_new = b.n_events + src.n - tail_from;  // the next open tail
  uint32_t *xy = nullptr, *tail_xy = nullptr;
  long long *bt = nullptr;
  PoseR *pose = nullptr;
  int64_t *tail_t = nullptr;
  size_t xy_cap = b.xy_cap, bt_cap = b.bt_cap, tail_cap = b.tail_cap;
  hipError_t he = hipSuccess;
  if ((size_t)(ap.plan.n_packed - b.base_sampled) > b.xy_cap) {
    xy_cap = 2 * need_xy;
    he = hipMalloc((void **)&xy, xy_cap * sizeof(uint32_t));
    if (he == hipSuccess && keep_xy) he = hipMemcpyAsync(xy, b.xy_at(b.rel_sampled), keep_xy * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream);
  }
  if (he == hipSuccess && (size_t)(ap.plan.nb - b.base_batches) > b.bt_cap) {
    bt_cap = 2 * need_bt;
    he = hipMalloc((void **)&bt, bt_cap * sizeof(long long));
    if (he == hipSuccess) he = hipMalloc((void **)&pose, bt_cap * sizeof(PoseR));
    if (he == hipSuccess && keep_bt) he = hipMemcpyAsync(bt, b.bt_at(b.rel_batches), keep_bt * sizeof(long long), hipMemcpyDeviceToDevice, c->stream);
  }
  if (he == hipSuccess && (size_t)tail_new > b.tail_cap) {
    tail_cap = (size_t)tail_new > 2 * b.tail_cap ? (size_t)tail_new : 2 * b.tail_cap;
    he = hipMalloc((void **)&tail_xy, tail_cap * sizeof(uint32_t));
    if (he == hipSuccess) he = hipMalloc((void **)&tail_t, tail_cap * sizeof(int64_t));
  }
  if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
  rc = he == hipSuccess ? (n_act > 0 ? b.ts.reserve(c, n_act, 2 * tiles, cp.max_chunks) : (int)CMX_OK)
                        : fail(c, CMX_ERR_HIP, "growing the binding: %s", hipGetErrorString(he));
  if (rc) {  // (the binding is as it was)
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(xy); (void)hipFree(bt); (void)hipFree(pose); (void)hipFree(tail_xy); (void)hipFree(tail_t);
    return rc;
  }
  // ---- commit: from here on only a runtime error can end the call
  if (xy) { (void)hipFree(b.d_xy); b.d_xy = xy; b.xy_cap = xy_cap; b.base_sampled = b.rel_sampled; }
  if (bt) { (void)hipFree(b.d_bt); (void)hipFree(b.d_poseR); b.d_bt = bt; b.d_poseR = pose; b.bt_cap = bt_cap; b.base_batches = b.rel_batches; }
  if (tail_xy) { (void)hipFree(b.d_tail_xy); (void)hipFree(b.d_tail_t); b.d_tail_xy = tail_xy; b.d_tail_t = tail_t; b.tail_cap = tail_cap; }
  b.n_events += src.n;
  b.plan = ap.plan;
  b.t_last = (long long)src.soa.t[src.n - 1];
  b.sorted = false;
  if (n_act > 0) {  // the chunk rule at the new (active) count
    if (fz.num_fixed > 0) { fz.chunk_events = cp.chunk_events; fz.max_chunks = (int)cp.max_chunks; }
    else { b.chunk_events = cp.chunk_events; b.max_chunks = (int)cp.max_chunks; }
  }
  if (sp.nb > 0) {
    HIP_TRY(c, hipMemcpyAsync(b.bt_at(ap.b_recut), s.d_bt, (size_t)sp.nb * sizeof(long long), hipMemcpyDeviceToDevice, c->stream));
    // (t_next = the smallest time: no event carries the old flag)
    launch_be_pack_from_store(r->d_app_xy, reinterpret_cast<const long long *>(r->d_app_t), (long long)m, r->B, r->rate, sp.per_batch,
                              (int)sp.n_packed, std::numeric_limits<long long>::min(), b.xy_at(ap.packed_at), c->stream);
    HIP_TRY(c, hipGetLastError());
  }
  rc = tail_keep(c, &b, r->d_app_xy + (tail_from - ap.keep_from), r->d_app_t + (tail_from - ap.keep_from), tail_new);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the store may be pushed to, compacted or closed from here on
  return CMX_OK;
}

// ---- cmx_backend_recon_solve's three hooks (the FR-CG loop itself is cmx_solver.cpp's)
// begin: every argument error, before anything changes; then the staging, the start knots on the device and -- asked for -- the
// frozen head at them
int recon_solve_begin(cmx_ctx *c, const double *knots_xyzw, int num_fixed, int freeze_head, double blur_sigma, int contrast_measure,
                      int *n_params) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return fail(c, CMX_ERR_STATE, "no events are bound (cmx_backend_recon_bind_from)");
  if (!knots_xyzw) return fail(c, CMX_ERR_INVALID_ARG, "null knot array");
  const int K = r->sup.K;
  if (num_fixed < 0 || num_fixed >= K) return fail(c, CMX_ERR_INVALID_ARG, "num_fixed=%d outside [0, %d)", num_fixed, K);
  if (!std::isfinite(blur_sigma)) return fail(c, CMX_ERR_INVALID_ARG, "blur_sigma is not finite");
  const bool keep = freeze_head == CMX_RECON_KEEP_HEAD;
  if (keep) {  // under the frozen head as it stands
    const ReconFrozen &fz = r->frozen;
    if (fz.num_fixed == 0) return fail(c, CMX_ERR_STATE, "no frozen head to keep (cmx_backend_recon_freeze_head / _advance_head)");
    if (num_fixed != fz.num_fixed) return fail(c, CMX_ERR_INVALID_ARG, "num_fixed=%d, the frozen head has %d", num_fixed, fz.num_fixed);
    if (memcmp(knots_xyzw, fz.knots.data(), (size_t)fz.num_fixed * sizeof(Quat)) != 0)
      return fail(c, CMX_ERR_INVALID_ARG, "the first %d knots differ from those the head was frozen at", fz.num_fixed);
  } else {
    rc = recon_refuse_released(c, r, "a solve that freezes again or drops the head");
    if (rc) return rc;
  }
  rc = recon_grad_precheck(c, r, blur_sigma);
  if (rc) return rc;
  ReconSolve &sv = r->solve;
  if (!sv.h_knots) {
    HIP_TRY(c, hipHostMalloc((void **)&sv.h_knots, (size_t)K * sizeof(Quat), hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void **)&sv.h_cm, 2 * sizeof(double), hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void **)&sv.h_cnt, 2 * sizeof(unsigned long long), hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void **)&sv.h_grad, 3 * (size_t)K * sizeof(double), hipHostMallocMapped));
    HIP_TRY(c, hipHostGetDevicePointer((void **)&sv.d_grad, sv.h_grad, 0));
  }
  sv.k0.assign(knots_xyzw, knots_xyzw + 4 * (size_t)K);
  sv.num_fixed = num_fixed;
  sv.sigma = blur_sigma;
  sv.measure = contrast_measure;
  sv.have_last = false;
  sv.evals = 0;
  sv.waits = 0;
  if (keep) {  // the start knots by extend's path: the head survives
    rc = cmx_backend_recon_extend(c, K, knots_xyzw);
  } else if (freeze_head) {  // at the start knots: they go to the device first (restart, which also drops an earlier head)
    rc = cmx_backend_recon_restart(c, knots_xyzw);
    if (!rc) rc = cmx_backend_recon_freeze_head(c, num_fixed);
  } else {  // every event, every time
    rc = cmx_backend_recon_freeze_head(c, 0);
  }
  if (rc) return rc;
  *n_params = 3 * (K - num_fixed);
  return CMX_OK;
}

// the knots of increment x: the start knots moved by cmx_traj_incremental_update itself, into the pinned staging
static void solve_moved(const ReconState *r, const ReconSolve &sv, const double *x, double *knots) {
  const int K = r->sup.K;
  memcpy(knots, sv.k0.data(), (size_t)K * sizeof(Quat));
  (void)cmx_traj_incremental_update(K, knots, sv.num_fixed, 3 * (K - sv.num_fixed), x);
}

int recon_solve_eval(cmx_ctx *c, const double *x, double *contrast, double *grad_free) {
  ReconState *r = c->recon;
  ReconSolve &sv = r->solve;
  solve_moved(r, sv, x, sv.h_knots);
  const int64_t w0 = r->host_waits;
  const int rc = bound_eval(c, r, sv.h_knots, sv.sigma, sv.measure, contrast, grad_free, &sv);
  sv.evals++;
  sv.waits += r->host_waits - w0;
  const size_t n = 3 * (size_t)(r->sup.K - sv.num_fixed);
  sv.last_x.assign(x, x + n);
  sv.have_last = rc == CMX_OK;
  return rc;
}

// end: the refined knots to the caller, and the reconstruction at their evaluation -- one more cost-only evaluation when the last
// trial point was another one
int recon_solve_end(cmx_ctx *c, const double *x, double *knots_out) {
  ReconState *r = c->recon;
  ReconSolve &sv = r->solve;
  const size_t n = 3 * (size_t)(r->sup.K - sv.num_fixed);
  int rc = CMX_OK;
  if (!sv.have_last || memcmp(sv.last_x.data(), x, n * sizeof(double)) != 0) {
    double con = 0;
    rc = recon_solve_eval(c, x, &con, nullptr);
  }
  solve_moved(r, sv, x, knots_out);
  return rc;
}

int cmx_diag_recon_solve_counts(cmx_ctx *c, int64_t *evaluations, int64_t *host_waits) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  if (evaluations) *evaluations = c->recon->solve.evals;
  if (host_waits) *host_waits = c->recon->solve.waits;
  return CMX_OK;
}

// cmx_pipeline.cpp -- one evaluation on the context's stream: accumulation buffers (ping-pong), destination-tile sort,
// image passes, gather, finalize and the completion ticket.  Shared by the front end and the back end.
#include <cstdlib>
#include "cmx_context.hpp"

// the host finalize of front-end gradient evaluations (arm_tail): on while CMX_OPT_TAIL_FINALIZE has not been set (an explicit 1
// means the device tail), and its shard count -- 8 / 16 / 32 measured a tie, and 8 sums the rows the device tail sums, in its order
// (profiles/tail_host_finalize.txt; A/B builds: tools/build_variant.sh recompiles this file with other values)
#ifndef CMX_TAIL_HOST_DEFAULT
#define CMX_TAIL_HOST_DEFAULT 1
#endif
#ifndef CMX_HOSTFIN_SHARDS
#define CMX_HOSTFIN_SHARDS 8
#endif
static constexpr bool kTailHostDefault = CMX_TAIL_HOST_DEFAULT != 0;
static constexpr int kHostShardsDefault = CMX_HOSTFIN_SHARDS;
static_assert(kHostShardsDefault >= 1 && kHostShardsDefault <= cmx::kHostShardsMax, "shard count of the host finalize");

// Fast path: swap to the partner buffer if it is known clean, otherwise clear the current one.  After this call
// c->d_accum is all-zero over `nplanes` planes and c->pingpong_planes tells the image pass to clear the partner.
int begin_accum(cmx_ctx *c, int nplanes, size_t np, bool fast) {
  c->pingpong_planes = 0;
  if (c->acc_dirty) {  // a split evaluation added to the accumulator rows and never reached its finalize (an error between the
                       // two halves): every later gradient would carry those sums -- the buffers are all-zero between launches
    if (c->d_gacc) HIP_TRY(c, hipMemsetAsync(c->d_gacc, 0, kGaccDoubles * sizeof(double), c->stream));
    if (c->d_tail_counters) HIP_TRY(c, hipMemsetAsync(c->d_tail_counters, 0, kTailCounterWords * sizeof(unsigned), c->stream));
    c->acc_dirty = false;
  }
  const size_t need = (size_t)nplanes * np;
  if (fast && !c->accum_external) {
    float *before = c->d_accum;
    int rc = ensure(c, c->d_accum, c->accum_cap, need);
    if (rc) return rc;
    if (c->d_accum != before) c->accum_clean = false;  // fresh allocation: contents undefined
    if (c->accum_alt_cap < need || !c->d_accum_alt) {
      rc = ensure(c, c->d_accum_alt, c->accum_alt_cap, c->accum_cap > need ? c->accum_cap : need);
      if (rc) return rc;
      c->alt_clean = false;
      c->alt_flagged = false;  // contents unknown: the next image pass clears every tile
    }
    if (c->alt_clean) {
      std::swap(c->d_accum, c->d_accum_alt);
      std::swap(c->accum_cap, c->accum_alt_cap);
      std::swap(c->accum_clean, c->alt_clean);
      std::swap(c->d_tflags, c->d_tflags_alt);
      std::swap(c->accum_flagged, c->alt_flagged);
    }
    if (!c->accum_clean) {
      Span sp(c, CMX_T_ZERO);
      HIP_TRY(c, hipMemsetAsync(c->d_accum, 0, need * sizeof(float), c->stream));
      if (c->d_tflags) HIP_TRY(c, hipMemsetAsync(c->d_tflags, 0, c->tflags_cap, c->stream));
    }
    c->accum_flagged = false;  // set by the caller once a flag-marking splat has been launched into the clean buffer
    c->accum_clean = false;  // about to be written
    c->alt_clean = false;    // holds the previous evaluation's planes until this evaluation's image pass clears it
    c->pingpong_planes = nplanes;
    return CMX_OK;
  }
  int rc = ensure_accum(c, need);
  if (rc) return rc;
  {
    Span sp(c, CMX_T_ZERO);
    HIP_TRY(c, hipMemsetAsync(c->d_accum, 0, need * sizeof(float), c->stream));
  }
  c->accum_clean = false;
  c->accum_flagged = false;
  return CMX_OK;
}

int ensure_accum(cmx_ctx *c, size_t need) {
  if (c->accum_external) {
    if (need > c->accum_cap)
      return fail(c, CMX_ERR_INVALID_ARG, "external accumulation buffer too small: %zu < %zu floats", c->accum_cap, need);
    return CMX_OK;
  }
  return ensure(c, c->d_accum, c->accum_cap, need);
}

// ---- sort the events by destination tile under the CURRENT parameters and build the chunk table (TileSort, cmx_tilesort.cpp).
// What is the window path's own stays here: the chunk divisor, the bearing / dt streams that ride along with the counting sort,
// the fused tables, and the state of the binning (id, launch bound, validity, re-sort statistics).
#ifndef CMX_FE_CHUNK_DIV
#define CMX_FE_CHUNK_DIV 256
#endif
int do_binning(cmx_ctx *c, const FeSplatArgs *fe, const BeSplatArgs *be) {
  const int n = c->n_packed;
  const int W = c->imgW, H = c->imgH;
  TileSortJob job;
  job.fe = fe; job.be = be;
  job.tiles_x = (W + kBinTile - 1) / kBinTile;
  const int tiles_y = (H + kBinTile - 1) / kBinTile;
  job.tiles = job.tiles_x * tiles_y;
  job.planes_per_tile = fe ? 1 : 2;  // back end: key = 2*tile + (IL_new ? 1 : 0)
  const int ntiles = job.tiles * job.planes_per_tile;
  const ChunkPlan cp = plan_chunks(n, ntiles, fe ? CMX_FE_CHUNK_DIV : kBackEndChunkDiv);
  const int max_chunks = (int)cp.max_chunks;
  int rc = c->sort.reserve(c, n, ntiles, max_chunks);
  if (rc) return rc;
  if (!c->h_nchunks) {
    HIP_TRY(c, hipHostMalloc((void **)&c->h_nchunks, sizeof(unsigned long long), hipHostMallocMapped));
    *c->h_nchunks = 0ull;
    HIP_TRY(c, hipHostGetDevicePointer((void **)&c->d_nchunks_host, c->h_nchunks, 0));
  }
  c->binning_id++;  // a build_chunks of an earlier binning that was never collected may still store its (id, count): ignored
  if (c->binning_id == 0) c->binning_id = 1;
  if (n > 0) {
    c->streams_valid = false;
    if (c->sort.counting && c->d_lut2) {  // the sorted order also carries every event's bearing (front end: and its dt)
      rc = ensure(c, c->d_sb, c->sb_cap, (size_t)2 * n);
      if (rc) return rc;
      if (fe) {
        rc = ensure(c, c->d_sdt, c->sdt_cap, (size_t)n);
        if (rc) return rc;
      }
      c->streams_valid = true;
    }
    FusedTables ft{};
    c->fused_bin_id = 0;
    if (fe && c->fused_image && fused_tables_ok(ntiles, job.planes_per_tile)) {  // tables of the fused splat + image pass (FusedArgs)
      rc = ensure(c, c->d_fnbr_expected, c->fnbr_cap, (size_t)ntiles * kFuseStrips);
      if (rc) return rc;
      rc = ensure(c, c->d_fnbr_cnt, c->fcnt_cap, (size_t)ntiles * kFuseStrips * kFuseCntStride);
      if (rc) return rc;
      rc = ensure(c, c->d_fpartials, c->fpartials_cap, (size_t)2 * ntiles * kFuseStrips);
      if (rc) return rc;
      if (!c->d_ftiles_done) {
        HIP_TRY(c, hipMalloc((void **)&c->d_ftiles_done, sizeof(unsigned)));
        HIP_TRY(c, hipMalloc((void **)&c->d_fn_active, sizeof(int)));
      }
      if ((size_t)ntiles * kFuseStrips * kFuseCntStride > c->fdone_cap || !c->d_ftile_done) {
        rc = ensure(c, c->d_ftile_done, c->fdone_cap, (size_t)ntiles * kFuseStrips * kFuseCntStride);
        if (rc) return rc;
        HIP_TRY(c, hipMemsetAsync(c->d_ftile_done, 0, c->fdone_cap * sizeof(unsigned), c->stream));  // (no launch has stamp 0)
      }
      ft.n_active = c->d_fn_active;
      ft.tiles_done = c->d_ftiles_done;
      ft.tiles_y = tiles_y;
      ft.nbr_expected = c->d_fnbr_expected;
      ft.nbr_cnt = c->d_fnbr_cnt;
      ft.partials = c->d_fpartials;
      job.fused = &ft;
      c->fused_bin_id = c->binning_id;
      c->fused_tiles_x = job.tiles_x;
      c->fused_tiles_y = tiles_y;
    }
    job.xy = c->d_xy; job.per_batch = c->per_batch; job.n = n;
    job.chunk_events = cp.chunk_events;
    if (c->streams_valid) { job.sb = c->d_sb; job.sdt = c->d_sdt; }
    job.count_host = c->d_nchunks_host; job.binning_id = c->binning_id;
    rc = c->sort.run(c, job);
    if (rc) return rc;
    c->nchunks = max_chunks;
    c->nchunks_exact = false;
  } else {
    HIP_TRY(c, hipMemsetAsync(c->sort.d_nchunks, 0, sizeof(int), c->stream));
    c->nchunks = 0;
    c->nchunks_exact = true;
  }
  c->bin_valid = true;
  c->force_rebin = false;
  c->rebin_count++;
  c->last_fallback_frac = 0;
  return CMX_OK;
}

int ensure_fixed(cmx_ctx *c, size_t n) {
  if (n <= c->fixed_cap && c->d_fixed) return CMX_OK;
  int rc = ensure(c, c->d_fixed, c->fixed_cap, n);
  if (rc) return rc;
  HIP_TRY(c, hipMemsetAsync(c->d_fixed, 0, c->fixed_cap * sizeof(unsigned long long), c->stream));
  return CMX_OK;
}

BinnedEvents binned(const cmx_ctx *c) {
  BinnedEvents b{};
  b.sxy = c->sort.d_sxy;
  b.sbatch = c->sort.d_sbatch;
  b.chunks = c->sort.d_chunks;
  b.nchunks = c->nchunks;
  b.nchunks_dev = c->sort.d_nchunks;
  b.fallback = c->sort.d_fallback;
  b.sort_tiles_x = (c->imgW + kBinTile - 1) / kBinTile;
  b.sort_tiles_y = (c->imgH + kBinTile - 1) / kBinTile;
  if (c->streams_valid) { b.sb = c->d_sb; b.sdt = c->kind == KIND_FE ? c->d_sdt : nullptr; }
  return b;
}

FeSplatArgs fe_args(const cmx_ctx *c, const double omega[3]) {
  FeSplatArgs a{};
  a.fx = c->fx; a.fy = c->fy; a.cx = c->cx; a.cy = c->cy;
  a.wx = omega[0]; a.wy = omega[1]; a.wz = omega[2];
  a.W = c->W; a.H = c->H;
  a.per_batch = c->per_batch;
  a.n = c->n_packed;
  a.xy = c->d_xy;
  a.batch_dt = c->d_batch_dt;
  a.lut = c->d_lut;
  a.lut2 = c->d_lut2;
  a.planes = c->d_accum;
  if (c->chain_active && !c->chain_first) {  // device-driven solve: omega and the end-of-solve flag live in device memory
    a.w_dev = c->d_chain->x_req;
    a.skip = &c->d_chain->done;
  }
  return a;
}

BeSplatArgs be_args(const cmx_ctx *c) {
  BeSplatArgs a{};
  a.W = c->W;
  a.Wp = c->Wp; a.Hp = c->Hp;
  a.fx = (double)((c->Wp / 360.0) * 180.0 / 3.1415926535897932384626433832795);  // focalFromFOV(.., 360, 180)
  a.fy = (double)((c->Hp / 180.0) * 180.0 / 3.1415926535897932384626433832795);
  a.cxp = (double)c->Wp / 2.0;
  a.cyp = (double)c->Hp / 2.0;
  a.per_batch = c->per_batch;
  a.n = c->n_packed;
  a.order = c->order;
  a.num_fixed = c->num_fixed;
  a.xy = c->d_xy;
  a.poseR = c->d_poseR;
  a.poses = c->d_poses;
  a.lut = c->d_lut;
  a.lut2 = c->d_lut2;
  a.planes = c->d_accum;
  return a;
}

// G^T folding assumes single reflections: image larger than the kernel.  The Sobel contrast (front end, measure 2) composes
// G^T with Sobel^T, whose folds stay on the filter's own 3 taps for any side >= 2 (image_adjoint_sobel_kernel) -- and
// 2r+1 >= 1 makes every side that passes the G^T rule at least 2: one rule for all measures.
bool adjoint_ok(const cmx_ctx *c) {
  return c->grad_mode == CMX_GRAD_ADJOINT && c->imgW > 2 * c->radius + 1 && c->imgH > 2 * c->radius + 1;
}
// the adjoint form of the Sobel gradient-magnitude contrast: its own image pass, everything behind it as for mean-square
static bool sobel_adjoint(const cmx_ctx *c) { return c->kind == KIND_FE && c->measure == CMX_GRADIENT_MAGNITUDE; }
// what the finalize of an ADJOINT evaluation computes from the moment rows and the gather's sums.  Gradient magnitude has no
// mean term: row 1 = sum (gx^2 + gy^2), contrast = row1 / N, grad = 2 S1 / N -- the mean-square expressions.  (measure 2 in
// FinalizeArgs means the Sobel partial table of the derivative-plane form, run_image_and_finalize.)
static int adjoint_finalize_measure(const cmx_ctx *c) { return sobel_adjoint(c) ? CMX_MEAN_SQUARE : c->measure; }

// result words a finalize writes: contrast, mean, gradient (+ what a chained one appends)
static int result_words(const FinalizeArgs &f) { return 2 + (f.P > f.gP ? f.P : f.gP) + (f.chain.sm ? kChainExtra : 0); }

// every evaluation ends in exactly one finalize -- its own launch (here) or the tail of the evaluation's last kernel
// (arm_tail) -- which carries the ticket sync_and_collect() waits for
void issue_finalize(cmx_ctx *c, FinalizeArgs &f, bool with_reduce) {
  f.ticket = ++c->ticket_issued;
  c->ticket_nout = result_words(f);
  Span sp(c, CMX_T_FINAL, /*exact=*/true);
  if (with_reduce) launch_finalize(f, c->stream, sp.t0(), sp.t1());
  else launch_finalize_only(f, c->stream, sp.t0(), sp.t1());
}

// Tail finalize (CMX_OPT_TAIL_FINALIZE): hand the finalize to the launch that is about to be issued.  Only the forms whose
// inputs are per-workgroup partial tables of that very launch or results of earlier launches qualify (f.direct, no
// reduce_partials pass in between).
bool arm_tail(cmx_ctx *c, FinalizeArgs &f, TailArgs &tail, bool gated) {
  tail.counters = nullptr;
  if (!c->tail_finalize || !c->d_tail_counters || !f.direct || f.measure == 2) return false;
  // back end, gradient evaluations: read as a 42-column x 196-row table by one 256-thread workgroup the tail is 1.5-2 us
  // SLOWER than the finalize launch (measured, config 3).  Outside CMX_OPT_DETERMINISTIC the per-batch pass therefore adds
  // its column sums to kTailShards rows of accumulators with device-scope fp64 atomics (the order of the adds varies run
  // to run -- so does the vote image in that mode) and the tail reads 8 x 42 values.  Option value 2 forces the table form.
  if (c->kind == KIND_BE && f.gP > 0 && c->tail_finalize < 2) {
    if (c->deterministic || !c->d_gacc || 2 * f.gP > kGaccStride) return false;
    f.gacc = c->d_gacc;
    f.gacc_stride = kGaccStride;
  }
  // front end: the same accumulators instead of the ~1000 x 6 table (gather + tail 14.9 -> 13.2 us); value 2 keeps the table
  if (c->kind == KIND_FE && f.gP > 0 && c->tail_finalize < 2 && !c->deterministic && c->d_gacc) {
    f.gacc = c->d_gacc;
    f.gacc_stride = kGaccStride;
  }
  if (gated) {  // the gated pass reports to the second result block with its own ticket sequence
    f.ticket = ++c->ticket2_issued;
    c->ticket2_nout = result_words(f);
  } else {
    f.ticket = ++c->ticket_issued;
    c->ticket_nout = result_words(f);
  }
  tail.counters = c->d_tail_counters;
  tail.fin = f;
  // CMX_OPT_TAIL_FINALIZE 3 (A/B, measured without gain): front-end gradient evaluations through accumulator rows let workgroup 0 poll
  // sharded arrival counts instead of finding the last arriver through two levels of returning tickets
  tail.poll = (c->kind == KIND_FE && f.gP > 0 && f.gacc && c->tail_poll && !f.chain.sm) ? 1 : 0;
  // CMX_OPT_TAIL_FINALIZE 4 (cmx_hostfin.hpp): the same evaluations -- host-driven, one result block, variance or mean square -- end
  // in one record per accumulator-row shard and a moments record; sync_and_collect forms contrast and gradient from them.  Gated
  // passes, the slots of a device-driven solve, eval_many's blocks and sharded or deterministic contexts keep the device finalize.
  tail.host_shards = 0;
  tail.host_rec = nullptr;
  const bool host = c->tail_host >= 0 ? c->tail_host != 0 : kTailHostDefault;
  if (host && c->kind == KIND_FE && f.gP > 0 && 2 * f.gP <= kHostRecCols && f.gacc && f.mu_free && !tail.poll && !gated && !f.chain.sm &&
      !c->chain_active && !c->result_override && !c->sharded() && (f.measure == 0 || f.measure == 1) && !f.macc) {
    const int S = c->host_shards > 0 ? c->host_shards : kHostShardsDefault;
    tail.host_shards = S;
    tail.host_rec = reinterpret_cast<unsigned long long *>(c->d_result + kHostRecBase);
    c->hostfin_ticket = f.ticket;
    c->hostfin_G = fe_gather_blocks(c->n_packed);
    c->hostfin_S = S;
    c->hostfin_gP = f.gP;
    c->hostfin_mu_free = f.mu_free;
    c->hostfin_measure = f.measure;
    c->hostfin_npix = f.npix;
  }
  return true;
}

// what every image pass takes from the context: size, blur, and the kind's sources (front end: the one vote plane)
void image_args(const cmx_ctx *c, ImgArgs &a) {
  a.W = c->imgW; a.H = c->imgH; a.r = c->radius;
  memcpy(a.taps, c->taps, sizeof(a.taps));
  a.src_a = c->d_accum;
  if (c->kind == KIND_BE) {
    a.src_b = c->d_accum + (size_t)c->imgW * c->imgH;
    a.igp = c->ig_nonzero ? c->d_IGp : nullptr;
    a.alpha = c->d_alpha;
  }
}

// the pass clears the ping-pong partner while it is at it, once per evaluation (call before attach_tiles)
void claim_partner_clear(cmx_ctx *c, ImgArgs &a) {
  if (c->pingpong_planes > 0 && c->d_accum_alt && !c->alt_clean) {
    a.zero_ptr = c->d_accum_alt;
    a.zero_planes = c->pingpong_planes;
    c->alt_clean = true;  // stream-ordered: clean by the time the next accumulate's splat runs
  }
}

// ping-pong partner clearing + tile-occupancy flags of an image pass (see ImgArgs)
int attach_tiles(cmx_ctx *c, ImgArgs &a, bool may_skip) {
  a.tiles_y = (a.H + kTileY - 1) / kTileY;
  if (a.zero_ptr) {
    if (c->alt_flagged && c->d_tflags_alt) {
      a.flags_other = c->d_tflags_alt;  // clear the dirty tiles only
    } else if (c->d_tflags_alt) {
      HIP_TRY(c, hipMemsetAsync(c->d_tflags_alt, 0, c->tflags_cap, c->stream));  // everything is cleared: no flag survives
    }
    c->alt_flagged = true;  // clean buffer, no flags: trivially consistent
  }
  if (may_skip && c->accum_flagged && c->d_tflags && (!a.igp || c->igp_flags_valid)) {
    a.flags_cur = c->d_tflags;
    a.flags_igp = a.igp ? c->d_igp_flags : nullptr;
  }
  return CMX_OK;
}

// large panoramas: compact the tiles that need work (call once a.partials / flags / zero_ptr are final)
int maybe_tile_list(cmx_ctx *c, ImgArgs &a, int reach) {
  if (!a.flags_cur || a.nblk <= kTileListMin) return CMX_OK;
  // The order of the list is the order finalize sums the tiles' moment rows in.  CMX_OPT_DETERMINISTIC: no list (which
  // tiles are listed -- dirty ones included -- depends on the history, and so would the grouping of the sum).  Sharded
  // evaluations: every rank must obtain bit-identical numbers or the replicated optimiser drivers stop taking the same
  // decisions; the ranks share flags and history, so a list built in TILE ORDER by one workgroup is the same on all of
  // them (the atomically compacted one is not).
  if (c->deterministic) return CMX_OK;
  const bool ordered = c->sharded();
  if ((size_t)a.nblk > c->tile_list_cap || !c->d_tile_list) {
    if (c->d_tile_list) HIP_TRY(c, hipFree(c->d_tile_list));
    if (c->d_tile_count) HIP_TRY(c, hipFree(c->d_tile_count));
    c->d_tile_list = c->d_tile_count = nullptr;
    HIP_TRY(c, hipMalloc((void **)&c->d_tile_list, (2 * (size_t)a.nblk + 8) * sizeof(unsigned)));  // list + dense scratch of the ordered form
    HIP_TRY(c, hipMalloc((void **)&c->d_tile_count, 2 * sizeof(unsigned)));
    HIP_TRY(c, hipMemsetAsync(c->d_tile_count, 0, 2 * sizeof(unsigned), c->stream));
    c->tile_list_cap = (size_t)a.nblk;
    c->tile_count_sel = 0;
  }
  unsigned *cur = c->d_tile_count + c->tile_count_sel, *next = c->d_tile_count + (c->tile_count_sel ^ 1);
  c->tile_count_sel ^= 1;  // this pass counts in `cur` and zeroes `next` for the pass after it
  launch_tile_list(a, reach, c->d_tile_list, cur, next, ordered, c->stream);
  a.tile_list = c->d_tile_list;
  a.tile_count = cur;
  return CMX_OK;
}

// image pass on the accumulated planes -> partial moments -> contrast/gradient in h_result
int run_image_and_finalize(cmx_ctx *c, int P, float *out_blur0, float *out_blurd) {
  const int W = c->imgW, H = c->imgH;
  const size_t np = (size_t)W * H;
  ImgArgs a{};
  image_args(c, a);
  a.dplanes = c->d_accum + (c->kind == KIND_FE ? 1 : 2) * np;
  a.P = P;
  a.out_blur0 = out_blur0;
  a.out_blurd = out_blurd;
  claim_partner_clear(c, a);
  a.tiles_x = (W + kTileX - 1) / kTileX;
  a.nblk = a.tiles_x * ((H + kTileY - 1) / kTileY);
  const size_t nq = 2 + 2 * (size_t)P;
  int rc = attach_tiles(c, a, /*may_skip=*/P == 0 && !out_blur0 && !out_blurd);
  if (rc) return rc;
  rc = ensure(c, c->d_partials, c->partials_cap, nq * a.nblk);
  if (rc) return rc;
  rc = ensure(c, c->d_sums, c->sums_cap, nq);
  if (rc) return rc;
  if (2 + (size_t)P > c->result_cap - 1) return fail(c, CMX_ERR_INVALID_ARG, "too many derivative planes (%d)", P);
  a.partials = c->d_partials;
  FinalizeArgs f{};
  f.P = P;
  f.nblk = a.nblk;
  f.measure = c->measure;
  f.npix = (double)np;
  f.partials = c->d_partials;
  f.sums = c->d_sums;
  f.result = result_ptr(c);
  f.fallback = c->sort.d_fallback;
  if (c->measure == CMX_GRADIENT_MAGNITUDE && c->kind == KIND_FE) {
    // blurred planes -> scratch, then Sobel moments (reference local_focus_funcs.cpp:47-73), then finalize
    float *blur = out_blur0;
    if (!blur) {
      rc = ensure(c, c->d_scratch, c->scratch_cap, 7 * np);
      if (rc) return rc;
      blur = c->d_scratch;
      a.out_blur0 = blur;
      a.out_blurd = blur + np;
    }
    SobelArgs sa{};
    sa.W = W; sa.H = H; sa.P = P;
    sa.planes = blur;
    sa.nblk = sobel_blocks(W, H);
    rc = ensure(c, c->d_gpartials, c->gpartials_cap, (size_t)(1 + P) * sa.nblk);
    if (rc) return rc;
    sa.partials = c->d_gpartials;
    Span sp(c, CMX_T_IMAGE, /*exact=*/true);
    launch_image_moments(a, c->stream, sp.t0(), sp.t1());
    launch_sobel_moments(sa, c->stream);
    f.P = 0; f.direct = 1;  // (measure 2: the derivative planes' moments are the Sobel partial table's)
    f.gpartials = c->d_gpartials; f.gblocks = sa.nblk; f.gP = P;
    issue_finalize(c, f, false);
    HIP_TRY(c, hipGetLastError());
    return CMX_OK;
  }
  bool tailed = false;
  {
    Span sp(c, CMX_T_IMAGE, /*exact=*/true);
    rc = maybe_tile_list(c, a, c->radius);
    if (rc) return rc;
    if (P == 0 && (a.nblk <= 2048 || a.tile_list)) {
      f.direct = 1;
      f.nvalid = a.tile_count;  // list path: partial rows are compact, one entry per listed tile
      if (!out_blur0 && !out_blurd) tailed = arm_tail(c, f, a.tail);  // the last-arriving workgroup finalizes
    }
    launch_image_moments(a, c->stream, sp.t0(), sp.t1());
  }
  if (!tailed) issue_finalize(c, f, /*with_reduce=*/!f.direct);
  HIP_TRY(c, hipGetLastError());
  return CMX_OK;
}

// A cost-only evaluation that a gradient evaluation at the same parameters is likely to follow (the optimiser's f-then-df
// pattern, CMX_OPT_REUSE_IMAGE): run the fused adjoint image pass instead of the moments-only pass, so that the df finds
// Jt and the moment rows ready and launches its gather straight away (adjoint_cost_only; +3..4 us per f, -12 us per df).
bool speculative_jt_ok(const cmx_ctx *c) {
  return c->reuse_image && adjoint_ok(c) && !c->accum_external && !c->sharded() && c->last_P == 0 && c->n_packed > 0;
}

// ---- adjoint gradient: fused image pass (B = G*A with its moments, Jt = G^T B^) -> gather over the events (S1, and S2 for
// the votes next to the border) -> finalize: contrast from the moments, grad = (2/N)(S1 - mu*S2).  First the steps, each
// present once; the five forms of the evaluation (adjoint_eval ... adjoint_gated_grad, below them) queue them top to bottom.
int ensure_jt(cmx_ctx *c) {
  float *jt_before = c->d_itilde;
  if (int rc = ensure(c, c->d_itilde, c->itilde_cap, (size_t)c->imgW * c->imgH)) return rc;
  if (c->d_itilde != jt_before)  // tiles the image pass skips keep whatever they held: make that finite from the start
    HIP_TRY(c, hipMemsetAsync(c->d_itilde, 0, c->itilde_cap * sizeof(float), c->stream));
  return CMX_OK;
}

// the adjoint pass on top of image_args: its own tiling, Jt (ensure_jt first), the composite operator where it applies
void image_adjoint_args(const cmx_ctx *c, ImgAdjArgs &ia) {
  image_args(c, ia.img);
  ia.img.P = 0;
  ia.img.tiles_x = image_adjoint_tiles_x(c->imgW);
  ia.img.nblk = image_adjoint_tiles(c->imgW, c->imgH);
  ia.jt = c->d_itilde;
  if (c->chain_active && !c->chain_first) ia.img.skip = &c->d_chain->done;  // device-driven solve: as the splat's (fe_args)
  // (no composite-operator form of the Sobel pass: Sobel sits between G and G^T)
  if (!sobel_adjoint(c) && c->composite_image && c->radius >= 1 && c->d_Mx && c->d_My && c->Mx_radius == c->radius) { ia.Mx = c->d_Mx; ia.My = c->d_My; }
}

struct AdjEval {    // what the steps of one evaluation share
  int P;
  bool fused_rows;  // the moment rows are those of a pass that ran inside the splat launch: d_fpartials, in the fused tiles' shape
  ImgAdjArgs ia;
  int gb, P2;                        // rows and doubles per row of the gather partial table
  int slice_shift, parts_per_batch;  // back-end gather: events per slice (as a shift), slices per batch
};

// image arguments, and every buffer the evaluation may touch
static int adjoint_begin(cmx_ctx *c, int P, AdjEval &e) {
  e = AdjEval{};
  e.P = P;
  e.fused_rows = c->adj_fused;  // (until an image step of this evaluation writes d_partials)
  if (int rc = ensure_jt(c)) return rc;
  image_adjoint_args(c, e.ia);
  if (int rc = ensure(c, c->d_partials, c->partials_cap, (size_t)2 * e.ia.img.nblk)) return rc;
  if (int rc = ensure(c, c->d_sums, c->sums_cap, 2)) return rc;
  // rows of the gather partial table: front end = gather workgroups; back end = workgroups of the per-batch pass
  e.gb = (c->kind == KIND_FE) ? fe_gather_blocks(c->n_packed) : be_batch_blocks(c->nb);
  e.P2 = 2 * (P > 0 ? P : 1);
  if (int rc = ensure(c, c->d_gpartials, c->gpartials_cap, (size_t)e.gb * e.P2)) return rc;
  // four events per lane in the back-end gather when a lane's four events cannot straddle a batch boundary
  e.slice_shift = (c->kind == KIND_BE && c->per_batch % 4 == 0) ? 8 : 6;
  e.parts_per_batch = ((c->per_batch + (1 << e.slice_shift) - 2) >> e.slice_shift) + 1;
  if (c->kind == KIND_BE)
    if (int rc = ensure(c, c->d_vparts, c->vparts_cap, (size_t)(c->nb > 0 ? c->nb : 1) * e.parts_per_batch * 6)) return rc;
  if (2 + (size_t)P > c->result_cap - 2) return fail(c, CMX_ERR_INVALID_ARG, "too many parameters (%d)", P);
  if (!c->gsum_external) {
    if (int rc = ensure(c, c->d_gsum, c->gsum_cap, (size_t)e.P2)) return rc;
  } else if ((size_t)e.P2 > c->gsum_cap) {
    return fail(c, CMX_ERR_INVALID_ARG, "external gradient buffer too small: %zu < %d doubles", c->gsum_cap, e.P2);
  }
  e.ia.img.partials = c->d_partials;
  return CMX_OK;
}

// where the finalize finds the gradient sums: nowhere (cost only), in the gather's block partials (one call), in the
// accumulator rows or in d_gsum (the two ways of a split call: acc_rows)
enum GradSums { GRAD_NONE, GRAD_BLOCKS, GRAD_ROWS, GRAD_GSUM };

// split call with the evaluator's own communicator: the workgroups' sums go to the accumulator rows (FinalizeArgs::gacc),
// the rows are all-reduced as they are (cmx_comm.cpp) and the finalize sums them -- no per-batch kernel, no
// reduce_gpartials launch.  Callers that all-reduce cmx_grad_ptr() themselves keep the 2P-double buffer.
// (rank-invariant condition: every rank must issue the same collective, also one whose shard is empty)
static bool acc_rows(const cmx_ctx *c, int P) { return c->shard_acc && !c->deterministic && c->d_gacc && 2 * P <= kGaccStride && P > 0; }

// second: the gated pass's result block (of a chain slot: its gradient block, stage 1); arm_gate: this finalize decides whether
// the pass queued behind it runs.  The moment rows have the shape image_step left in adj_direct / adj_tile_count
static FinalizeArgs finalize_args(const cmx_ctx *c, const AdjEval &e, GradSums grad, bool second = false, bool arm_gate = false) {
  FinalizeArgs f{};
  f.P = 0;
  f.nblk = e.fused_rows ? c->fused_tiles_x * c->fused_tiles_y * kFuseStrips : e.ia.img.nblk;
  f.measure = adjoint_finalize_measure(c);
  f.npix = (double)((size_t)c->imgW * c->imgH);
  f.partials = e.fused_rows ? c->d_fpartials : c->d_partials;
  f.sums = c->d_sums;
  f.result = second ? c->d_result2 : result_ptr(c);
  if (c->chain_active) {  // device-driven solve: this finalize advances the machine; results go to the slot's blocks of the ring
    f.result = second ? c->chain_block_g : c->chain_block_a;
    f.chain.sm = &c->d_chain->sm;
    f.chain.x_req = c->d_chain->x_req;
    f.chain.done = &c->d_chain->done;
    f.chain.stage = second ? 1 : 0;
  }
  f.direct = c->adj_direct ? 1 : 0;
  f.nvalid = c->adj_tile_count;
  f.mu_free = 1;
  if (grad == GRAD_BLOCKS) { f.gpartials = c->d_gpartials; f.gblocks = e.gb; }
  else if (grad == GRAD_ROWS) { f.gacc = c->d_gacc; f.gacc_stride = kGaccStride; }
  else if (grad == GRAD_GSUM) { f.gpartials = c->d_gsum; f.gblocks = 1; }  // the (all-reduced) per-parameter sums
  f.gP = grad == GRAD_NONE ? 0 : e.P;
  f.fallback = c->sort.d_fallback;
  if (arm_gate) { f.gate_out = c->d_gate; f.gate_thr = c->gate_thr; f.gate_mode = c->gate_mode; }
  return f;
}

// the image pass for planes that have none yet; builds `f` once the shape of its moment rows is decided.  cost_tailed (the
// cost-only form): the pass may carry the finalize as its tail, and whether it does
static int image_step(cmx_ctx *c, AdjEval &e, GradSums grad, FinalizeArgs &f, bool arm_gate = false, bool *cost_tailed = nullptr) {
  ImgArgs &a = e.ia.img;
  const bool sobel = sobel_adjoint(c);
  claim_partner_clear(c, a);  // (before attach_tiles: it decides its flag memset from a.zero_ptr)
  if (int rc = attach_tiles(c, a, /*may_skip=*/true)) return rc;
  Span sp(c, CMX_T_IMAGE, /*exact=*/true);
  // large panoramas: compact work list (a pre-pass kernel; partial rows become compact too)
  // (not the Sobel pass: it has no list form -- front-end images stay below kTileListMin tiles -- and takes its reach, 2r+2, itself)
  if (!sobel)
    if (int rc = maybe_tile_list(c, a, 2 * c->radius)) return rc;
  c->adj_direct = a.nblk <= 2048 || a.tile_list;  // few entries: finalize sums the per-tile moments itself
  c->adj_tile_count = a.tile_count;
  c->adj_fused = e.fused_rows = false;  // this pass writes d_partials
  f = finalize_args(c, e, grad, /*second=*/false, arm_gate);
  // the three-phase image pass has the registers to carry the finalize as its tail
  // (the five-phase kernel did not: inlined, its taps spilled and the pass went 11 -> 20 us)
  if (cost_tailed && !sobel && e.ia.Mx && c->radius == 4) *cost_tailed = arm_tail(c, f, a.tail);
  if (sobel) launch_image_adjoint_sobel(e.ia, c->stream, sp.t0(), sp.t1());
  else launch_image_adjoint(e.ia, c->stream, sp.t0(), sp.t1());
  if (!c->adj_direct) launch_reduce_partials(f, c->stream);
  return CMX_OK;
}

// ---- gather step.  What the launch carries behind its sums: the finalize as its tail (whole and gated forms), the
// accumulator rows of a split (f.gacc; no counters: accumulators without the tail), or nothing
enum GatherForm { GATHER_WHOLE, GATHER_GATED, GATHER_SPLIT };
static bool gate_fits(const FeGatherArgs &) { return true; }
static bool gate_fits(const BeGatherArgs &g) { return be_gather_folds(g); }  // only the one-kernel form can be gated
// false: no tail available in this configuration, or no gather that fits: no gated pass (the df will run as usual)
template <class GatherArgs> static bool arm_gather(cmx_ctx *c, GatherForm form, FinalizeArgs &f, GatherArgs &g, bool *tailed) {
  if (form != GATHER_SPLIT) *tailed = arm_tail(c, f, g.tail, form == GATHER_GATED);
  else if (f.gacc) g.tail.fin = f;
  if (form != GATHER_GATED) return true;
  if (!*tailed || !gate_fits(g)) return false;
  g.gate = c->d_gate;
  c->gated_pending = true;
  c->gated_launches++;
  return true;
}

static int fe_gather_step(cmx_ctx *c, const AdjEval &e, FinalizeArgs &f, GatherForm form, Span &sp, bool *tailed) {
  FeGatherArgs g{};
  g.ev = fe_args(c, c->last_x);
  g.itilde = c->d_itilde;
  g.gpartials = c->d_gpartials;
  g.cx = c->d_cx; g.cy = c->d_cy; g.r = c->radius;
  if (c->splat_mode == 1 && c->bin_valid && !c->deterministic) {  // tile order: the sorted arrays the LDS splat consumes
    // (deterministic mode: time order -- the order inside a tile depends on the scatter's atomics)
    g.sxy = c->sort.d_sxy;
    g.sbatch = c->sort.d_sbatch;
    if (c->streams_valid) { g.sb = c->d_sb; g.sdt = c->d_sdt; }
  }
  if (!g.sxy && c->d_lut2 && c->n_packed > 0) {  // time-ordered gather: the events' bearings as a stream, once per packet
    if (!c->tb_valid) {
      if (int rc = ensure(c, c->d_tb, c->tb_cap, (size_t)2 * c->n_packed)) return rc;
      launch_bearing_stream(c->d_xy, c->d_lut2, c->W, c->n_packed, c->d_tb, c->stream);
      c->tb_valid = true;
    }
    g.tb = c->d_tb;
  }
  if (c->n_packed > 0) {
    if (arm_gather(c, form, f, g, tailed)) launch_fe_gather(g, c->stream, sp.t0(), sp.t1());
  } else {
    HIP_TRY(c, hipMemsetAsync(c->d_gpartials, 0, (size_t)e.gb * e.P2 * sizeof(double), c->stream));
  }
  return CMX_OK;
}

static int be_gather_step(cmx_ctx *c, const AdjEval &e, FinalizeArgs &f, GatherForm form, Span &sp, bool *tailed) {
  BeGatherArgs g{};
  g.ev = be_args(c);
  g.itilde = c->d_itilde;
  g.P = e.P;
  g.gpartials = c->d_gpartials;
  g.cx = c->d_cx; g.cy = c->d_cy; g.r = c->radius;
  g.vparts = c->d_vparts;
  g.parts_per_batch = e.parts_per_batch;
  g.slice_shift = e.slice_shift;
  g.deterministic = c->deterministic ? 1 : 0;
  g.fold = c->fold_batch ? 1 : 0;
  if (c->d_lut2 && e.slice_shift == 8 && c->n_packed > 0) {  // once per window: the events' bearings in time order
    if (int rc = be_ensure_time_bearings(c)) return rc;
    g.tb = c->d_tb;
  }
  if (c->n_packed > 0 && e.P > 0) {
    if (!arm_gather(c, form, f, g, tailed)) return CMX_OK;
    if (be_gather_folds(g)) {  // one kernel: gather, per-batch pass and finalize
      launch_be_gather(g, c->nb, c->stream, sp.t0(), sp.t1(), nullptr, nullptr);
    } else {
      Span sb(c, CMX_T_BATCH, /*exact=*/true);
      launch_be_gather(g, c->nb, c->stream, sp.t0(), sp.t1(), sb.t0(), sb.t1());
    }
  } else {
    HIP_TRY(c, hipMemsetAsync(c->d_gpartials, 0, (size_t)e.gb * e.P2 * sizeof(double), c->stream));
  }
  return CMX_OK;
}

static int gather_step(cmx_ctx *c, const AdjEval &e, FinalizeArgs &f, GatherForm form, bool *tailed) {
  // (a gated launch may return on its first instruction: it is not a sample of the gather's duration)
  Span sp(c, CMX_T_GATHER, /*exact=*/true, /*enable=*/form != GATHER_GATED);
  return c->kind == KIND_FE ? fe_gather_step(c, e, f, form, sp, tailed) : be_gather_step(c, e, f, form, sp, tailed);
}

// ---- the five forms.  Whole gradient evaluation: image pass unless Jt is resident (a cost-only evaluation of this point, or
// a splat that carried the pass), gather with the finalize as its tail where one is available, else the finalize launch
int adjoint_eval(cmx_ctx *c, int P) {
  AdjEval e;
  FinalizeArgs f{};
  bool tailed = false;  // the gather launch carries the finalize
  if (int rc = adjoint_begin(c, P, e)) return rc;
  if (c->jt_valid) {
    f = finalize_args(c, e, GRAD_BLOCKS);
    if (!c->fused_done) c->spec_hits++;
  } else if (int rc = image_step(c, e, GRAD_BLOCKS, f)) {
    return rc;
  }
  if (int rc = gather_step(c, e, f, GATHER_WHOLE, &tailed)) return rc;
  if (!tailed) issue_finalize(c, f, false);
  HIP_TRY(c, hipGetLastError());
  return CMX_OK;
}

// split evaluation, first half: image pass and gather, up to this rank's partial sums (accumulator rows, or d_gsum: 2P doubles)
int adjoint_partial_sums(cmx_ctx *c, int P) {
  AdjEval e;
  FinalizeArgs f{};
  bool tailed = false;
  if (int rc = adjoint_begin(c, P, e)) return rc;
  const bool rows = acc_rows(c, P);
  if (rows) c->acc_dirty = true;  // until adjoint_finalize_sums has queued its finalize (see begin_accum)
  if (int rc = image_step(c, e, rows ? GRAD_ROWS : GRAD_GSUM, f)) return rc;
  if (int rc = gather_step(c, e, f, GATHER_SPLIT, &tailed)) return rc;
  if (!rows) launch_reduce_gpartials(c->d_gpartials, e.gb, 2 * P, c->d_gsum, c->stream);
  HIP_TRY(c, hipGetLastError());
  return CMX_OK;
}

// ... second half: the finalize, from the (all-reduced) sums
int adjoint_finalize_sums(cmx_ctx *c, int P) {
  AdjEval e;
  if (int rc = adjoint_begin(c, P, e)) return rc;
  e.fused_rows = false;  // the first half ran its own image pass, whatever a splat in between may have left
  FinalizeArgs f = finalize_args(c, e, acc_rows(c, P) ? GRAD_ROWS : GRAD_GSUM);
  issue_finalize(c, f, false);
  HIP_TRY(c, hipGetLastError());
  c->acc_dirty = false;  // that finalize stores the zeros back
  return CMX_OK;
}

// cost only: contrast from the moment rows; Jt and the rows stay for a gradient call at the same point (speculative_jt_ok).
// arm_gate: the finalize also decides whether the pass queued behind it (adjoint_gated_grad) runs
int adjoint_cost_only(cmx_ctx *c, int P, bool arm_gate) {
  AdjEval e;
  FinalizeArgs f{};
  bool tailed = false;  // the image launch carries the finalize
  if (int rc = adjoint_begin(c, P, e)) return rc;
  if (int rc = image_step(c, e, GRAD_NONE, f, arm_gate, &tailed)) return rc;
  if (!tailed) issue_finalize(c, f, false);
  HIP_TRY(c, hipGetLastError());
  c->jt_valid = true;
  c->spec_images++;
  return CMX_OK;
}

// the gradient pass queued behind a cost-only evaluation of the same point: gather + tail finalize into the second result
// block, running only if that evaluation's finalize opens the gate (cmx_hint_next_df).  Sets gated_pending when it could be queued
int adjoint_gated_grad(cmx_ctx *c, int P) {
  if (!c->jt_valid) return CMX_OK;
  AdjEval e;
  bool tailed = false;
  if (int rc = adjoint_begin(c, P, e)) return rc;
  FinalizeArgs f = finalize_args(c, e, GRAD_BLOCKS, /*second=*/true);
  if (int rc = gather_step(c, e, f, GATHER_GATED, &tailed)) return rc;
  if (!c->gated_pending) return CMX_OK;  // given up: nothing was launched
  HIP_TRY(c, hipGetLastError());
  return CMX_OK;
}

// spin on a completion ticket in a mapped result block; true once a consistent snapshot carrying `want` has been read
// (budget_us >= 0: give up after that long -- the caller then blocks in hipStreamSynchronize; -1: the 20 ms safety bound only)
bool spin_for_ticket(const double *h_block, unsigned long long want, int nout, int budget_us) {
  const volatile unsigned long long *w = reinterpret_cast<const volatile unsigned long long *>(h_block);
  const auto t0 = std::chrono::steady_clock::now();
  bool done = false;
  const double limit_ms = budget_us >= 0 ? budget_us * 1e-3 : 20.0;
  const unsigned check = budget_us >= 0 ? 63u : 1023u;
  for (unsigned spins = 0;; spins++) {
    if (w[kTicketSlot] == want) {  // ticket seen: accept only a consistent snapshot of the results
      unsigned long long x = w[kFallbackSlot];
      for (int k = 0; k < nout; k++) x ^= w[k];
      if ((x ^ (want * kTicketMix)) == w[kChecksumSlot]) { done = true; break; }
    }
    __builtin_ia32_pause();
    if ((spins & check) == check &&
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > limit_ms)
      break;
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return done;
}

// the same wait for an evaluation that ends in host records (arm_tail: host finalize); the accepted payloads stay in `r`
static bool spin_for_records(const double *h_block, unsigned long long want, uint64_t expected, int budget_us, HostFinRecords &r) {
  const volatile unsigned long long *recs = reinterpret_cast<const volatile unsigned long long *>(h_block + kHostRecBase);
  const auto t0 = std::chrono::steady_clock::now();
  bool done = false;
  const double limit_ms = budget_us >= 0 ? budget_us * 1e-3 : 20.0;
  const unsigned check = budget_us >= 0 ? 63u : 1023u;
  for (unsigned spins = 0;; spins++) {
    if (hostfin_poll(recs, want, expected, r)) { done = true; break; }
    __builtin_ia32_pause();
    if ((spins & check) == check &&
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > limit_ms)
      break;
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return done;
}

// contrast, mean, gradient and fallback word of such an evaluation into the result block, where the device finalize puts them
static void hostfin_deliver(cmx_ctx *c, const HostFinRecords &r) {
  const HostFinResult o = hostfin_combine(r, c->hostfin_S, c->hostfin_gP, c->hostfin_mu_free, c->hostfin_measure, c->hostfin_npix);
  c->h_result[0] = o.contrast;
  c->h_result[1] = o.mu;
  for (int k = 0; k < c->hostfin_gP; k++) c->h_result[2 + k] = o.grad[k];
  c->h_result[kFallbackSlot] = o.fallback;
  // (ticket and checksum as the device finalize leaves them: the block stays a consistent snapshot of the last evaluation)
  unsigned long long *w = reinterpret_cast<unsigned long long *>(c->h_result);
  unsigned long long x = w[kFallbackSlot];
  for (int k = 0; k < c->ticket_nout; k++) x ^= w[k];
  w[kChecksumSlot] = x ^ (c->hostfin_ticket * kTicketMix);
  w[kTicketSlot] = c->hostfin_ticket;
  c->hostfin_evals++;
}

// the wait of an evaluation whose last launch hands over per-shard sums and the image moments: the finalize step runs here
static int wait_hostfin(cmx_ctx *c, bool *spun) {
  HostFinRecords r;
  const uint64_t expected = hostfin_expected(c->hostfin_G, c->hostfin_S);
  const bool done = c->ticket_wait && spin_for_records(c->h_result, c->ticket_issued, expected, c->spin_eval_us, r);
  *spun = done;
  if (!done) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // the stream is idle: every record must be there
    const volatile unsigned long long *recs = reinterpret_cast<const volatile unsigned long long *>(c->h_result + kHostRecBase);
    if (!hostfin_poll(recs, c->ticket_issued, expected, r)) {
      if (c->d_tail_counters) (void)hipMemsetAsync(c->d_tail_counters, 0, kTailCounterWords * sizeof(unsigned), c->stream);
      if (c->d_gacc) (void)hipMemsetAsync(c->d_gacc, 0, kGaccDoubles * sizeof(double), c->stream);
      c->hostfin_ticket = 0;
      return fail(c, CMX_ERR_HIP, "evaluation ended without its records (ticket %llu, records 0x%llx of 0x%llx)",
                  (unsigned long long)c->ticket_issued, (unsigned long long)r.have, (unsigned long long)expected);
    }
  }
  hostfin_deliver(c, r);
  c->hostfin_ticket = 0;
  return CMX_OK;
}

int sync_and_collect(cmx_ctx *c, bool ends_in_finalize, bool finalize_ran) {
  // ends_in_finalize: the last thing queued on the stream is an evaluation's finalize kernel.  Wait for it through
  // its completion ticket in mapped host memory (a few microseconds earlier than the runtime reports the stream idle);
  // anything slower than the spin budget, and every caller that queued copies or other kernels after the finalize,
  // takes the ordinary stream synchronisation.
  // finalize_ran: a finalize of this call ran, with copies or other kernels queued behind it (a blurred image read-back): once the
  // stream is idle the result block is this call's, fallback word included.
  bool done = false;
  const bool hostfin = ends_in_finalize && c->ticket_issued && c->hostfin_ticket == c->ticket_issued;
  if (hostfin) {
    const int rc = wait_hostfin(c, &done);
    if (rc) return rc;
  } else if (ends_in_finalize && c->ticket_wait && c->ticket_issued) done = spin_for_ticket(c->h_result, c->ticket_issued, c->ticket_nout, c->spin_eval_us);
  if (!done && !hostfin) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (ends_in_finalize && c->ticket_issued) {
      // the stream is idle: the finalize (its own launch, or the tail of the last kernel) must have delivered its ticket
      const volatile unsigned long long *w = reinterpret_cast<const volatile unsigned long long *>(c->h_result);
      if (w[kTicketSlot] != c->ticket_issued) {
        const unsigned long long got = w[kTicketSlot];
        if (c->d_tail_counters) (void)hipMemsetAsync(c->d_tail_counters, 0, kTailCounterWords * sizeof(unsigned), c->stream);
        if (c->d_gacc) (void)hipMemsetAsync(c->d_gacc, 0, kGaccDoubles * sizeof(double), c->stream);
        return fail(c, CMX_ERR_HIP, "evaluation ended without its finalize step (ticket %llu, expected %llu)", got,
                    (unsigned long long)c->ticket_issued);
      }
    }
  }
  if (!c->nchunks_exact && c->bin_valid && c->sort.d_nchunks) {  // once per binning: launch exactly the chunks that exist
    // the kernel that built the table also stored its length in mapped host memory; a kernel queued behind it has delivered
    // its completion ticket by now, so that store has landed (no synchronous read-back: ~10 us per packet)
    int nch = -1;
    if (c->h_nchunks) {
      const unsigned long long w = *reinterpret_cast<volatile unsigned long long *>(c->h_nchunks);
      if ((unsigned)(w >> 32) == c->binning_id) nch = (int)(unsigned)(w & 0xffffffffull);
    }
    if (nch < 0 && hipMemcpy(&nch, c->sort.d_nchunks, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) nch = -1;
    if (nch >= 0 && nch <= c->nchunks) c->nchunks = nch;
    c->nchunks_exact = true;
  }
  if (c->fallback_pending && c->n_packed > 0) {
    if (ends_in_finalize || finalize_ran) {
      c->last_fallback_frac = fallback_count(c->h_result[kFallbackSlot]) / (double)c->n_packed;
      c->last_fallback_flags = fallback_flags(c->h_result[kFallbackSlot]);
    } else {
      // unblurred image read-backs and renders: no finalize of this call has reported the splat's fallback word to the result
      // block, which still holds an earlier evaluation's.  Where these votes went is not known: the next fused evaluation must
      // not take the partner as covered by its tiles' passes (it clears it with the memset)
      c->last_fallback_flags = kFuseUnsafe;
    }
  }
  c->fallback_pending = false;
  // timing spans are resolved lazily (cmx_timing_get) so that timed evaluations wait exactly like untimed ones
  if (c->spans.size() > 4096) {
    if (done) HIP_TRY(c, hipStreamSynchronize(c->stream));
    collect_spans(c);
  }
  return CMX_OK;
}

bool can_reuse(const cmx_ctx *c, const double *x, int n, bool want_grad) {
  if (!want_grad || !c->reuse_image || !c->have_data || !c->accumulated || !c->x_valid) return false;
  if (!adjoint_ok(c) || c->accum_external) return false;
  return memcmp(x, c->last_x, sizeof(double) * (size_t)n) == 0;
}

// ---- gated gradient pass (cmx_hint_next_df).  The FR-CG line search asks for the gradient at the point of a cost-only
// evaluation exactly when that evaluation's cost passes a test it knows beforehand (f < fa on the trial step, !(f >= fa)
// in the bracketing loop, f <= fb in Brent's loop).  With the test handed over in front of the cost-only evaluation, its
// finalize writes the outcome to d_gate and the gradient pass -- queued behind it right away, reporting to the second result
// block -- runs or returns at once.  The df call that follows finds its result in flight instead of starting a launch:
// one host-to-GPU turnaround (~6 us) less per accepted point.
int finish_cost_only_speculative(cmx_ctx *c, int P) {
  const bool want_gate = c->gated_df && c->gate_mode != 0 && !c->sharded() && !c->accum_external && c->ticket_wait;
  c->gated_pending = false;
  int rc = adjoint_cost_only(c, P, /*arm_gate=*/want_gate);
  const int mode = c->gate_mode;
  const double thr = c->gate_thr;
  c->gate_mode = 0;  // the hint is for ONE evaluation
  if (rc) return rc;
  if (want_gate) {
    rc = adjoint_gated_grad(c, P);  // sets gated_pending when the pass could be queued
    if (rc) return rc;
  }
  rc = sync_and_collect(c, true);  // waits for the cost-only finalize's ticket, not for the pass queued behind it
  if (rc) { c->gated_pending = false; return rc; }
  if (c->gated_pending) c->gated_fired = gate_condition(c->h_result[0], thr, mode) != 0;  // the device evaluated the same expression
  return CMX_OK;
}

// gradient evaluation at the point of the last cost-only evaluation: served by the gated pass if one is in flight
int collect_gated(cmx_ctx *c, int P, double *contrast, double *grad, bool *served) {
  *served = false;
  if (!c->gated_pending) return CMX_OK;
  c->gated_pending = false;
  if (!c->gated_fired) return CMX_OK;  // the gate stayed shut (the caller asks anyway): ordinary gradient pass
  bool done = spin_for_ticket(c->h_result2, c->ticket2_issued, c->ticket2_nout, c->spin_eval_us);
  if (!done) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (reinterpret_cast<const unsigned long long *>(c->h_result2)[kTicketSlot] != c->ticket2_issued)
      return CMX_OK;  // the stream is idle and the pass did not report (its gate stayed shut): ordinary gradient pass
  }
  read_result(c, P, contrast, grad, c->h_result2);
  c->gated_hits++;
  c->spec_hits++;
  *served = true;
  return CMX_OK;
}

// ---- three-step finish for sharded adjoint evaluations: begin (image, adjoint blur, gather -> partial gradient
// sums on the device), caller all-reduces cmx_grad_ptr(), end (finalize + read-back)
int finish_begin(cmx_ctx *c, int kind, int want_grad) {
  if (!c || c->kind != kind) return fail(c, CMX_ERR_STATE, "wrong context kind");
  if (!c->accumulated) return fail(c, CMX_ERR_STATE, "finish_begin without accumulate");
  int rc = bind_device(c);
  if (rc) return rc;
  const int P = n_params(c);
  if (kind == KIND_BE) {
    rc = be_first_iter(c);
    if (rc) return rc;
  }
  if (want_grad && c->last_adjoint) {
    rc = adjoint_partial_sums(c, P);
    c->pending_P = P;
  } else {
    if (want_grad && c->last_P != P) return fail(c, CMX_ERR_STATE, "gradient requested but accumulate ran without it");
    rc = run_image_and_finalize(c, want_grad ? P : 0, nullptr, nullptr);
    c->pending_P = -1;  // nothing left to exchange: finish_end only synchronises
  }
  if (rc) return rc;
  c->finish_pending = true;
  return CMX_OK;
}
int finish_end(cmx_ctx *c, int kind, double *contrast, double *grad) {
  if (!c || c->kind != kind) return fail(c, CMX_ERR_STATE, "wrong context kind");
  if (!c->finish_pending) return fail(c, CMX_ERR_STATE, "finish_end without finish_begin");
  if (!contrast) return fail(c, CMX_ERR_INVALID_ARG, "null contrast");
  int rc = bind_device(c);
  if (rc) return rc;
  if (c->pending_P >= 0) {
    rc = adjoint_finalize_sums(c, c->pending_P);
    if (rc) return rc;
  }
  c->finish_pending = false;
  rc = sync_and_collect(c, true);
  if (rc) return rc;
  read_result(c, n_params(c), contrast, grad);
  return CMX_OK;
}
int cmx_frontend_finish_begin(cmx_ctx *c, int want_grad) { return finish_begin(c, KIND_FE, want_grad); }
int cmx_frontend_finish_end(cmx_ctx *c, double *contrast, double *grad) { return finish_end(c, KIND_FE, contrast, grad); }
int cmx_backend_finish_begin(cmx_ctx *c, int want_grad) { CMX_NOT_FOR_GROUPS(c, "the split-phase interface"); return finish_begin(c, KIND_BE, want_grad); }
int cmx_backend_finish_end(cmx_ctx *c, double *contrast, double *grad) { CMX_NOT_FOR_GROUPS(c, "the split-phase interface"); return finish_end(c, KIND_BE, contrast, grad); }
void *cmx_grad_ptr(const cmx_ctx *c) { return c ? c->d_gsum : nullptr; }
size_t cmx_grad_count(const cmx_ctx *c) { return (c && c->finish_pending && c->pending_P > 0) ? (size_t)(2 * c->pending_P) : 0; }
int cmx_set_grad_buffer(cmx_ctx *c, void *device_ptr, size_t n_doubles) {
  if (!c) return CMX_ERR_INVALID_ARG;
  CMX_NOT_FOR_GROUPS(c, "a caller-owned gradient buffer");
  int rc = bind_device(c);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (!c->gsum_external && c->d_gsum) HIP_TRY(c, hipFree(c->d_gsum));
  c->d_gsum = (double *)device_ptr;
  c->gsum_cap = device_ptr ? n_doubles : 0;
  c->gsum_external = device_ptr != nullptr;
  return CMX_OK;
}


// ---- several INDEPENDENT evaluations per call (cmx_*_eval_many): the launch chains of the m evaluations are queued back
// to back on the stream, every finalize writes to its own block of mapped host memory, and the host waits ONCE.  What a
// sequential caller pays per evaluation on top of the kernels -- ticket -> host -> next launch, ~3 us -- disappears, and
// the GPU never idles between evaluations.  For candidate lists (multi-start, grid initialisation, finite-difference
// checks); a line search cannot use it (each trial point depends on the previous result).
static int eval_many(cmx_ctx *c, int kind, int m, const double *xs, double *contrasts, double *grads) {
  if (!c || c->kind != kind) return fail(c, CMX_ERR_STATE, "wrong context kind");
  if (!c->have_data) return fail(c, CMX_ERR_STATE, "no packet / window handed over");
  if (m < 0 || (m > 0 && (!xs || !contrasts))) return fail(c, CMX_ERR_INVALID_ARG, "bad arguments");
  if (c->sharded()) return fail(c, CMX_ERR_STATE, "eval_many is not available with a communicator attached");
  int rc = bind_device(c);
  if (rc) return rc;
  const int n = n_params(c);
  constexpr int kBlock = 4096;  // doubles per evaluation: the layout of the one-evaluation result buffer (slots at its tail)
  if ((size_t)m > c->many_cap) {
    if (c->h_many) HIP_TRY(c, hipHostFree(c->h_many));
    c->h_many = c->d_many = nullptr;
    c->many_cap = 0;
    HIP_TRY(c, hipHostMalloc((void **)&c->h_many, (size_t)m * kBlock * sizeof(double), hipHostMallocMapped));
    HIP_TRY(c, hipHostGetDevicePointer((void **)&c->d_many, c->h_many, 0));
    c->many_cap = (size_t)m;
  }
  const int reuse = c->reuse_image;
  c->reuse_image = 0;  // every evaluation of the list is a full one; no speculative work for a follow-up call
  c->gate_mode = 0;    // (a hint belongs to the ONE cost-only evaluation it was given for)
  c->gated_pending = false;
  for (int i = 0; i < m && rc == CMX_OK; i++) {
    const double *x = xs + (size_t)i * n;
    rc = kind == KIND_FE ? cmx_frontend_accumulate(c, x, grads != nullptr) : cmx_backend_accumulate(c, x, grads != nullptr);
    if (rc) break;
    if (kind == KIND_BE) {
      rc = be_first_iter(c);
      if (rc) break;
    }
    c->result_override = c->d_many + (size_t)i * kBlock;
    if (grads && c->last_adjoint) rc = adjoint_eval(c, n);
    else rc = run_image_and_finalize(c, grads ? n : 0, nullptr, nullptr);
    c->result_override = nullptr;
  }
  c->reuse_image = reuse;
  c->x_valid = false;  // (the resident image belongs to the last point of the list: not worth tracking)
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (rc) return rc;
  HIP_TRY(c, e);
  for (int i = 0; i < m; i++) read_result(c, n, contrasts + i, grads ? grads + (size_t)i * n : nullptr, c->h_many + (size_t)i * kBlock);
  if (m > 0 && c->n_packed > 0 && c->last_used_lds) {
    // the planes hold the votes of the list's LAST point: count and reach flags of that point's block, as sync_and_collect takes them
    const double slot = c->h_many[(size_t)(m - 1) * kBlock + kFallbackSlot];
    c->last_fallback_frac = fallback_count(slot) / (double)c->n_packed;
    c->last_fallback_flags = fallback_flags(slot);
  }
  c->fallback_pending = false;
  return CMX_OK;
}
int cmx_frontend_eval_many(cmx_ctx *c, int m, const double *omegas, double *contrasts, double *grads) {
  UrgentScope urgent(c);
  return eval_many(c, KIND_FE, m, omegas, contrasts, grads);
}
int cmx_backend_eval_many(cmx_ctx *c, int m, const double *drotvs, double *contrasts, double *grads) {
  UrgentScope urgent(c);
  return eval_many(c, KIND_BE, m, drotvs, contrasts, grads);
}

// ---- m DEPENDENT-style evaluations per call (cmx_*_eval_each): exactly m calls of cmx_*_eval, each waited for before the
// next is issued, without returning to the caller in between -- what an optimiser loop written in C/C++ does.  For hosts
// whose own loop is expensive per call (an interpreter): the evaluation sequence of a line search cannot be known in
// advance, but replaying a recorded one, or timing the evaluator without the caller's overhead, can use it.
int cmx_frontend_eval_each(cmx_ctx *c, int m, const double *omegas, double *contrasts, double *grads) {
  UrgentScope urgent(c);
  if (!c || m < 0 || (m > 0 && (!omegas || !contrasts))) return c ? fail(c, CMX_ERR_INVALID_ARG, "bad arguments") : CMX_ERR_INVALID_ARG;
  for (int i = 0; i < m; i++) {
    const int rc = cmx_frontend_eval(c, omegas + 3 * (size_t)i, contrasts + i, grads ? grads + 3 * (size_t)i : nullptr);
    if (rc) return rc;
  }
  return CMX_OK;
}
int cmx_backend_eval_each(cmx_ctx *c, int m, const double *drotvs, double *contrasts, double *grads) {
  UrgentScope urgent(c);
  if (!c || m < 0 || (m > 0 && (!drotvs || !contrasts))) return c ? fail(c, CMX_ERR_INVALID_ARG, "bad arguments") : CMX_ERR_INVALID_ARG;
  const size_t P = (size_t)(c->order > 0 ? 3 * (c->K - c->num_fixed) : 0);
  for (int i = 0; i < m; i++) {
    const int rc = cmx_backend_eval(c, drotvs + P * i, contrasts + i, grads ? grads + P * i : nullptr);
    if (rc) return rc;
  }
  return CMX_OK;
}

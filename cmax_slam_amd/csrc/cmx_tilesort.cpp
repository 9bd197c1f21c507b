// cmx_tilesort.cpp -- the destination-tile sort and its chunk table (TileSort, cmx_tilesort.hpp).  Kernels: cmx_binning.hip.
#include "cmx_context.hpp"

int TileSort::reserve(cmx_ctx *c, int64_t n, int keys, int64_t max_chunks) {
  counting = count_sort_ok(keys + 1);
  if ((size_t)n > cap || !d_keys) {
    // (the pair buffers have the arrays' length: they go with them, and the next sort on the radix route brings them back)
    uint32_t **ptrs[6] = {&d_keys, &d_sxy, &d_sbatch, &d_keys_s, &d_idx, &d_idx_s};
    cap = 0;
    for (int k = 0; k < 6; k++) {
      if (*ptrs[k]) HIP_TRY(c, hipFree(*ptrs[k]));
      *ptrs[k] = nullptr;
    }
    const size_t want = (size_t)(n > 0 ? n : 1);
    for (int k = 0; k < 3; k++) HIP_TRY(c, hipMalloc((void **)ptrs[k], want * sizeof(uint32_t)));
    cap = want;
  }
  int rc = CMX_OK;
  if (counting && n > 0) rc = ensure(c, d_hist, hist_cap, count_sort_scratch_ints((int)n, keys + 1));
  if (!rc) rc = ensure(c, d_tile_start, tile_start_cap, (size_t)keys + 2);
  if (!rc) rc = ensure(c, d_chunks, chunks_cap, (size_t)max_chunks);
  if (rc) return rc;
  if (!d_nchunks) {
    HIP_TRY(c, hipMalloc((void **)&d_nchunks, sizeof(int)));
    HIP_TRY(c, hipMemsetAsync(d_nchunks, 0, sizeof(int), c->stream));
  }
  if (!d_fallback) {
    HIP_TRY(c, hipMalloc((void **)&d_fallback, sizeof(unsigned)));
    HIP_TRY(c, hipMemsetAsync(d_fallback, 0, sizeof(unsigned), c->stream));
  }
  return CMX_OK;
}

int TileSort::run(cmx_ctx *c, const TileSortJob &j) {
  const int n = j.n, keys = j.tiles * j.planes_per_tile;
  if (counting) {
    // counting sort: keys + per-slice histograms, column prefixes, bin scan, scatter (cmx_binning.hip)
    launch_count_sort(j.fe, j.be, j.tiles_x, j.tiles, j.xy, j.per_batch, n, d_keys, d_hist, d_tile_start, d_sxy, d_sbatch, j.sb, j.sdt,
                      c->stream);
  } else {  // more destination tiles than an LDS histogram holds: keys, (key, index) radix sort, permutation, tile offsets
    if (!d_keys_s) {
      uint32_t **ptrs[3] = {&d_keys_s, &d_idx, &d_idx_s};
      for (auto p : ptrs) HIP_TRY(c, hipMalloc((void **)p, cap * sizeof(uint32_t)));
    }
    if (j.fe) launch_fe_bin_keys(*j.fe, j.tiles_x, j.tiles, d_keys, d_idx, c->stream);
    else launch_be_bin_keys(*j.be, j.tiles_x, j.tiles, d_keys, d_idx, c->stream);
    int end_bit = 1;
    while ((1 << end_bit) <= keys) end_bit++;
    size_t tb = 0;
    if (sort_pairs_u32(nullptr, &tb, d_keys, d_keys_s, d_idx, d_idx_s, (unsigned)n, end_bit, c->stream) != 0)
      return fail(c, CMX_ERR_HIP, "rocprim radix sort (size query) failed");
    if (tb > sort_temp_cap || !d_sort_temp) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));  // (a sort queued earlier may still be reading the buffer)
      (void)hipFree(d_sort_temp);
      d_sort_temp = nullptr;
      sort_temp_cap = 0;
      HIP_TRY(c, hipMalloc(&d_sort_temp, tb ? tb : 1));  // (never null: a null buffer would turn the call below into a size query)
      sort_temp_cap = tb;
    }
    if (sort_pairs_u32(d_sort_temp, &tb, d_keys, d_keys_s, d_idx, d_idx_s, (unsigned)n, end_bit, c->stream) != 0)
      return fail(c, CMX_ERR_HIP, "rocprim radix sort failed");
    launch_apply_perm(j.xy, d_idx_s, j.per_batch, n, d_sxy, d_sbatch, c->stream);
    launch_tile_lower_bound(d_keys_s, n, keys + 2, d_tile_start, c->stream);
  }
  // the chunk table is built where the offsets are: no read-back, no host loop, no synchronisation
  launch_build_chunks(d_tile_start, keys, j.planes_per_tile, j.tiles_x, kBinMargin, j.chunk_events, d_chunks, d_nchunks, j.count_host,
                      j.binning_id, c->stream, j.fused);
  HIP_TRY(c, hipGetLastError());
  return CMX_OK;
}

void TileSort::release() {
  void *dev[] = {d_keys, d_sxy, d_sbatch, d_keys_s, d_idx, d_idx_s, d_sort_temp, d_hist, d_tile_start, d_chunks, d_nchunks, d_fallback};
  for (void *p : dev) (void)hipFree(p);
  *this = TileSort{};
}

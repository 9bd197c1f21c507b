// cmx_tilesort.hpp -- TileSort: events sorted by the destination tile of their vote, and the chunk table over the sorted order.
// The ONE owner of the sort's device buffers and the one place the sort is queued (cmx_tilesort.cpp).  A context holds one for
// its window or packet (cmx_ctx::sort, driven by do_binning), a binding of whole-trajectory events another (ReconBound::ts):
// neither touches the other's.
#pragma once
#include "cmx_internal.hpp"

struct cmx_ctx;

// one sort: what the launchers take.  Exactly one of fe / be is set -- the warp that makes the keys; every other pointer is optional.
struct TileSortJob {
  const cmx::FeSplatArgs *fe = nullptr;
  const cmx::BeSplatArgs *be = nullptr;
  int tiles_x = 0, tiles = 0, planes_per_tile = 1;  // the sort-tile grid; keys = tiles x planes_per_tile
  const uint32_t *xy = nullptr;                     // [n] packed events in time order, per_batch slots per batch
  int per_batch = 1, n = 0;
  int chunk_events = 0;                             // events of a full chunk (plan_chunks)
  double *sb = nullptr, *sdt = nullptr;             // counting route: every sorted event's bearing / dt, written along
  unsigned long long *count_host = nullptr;         // mapped host word that receives (binning_id << 32 | table length)
  unsigned binning_id = 0;
  const cmx::FusedTables *fused = nullptr;          // tables of the fused splat + image pass, built with the chunk table
};

struct TileSort {
  uint32_t *d_keys = nullptr, *d_sxy = nullptr, *d_sbatch = nullptr;  // [cap] sort keys; events and batch indices in tile order
  uint32_t *d_keys_s = nullptr, *d_idx = nullptr, *d_idx_s = nullptr; // [cap] radix route: (key, index) pairs, allocated by the first sort that takes it
  size_t cap = 0;
  void *d_sort_temp = nullptr;  // radix route: rocprim's temporary storage
  size_t sort_temp_cap = 0;
  int *d_hist = nullptr;        // counting route scratch: [bin totals | slices x bins prefix table]
  size_t hist_cap = 0;
  int *d_tile_start = nullptr;  // [keys + 2]
  size_t tile_start_cap = 0;
  cmx::Chunk *d_chunks = nullptr;
  size_t chunks_cap = 0;
  int *d_nchunks = nullptr;        // the chunk table's true length
  unsigned *d_fallback = nullptr;  // votes that left their LDS window (counted by the splat / vote kernels)
  bool counting = false;           // route of the sort reserved for: counting sort (the key space fits an LDS histogram) or radix sort

  // everything a sort of n events over `keys` keys with a chunk table of up to max_chunks entries needs, the radix route's pair and
  // temporary buffers excepted.  Buffers of an earlier reserve that are large enough are left alone; a failure leaves them valid.
  int reserve(cmx_ctx *c, int64_t n, int keys, int64_t max_chunks);
  // queue the sort under the job's current parameters, then the chunk table (needs a reserve for at least job.n events, n > 0)
  int run(cmx_ctx *c, const TileSortJob &job);
  void release();
};

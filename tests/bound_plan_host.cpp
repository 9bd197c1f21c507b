// bound_plan_host.cpp -- the host arithmetic of a tile sort's chunk table and of a pass in slices (plan_chunks, slice_batches_of,
// slice_at: cmax_slam_amd/csrc/cmx_ingest.hpp), as the window path, every recon_add* and a binding use it, on its own: no HIP, no
// context, no GPU.
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all tests/bound_plan_host.cpp -o bound_plan_host
// Checks, for batch sizes, sample rates, counts and slice sizes around every edge:
//   - the slices of a pass tile the packed events [0, n_packed) in order, without gap or overlap, each a whole number of batches
//     and none above the slice bound; their ranges of events as handed in tile [0, n) the same way (all but a lone single event,
//     which is in no batch);
//   - the chunk rule with the front end's divisor is the formula the window path's sort had written out;
//   - the chunk table's bound holds for the chunk tables build_chunks can make: random, single-tile, all-in-the-no-window-tile
//     and one-event-per-tile distributions of the events;
//   - at the limits (2^30 events, 2^20 tiles) every quantity fits the 32-bit integers the kernels index with.
// Prints "ok <checks>" and exits 0, or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../cmax_slam_amd/csrc/cmx_ingest.hpp"

using namespace cmx;

static long long checks = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    checks++;                                \
    if (!(cond)) {                           \
      std::fprintf(stderr, "FAILED %s: ", #cond); \
      std::fprintf(stderr, __VA_ARGS__);     \
      std::fprintf(stderr, "\n");            \
      std::exit(1);                          \
    }                                        \
  } while (0)

// chunks build_chunks makes of a tile holding `len` events: full chunks of M and one remainder
static long long chunks_of(long long len, long long M) { return len / M + (len % M ? 1 : 0); }

static void check_slices(int64_t n, int B, int rate, int64_t slice_events) {
  BatchPlan p;
  CHECK(plan_batches(n, B, rate, &p), "n=%lld B=%d", (long long)n, B);
  const int64_t sb = slice_events / B;
  const int slice_batches = (int)(sb < 1 ? 1 : sb);
  CHECK(slice_batches_of(slice_events, B) == slice_batches, "slice=%lld B=%d", (long long)slice_events, B);
  int64_t next = 0, ev_next = 0;
  int slices = 0;
  for (int b_lo = 0; b_lo < p.nb; b_lo += slice_batches, slices++) {
    const Slice s = slice_at(p, n, b_lo, slice_batches);
    CHECK(s.ev_first == ev_next && s.ev_first == (int64_t)b_lo * B, "n=%lld B=%d rate=%d: slice at batch %d starts at event %lld, expected %lld",
          (long long)n, B, rate, b_lo, (long long)s.ev_first, (long long)ev_next);
    CHECK(s.ev_n > 0 && (s.b_hi == p.nb || s.ev_n == (int64_t)(s.b_hi - b_lo) * B), "an inner slice spans whole batches: %lld events",
          (long long)s.ev_n);
    // (the last slice: its batches, and the one event behind a full last batch that no batch holds)
    CHECK(s.b_hi != p.nb || (s.ev_n > (int64_t)(s.b_hi - b_lo - 1) * B && s.ev_n <= (int64_t)(s.b_hi - b_lo) * B + 1),
          "last slice of %lld events over %d batches", (long long)s.ev_n, s.b_hi - b_lo);
    ev_next += s.ev_n;
    CHECK(s.first == next, "n=%lld B=%d rate=%d: slice at batch %d starts at %lld, expected %lld", (long long)n, B, rate, b_lo,
          (long long)s.first, (long long)next);
    CHECK(s.b_hi > b_lo && s.b_hi <= p.nb && s.b_hi - b_lo <= slice_batches, "batches [%d, %d) of %d", b_lo, s.b_hi, p.nb);
    CHECK(s.n > 0 && s.n <= (int64_t)slice_batches * p.per_batch, "slice of %lld events", (long long)s.n);
    CHECK(s.b_hi == p.nb || s.n == (int64_t)(s.b_hi - b_lo) * p.per_batch, "an inner slice holds whole batches");
    next += s.n;
  }
  CHECK(next == p.n_packed, "n=%lld B=%d rate=%d slice=%lld: slices cover %lld of %lld", (long long)n, B, rate, (long long)slice_events,
        (long long)next, (long long)p.n_packed);
  CHECK(p.nb == 0 || slices == (p.nb + slice_batches - 1) / slice_batches, "slice count");
  // the events handed in: [0, n) exactly; a lone event (n == 1) opens no batch and is in no slice
  CHECK(ev_next == (p.nb > 0 ? n : 0) && (p.nb > 0 || n <= 1), "n=%lld B=%d rate=%d slice=%lld: slices span %lld of %lld events", (long long)n,
        B, rate, (long long)slice_events, (long long)ev_next, (long long)n);
}

// the front end's rule as the window path's sort stated it before it became plan_chunks (div = 256, ints)
static void check_front_end_rule(int n, int ntiles) {
  int M = n / 256;
  M = M < 1536 ? 1536 : (M > 32768 ? 32768 : M);
  M = (M + 255) / 256 * 256;
  const int max_chunks = (n / M) + ntiles + 2 + n / 256;
  const ChunkPlan c = plan_chunks(n, ntiles, 256);
  CHECK(c.chunk_events == M && c.max_chunks == max_chunks, "n=%d tiles=%d: %d / %lld, expected %d / %d", n, ntiles, c.chunk_events,
        (long long)c.max_chunks, M, max_chunks);
}

static void check_chunk_bound(int64_t n, int64_t keys, std::mt19937_64 &rng) {
  const ChunkPlan b = plan_chunks(n, keys, 768);
  CHECK(kBackEndChunkDiv == 768, "back-end divisor %d", kBackEndChunkDiv);
  CHECK(b.chunk_events % 256 == 0 && b.chunk_events >= 1536 && b.chunk_events <= 32768, "chunk of %d events", b.chunk_events);
  const long long M = b.chunk_events, Ms = M < 256 ? M : 256;
  // everything in one tile; everything in the no-window tile; one event per tile as far as they go; random
  CHECK(chunks_of(n, M) <= b.max_chunks, "one tile: n=%lld", (long long)n);
  CHECK(chunks_of(n, Ms) <= b.max_chunks, "no-window tile: n=%lld needs %lld, bound %lld", (long long)n, chunks_of(n, Ms), (long long)b.max_chunks);
  const long long spread = n < keys ? n : keys;
  CHECK(spread + chunks_of(n - spread, Ms) <= b.max_chunks, "spread: n=%lld keys=%lld", (long long)n, (long long)keys);
  if (keys <= 1 << 16) {
    for (int trial = 0; trial < 4; trial++) {
      std::vector<long long> len((size_t)keys + 1, 0);
      long long left = n;
      for (size_t t = 0; t <= (size_t)keys && left > 0; t++) {
        const long long take = t == (size_t)keys ? left : (long long)(rng() % (unsigned long long)(2 * left / (keys + 1 - (long long)t) + 2));
        len[t] = take < left ? take : left;
        left -= len[t];
      }
      len[(size_t)keys] += left;
      long long total = 0;
      for (size_t t = 0; t <= (size_t)keys; t++) total += chunks_of(len[t], t == (size_t)keys ? Ms : M);
      CHECK(total <= b.max_chunks, "random tiles: n=%lld keys=%lld needs %lld, bound %lld", (long long)n, (long long)keys, total,
            (long long)b.max_chunks);
    }
  }
}

int main() {
  std::mt19937_64 rng(12345);
  const int64_t counts[] = {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 999, 1000, 1001, 4999, 5000, 5001, 12345, 60007, 1000003};
  const int batches[] = {1, 2, 3, 64, 100, 5000};
  const int rates[] = {1, 2, 3, 7, 100};
  const int64_t slices[] = {1, 64, 1000, 4096, 1 << 22};
  for (int64_t n : counts)
    for (int B : batches)
      for (int rate : rates)
        for (int64_t s : slices) check_slices(n, B, rate, s);
  check_slices(1LL << 30, 100, 1, 1 << 22);
  check_slices(1LL << 30, 1 << 30, 1, 1 << 22);  // one batch as long as the limit: one slice
  check_slices((1LL << 30) - 1, 1, 1, 1 << 30);
  const int64_t keys[] = {2, 8, 16, 512, 2048, 16384, 16514};
  for (int64_t n : counts)
    for (int64_t k : keys)
      if (n > 0) check_chunk_bound(n, k, rng);
  check_chunk_bound(20000000, 16384, rng);
  check_chunk_bound(1LL << 30, 1LL << 21, rng);
  // around the 1536 floor (n / 256 = 1535 | 1536) and the 32768 cap (8 388 608 = 256 x 32768) of the front end's divisor
  const int fe_counts[] = {0, 1, 393215, 393216, 1000000, 8388608, 1 << 30};
  const int fe_tiles[] = {1, 12, 300, 16514};
  for (int n : fe_counts)
    for (int t : fe_tiles) check_front_end_rule(n, t);
  // the limits: 2^30 sampled events over the 2 x 2^20 keys of the largest panorama
  const ChunkPlan big = plan_chunks(1LL << 30, 1LL << 21, kBackEndChunkDiv);
  CHECK(big.max_chunks < (1LL << 31), "chunk bound %lld does not fit an int", (long long)big.max_chunks);
  BatchPlan p;
  CHECK(plan_batches(1LL << 30, 1, 1, &p) && p.n_packed == (1LL << 30) - 1 && p.nb == (1 << 30) - 1, "batches of one event");
  std::printf("ok %lld\n", checks);
  return 0;
}

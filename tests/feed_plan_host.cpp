// feed_plan_host.cpp -- the slice planner of cmx_backend_recon_add* / _grad_add* / _warp* (feed_slice_at:
// cmax_slam_amd/csrc/cmx_ingest.hpp) on its own: no HIP, no context, no GPU.
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all tests/feed_plan_host.cpp -o feed_plan_host
// Every n in 0 .. 3 B + 2 with B in {1, 3, 64}, rates 1 to 3, 1, 2 and 7 batches per slice, in both modes -- a sampling pass (votes,
// gradient) and "every event, lone tail included" (the export) -- against a brute-force enumeration of the reference's batch loop,
//   for (beg = 0; beg < n - 1; beg += B) { end = (n - beg > B) ? beg + B : n; }  every rate-th event from beg:
//   - the slices' batch ranges tile [0, nb) in order, none empty, none longer than the slice size;
//   - the event ranges tile [0, n) exactly once (in the sampling mode too: the batch-time pass cuts the last batch by them),
//     each starts at its first batch, and a slice of batches only holds whole ones;
//   - the lone event n = nb B + 1 rides on the last slice of the export alone, as its last element, and on none of a sampling pass;
//   - n == 1 is one slice of zero batches for the export and no slice for a sampling pass; n == 0 gives no slice;
//   - the packed ranges are the brute-force counts, equal BatchPlan::packed, follow each other and sum to n_packed.
// Prints "ok <checks>" and exits 0, or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cmax_slam_amd/csrc/cmx_ingest.hpp"

using namespace cmx;

static long long checks = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    checks++;                                     \
    if (!(cond)) {                                \
      std::fprintf(stderr, "FAILED %s: ", #cond); \
      std::fprintf(stderr, __VA_ARGS__);          \
      std::fprintf(stderr, "\n");                 \
      std::exit(1);                               \
    }                                             \
  } while (0)

struct Batch {
  int64_t beg, end, sampled;
};

int main() {
  long long slices = 0, lone_slices = 0, short_last = 0;
  for (int B : {1, 3, 64})
    for (int rate : {1, 2, 3})
      for (int sb : {1, 2, 7})
        for (int every = 0; every < 2; every++)
          for (int64_t n = 0; n <= 3 * (int64_t)B + 2; n++) {
#define WHERE "B=%d rate=%d slice_batches=%d every=%d n=%lld k=%lld", B, rate, sb, every, (long long)n, (long long)k
            // brute force: the batches, and how many events of each the sampling takes
            std::vector<Batch> bat;
            int64_t sampled_all = 0;
            for (int64_t beg = 0; beg < n - 1; beg += B) {
              const int64_t end = (n - beg > B) ? beg + B : n;
              int64_t cnt = 0;
              for (int64_t i = beg; i < end; i += rate) cnt++;
              bat.push_back(Batch{beg, end, cnt});
              sampled_all += cnt;
            }
            const int nb = (int)bat.size();
            const bool lone = nb > 0 ? bat.back().end < n : n == 1;  // an event behind the last batch
            BatchPlan p;
            int64_t k = 0;
            CHECK(plan_batches(n, B, rate, &p) && p.nb == nb && p.n_packed == sampled_all, WHERE);
            if (nb > 0 && bat.back().end - bat.back().beg < B) short_last++;
            std::vector<int> ev_seen((size_t)n, 0);
            int b_next = 0, lone_seen = 0;
            int64_t ev_next = 0, packed_next = 0, packed_sum = 0;
            FeedSlice f;
            for (; feed_slice_at(p, n, sb, every != 0, k, &f); k++) {
              slices++;
              CHECK(f.b_lo == b_next && f.b_hi <= nb, WHERE);
              CHECK(f.ev_first == ev_next && f.ev_n > 0 && f.ev_first + f.ev_n <= n, WHERE);
              for (int64_t i = f.ev_first; i < f.ev_first + f.ev_n; i++) ev_seen[(size_t)i]++;
              const bool last = f.b_hi == nb;
              if (nb == 0) {  // the degenerate slice of the export: the lone event alone
                CHECK(every && n == 1 && k == 0 && f.b_lo == 0 && f.b_hi == 0 && f.ev_n == 1 && f.n == 0 && f.lone, WHERE);
              } else {
                CHECK(f.b_hi > f.b_lo && f.b_hi - f.b_lo <= sb && (last || f.b_hi - f.b_lo == sb), WHERE);
                CHECK(f.ev_first == bat[(size_t)f.b_lo].beg, WHERE);
                CHECK(f.ev_first + f.ev_n == (last ? n : bat[(size_t)f.b_hi].beg), WHERE);
                int64_t want = 0;
                for (int b = f.b_lo; b < f.b_hi; b++) want += bat[(size_t)b].sampled;
                CHECK(f.n == want && f.n == p.packed(f.b_lo, f.b_hi), WHERE);
                CHECK(f.first == packed_next && f.first == (int64_t)f.b_lo * p.per_batch, WHERE);
                CHECK(f.lone == (every && last && lone), WHERE);
              }
              if (f.lone) {
                lone_seen++;
                lone_slices++;
                CHECK(f.ev_first + f.ev_n == n && last, WHERE);  // the slice's last element is the call's last event
              }
              b_next = f.b_hi;
              ev_next = f.ev_first + f.ev_n;
              packed_next = f.first + (int64_t)(f.b_hi - f.b_lo) * p.per_batch;
              packed_sum += f.n;
            }
            CHECK(!feed_slice_at(p, n, sb, every != 0, k + 1, &f), WHERE);  // behind the last: nothing, again
            CHECK(b_next == nb, WHERE);
            CHECK(packed_sum == p.n_packed, WHERE);
            CHECK(lone_seen == (every && lone ? 1 : 0), WHERE);
            if (n == 0) CHECK(k == 0, WHERE);
            if (n == 1) CHECK(k == (every ? 1 : 0), WHERE);
            if (nb > 0) CHECK(k == (nb + sb - 1) / sb, WHERE);
            if (nb > 0 || every) {
              CHECK(ev_next == n, WHERE);
              for (int64_t i = 0; i < n; i++) CHECK(ev_seen[(size_t)i] == 1, WHERE);
            }
#undef WHERE
          }
  CHECK(lone_slices > 0 && short_last > 0, "cases met: %lld lone events, %lld short last batches", lone_slices, short_last);
  std::printf("ok %lld (%lld slices, %lld with a lone event, %lld plans with a short last batch)\n", checks, slices, lone_slices, short_last);
  return 0;
}

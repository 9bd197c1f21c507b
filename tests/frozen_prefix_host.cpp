// frozen_prefix_host.cpp -- the prefix rule of a frozen head (frozen_prefix, batch_is_frozen: cmax_slam_amd/csrc/cmx_ingest.hpp)
// on its own: no HIP, no context, no GPU.
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all tests/frozen_prefix_host.cpp -o frozen_prefix_host
// Against a brute-force loop that, per batch, walks the knots its pose reads and asks whether every one of them is fixed:
//   - orders 2 and 4, num_fixed in {0, order - 1, order, K - 1}, over dense, sparse and clustered batch times;
//   - a batch time exactly on a knot boundary (it belongs to the segment that STARTS there), and one nanosecond before it;
//   - a recording that ends before the first free knot's support: b_act = nb;
//   - one batch; zero batches (a null table);
//   - the last segment's clamp (a batch time at the very end of the support);
//   - the cut of a batch plan at b_act: the head is packed(0, b_act) events, and slice_at's slices from b_act on (the gather pass
//     of a frozen evaluation) tile the rest exactly.
// Prints "ok <checks>" and exits 0, or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <random>
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

// is every knot the pose at t reads among the first num_fixed?  Written from the spline's definition, knot by knot.
static bool brute_frozen(const KnotSupport &sup, int num_fixed, long long t) {
  long long s = (t - sup.start_ns) / sup.dt_ns;
  if (s > sup.K - sup.order) s = sup.K - sup.order;  // the kernels' clamp: the last segment also serves t = end of support
  if (s < 0) s = 0;
  for (long long k = s; k < s + sup.order; k++)
    if (k >= num_fixed) return false;
  return true;
}

static void check_times(const KnotSupport &sup, int num_fixed, const std::vector<long long> &bt, const char *what) {
  const int nb = (int)bt.size();
  int want = 0;
  while (want < nb && brute_frozen(sup, num_fixed, bt[(size_t)want])) want++;
  const int got = frozen_prefix(sup, num_fixed, nb ? bt.data() : nullptr, nb);
  CHECK(got == want, "%s: order %d K %d num_fixed %d nb %d: b_act %d, brute force %d", what, sup.order, sup.K, num_fixed, nb, got, want);
  CHECK(got >= 0 && got <= nb, "%s: b_act %d outside [0, %d]", what, got, nb);
  for (int b = 0; b < nb; b++) {
    CHECK(batch_is_frozen(sup, num_fixed, bt[(size_t)b]) == brute_frozen(sup, num_fixed, bt[(size_t)b]), "%s: batch %d", what, b);
    // times that do not decrease: the frozen batches ARE the prefix
    if (b >= got) CHECK(!brute_frozen(sup, num_fixed, bt[(size_t)b]), "%s: batch %d behind b_act %d is frozen", what, b, got);
  }
  if (num_fixed == 0 || num_fixed == sup.order - 1) CHECK(got == 0, "%s: num_fixed %d freezes %d batches", what, num_fixed, got);
}

static void check_slices(int64_t n, int B, int rate, int64_t slice_events, int b_act) {
  BatchPlan p;
  CHECK(plan_batches(n, B, rate, &p), "n=%lld B=%d", (long long)n, B);
  if (b_act > p.nb) b_act = p.nb;
  const int slice_batches = slice_batches_of(slice_events, B);
  // the frozen head is the packed events [0, packed(0, b_act)): whole batches in front of an active one, everything otherwise
  const int64_t next = p.packed(0, b_act);
  CHECK(next == (b_act < p.nb ? (int64_t)b_act * p.per_batch : p.n_packed), "n=%lld B=%d rate=%d b_act=%d: head of %lld events", (long long)n, B,
        rate, b_act, (long long)next);
  // the active part behind it, in slice_at's slices from b_act on (the gather pass of a frozen evaluation): the rest, exactly
  int64_t rest = 0;
  for (int b_lo = b_act; b_lo < p.nb; b_lo += slice_batches) {
    const Slice s = slice_at(p, n, b_lo, slice_batches);
    CHECK(s.first == p.packed(0, b_act) + rest, "active slice at batch %d", b_lo);
    rest += s.n;
  }
  CHECK(next + rest == p.n_packed, "head %lld + active %lld != %lld", (long long)next, (long long)rest, (long long)p.n_packed);
}

int main() {
  std::mt19937_64 rng(777);
  const long long start = 1000000007LL, dt = 50000000LL;  // (a start that is no multiple of dt)
  for (int order : {2, 4}) {
    for (int K : {order, order + 1, 12, 401}) {
      const KnotSupport sup{order, K, start, dt};
      const long long span = (long long)(K - order + 1) * dt;  // the support is [start, start + span)
      int fixed_set[] = {0, order - 1, order, K - 1};
      for (int num_fixed : fixed_set) {
        if (num_fixed < 0 || num_fixed >= K) continue;
        // dense: a few batches per knot interval, from the first nanosecond to the last
        std::vector<long long> bt;
        for (long long t = start; t < start + span; t += dt / 3 + 1) bt.push_back(t);
        bt.push_back(start + span - 1);
        check_times(sup, num_fixed, bt, "dense");
        // exactly on every knot boundary, and one nanosecond before it
        bt.clear();
        for (int j = 0; j <= K - order; j++) {
          if (j > 0) bt.push_back(start + (long long)j * dt - 1);
          bt.push_back(start + (long long)j * dt);
        }
        check_times(sup, num_fixed, bt, "on the boundaries");
        // the boundary that decides: the first segment with a free knot starts at s = num_fixed - order + 1
        const long long s_free = num_fixed - order + 1;
        if (s_free > 0 && s_free <= K - order) {
          const long long t_free = start + s_free * dt;
          CHECK(!batch_is_frozen(sup, num_fixed, t_free), "order %d K %d num_fixed %d: a batch ON the boundary reads knot %d", order, K,
                num_fixed, num_fixed);
          CHECK(batch_is_frozen(sup, num_fixed, t_free - 1), "order %d K %d num_fixed %d: a batch one ns before the boundary is frozen", order,
                K, num_fixed);
          // a recording that ends before the first free knot's support: everything is frozen
          bt.clear();
          for (long long t = start; t < t_free; t += dt / 7 + 3) bt.push_back(t);
          check_times(sup, num_fixed, bt, "ends before the free knots");
          CHECK(frozen_prefix(sup, num_fixed, bt.data(), (int)bt.size()) == (int)bt.size(), "order %d K %d num_fixed %d: not all frozen", order,
                K, num_fixed);
          // one batch: on either side of the boundary
          check_times(sup, num_fixed, {t_free - 1}, "one batch, frozen");
          check_times(sup, num_fixed, {t_free}, "one batch, active");
        }
        // the very end of the support (segment K - order + 1 before the clamp) and one batch at the start
        check_times(sup, num_fixed, {start + span}, "end of the support");
        check_times(sup, num_fixed, {start}, "one batch at the start");
        // zero batches
        check_times(sup, num_fixed, {}, "zero batches");
        CHECK(frozen_prefix(sup, num_fixed, nullptr, 0) == 0, "zero batches, null table");
        // random non-decreasing times, with repeats
        for (int trial = 0; trial < 8; trial++) {
          bt.clear();
          long long t = start;
          while (t < start + span) {
            bt.push_back(t);
            t += (long long)(rng() % (unsigned long long)(trial < 4 ? dt / 2 : 3 * dt));
          }
          check_times(sup, num_fixed, bt, "random");
        }
      }
    }
  }
  // the cut of a plan at b_act
  const int64_t counts[] = {0, 1, 2, 3, 64, 65, 999, 1001, 5001, 60007};
  const int batches[] = {1, 3, 100, 5000};
  const int rates[] = {1, 3, 7};
  const int64_t slices[] = {1, 64, 1000, 1 << 22};
  for (int64_t n : counts)
    for (int B : batches)
      for (int rate : rates)
        for (int64_t s : slices)
          for (int b_act : {0, 1, 2, 7, 100, 1 << 30}) check_slices(n, B, rate, s, b_act);
  std::printf("ok %lld\n", checks);
  return 0;
}

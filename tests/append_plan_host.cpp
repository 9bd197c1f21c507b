// append_plan_host.cpp -- the planner of cmx_backend_recon_bind_append_from (plan_append, open_tail_from:
// cmax_slam_amd/csrc/cmx_ingest.hpp) on its own: no HIP, no context, no GPU.
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all tests/append_plan_host.cpp -o append_plan_host
// A binding is replayed on the host the way the library keeps it on the device -- the packed events, the batch times, and the raw
// events of the open tail ALONE -- and grown by plan_append: the scratch stream "kept tail ++ new range" goes through the one
// packing pass and the one batch-time pass, and lands where the plan says.  After every append the result is compared with a
// brute-force plan, pack and batch-time pass over the concatenation of everything bound so far:
//   - B in {1, 3, 64, 5000}, rates 1 to 3;
//   - a binding of 0, 1 and 2 events, and of B - 1, B, B + 1 and 2 B + 1;
//   - appends of 0, 1, B - 1, B and B + 1 events, several in a row, so that every kind of open tail (none, a short batch, a lone
//     trailing event) meets every kind of append;
//   - the kept tail never exceeds B events, and the events in front of it are not kept at all: an append cannot read them.
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

constexpr unsigned kW = 256, kH = 256;

struct Stream {
  std::vector<uint16_t> x, y;
  std::vector<int64_t> t;
  EvSoa view() const { return EvSoa{x.data(), y.data(), t.data()}; }
  int64_t size() const { return (int64_t)t.size(); }
  void push(uint16_t ex, uint16_t ey, int64_t et) { x.push_back(ex); y.push_back(ey); t.push_back(et); }
};

// what the library keeps of a binding
struct Binding {
  int64_t n = 0;
  BatchPlan plan;
  std::vector<uint32_t> xy;    // packed, time order
  std::vector<long long> bt;   // batch times
  Stream tail;                 // raw events of the open tail
};

// plan, pack and batch times of a whole stream: bind_from
static void brute(const Stream &s, int B, int rate, Binding *b) {
  b->n = s.size();
  CHECK(plan_batches(b->n, B, rate, &b->plan), "n=%lld", (long long)b->n);
  b->xy.assign((size_t)b->plan.n_packed, 0xdeadbeefu);
  b->bt.assign((size_t)b->plan.nb, -1);
  if (b->plan.nb == 0) return;
  CHECK(pack_events<false>(s.view(), b->n, b->plan.nb, B, rate, kW, kH, 0, b->xy.data()) == 0, "an event outside the sensor");
  const BatchTimeError e = batch_times(s.view(), b->n, B, 0, b->plan.nb, nullptr, [&](int64_t j, long long tb) { b->bt[(size_t)j] = tb; });
  CHECK(e.kind == CMX_OK, "batch times");
}

static void keep_tail(const Stream &s, int64_t from, Stream *tail) {
  Stream t;
  for (int64_t i = from; i < s.size(); i++) t.push(s.x[(size_t)i], s.y[(size_t)i], s.t[(size_t)i]);
  *tail = t;
}

// one append of `add` to the binding, by the plan
static void append(Binding *b, const Stream &add, int B, int rate) {
  AppendPlan ap;
  CHECK(plan_append(b->n, add.size(), B, rate, &ap), "plan_append");
  CHECK(ap.keep_from == (int64_t)ap.b_recut * B && ap.tail_n == b->n - ap.keep_from, "the open tail starts on a batch cut");
  CHECK(ap.tail_n >= 0 && ap.tail_n <= B, "a tail of %lld events, B = %d", (long long)ap.tail_n, B);
  CHECK(ap.tail_n == b->tail.size(), "the binding kept %lld raw events, the plan wants %lld", (long long)b->tail.size(), (long long)ap.tail_n);
  CHECK(ap.b_recut <= b->plan.nb && ap.b_recut >= b->plan.nb - 1, "batch %d is cut again, of %d", ap.b_recut, b->plan.nb);
  CHECK(ap.packed_at == b->plan.packed(0, ap.b_recut) || ap.b_recut == b->plan.nb, "packed_at");
  CHECK(ap.packed_at == (int64_t)ap.b_recut * b->plan.per_batch, "packed_at is a whole number of batches");
  // the new plan is the scratch plan behind the closed batches
  CHECK(ap.plan.nb == ap.b_recut + ap.scratch.nb, "nb %d != %d + %d", ap.plan.nb, ap.b_recut, ap.scratch.nb);
  CHECK(ap.plan.n_packed == ap.packed_at + ap.scratch.n_packed || ap.scratch.nb == 0, "n_packed");
  if (ap.scratch.nb == 0) CHECK(ap.plan.nb == ap.b_recut && ap.plan.n_packed == b->plan.n_packed, "nothing new to pack");
  // the scratch stream: kept tail ++ new range -- nothing else of the bound events is read
  Stream scr = b->tail;
  for (int64_t i = 0; i < add.size(); i++) scr.push(add.x[(size_t)i], add.y[(size_t)i], add.t[(size_t)i]);
  CHECK(scr.size() == ap.tail_n + add.size() && scr.size() <= add.size() + B, "scratch of %lld events", (long long)scr.size());
  b->xy.resize((size_t)ap.plan.n_packed, 0xdeadbeefu);
  b->bt.resize((size_t)ap.plan.nb, -1);
  if (ap.scratch.nb > 0) {
    CHECK((size_t)(ap.packed_at + ap.scratch.n_packed) <= b->xy.size(), "the packed events land inside the buffer");
    pack_events<false>(scr.view(), scr.size(), ap.scratch.nb, B, rate, kW, kH, 0, b->xy.data() + ap.packed_at);
    batch_times(scr.view(), scr.size(), B, 0, ap.scratch.nb, nullptr, [&](int64_t j, long long tb) { b->bt[(size_t)(ap.b_recut + j)] = tb; });
  }
  const int64_t n_new = b->n + add.size();
  const int64_t from = open_tail_from(n_new, ap.plan);
  CHECK(from >= ap.keep_from && from <= n_new && n_new - from <= B, "the next tail [%lld, %lld)", (long long)from, (long long)n_new);
  keep_tail(scr, from - ap.keep_from, &b->tail);
  b->n = n_new;
  b->plan = ap.plan;
}

static void same(const Binding &got, const Binding &want, const char *what, int B, int rate) {
  CHECK(got.n == want.n, "%s B=%d rate=%d: n", what, B, rate);
  CHECK(got.plan.nb == want.plan.nb && got.plan.n_packed == want.plan.n_packed && got.plan.last_len == want.plan.last_len &&
            got.plan.per_batch == want.plan.per_batch,
        "%s B=%d rate=%d n=%lld: plan nb %d / %d, packed %lld / %lld, last %lld / %lld", what, B, rate, (long long)got.n, got.plan.nb,
        want.plan.nb, (long long)got.plan.n_packed, (long long)want.plan.n_packed, (long long)got.plan.last_len, (long long)want.plan.last_len);
  CHECK(got.xy == want.xy, "%s B=%d rate=%d n=%lld: packed events differ", what, B, rate, (long long)got.n);
  CHECK(got.bt == want.bt, "%s B=%d rate=%d n=%lld: batch times differ", what, B, rate, (long long)got.n);
}

int main() {
  std::mt19937_64 rng(4242);
  long long appends = 0, recut_short = 0, recut_lone = 0, recut_none = 0;
  for (int B : {1, 3, 64, 5000}) {
    for (int rate : {1, 2, 3}) {
      const int64_t firsts[] = {0, 1, 2, B - 1, B, B + 1, 2 * (int64_t)B + 1};
      const int64_t adds[] = {0, 1, B - 1, B, B + 1};
      for (int64_t n0 : firsts) {
        if (n0 < 0) continue;
        for (int64_t a0 : adds)
          for (int64_t a1 : adds)
            for (int64_t a2 : {(int64_t)0, (int64_t)1, (int64_t)B + 1}) {
              if (a0 < 0 || a1 < 0) continue;
              // the whole stream: non-decreasing times with repeats, every event its own (x, y)
              Stream all;
              int64_t t = 1000000007LL;
              const int64_t total = n0 + a0 + a1 + a2;
              for (int64_t i = 0; i < total; i++) {
                t += (int64_t)(rng() % 3) * 1000;
                all.push((uint16_t)(i % kW), (uint16_t)((i / kW) % kH), t);
              }
              auto range = [&](int64_t lo, int64_t n) {
                Stream s;
                for (int64_t i = lo; i < lo + n; i++) s.push(all.x[(size_t)i], all.y[(size_t)i], all.t[(size_t)i]);
                return s;
              };
              Binding got;
              const Stream first = range(0, n0);
              brute(first, B, rate, &got);
              keep_tail(first, open_tail_from(n0, got.plan), &got.tail);
              int64_t done = n0;
              for (int64_t a : {a0, a1, a2}) {
                const int64_t tail = got.tail.size();
                (tail == 0 ? recut_none : (got.plan.nb > 0 && tail == got.plan.last_len && tail < B ? recut_short : recut_lone))++;
                append(&got, range(done, a), B, rate);
                done += a;
                Binding want;
                brute(range(0, done), B, rate, &want);
                same(got, want, "append", B, rate);
                appends++;
              }
            }
      }
    }
  }
  CHECK(recut_short > 0 && recut_lone > 0 && recut_none > 0, "kinds of open tail met: %lld short, %lld lone, %lld none", recut_short, recut_lone,
        recut_none);
  std::printf("ok %lld (%lld appends: %lld on a short batch, %lld on a lone event, %lld on none)\n", checks, appends, recut_short, recut_lone,
              recut_none);
  return 0;
}

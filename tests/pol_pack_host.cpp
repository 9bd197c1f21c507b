// pol_pack_host.cpp -- the host packing WITH polarity (cmax_slam_amd/csrc/cmx_ingest.hpp) on its own: no HIP, no context, no GPU.
//   g++ -O2 -std=c++17 -pthread tests/pol_pack_host.cpp -o pol_pack_host      (and once more with -fsanitize=address,undefined)
//   pol_pack_host CASE_IN CASE_OUT
// CASE_IN : 12 int64 {n, B, rate, W, H, stride, off_x, off_y, off_sec, off_nsec, off_polarity, slice_batches}, then x[n], y[n]
//           (uint16), t[n] (int64), pol[n] (uint8) and the same events as n records of `stride` bytes.
// CASE_OUT: int64 arrays, each behind its length, in the order main() writes them (tests/test_pol_pack_cpu.py reads them back).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cmax_slam_amd/csrc/cmx_hostpool.hpp"
#include "../cmax_slam_amd/csrc/cmx_ingest.hpp"
#include "../include/cmax_hip.h"

using namespace cmx;

static FILE *g_out = nullptr;
template <typename T>
static void put(const std::vector<T> &v) {
  const int64_t n = (int64_t)v.size();
  fwrite(&n, sizeof(n), 1, g_out);
  for (const T &e : v) {
    const int64_t w = (int64_t)e;
    fwrite(&w, sizeof(w), 1, g_out);
  }
}
static void put(std::initializer_list<int64_t> v) { put(std::vector<int64_t>(v)); }
template <typename T>
static bool get(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s CASE_IN CASE_OUT\n", argv[0]); return 2; }
  FILE *in = fopen(argv[1], "rb");
  std::vector<int64_t> h, t;
  std::vector<uint16_t> x, y;
  std::vector<uint8_t> pol;
  std::vector<unsigned char> rec;
  if (!in || !get(in, h, 12)) { fprintf(stderr, "cannot read the header of %s\n", argv[1]); return 2; }
  const int64_t n = h[0];
  const int B = (int)h[1], rate = (int)h[2], slice_batches = (int)h[11];
  const unsigned W = (unsigned)h[3], H = (unsigned)h[4];
  const cmx_aos_layout layout{(size_t)h[5], (size_t)h[6], (size_t)h[7], (size_t)h[8], (size_t)h[9]};
  const size_t off_pol = (size_t)h[10];
  if (!get(in, x, (size_t)n) || !get(in, y, (size_t)n) || !get(in, t, (size_t)n) || !get(in, pol, (size_t)n) ||
      !get(in, rec, (size_t)n * layout.stride)) {
    fprintf(stderr, "%s is shorter than its header says\n", argv[1]);
    return 2;
  }
  fclose(in);
  g_out = fopen(argv[2], "wb");
  if (!g_out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }

  const EvSoa soa{x.data(), y.data(), t.data(), pol.data()};
  EvAos aos, bad;
  const bool layout_ok = aos_view_pol(rec.data(), &layout, off_pol, &aos);
  // a polarity byte outside the record is refused, inside its last byte accepted
  put({layout_ok, aos_view_pol(rec.data(), &layout, layout.stride, &bad), aos_view_pol(rec.data(), &layout, layout.stride - 1, &bad)});
  if (!layout_ok) { fclose(g_out); return 0; }

  BatchPlan p;
  if (!plan_batches(n, B, rate, &p)) return 3;
  put({p.nb, p.n_packed});

  // the packed words with the polarity in bit 31, SoA and AoS view; and without it through the same views (bit 31 stays clear)
  {
    std::vector<uint32_t> ws((size_t)p.n_packed, 0xdeadbeefu), wa((size_t)p.n_packed, 0xdeadbeefu), plain((size_t)p.n_packed, 0xdeadbeefu);
    const unsigned os = pack_events<false, true>(soa, n, p.nb, B, rate, W, H, 0, ws.data());
    const unsigned oa = pack_events<false, true>(aos, n, p.nb, B, rate, W, H, 0, wa.data());
    const unsigned op = pack_events<false>(aos, n, p.nb, B, rate, W, H, 0, plain.data());
    put({os != 0, oa != 0, op != 0});
    put(ws);
    put(wa);
    put(plain);
  }
  // ... slice by slice, as the reconstruction's feeder packs a long input
  {
    std::vector<uint32_t> w((size_t)p.n_packed, 0xdeadbeefu);
    int64_t at = 0;
    FeedSlice f;
    for (int64_t k = 0; feed_slice_at(p, n, slice_batches, false, k, &f); k++) {
      pack_events<false, true>(soa.from(f.ev_first), n - f.ev_first, f.b_hi - f.b_lo, B, rate, W, H, 0, w.data() + at);
      at += f.n;
    }
    put({at});
    put(w);
  }
  // every event's polarity byte, as the event store packs a _pol push
  {
    std::vector<uint8_t> bs((size_t)n, 7), ba((size_t)n, 7);
    pack_polarity(soa, n, bs.data());
    pack_polarity(aos, n, ba.data());
    put(bs);
    put(ba);
  }
  return fclose(g_out) == 0 ? 0 : 2;
}

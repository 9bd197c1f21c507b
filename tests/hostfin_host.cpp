// hostfin_host.cpp -- the host finalize (cmax_slam_amd/csrc/cmx_hostfin.hpp) on its own: no HIP, no context, no GPU.
//   g++ -O2 -std=c++17 -ffp-contract=off tests/hostfin_host.cpp -o hostfin_host     (also the program the sanitizer builds use)
//   hostfin_host CASE_IN CASE_OUT
// CASE_IN : 8 int64 {G, S, gP, mu_free, measure, ticket, damage, damage_record}, the pixel count N (double), then the records as the
//           device would leave them: kHostRecCount x kHostRecWords words of 8 bytes.  The program stamps ticket and checksum of every
//           record it is told exists (the first min(G, S) shard records and the moments record) itself, then applies `damage` to
//           record `damage_record`:  0 none, 1 stale ticket (the previous evaluation's, with that evaluation's checksum), 2 wrong
//           checksum, 3 torn: the first four words are the new record's, the last four still the previous evaluation's,
//           4 torn the other way round, 5 the record never arrives (all zero).
// CASE_OUT: int64 {accepted (0 / 1), have mask, expected mask}, then doubles {contrast, mu, grad[6], fallback} (zeros if not accepted).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cmax_slam_amd/csrc/cmx_hostfin.hpp"

using namespace cmx;

static void stamp(unsigned long long *rec, unsigned long long ticket) {
  unsigned long long x = 0;
  for (int k = 0; k < kHostRecCols; k++) x ^= rec[k];
  rec[kHostRecTicket] = ticket;
  rec[kHostRecCheck] = x ^ (ticket * kTicketMix);
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s CASE_IN CASE_OUT\n", argv[0]); return 2; }
  FILE *in = fopen(argv[1], "rb");
  long long h[8];
  double N = 0;
  std::vector<unsigned long long> recs((size_t)kHostRecCount * kHostRecWords);
  if (!in || fread(h, sizeof(long long), 8, in) != 8 || fread(&N, sizeof(double), 1, in) != 1 ||
      fread(recs.data(), sizeof(unsigned long long), recs.size(), in) != recs.size()) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  fclose(in);
  const int G = (int)h[0], S = (int)h[1], gP = (int)h[2], mu_free = (int)h[3], measure = (int)h[4], damage = (int)h[6], dr = (int)h[7];
  const unsigned long long ticket = (unsigned long long)h[5];
  if (S < 1 || S > kHostShardsMax || G < 1 || gP < 0 || 2 * gP > kHostRecCols || dr < 0 || dr >= kHostRecCount) {
    fprintf(stderr, "bad case header\n");
    return 2;
  }
  const uint64_t expected = hostfin_expected(G, S);
  for (int q = 0; q < kHostRecCount; q++) {
    unsigned long long *rec = recs.data() + (size_t)q * kHostRecWords;
    if (!((expected >> q) & 1ull)) {  // no member workgroup: the device writes nothing there
      for (int k = 0; k < kHostRecWords; k++) rec[k] = 0ull;
      continue;
    }
    unsigned long long prev[kHostRecWords];  // what the previous evaluation left in this line: other sums, ticket - 1
    for (int k = 0; k < kHostRecWords; k++) prev[k] = k < kHostRecCols ? rec[k] ^ (0x3ff0000000000000ull + 977ull * (unsigned)(q + k + 1)) : 0ull;
    stamp(prev, ticket - 1ull);
    stamp(rec, ticket);
    if (q != dr || damage == 0) continue;
    if (damage == 1) for (int k = 0; k < 8; k++) rec[k] = prev[k];
    else if (damage == 2) rec[kHostRecCheck] ^= 0x10ull;
    else if (damage == 3) for (int k = 4; k < 8; k++) rec[k] = prev[k];
    else if (damage == 4) for (int k = 0; k < 4; k++) rec[k] = prev[k];
    else if (damage == 5) for (int k = 0; k < 8; k++) rec[k] = 0ull;
  }
  HostFinRecords r;
  bool ok = false;
  for (int pass = 0; pass < 3; pass++) ok = hostfin_poll(recs.data(), ticket, expected, r);  // (polling again changes nothing)
  HostFinResult o{};
  if (ok) o = hostfin_combine(r, S, gP, mu_free, measure, N);
  FILE *out = fopen(argv[2], "wb");
  if (!out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  const long long head[3] = {ok ? 1 : 0, (long long)r.have, (long long)expected};
  fwrite(head, sizeof(long long), 3, out);
  const double vals[9] = {o.contrast, o.mu, o.grad[0], o.grad[1], o.grad[2], o.grad[3], o.grad[4], o.grad[5], o.fallback};
  fwrite(vals, sizeof(double), 9, out);
  fclose(out);
  return 0;
}

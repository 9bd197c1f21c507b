// cmx_hostfin.hpp -- host-side finalize of a front-end gradient evaluation (CMX_OPT_TAIL_FINALIZE = 4), and the few definitions it
// shares with the device finalize (cmx_kernels.hip: finalize_body).  No HIP types: tests/hostfin_host.cpp builds it with the plain
// host compiler.
//
// The gather launch of such an evaluation does not look for its overall last workgroup.  The last arriver of every accumulator-row
// shard writes ONE record -- the shard's column sums -- to mapped host memory, and one extra workgroup of the launch writes the
// moments record (sum B, sum B^2, the splat's fallback word).  The host, which spins through the evaluation anyway, waits for the
// records and forms contrast and gradient itself with the expressions of finalize_body.
//   record = 16 words of 8 bytes, one 128-byte line of its own; the device stores words 0..7 with eight contiguous lanes:
//     [0..5] payload   shard record: column sums S1 (gP) | S2 (gP), unused columns 0;  moments record: s0, s1, fallback word, 0, 0, 0
//     [6]    ticket of the evaluation
//     [7]    xor of the payload's bit patterns ^ ticket * kTicketMix
//   As with the result block's ticket + checksum (cmx_internal.hpp) no system-scope fence orders the eight words over PCIe: a record
//   is accepted only when the ticket AND the checksum over the words read match; a torn or stale read fails and is repeated.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define CMX_HOSTFIN_HD __host__ __device__
#else
#define CMX_HOSTFIN_HD
#endif

namespace cmx {

constexpr unsigned long long kTicketMix = 0x9E3779B97F4A7C15ull;

// contrast from the two image moments: the one expression shared by the finalize step (device or host) and by the workgroups of a
// self-gating gradient pass (they must take the machine's decision from bitwise the same number)
static inline CMX_HOSTFIN_HD double contrast_from_sums(double s0, double s1, double N, int measure, double *mu_out) {
  const double mu = s0 / N;
  *mu_out = mu;
  if (measure == 1) return s1 / N;
  double var = s1 / N - mu * mu;
  if (var < 0) var = 0;
  const double sd = sqrt(var);
  return sd * sd;
}

constexpr int kHostShardsMax = 32;   // accumulator rows / shard records of the host-finalize form (launch parameter S: 8, 16 or 32)
constexpr int kHostRecWords = 16;    // one 128-byte line per record
constexpr int kHostRecCols = 6;      // payload words
constexpr int kHostRecTicket = 6, kHostRecCheck = 7;
constexpr int kHostRecMoments = kHostShardsMax;               // index of the moments record, whatever S is
constexpr int kHostRecBase = 2048;                            // first record, in doubles from the start of the mapped result block
constexpr int kHostRecCount = kHostShardsMax + 1;

// shards that have a member workgroup among G event workgroups (workgroup b adds to shard b % S): the first min(G, S)
static inline int hostfin_shard_records(int G, int S) { return G < S ? G : S; }
// bit q: record q is expected (bit kHostRecMoments: the moments record)
static inline uint64_t hostfin_expected(int G, int S) {
  const int m = hostfin_shard_records(G, S);
  return (m >= 64 ? ~0ull : ((1ull << m) - 1ull)) | (1ull << kHostRecMoments);
}

// one record: true, with its payload in out[], iff it carries `want` and its checksum matches the words read
static inline bool hostfin_read_record(const volatile unsigned long long *rec, unsigned long long want, unsigned long long out[kHostRecCols]) {
  if (rec[kHostRecTicket] != want) return false;
  unsigned long long x = 0ull;
  for (int k = 0; k < kHostRecCols; k++) {
    out[k] = rec[k];
    x ^= out[k];
  }
  return (x ^ (want * kTicketMix)) == rec[kHostRecCheck];
}

struct HostFinRecords {
  uint64_t have = 0;                                        // records accepted so far (bits as in hostfin_expected)
  unsigned long long w[kHostRecCount][kHostRecCols] = {};   // their payloads (rows never accepted stay zero)
};

// one pass over the records still missing; true once every expected record has been accepted
static inline bool hostfin_poll(const volatile unsigned long long *recs, unsigned long long want, uint64_t expected, HostFinRecords &r) {
  uint64_t missing = expected & ~r.have;
  while (missing) {
    const int q = __builtin_ctzll(missing);
    missing &= missing - 1;
    if (hostfin_read_record(recs + (size_t)q * kHostRecWords, want, r.w[q])) r.have |= 1ull << q;
  }
  return (expected & ~r.have) == 0;
}

static inline double hostfin_f64(unsigned long long bits) {
  double v;
  memcpy(&v, &bits, sizeof v);
  return v;
}

// contrast, mean, gradient and fallback word from the accepted records: the shard rows are summed in shard order q = 0 .. S-1
// (a shard without a member contributes the zeros its row holds), then finalize_body's expressions.  Compiled without
// floating-point contraction the numbers are the device finalize's bit for bit, given the same sums (S = 8: the same order too).
struct HostFinResult {
  double contrast, mu, grad[kHostRecCols], fallback;
};
static inline HostFinResult hostfin_combine(const HostFinRecords &r, int S, int gP, int mu_free, int measure, double N) {
  HostFinResult o{};
  const unsigned long long *m = r.w[kHostRecMoments];
  const double s0 = hostfin_f64(m[0]), s1 = hostfin_f64(m[1]);
  o.fallback = hostfin_f64(m[2]);
  o.contrast = contrast_from_sums(s0, s1, N, measure, &o.mu);
  const int ncol = mu_free ? 2 * gP : gP;
  double cols[kHostRecCols] = {};
  for (int k = 0; k < ncol && k < kHostRecCols; k++) {
    double w = 0;
    for (int q = 0; q < S; q++) w += hostfin_f64(r.w[q][k]);
    cols[k] = w;
  }
  for (int k = 0; k < gP && k < kHostRecCols; k++) {
    const double s = cols[k], s2 = (mu_free && gP + k < kHostRecCols) ? cols[gP + k] : 0.0;
    o.grad[k] = 2.0 * (s - ((mu_free && measure != 1) ? o.mu * s2 : 0.0)) / N;
  }
  return o;
}

}  // namespace cmx

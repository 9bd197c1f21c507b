// cmx_select.hip -- device code of the event store (cmx_events_select*, cmx_events_pixel_counts*).
//
// Stable stream compaction of a range of one store into another, as THREE launches on one stream; no workgroup ever waits on
// another one (no look-back scan: its spinning needs the forward progress of other workgroups, and the launch floors saved are
// nothing against the bytes this call moves):
//   select_mark_kernel     one workgroup per tile of kSelTile = 4096 events = 64 wave-sized groups.  Each lane evaluates the
//                          predicate of its event -- only the criteria that are given are loaded (workgroup-uniform branches on the
//                          pointers), the packed word only for the pixel mask -- and the wave's 64-bit ballot is stored as ONE word
//                          per 64 events by one lane (a plain vector store).  Lanes at or past n ballot zero, and every word of the
//                          last tile is written.  The tile's kept count goes through LDS into counts[tile].
//   select_scan_kernel     ONE workgroup: exclusive scan of the tile counts into 64-bit offsets, kSelScanThreads tiles per pass
//                          with a running carry; offsets[ntiles] is the total, which the host reads before it launches the scatter.
//   select_scatter_kernel  one workgroup per tile.  Wave 0 turns the tile's 64 ballot words into 64 exclusive prefixes (one
//                          popcount per lane, a wave scan), then every wave re-reads its words: a kept lane's slot is
//                          offsets[tile] + prefix[word] + popcount(mask below the lane), so a wave's events land side by side and the
//                          4-, 8- and 1-byte stores coalesce.  Element-wide loads and stores only: src + first and dst + size sit
//                          at arbitrary element offsets.  The host launches it only when offsets[ntiles] fits the destination.
// The histogram is one grid-stride kernel, one 32-bit atomic add per event into the zeroed W*H array (exact for any distribution).
#include <algorithm>

#include "cmx_internal.hpp"

namespace cmx {

static_assert(kSelTile == 64 * 64, "a tile is 64 ballot words: one lane of wave 0 per word in the scatter's prefix scan");
constexpr int kSelThreads = 256, kSelWaves = kSelThreads / 64, kSelSteps = kSelTile / kSelThreads;

__global__ __launch_bounds__(kSelThreads) void select_mark_kernel(SelectArgs a) {
  __shared__ unsigned s_cnt[kSelWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long word0 = (long long)blockIdx.x * 64;
  unsigned kept = 0;
  for (int j = 0; j < kSelSteps; j++) {
    const long long word = word0 + j * kSelWaves + wave, i = word * 64 + lane;
    bool k = i < a.n;
    if (k) {
      if (a.keep) k = a.keep[i] != 0;
      if (a.score) k = k && (a.score[i] >= a.min_score);  // NaN compares false: dropped
      if (a.flags) k = k && ((a.flags[i] & a.flags_mask) == a.flags_value);
      if (a.pixel_keep) {
        const uint32_t w = a.src_xy[i];
        k = k && a.pixel_keep[(size_t)((w >> 16) & 0x7fffu) * (size_t)a.W + (w & 0xffffu)] != 0;
      }
    }
    const unsigned long long m = __ballot(k);
    if (lane == 0) a.ballot[word] = m;
    kept += (unsigned)__popcll(m);
  }
  if (lane == 0) s_cnt[wave] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
#pragma unroll
    for (int w = 0; w < kSelWaves; w++) t += s_cnt[w];
    a.counts[blockIdx.x] = t;
  }
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ unsigned wave_scan_incl(unsigned v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned u = __shfl_up(v, off);
    if (lane >= off) v += u;
  }
  return v;
}

__global__ __launch_bounds__(kSelScanThreads) void select_scan_kernel(const unsigned *__restrict__ counts, long long ntiles,
                                                                      long long *__restrict__ offsets) {
  __shared__ unsigned s_wave[kSelScanThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long carry = 0;
  for (long long t0 = 0; t0 < ntiles; t0 += kSelScanThreads) {
    const long long t = t0 + threadIdx.x;
    const unsigned c = t < ntiles ? counts[t] : 0u;
    const unsigned incl = wave_scan_incl(c, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned before = 0, all = 0;  // a pass holds at most kSelScanThreads * kSelTile = 2^20 events: 32 bits
#pragma unroll
    for (int w = 0; w < kSelScanThreads / 64; w++) {
      if (w < wave) before += s_wave[w];
      all += s_wave[w];
    }
    if (t < ntiles) offsets[t] = carry + (long long)(before + incl - c);
    carry += (long long)all;
    __syncthreads();  // s_wave is rewritten by the next pass
  }
  if (threadIdx.x == 0) offsets[ntiles] = carry;
}

__global__ __launch_bounds__(kSelThreads) void select_scatter_kernel(SelectArgs a) {
  const long long base = a.offsets[blockIdx.x];
  if (a.offsets[blockIdx.x + 1] == base) return;  // an empty tile (workgroup-uniform)
  __shared__ unsigned s_pre[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long word0 = (long long)blockIdx.x * 64;
  if (wave == 0) {
    const unsigned c = (unsigned)__popcll(a.ballot[word0 + lane]);
    s_pre[lane] = wave_scan_incl(c, lane) - c;
  }
  __syncthreads();
  for (int j = 0; j < kSelSteps; j++) {
    const int q = j * kSelWaves + wave;
    const unsigned long long m = a.ballot[word0 + q];
    if (m == 0) continue;  // an empty wave (wave-uniform)
    if ((m >> lane) & 1ull) {
      const long long i = (word0 + q) * 64 + lane;  // < n: the mark kernel ballots zero past the end
      const long long d = base + s_pre[q] + __popcll(m & ((1ull << lane) - 1ull));
      a.dst_xy[d] = a.src_xy[i];
      a.dst_t[d] = a.src_t[i];
      if (a.src_pol) a.dst_pol[d] = a.src_pol[i];
    }
  }
}

void launch_select_mark(const SelectArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(select_mark_kernel, dim3((unsigned)sel_tiles(a.n)), dim3(kSelThreads), 0, s, a);
}
void launch_select_scan(const unsigned *counts, long long ntiles, long long *offsets, hipStream_t s) {
  hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(kSelScanThreads), 0, s, counts, ntiles, offsets);
}
void launch_select_scatter(const SelectArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(select_scatter_kernel, dim3((unsigned)sel_tiles(a.n)), dim3(kSelThreads), 0, s, a);
}

// counts[y * W + x] += 1 per event; the array is zeroed in front of the launch
__global__ __launch_bounds__(256) void pixel_counts_kernel(const uint32_t *__restrict__ xy, long long n, int W, uint32_t *counts) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const uint32_t w = xy[i];
    atomicAdd(&counts[(size_t)((w >> 16) & 0x7fffu) * (size_t)W + (w & 0xffffu)], 1u);
  }
}
void launch_pixel_counts(const uint32_t *xy, long long n, int W, uint32_t *counts, hipStream_t s) {
  if (n <= 0) return;
  const long long blocks = std::min<long long>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(pixel_counts_kernel, dim3((unsigned)blocks), dim3(256), 0, s, xy, n, W, counts);
}

}  // namespace cmx

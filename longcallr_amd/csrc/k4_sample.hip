// k4_sample.hip — K4, down-sampling: which fragment rows of a deep region the optimiser sees (reference src/thread.rs:144-151,
// phase.rs:693-701: a fixed-size random sample of the region's fragments).  Host control: k4_phase.hip (PhaseHost::sample).
//
// The reference shuffles the row indices with StdRng and takes the first `depth`; here the sample of a region with F >= depth rows is
// the `depth` rows with the SMALLEST keys
//     key(r) = mix64(region_seed(seed, start0) + (r + 1) * 0x9E3779B97F4A7C15),   r = 0 .. F - 1 (region relative)
// -- the 64-bit value inside u01(region_seed, r).  mix64 is a bijection and the arguments are distinct, so the keys are distinct: no
// ties, exactly `depth` rows, a uniform depth-subset like shuffle-and-take, and a pure function of (seed, region start, row): free of
// order and of the batch's other regions, as every stage is.
#include "k4_dev.h"
#include "k4_kernels.h"

namespace {

__device__ __forceinline__ uint64_t sample_key(uint64_t rseed, int r) { return mix64(rseed + ((uint64_t)r + 1ull) * 0x9E3779B97F4A7C15ULL); }

// One workgroup per down-sampled region: MSB-first radix select of the depth-th smallest key, eight digits of eight bits, the digit
// histogram in LDS.  The keys are recomputed in every pass (a dozen integer operations) instead of being stored: the kernel's only
// memory traffic is the region's two row offsets and the byte per row of the last pass.
__global__ void __launch_bounds__(SAMPLE_THREADS) k4_sample(const int32_t* __restrict__ slots, const int32_t* __restrict__ row_region_off,
                                                            const int64_t* __restrict__ start0, uint32_t depth, uint64_t seed,
                                                            uint8_t* __restrict__ sampled) {
  __shared__ unsigned int hist[256];
  __shared__ unsigned int s_pick[2];   // the digit that holds the wanted rank, keys of the prefix below that digit
  const int g = slots[blockIdx.x], tid = threadIdx.x, lane = tid & 63;
  const int r0 = row_region_off[g], F = row_region_off[g + 1] - r0;
  const uint64_t rseed = region_seed(seed, start0[g]);
  uint64_t prefix = 0;     // the digits found so far, in place
  uint32_t want = depth;   // rank (from 1) of the wanted key among the keys that carry the prefix; 1 <= depth <= F (the host launches no other region)
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const uint64_t hi_mask = shift == 56 ? 0ull : ~0ull << (shift + 8);
    for (int r = tid; r < F; r += SAMPLE_THREADS) {
      const uint64_t k = sample_key(rseed, r);
      if ((k & hi_mask) == prefix) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {   // lane l owns digits 4 l .. 4 l + 3: the lane whose inclusive count first reaches the rank walks its four
      unsigned int c[4];
#pragma unroll
      for (int j = 0; j < 4; j++) c[j] = hist[4 * lane + j];
      const int sum = (int)(c[0] + c[1] + c[2] + c[3]);
      const int incl = wave_incl_scan(sum);
      unsigned int below = (unsigned int)(incl - sum);
      if (below < want && want <= (unsigned int)incl) {
        int j = 0;
        while (below + c[j] < want) { below += c[j]; j++; }
        s_pick[0] = (unsigned int)(4 * lane + j); s_pick[1] = below;
      }
    }
    __syncthreads();
    prefix |= (uint64_t)s_pick[0] << shift;
    want -= s_pick[1];
  }
  // prefix = the depth-th smallest key
  for (int r = tid; r < F; r += SAMPLE_THREADS) sampled[r0 + r] = sample_key(rseed, r) <= prefix ? 1 : 0;
}

}  // namespace

void launch_k4_sample(int32_t n_slots, const int32_t* d_slots, const int32_t* d_row_region_off, const int64_t* d_start0, uint32_t depth, uint64_t seed,
                      uint8_t* d_sampled, hipStream_t s) {
  if (n_slots > 0) hipLaunchKernelGGL(k4_sample, dim3((unsigned)n_slots), dim3(SAMPLE_THREADS), 0, s, d_slots, d_row_region_off, d_start0, depth, seed, d_sampled);
}

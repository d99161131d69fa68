// k5_regions.hip — region discovery on gfx950.
//
// Replaces find_isolated_regions_with_depth (reference src/util.rs:236-332, with and without --truncation): the
// per-contig depth vector (+1 per reference position of every read span, introns and deletions
// included, util.rs:281-285) as a difference array + prefix scan, and the split into coverage islands
// as an ordered compaction of the positions where the columns switch between break (depth 0, or above the
// truncation cap) and kept, with the maxima of the reference's emission intervals beside them.
#include "lcr_dev.h"

// the part of the contig any read covers: out[0] = min start, out[1] = max end over the valid spans (out preset to INT_MAX, 0).
// The dense passes below run over that window only: a file with 1 700 reads on 13 kb of a 64 Mb contig (demo.bam) no longer
// clears, scans and compacts 64 M positions.
__global__ void __launch_bounds__(LCR_BLOCK)
k5_span_window(const int32_t* __restrict__ ref_start, const int32_t* __restrict__ ref_end, int32_t n, int64_t contig_len, int32_t* __restrict__ out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  int lo = INT_MAX, hi = 0;
  if (r < n) {
    const int64_t s = ref_start[r];
    const int64_t e = min((int64_t)ref_end[r], contig_len);
    if (s >= 0 && s < e) { lo = (int)s; hi = (int)e; }
  }
  for (int d = 32; d >= 1; d >>= 1) { lo = min(lo, __shfl_xor(lo, d, 64)); hi = max(hi, __shfl_xor(hi, d, 64)); }
  if ((threadIdx.x & 63) == 0 && hi > 0) { atomicMin(&out[0], lo); atomicMax(&out[1], hi); }
}
void launch_k5_span_window(const int32_t* ref_start, const int32_t* ref_end, int32_t n, int64_t contig_len, int32_t* out, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k5_span_window, dim3((n + LCR_BLOCK - 1) / LCR_BLOCK), dim3(LCR_BLOCK), 0, s, ref_start, ref_end, n, contig_len, out);
}

// diff is indexed from `lo` (the window's first position)
__global__ void __launch_bounds__(LCR_BLOCK)
k5_span_diff(const int32_t* __restrict__ ref_start, const int32_t* __restrict__ ref_end, int32_t n, int64_t contig_len, int64_t lo,
             uint32_t* __restrict__ diff) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int64_t s = ref_start[r];
  int64_t e = ref_end[r];
  if (e > contig_len) e = contig_len;
  if (s < 0 || s >= e) return;
  atomicAdd(&diff[s - lo], 1u);
  atomicAdd(&diff[e - lo], 0xFFFFFFFFu);
}

// depth[i] = ex[i + 1] (ex = exclusive scan of diff).  A column is KEPT when 0 < depth <= cap and is a BREAK otherwise
// (util.rs:294-296; cap = UINT32_MAX: truncation off, only uncovered columns break); islands are the maximal runs of
// kept columns.  One block per 1024 positions counts the island starts it contains (and, with n_trunc, its columns
// above the cap); after the scan of the counts the same walk writes starts and ends in order and the maxima of the
// reference's emission intervals.
//
// The maxima (imax, 2 n_islands + 1 entries, zeroed): the reference takes max_coverage from EVERY column, breaks
// included, and resets it only where a region is emitted -- at the first break behind an island.  So island j gets
//   imax[2 j + 1]  its own columns and the column that closes it (the break right behind its end),
//   imax[2 j]      the breaks in front of it, from behind the previous island's closing column on,
// and the host folds the two into the pending region.  The key of a column (the index into imax) never decreases along
// the window, so equal keys are contiguous: every thread reduces the runs of its four columns, a segmented max-scan
// over the wave joins the threads' last runs, and the last lane of every segment does one atomicMax (order-free on
// u32, the result is deterministic).  The cost follows the window: one atomic per run and wave, whatever the number of islands.
__device__ __forceinline__ bool k5_keep(int d, uint32_t cap) { return d > 0 && (uint32_t)d <= cap; }

template <bool WRITE>
__global__ void __launch_bounds__(LCR_BLOCK)
k5_bounds(const int32_t* __restrict__ ex, int64_t contig_len, uint32_t cap, int32_t* __restrict__ blk_cnt, const int32_t* __restrict__ blk_off,
          int32_t* __restrict__ starts, int32_t* __restrict__ ends, uint32_t* __restrict__ imax, int32_t n_keys, uint32_t* __restrict__ n_trunc) {
  __shared__ int wsum_s[LCR_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * 1024 + (int64_t)tid * 4;
  int fs[4], fe[4], cl[4], dv[4], cs = 0, over = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int64_t i = base + k;
    fs[k] = fe[k] = cl[k] = dv[k] = 0;
    if (i < contig_len) {
      const int d = ex[i + 1];
      const int dp = i > 0 ? ex[i] : 0;                       // depth[i-1]
      const int dn = i + 1 < contig_len ? ex[i + 2] : 0;      // depth[i+1]
      const bool kd = k5_keep(d, cap), kp = k5_keep(dp, cap);
      fs[k] = kd && !kp;
      fe[k] = kd && !k5_keep(dn, cap);
      cl[k] = kd || kp;                                       // an island's column, or the break that closes one
      dv[k] = d;
      over += d > 0 && !kd;
    }
    cs += fs[k];
  }
  if (!WRITE && n_trunc) {   // (a uniform branch: all lanes shuffle)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) over += __shfl_xor(over, d, 64);
    if (lane == 0 && over) atomicAdd(n_trunc, (uint32_t)over);
  }
  // block prefix of the start counts
  int is = cs;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int ts = __shfl_up(is, d, 64);
    if (lane >= d) is += ts;
  }
  if (lane == 63) wsum_s[w] = is;
  __syncthreads();
  int as = 0;
  for (int k = 0; k < w; k++) as += wsum_s[k];
  if (!WRITE) {
    if (tid == LCR_BLOCK - 1) blk_cnt[blockIdx.x] = is + as;   // island starts in this block
    return;
  }
  // islands are numbered by their start; an end at position i closes island number (#starts at or before i) - 1
  int rs = blk_off[blockIdx.x] + as + is - cs;
  int ck = -1, hk = -1;        // key of the thread's current (in the end: last) run and of its first run, once there are two
  uint32_t cv = 0, hv = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (fs[k]) starts[rs] = (int32_t)(base + k);
    rs += fs[k];
    if (fe[k]) ends[rs - 1] = (int32_t)(base + k);
    if (base + k < contig_len) {
      const int key = 2 * rs - cl[k];
      if (key != ck) {
        if (ck >= 0) {
          if (hk < 0) { hk = ck; hv = cv; }
          else if (cv && ck < n_keys) atomicMax(&imax[ck], cv);   // a run inside the thread's columns
        }
        ck = key; cv = (uint32_t)dv[k];
      } else cv = max(cv, (uint32_t)dv[k]);
    }
  }
  if (hk >= 0 && hv && hk < n_keys) atomicMax(&imax[hk], hv);
  // segmented inclusive max-scan of (ck, cv) over the wave (equal keys are contiguous; -1 = no column, the window's tail)
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int k2 = __shfl_up(ck, d, 64);
    const uint32_t v2 = __shfl_up(cv, d, 64);
    if (lane >= d && k2 == ck) cv = max(cv, v2);
  }
  const int kn = __shfl_down(ck, 1, 64);
  if ((lane == 63 || kn != ck) && ck >= 0 && ck < n_keys && cv) atomicMax(&imax[ck], cv);
}

void launch_k5_span_diff(const int32_t* ref_start, const int32_t* ref_end, int32_t n, int64_t contig_len, int64_t lo, uint32_t* diff, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(k5_span_diff, dim3((n + LCR_BLOCK - 1) / LCR_BLOCK), dim3(LCR_BLOCK), 0, s, ref_start, ref_end, n, contig_len, lo, diff);
}
void launch_k5_bounds(bool write, const int32_t* ex, int64_t contig_len, uint32_t cap, int32_t n_blocks, int32_t* blk_cnt, const int32_t* blk_off,
                      int32_t* starts, int32_t* ends, uint32_t* imax, int32_t n_keys, uint32_t* n_trunc, hipStream_t s) {
  if (n_blocks == 0) return;
  if (write) hipLaunchKernelGGL(k5_bounds<true>, dim3(n_blocks), dim3(LCR_BLOCK), 0, s, ex, contig_len, cap, blk_cnt, blk_off, starts, ends, imax, n_keys, n_trunc);
  else hipLaunchKernelGGL(k5_bounds<false>, dim3(n_blocks), dim3(LCR_BLOCK), 0, s, ex, contig_len, cap, blk_cnt, blk_off, starts, ends, imax, n_keys, n_trunc);
}

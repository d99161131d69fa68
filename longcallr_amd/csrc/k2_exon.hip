// k2_exon.hip — the exon-only mask of lcr_set_exon_mask (longcallR --exon-only; candidate.rs:73-89): the bound batch's interval lists -> one
// bit per global column, read by pass 1 of the candidate filters (k2_eval.h: exon_bit).
//
// Region g owns intervals [iv_off[g], iv_off[g + 1]) in reference coordinates, 0-based half-open, in any order, overlapping, nested, abutting,
// reaching past the region or outside it.  Regions do not start on word boundaries (col_off is a running sum of lengths), so two regions share
// a word and two intervals share bits: the builder sets its bits with atomicOr.  OR is commutative and idempotent, so the plane is the same
// from run to run whatever order the waves arrive in; the alternative -- one owner per word -- would have every word search the interval
// list of its one or two regions, or need the lists sorted and merged first: work per column instead of per interval.  A wave per interval,
// its lanes over the words the clipped interval covers: the cost follows the intervals and their words, not n_cols (the plane's clear apart).
#include "lcr_dev.h"

namespace {

// contract of device-resident lists (host ones are checked on the host), part 1: iv_off[0] == 0, ascending.  verdict[1] = the interval count.
__global__ void __launch_bounds__(LCR_BLOCK) k2_exon_check_off(const int32_t* __restrict__ iv_off, int32_t ng, int32_t* __restrict__ verdict) {
  const int32_t i = (int32_t)(blockIdx.x * LCR_BLOCK + threadIdx.x);
  if (i > ng) return;
  const int32_t v = iv_off[i];
  if (i == 0 ? v != 0 : iv_off[i - 1] > v) verdict[0] = 1;   // (every writer stores the same value: a plain store)
  if (i == ng) verdict[1] = v;
}

// ... part 2, behind part 1 on the stream: only offsets that passed say how many intervals there are.  end0 >= start0, arrays beside a count.
__global__ void __launch_bounds__(LCR_BLOCK) k2_exon_check_iv(const int64_t* __restrict__ s0, const int64_t* __restrict__ e0, int32_t* verdict) {
  if (*(volatile int32_t*)verdict != 0) return;
  const int32_t n = verdict[1];
  if (n > 0 && (!s0 || !e0)) { verdict[0] = 1; return; }
  for (int32_t i = (int32_t)(blockIdx.x * LCR_BLOCK + threadIdx.x); i < n; i += (int32_t)(gridDim.x * LCR_BLOCK))
    if (e0[i] < s0[i]) verdict[0] = 1;
}

__global__ void __launch_bounds__(LCR_BLOCK)
k2_exon_build(const int32_t* __restrict__ iv_off, const int64_t* __restrict__ s0, const int64_t* __restrict__ e0, int32_t n_iv,
              const int64_t* __restrict__ start0, const int32_t* __restrict__ len, const int64_t* __restrict__ col_off, int32_t ng,
              uint32_t* __restrict__ plane) {
  const int32_t i = (int32_t)((blockIdx.x * LCR_BLOCK + threadIdx.x) / LCR_WAVE), lane = threadIdx.x & (LCR_WAVE - 1);
  if (i >= n_iv) return;
  int lo = 0, hi = ng;   // the interval's region: the first g with iv_off[g + 1] > i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (iv_off[mid + 1] > i) hi = mid; else lo = mid + 1;
  }
  if (lo >= ng) return;
  const int64_t r0 = start0[lo], r1 = r0 + len[lo];
  const int64_t a = max(s0[i], r0), b = min(e0[i], r1);   // clipped to the region; empty: outside it, or end0 == start0
  if (b <= a) return;
  const int64_t c0 = col_off[lo] + (a - r0), c1 = col_off[lo] + (b - r0) - 1;   // first and last global column, both inside the region's columns
  const int64_t w0 = c0 >> 5, w1 = c1 >> 5;
  for (int64_t w = w0 + lane; w <= w1; w += LCR_WAVE) {
    uint32_t m = 0xFFFFFFFFu;
    if (w == w0) m &= 0xFFFFFFFFu << (c0 & 31);
    if (w == w1) m &= 0xFFFFFFFFu >> (31 - (c1 & 31));
    atomicOr(&plane[w], m);
  }
}

}  // namespace

void launch_k2_exon_check(const int32_t* iv_off, const int64_t* iv_start0, const int64_t* iv_end0, int32_t n_regions, int32_t* verdict, hipStream_t s) {
  hipLaunchKernelGGL(k2_exon_check_off, dim3(n_regions / LCR_BLOCK + 1), dim3(LCR_BLOCK), 0, s, iv_off, n_regions, verdict);
  hipLaunchKernelGGL(k2_exon_check_iv, dim3(256), dim3(LCR_BLOCK), 0, s, iv_start0, iv_end0, verdict);
}

void launch_k2_exon_build(const BatchView& b, const int32_t* iv_off, const int64_t* iv_start0, const int64_t* iv_end0, int32_t n_iv, uint32_t* plane, hipStream_t s) {
  const int wpb = LCR_BLOCK / LCR_WAVE;
  if (n_iv > 0 && b.n_regions > 0)
    hipLaunchKernelGGL(k2_exon_build, dim3((n_iv + wpb - 1) / wpb), dim3(LCR_BLOCK), 0, s, iv_off, iv_start0, iv_end0, n_iv, b.start0, b.len, b.col_off, b.n_regions, plane);
}

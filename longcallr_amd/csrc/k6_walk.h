// k6_walk.h — the junction walk of a read that k6_junctions.hip (lcr_junctions) and k15_isoforms.hip (lcr_isoforms) share.
#pragma once
#include "lcr_dev.h"

#ifdef __HIPCC__
// Sixteen lanes per read (one DPP row; four reads per wave64): ops spread over the lanes, reference offsets from a row scan of the
// reference-consuming lengths (M D N = X), a carry between rounds of 16 ops.  Every lane of a row takes the same branches and has to
// call.  sink(s, len, k) runs in the lane of every N op of length >= 1: the read's k-th junction (s rises with k), s the contig column
// of its first skipped base.  *n_junc: the junctions of the read; *rend: pos + all reference-consuming lengths (both row-uniform).
template <class Sink>
__device__ __forceinline__ void row16_walk_junctions(const BatchView& b, int r, Sink sink, int* n_junc, int* rend) {
  const int lane = threadIdx.x & 63, l16 = lane & 15, rbase = lane & 48;
  const uint32_t ncig = b.n_cig[r];
  const uint32_t* __restrict__ cg = b.cigar + b.cig_off[r];
  int ref_cur = b.pos[r], n_n = 0;
  for (uint32_t c0 = 0; c0 < ncig; c0 += 16) {
    const uint32_t w = c0 + l16 < ncig ? cg[c0 + l16] : 0u;   // (a padding word is a 0-length M)
    const int op = w & 15, len = (int)(w >> 4);
    const int dr = (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? len : 0;   // I S H P consume no reference
    const int ir = row16_incl_scan(dr);
    const bool is_n = op == 3 && len >= 1;
    const unsigned int m = (unsigned int)(__ballot(is_n) >> rbase) & 0xffffu;
    if (is_n) sink(ref_cur + ir - dr, len, n_n + __popc(m & ((1u << l16) - 1u)));
    n_n += __popc(m);
    ref_cur += __shfl(ir, rbase + 15, 64);
  }
  *n_junc = n_n; *rend = ref_cur;
}
#endif

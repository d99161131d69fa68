// k6_walk.h — what the junction kernels share: the junction walk of a read (k6_junctions.hip, k15_isoforms.hip), the splice motif of a
// junction (k6_rank, k9_rank) and the four-cell phase-set sweep of the table kernels (k6_tables, k9_tables, k15_tables).
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

// The motif of the junction [s, s + l) of region g on the window's reference, either case: 1 = GT-AG, 2 = CT-AC, 0 = neither, or the
// junction does not lie inside the window
__device__ __forceinline__ uint8_t splice_motif(const BatchView& b, int g, int32_t s, int32_t l) {
  const long long sl = (long long)s - b.start0[g];
  if (!(l >= 2 && sl >= 0 && sl + l <= (long long)b.len[g])) return 0;
  const auto upper = [](uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c; };
  const uint8_t* __restrict__ w = b.ref + b.col_off[g];
  const uint8_t d0 = upper(w[sl]), d1 = upper(w[sl + 1]), a0 = upper(w[sl + l - 2]), a1 = upper(w[sl + l - 1]);
  if (d0 == 'G' && d1 == 'T' && a0 == 'A' && a1 == 'G') return 1;
  if (d0 == 'C' && d1 == 'T' && a0 == 'A' && a1 == 'C') return 2;
  return 0;
}

struct K6Cells { uint32_t ps, n_sets, n[4]; };   // the phase set with the most rows, distinct sets, its rows per cell

// Called by every thread of one workgroup.  Over the rows [p0, p_end) that meets(row) lets through: their phase sets
// are visited in ascending order, one sweep over the rows each.  Sweep k counts the cells cell(row) = 0..3 of the k-th smallest value and
// finds the next one (the first sweep only finds the smallest); phase set 0 is a group like any other, so "a current value" is a flag of
// its own.  "Most rows, ties to the smallest value" is then a strict > against the best so far.  A region has a handful of phase sets --
// one per group of linked heterozygous sites --, so this is two to four sweeps; cell() -- presence, a scan of the row's own keys -- is
// evaluated once per row, in the sweep of its phase set.  Six words of LDS; the result is the same in all threads.
// (k7_sweep_phase_sets, k7_sweep.h, is another sweep: it skips phase set 0 and counts h1 / h2 of counting rows.)
template <class Row, class Meets, class Cell>
__device__ __forceinline__ K6Cells sweep_phase_set_cells(const Row* __restrict__ rows, int p0, int p_end, Meets meets, Cell cell) {
  __shared__ uint32_t sh_next, sh_found, sh_cnt[4];
  const int tid = threadIdx.x;
  bool have_cur = false;
  uint32_t cur = 0, best_tot = 0;
  K6Cells best{0, 0, {0, 0, 0, 0}};
  for (;;) {   // (every value of the loop's state is the same in all threads)
    if (tid == 0) { sh_next = 0xffffffffu; sh_found = 0; sh_cnt[0] = sh_cnt[1] = sh_cnt[2] = sh_cnt[3] = 0; }
    __syncthreads();
    for (int p = p0 + tid; p < p_end; p += LCR_BLOCK) {
      const Row row = rows[p];
      if (!meets(row)) continue;
      if (have_cur && row.ps == cur) atomicAdd(&sh_cnt[cell(row)], 1u);
      if (!have_cur || row.ps > cur) { atomicMin(&sh_next, row.ps); atomicOr(&sh_found, 1u); }
    }
    __syncthreads();
    const uint32_t nxt = sh_next, found = sh_found, c0 = sh_cnt[0], c1 = sh_cnt[1], c2 = sh_cnt[2], c3 = sh_cnt[3];
    __syncthreads();
    if (have_cur) {
      best.n_sets++;
      const uint32_t tot = c0 + c1 + c2 + c3;
      if (tot > best_tot) { best_tot = tot; best.ps = cur; best.n[0] = c0; best.n[1] = c1; best.n[2] = c2; best.n[3] = c3; }
    }
    if (!found) break;
    cur = nxt; have_cur = true;
  }
  return best;
}
#endif

// col_segments.h — the per-candidate segments of the fragment matrix that K12 (k12_site_counts.hip) and K14 (k14_somatic.hip) share.  The
// matrix is row-major and their results are per column, so the entries are grouped by destination first and summed afterwards:
//   colseg_count  eight lanes per row over its entries: one integer atomic per entry on its candidate's counter (launch_colseg_count,
//                 k12_site_counts.hip); launch_scan_i32_to_i64 turns the counters into 64-bit segment offsets
//   colseg_fill   the same walk: one 8-byte word per entry into its candidate's segment.  The slot comes from the counter, counted back down
//                 to 0: the order inside a segment is arbitrary, and everything behind it is a count or a sum
//   colseg_pick   a wave64 per candidate over its segment: the first pass of the two units' site kernels
// An entry's word: bits 0-31 the row's phase set (0: not a counting row -- assignment 1 / 2 and a phase set), 32-33 its haplotype (1 / 2 for
// a counting row, else 0), 34 and above the unit's own (Entry).  Device code only.
#pragma once
#include "k7_sweep.h"

constexpr int COLSEG_HAP = 32, COLSEG_OWN = 34;

// entry(c, v): the unit's bits of the word of an entry of candidate c with the matrix value v, at COLSEG_OWN and above
template <class Entry>
__global__ void __launch_bounds__(LCR_BLOCK) colseg_fill(int32_t n_rows, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                          const uint8_t* __restrict__ val, const lcr_read_record* __restrict__ rec, Entry entry,
                                                          int32_t n_cand, uint32_t* __restrict__ cnt, const int64_t* __restrict__ off,
                                                          uint64_t* __restrict__ seg) {
  const int l = threadIdx.x & (K7_GROUP - 1);
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) / K7_GROUP;
  if (rl >= n_rows) return;
  const lcr_read_record rr = rec[rl];
  const bool counting = (rr.assignment == 1 || rr.assignment == 2) && rr.phase_set != 0;
  const uint64_t row_word = counting ? (uint64_t)rr.phase_set | ((uint64_t)rr.assignment << COLSEG_HAP) : 0;
  const int64_t e1 = row_ptr[rl + 1];
  for (int64_t e = row_ptr[rl] + l; e < e1; e += K7_GROUP) {   // (a row longer than its lane group loops)
    const int32_t c = col[e];
    if ((uint32_t)c >= (uint32_t)n_cand) continue;
    const uint8_t v = val[e];
    const uint32_t left = atomicSub(&cnt[c], 1u);   // colseg_count counted this entry: left is in [1, segment length]
    const int64_t lo = off[c], hi = off[c + 1];
    const int64_t at = lo + (int64_t)left - 1;
    if (left == 0 || at >= hi) continue;            // (cannot happen while both walks see the same matrix)
    seg[at] = row_word | entry(c, v);
  }
}

template <class Entry>
void launch_colseg_fill(int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, const lcr_read_record* rec, Entry entry,
                        int32_t n_cand, uint32_t* cnt, const int64_t* off, uint64_t* seg, hipStream_t s) {
  if (n_rows <= 0 || n_cand <= 0) return;
  const long long threads = (long long)n_rows * K7_GROUP;
  hipLaunchKernelGGL(colseg_fill<Entry>, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, n_rows, row_ptr, col, val, rec,
                     entry, n_cand, cnt, off, seg);
}

struct ColPick { uint32_t lowq, best_ps, n_sets; };   // entries that do not count; the phase set with the most counted entries; distinct sets

// Called by the 64 lanes of the wave of one candidate, whose segment is [e0, e1); counted(w): the entry's quality reaches the threshold.
// One pass: the entries that do not count, minimum and maximum phase set of the counted entries of counting rows.  Where they differ,
// ascending sweeps over the distinct values, one pass each: "most entries, ties to the smallest value" is a strict > against the best so
// far, and nothing bounds the number of sets.  The result is the same in all lanes.
template <class Counted>
__device__ __forceinline__ ColPick colseg_pick(const uint64_t* __restrict__ seg, int64_t e0, int64_t e1, int lane, Counted counted) {
  uint32_t lowq = 0, lo = 0xffffffffu, hi = 0;
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const uint64_t w = seg[e];
    if (!counted(w)) { lowq++; continue; }
    const uint32_t ps = (uint32_t)w;
    if (ps != 0) { lo = min(lo, ps); hi = max(hi, ps); }
  }
  lowq = wave_sum_u32(lowq); lo = wave_min_u32(lo); hi = wave_max_u32(hi);
  ColPick r{lowq, 0, 0};
  if (hi != 0 && lo == hi) { r.n_sets = 1; r.best_ps = lo; }   // the usual column: one set
  else if (hi != 0) {
    uint32_t cur = lo, best_tot = 0;
    for (;;) {   // ascending over the distinct values: the count of `cur`, and the next one
      uint32_t n = 0, nxt = 0xffffffffu;
      for (int64_t e = e0 + lane; e < e1; e += 64) {
        const uint64_t w = seg[e];
        const uint32_t ps = (uint32_t)w;
        if (!counted(w) || ps == 0) continue;
        if (ps == cur) n++;
        else if (ps > cur) nxt = min(nxt, ps);
      }
      n = wave_sum_u32(n); nxt = wave_min_u32(nxt);
      r.n_sets++;
      if (n > best_tot) { best_tot = n; r.best_ps = cur; }   // (a strict >: ties to the smallest value)
      if (nxt == 0xffffffffu) break;
      cur = nxt;
    }
  }
  return r;
}

// k12_site_counts.hip — K12: allele x haplotype counts per candidate over the fragment matrix (lcr_site_counts).
//
// The contract (include/lcr.h) per candidate c, over the CSR entries with col == c.  The matrix is row-major, so the entries are grouped
// by destination first and summed per destination afterwards:
//   k12_count  eight lanes per row over its entries: one integer atomic per entry on its candidate's counter            -> cnt
//   (scan)     the counters to 64-bit segment offsets (launch_scan_i32_to_i64)                                           -> off
//   k12_fill   the same walk: one 8-byte word per entry into its candidate's segment -- the row's phase set (0 for a row that does not
//              count), its haplotype class, the base code, the low-quality bit.  The slot comes from the counter, counted back down to 0:
//              the order inside a segment is arbitrary, and everything behind it is a count                              -> seg
//   k12_sites  a wave64 per candidate, looping over its segment: low-quality entries, minimum and maximum phase set of the counted entries
//              of counting rows; where they differ, k7_sweep_phase_sets' ascending sweeps (a strict > keeps the smallest value; nothing
//              bounds the number of sets); then the twelve cells.  The first lane writes the record to HBM and to pinned host memory.
// All arithmetic is integer adds; nothing depends on the order in which atomics land.
#include "k7_sweep.h"

namespace {

// an entry's word: bits 0-31 phase set (0: not a counting row), 32-33 haplotype class (1 / 2 for a counting row, else 0), 34-35 base code,
// 36 quality below the threshold
constexpr int K12_CLS = 32, K12_BASE = 34, K12_LOWQ = 36;

__device__ __forceinline__ uint32_t k12_wave_max(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor(v, d, 64));
  return v;
}

__global__ void __launch_bounds__(LCR_BLOCK) k12_count(int32_t n_rows, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                        int32_t n_cand, uint32_t* __restrict__ cnt) {
  const int l = threadIdx.x & (K7_GROUP - 1);
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) / K7_GROUP;
  if (rl >= n_rows) return;
  const int64_t e1 = row_ptr[rl + 1];
  for (int64_t e = row_ptr[rl] + l; e < e1; e += K7_GROUP) {   // (a row longer than its lane group loops)
    const int32_t c = col[e];
    if ((uint32_t)c < (uint32_t)n_cand) atomicAdd(&cnt[c], 1u);
  }
}

__global__ void __launch_bounds__(LCR_BLOCK) k12_fill(int32_t n_rows, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                       const uint8_t* __restrict__ val, const lcr_read_record* __restrict__ rec, uint32_t min_baseq,
                                                       int32_t n_cand, uint32_t* __restrict__ cnt, const int64_t* __restrict__ off,
                                                       uint64_t* __restrict__ seg) {
  const int l = threadIdx.x & (K7_GROUP - 1);
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) / K7_GROUP;
  if (rl >= n_rows) return;
  const lcr_read_record rr = rec[rl];
  const bool counting = (rr.assignment == 1 || rr.assignment == 2) && rr.phase_set != 0;
  const uint64_t row_word = counting ? (uint64_t)rr.phase_set | ((uint64_t)rr.assignment << K12_CLS) : 0;
  const int64_t e1 = row_ptr[rl + 1];
  for (int64_t e = row_ptr[rl] + l; e < e1; e += K7_GROUP) {
    const int32_t c = col[e];
    if ((uint32_t)c >= (uint32_t)n_cand) continue;
    const uint8_t v = val[e];
    const uint32_t left = atomicSub(&cnt[c], 1u);   // k12_count counted this entry: left is in [1, segment length]
    const int64_t lo = off[c], hi = off[c + 1];
    const int64_t at = lo + (int64_t)left - 1;
    if (left == 0 || at >= hi) continue;            // (cannot happen while both walks see the same matrix)
    seg[at] = row_word | ((uint64_t)(v >> 6) << K12_BASE) | ((uint64_t)((uint32_t)(v & 31) < min_baseq) << K12_LOWQ);
  }
}

// One wave64 per candidate (four per workgroup); every value of the loops' state is the same in all lanes of the wave.
__global__ void __launch_bounds__(LCR_BLOCK) k12_sites(const lcr_candidate* __restrict__ cand, int32_t n_cand, const int64_t* __restrict__ off,
                                                        const uint64_t* __restrict__ seg, lcr_site_count* __restrict__ out,
                                                        lcr_site_count* __restrict__ host_out) {
  const int lane = threadIdx.x & 63;
  const long long cl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) >> 6;
  if (cl >= n_cand) return;   // (a whole wave leaves)
  const int c = (int)cl;
  const int64_t e0 = off[c], e1 = off[c + 1];
  const uint32_t own = cand[c].phase_set;
  // low-quality entries; the range of the phase sets among the counted entries of counting rows
  uint32_t lowq = 0, lo = 0xffffffffu, hi = 0;
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const uint64_t w = seg[e];
    if ((w >> K12_LOWQ) & 1) { lowq++; continue; }
    const uint32_t ps = (uint32_t)w;
    if (ps != 0) { lo = min(lo, ps); hi = max(hi, ps); }
  }
  lowq = k7_wave_sum(lowq); lo = k7_wave_min(lo); hi = k12_wave_max(hi);
  uint32_t n_sets = 0, best_ps = 0;
  if (hi != 0 && lo == hi) { n_sets = 1; best_ps = lo; }   // the usual column: one set
  else if (hi != 0) {
    uint32_t cur = lo, best_tot = 0;
    for (;;) {   // ascending over the distinct values: the count of `cur`, and the next one
      uint32_t n = 0, nxt = 0xffffffffu;
      for (int64_t e = e0 + lane; e < e1; e += 64) {
        const uint64_t w = seg[e];
        const uint32_t ps = (uint32_t)w;
        if (((w >> K12_LOWQ) & 1) || ps == 0) continue;
        if (ps == cur) n++;
        else if (ps > cur) nxt = min(nxt, ps);
      }
      n = k7_wave_sum(n); nxt = k7_wave_min(nxt);
      n_sets++;
      if (n > best_tot) { best_tot = n; best_ps = cur; }   // (a strict >: ties to the smallest value)
      if (nxt == 0xffffffffu) break;
      cur = nxt;
    }
  }
  const uint32_t site_ps = own != 0 ? own : best_ps;
  // the twelve cells: k = the row's haplotype when it counts and is in the site's set, else 0
  uint32_t n[12];
#pragma unroll
  for (int j = 0; j < 12; j++) n[j] = 0;
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const uint64_t w = seg[e];
    if ((w >> K12_LOWQ) & 1) continue;
    const uint32_t ps = (uint32_t)w;
    const int k = (ps != 0 && ps == site_ps) ? (int)((w >> K12_CLS) & 3) : 0;
    const int cell = k * 4 + (int)((w >> K12_BASE) & 3);
#pragma unroll
    for (int j = 0; j < 12; j++) n[j] += (cell == j);
  }
#pragma unroll
  for (int j = 0; j < 12; j++) n[j] = k7_wave_sum(n[j]);
  if (lane != 0) return;
  lcr_site_count o;
  o.phase_set = site_ps; o.n_phase_sets = n_sets; o.n_entries = (uint32_t)(e1 - e0); o.n_lowq = lowq;
#pragma unroll
  for (int j = 0; j < 12; j++) o.n[j >> 2][j & 3] = n[j];
  out[c] = o;
  host_out[c] = o;
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_k12_count(int32_t n_rows, const int64_t* row_ptr, const int32_t* col, int32_t n_cand, uint32_t* cnt, hipStream_t s) {
  if (n_rows <= 0 || n_cand <= 0) return;
  const long long threads = (long long)n_rows * K7_GROUP;
  hipLaunchKernelGGL(k12_count, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, n_rows, row_ptr, col, n_cand, cnt);
}
void launch_k12_fill(int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, const lcr_read_record* rec, uint32_t min_baseq,
                     int32_t n_cand, uint32_t* cnt, const int64_t* off, uint64_t* seg, hipStream_t s) {
  if (n_rows <= 0 || n_cand <= 0) return;
  const long long threads = (long long)n_rows * K7_GROUP;
  hipLaunchKernelGGL(k12_fill, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, n_rows, row_ptr, col, val, rec, min_baseq,
                     n_cand, cnt, off, seg);
}
void launch_k12_sites(const lcr_candidate* cand, int32_t n_cand, const int64_t* off, const uint64_t* seg, lcr_site_count* out, lcr_site_count* host_out,
                      hipStream_t s) {
  if (n_cand <= 0) return;
  const long long threads = (long long)n_cand * 64;
  hipLaunchKernelGGL(k12_sites, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, cand, n_cand, off, seg, out, host_out);
}

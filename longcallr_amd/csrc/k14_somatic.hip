// k14_somatic.hip — K14: the three-class model (reference / heterozygous / somatic) per haplotype at every candidate, over the fragment
// matrix (lcr_somatic).
//
// The contract (include/lcr.h) per candidate c, over the CSR entries with col == c.  The matrix is row-major and the result is per column:
// K12's answer (k12_site_counts.hip), group by destination first, sum afterwards.  The per-candidate entry counts and their 64-bit offsets
// are K12's own launches (launch_k12_count, launch_scan_i32_to_i64); what differs is the word and what is summed:
//   k14_fill   eight lanes per row over its entries: one 8-byte word per entry into its candidate's segment -- the row's phase set (0 for a
//              row that does not count), its haplotype, whether the base is the candidate's reference base, and q as five bits.  The slot
//              comes from the counter, counted back down to 0: the order inside a segment is arbitrary, and every result is a sum -> seg
//   k14_sites  a wave64 per candidate, looping over its segment: entries below the threshold; minimum and maximum phase set of the counted
//              entries of counting rows and, where they differ, k12_sites' ascending sweeps; then one pass with the four counts, n_other and
//              the six 64-bit sums from the tables in LDS, folded with xor shuffles.  The first lane compares integers and writes the record
//              to HBM and to pinned host memory.
// All arithmetic is integer adds and compares; nothing depends on the order in which atomics land.
#include "k7_sweep.h"

namespace {

// an entry's word: bits 0-31 phase set (0: not a counting row), 32-33 haplotype (1 / 2 for a counting row, else 0), 34 the base is the
// candidate's reference base, 35-39 q
constexpr int K14_HAP = 32, K14_REF = 34, K14_Q = 35;
constexpr uint32_t K14_DEEP = 1u << 20;   // counted entries per haplotype up to which the sums are exact (every table entry is below 2^42)

__device__ __forceinline__ uint32_t k14_wave_max(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor(v, d, 64));
  return v;
}
// (a 64-bit shuffle is two 32-bit ones; the adds wrap as unsigned, so a column beyond K14_DEEP -- whose sums are discarded -- is defined too)
__device__ __forceinline__ unsigned long long k14_wave_sum64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ void __launch_bounds__(LCR_BLOCK) k14_fill(int32_t n_rows, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                       const uint8_t* __restrict__ val, const lcr_read_record* __restrict__ rec,
                                                       const lcr_candidate* __restrict__ cand, int32_t n_cand, uint32_t* __restrict__ cnt,
                                                       const int64_t* __restrict__ off, uint64_t* __restrict__ seg) {
  const int l = threadIdx.x & (K7_GROUP - 1);
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) / K7_GROUP;
  if (rl >= n_rows) return;
  const lcr_read_record rr = rec[rl];
  const bool counting = (rr.assignment == 1 || rr.assignment == 2) && rr.phase_set != 0;
  const uint64_t row_word = counting ? (uint64_t)rr.phase_set | ((uint64_t)rr.assignment << K14_HAP) : 0;
  const int64_t e1 = row_ptr[rl + 1];
  for (int64_t e = row_ptr[rl] + l; e < e1; e += K7_GROUP) {   // (a row longer than its lane group loops)
    const int32_t c = col[e];
    if ((uint32_t)c >= (uint32_t)n_cand) continue;
    const uint8_t v = val[e];
    const uint32_t left = atomicSub(&cnt[c], 1u);   // launch_k12_count counted this entry: left is in [1, segment length]
    const int64_t lo = off[c], hi = off[c + 1];
    const int64_t at = lo + (int64_t)left - 1;
    if (left == 0 || at >= hi) continue;            // (cannot happen while both walks see the same matrix)
    const uint64_t is_ref = (int)(v >> 6) == base_code(cand[c].ref_base);
    seg[at] = row_word | (is_ref << K14_REF) | ((uint64_t)(v & 31) << K14_Q);
  }
}

// One wave64 per candidate (four per workgroup); every value of the loops' state is the same in all lanes of the wave.
__global__ void __launch_bounds__(LCR_BLOCK) k14_sites(const lcr_candidate* __restrict__ cand, int32_t n_cand, const int64_t* __restrict__ off,
                                                        const uint64_t* __restrict__ seg, K14Tables t, uint32_t min_baseq,
                                                        lcr_somatic_site* __restrict__ out, lcr_somatic_site* __restrict__ host_out) {
  // the tables: a lane's q is its own, so the kernel argument (scalar registers) goes to LDS once per workgroup and is read per lane
  __shared__ int64_t tab[4 * 31];   // fe, f1e, fs_ref, fs_alt
  if (threadIdx.x < 4 * 31) tab[threadIdx.x] = t.tab[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long long cl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) >> 6;
  if (cl >= n_cand) return;   // (a whole wave leaves, behind the workgroup's only barrier)
  const int c = (int)cl;
  const int64_t e0 = off[c], e1 = off[c + 1];
  const uint32_t own = cand[c].phase_set;
  // entries below the threshold; the range of the phase sets among the counted entries of counting rows
  uint32_t lowq = 0, lo = 0xffffffffu, hi = 0;
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const uint64_t w = seg[e];
    if ((uint32_t)(w >> K14_Q) < min_baseq) { lowq++; continue; }   // (q is the word's top field)
    const uint32_t ps = (uint32_t)w;
    if (ps != 0) { lo = min(lo, ps); hi = max(hi, ps); }
  }
  lowq = k7_wave_sum(lowq); lo = k7_wave_min(lo); hi = k14_wave_max(hi);
  uint32_t best_ps = 0;
  if (hi != 0 && lo == hi) best_ps = lo;   // the usual column: one set
  else if (hi != 0) {
    uint32_t cur = lo, best_tot = 0;
    for (;;) {   // ascending over the distinct values: the count of `cur`, and the next one (k12_sites' sweeps)
      uint32_t n = 0, nxt = 0xffffffffu;
      for (int64_t e = e0 + lane; e < e1; e += 64) {
        const uint64_t w = seg[e];
        const uint32_t ps = (uint32_t)w;
        if ((uint32_t)(w >> K14_Q) < min_baseq || ps == 0) continue;
        if (ps == cur) n++;
        else if (ps > cur) nxt = min(nxt, ps);
      }
      n = k7_wave_sum(n); nxt = k7_wave_min(nxt);
      if (n > best_tot) { best_tot = n; best_ps = cur; }   // (a strict >: ties to the smallest value)
      if (nxt == 0xffffffffu) break;
      cur = nxt;
    }
  }
  const uint32_t site_ps = own != 0 ? own : best_ps;
  // the four counts, n_other and the six sums: [haplotype - 1][ref, het, som]
  uint32_t n[4] = {0, 0, 0, 0}, other = 0;
  unsigned long long s[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const uint64_t w = seg[e];
    const uint32_t q = (uint32_t)(w >> K14_Q);
    if (q < min_baseq) continue;
    const uint32_t ps = (uint32_t)w;
    if (ps == 0 || ps != site_ps) { other++; continue; }
    const int h = (int)((w >> K14_HAP) & 3) - 1;   // 0 / 1: a word with a phase set is a counting row's
    const bool is_ref = (w >> K14_REF) & 1;
    const uint32_t qi = min(q, 30u);   // (the fragment matrix clamps qualities to 30; the table has 31 rows)
    const unsigned long long fe = (unsigned long long)tab[qi], f1e = (unsigned long long)tab[31 + qi],
                             fs = (unsigned long long)tab[(is_ref ? 62 : 93) + qi];
    const unsigned long long a_ref = is_ref ? f1e : fe, a_het = is_ref ? fe : f1e;
#pragma unroll
    for (int k = 0; k < 2; k++) {   // (static register indices)
      const bool m = h == k;
      n[k * 2] += m && is_ref; n[k * 2 + 1] += m && !is_ref;
      s[k * 3] += m ? a_ref : 0; s[k * 3 + 1] += m ? a_het : 0; s[k * 3 + 2] += m ? fs : 0;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; j++) n[j] = k7_wave_sum(n[j]);
  other = k7_wave_sum(other);
#pragma unroll
  for (int j = 0; j < 6; j++) s[j] = k14_wave_sum64(s[j]);
  if (lane != 0) return;
  const lcr_candidate& cc = cand[c];
  lcr_somatic_site o;
  o.phase_set = site_ps;
  o.n[0][0] = n[0]; o.n[0][1] = n[1]; o.n[1][0] = n[2]; o.n[1][1] = n[3];
  o.n_other = other; o.n_lowq = lowq;
  o.cls[0] = o.cls[1] = 0; o.call = 0;
#pragma unroll
  for (int j = 0; j < 6; j++) o.L[j / 3][j % 3] = 0;
  o.status = (cc.allele1 != cc.ref_base && cc.allele2 != cc.ref_base) ? LCR_SOM_ALLELES
             : (n[0] + n[1] > K14_DEEP || n[2] + n[3] > K14_DEEP) ? LCR_SOM_DEEP : LCR_SOM_OK;
  if (o.status == LCR_SOM_OK) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int64_t l_ref = t.prior[0] + (int64_t)s[h * 3], l_het = t.prior[1] + (int64_t)s[h * 3 + 1], l_som = t.prior[2] + (int64_t)s[h * 3 + 2];
      o.L[h][0] = l_ref; o.L[h][1] = l_het; o.L[h][2] = l_som;
      o.cls[h] = (l_som > l_ref && l_som > l_het) ? 2 : (l_het > l_ref && l_het > l_som) ? 1 : 0;   // somatic.rs:38-44
    }
    if (cc.flags & LCR_F_CAND_SOMATIC) o.call = (o.cls[0] == 0 && o.cls[1] == 2) ? 2 : (o.cls[0] == 2 && o.cls[1] == 0) ? 1 : 0;   // snpfrags.rs:753-765
  }
  out[c] = o;
  host_out[c] = o;
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_k14_fill(int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, const lcr_read_record* rec, const lcr_candidate* cand,
                     int32_t n_cand, uint32_t* cnt, const int64_t* off, uint64_t* seg, hipStream_t s) {
  if (n_rows <= 0 || n_cand <= 0) return;
  const long long threads = (long long)n_rows * K7_GROUP;
  hipLaunchKernelGGL(k14_fill, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, n_rows, row_ptr, col, val, rec, cand,
                     n_cand, cnt, off, seg);
}
void launch_k14_sites(const lcr_candidate* cand, int32_t n_cand, const int64_t* off, const uint64_t* seg, const K14Tables& t, uint32_t min_baseq,
                      lcr_somatic_site* out, lcr_somatic_site* host_out, hipStream_t s) {
  if (n_cand <= 0) return;
  const long long threads = (long long)n_cand * 64;
  hipLaunchKernelGGL(k14_sites, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, cand, n_cand, off, seg, t, min_baseq,
                     out, host_out);
}

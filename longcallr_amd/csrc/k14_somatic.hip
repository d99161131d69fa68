// k14_somatic.hip — K14: the three-class model (reference / heterozygous / somatic) per haplotype at every candidate, over the fragment
// matrix (lcr_somatic).
//
// The contract (include/lcr.h) per candidate c, over the CSR entries with col == c, grouped into K12's per-candidate segments
// (col_segments.h; launch_colseg_count and launch_scan_i32_to_i64 size them); what differs is the word and what is summed:
//   colseg_fill<K14Entry>   one word per entry into its candidate's segment: beside the row's part whether the base is the candidate's
//                           reference base, and q as five bits                                                                -> seg
//   k14_sites               a wave64 per candidate, looping over its segment: colseg_pick (entries below the threshold, the phase set with
//                           the most counted entries); then one pass with the four counts, n_other and the six 64-bit sums from the tables
//                           in LDS, folded with xor shuffles (the adds wrap as unsigned, so a column beyond K14_DEEP -- whose sums are
//                           discarded -- is defined too).  The first lane compares integers and writes the record to HBM and to pinned
//                           host memory.
// All arithmetic is integer adds and compares; nothing depends on the order in which atomics land.
#include "col_segments.h"

namespace {

// the unit's bits of an entry's word: 34 the base is the candidate's reference base, 35-39 q (the word's top field)
constexpr int K14_REF = COLSEG_OWN, K14_Q = COLSEG_OWN + 1;
constexpr uint32_t K14_DEEP = 1u << 20;   // counted entries per haplotype up to which the sums are exact (every table entry is below 2^42)

struct K14Entry {
  const lcr_candidate* cand;
  __device__ uint64_t operator()(int32_t c, uint8_t v) const {
    const uint64_t is_ref = (int)(v >> 6) == base_code(cand[c].ref_base);
    return (is_ref << K14_REF) | ((uint64_t)(v & 31) << K14_Q);
  }
};

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
  const ColPick pick = colseg_pick(seg, e0, e1, lane, [&](uint64_t w) { return (uint32_t)(w >> K14_Q) >= min_baseq; });
  const uint32_t site_ps = own != 0 ? own : pick.best_ps;
  // the four counts, n_other and the six sums: [haplotype - 1][ref, het, som]
  uint32_t n[4] = {0, 0, 0, 0}, other = 0;
  unsigned long long s[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const uint64_t w = seg[e];
    const uint32_t q = (uint32_t)(w >> K14_Q);
    if (q < min_baseq) continue;
    const uint32_t ps = (uint32_t)w;
    if (ps == 0 || ps != site_ps) { other++; continue; }
    const int h = (int)((w >> COLSEG_HAP) & 3) - 1;   // 0 / 1: a word with a phase set is a counting row's
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
  for (int j = 0; j < 4; j++) n[j] = wave_sum_u32(n[j]);
  other = wave_sum_u32(other);
#pragma unroll
  for (int j = 0; j < 6; j++) s[j] = wave_sum_u64(s[j]);
  if (lane != 0) return;
  const lcr_candidate& cc = cand[c];
  lcr_somatic_site o;
  o.phase_set = site_ps;
  o.n[0][0] = n[0]; o.n[0][1] = n[1]; o.n[1][0] = n[2]; o.n[1][1] = n[3];
  o.n_other = other; o.n_lowq = pick.lowq;
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
  launch_colseg_fill(n_rows, row_ptr, col, val, rec, K14Entry{cand}, n_cand, cnt, off, seg, s);
}
void launch_k14_sites(const lcr_candidate* cand, int32_t n_cand, const int64_t* off, const uint64_t* seg, const K14Tables& t, uint32_t min_baseq,
                      lcr_somatic_site* out, lcr_somatic_site* host_out, hipStream_t s) {
  if (n_cand <= 0) return;
  const long long threads = (long long)n_cand * 64;
  hipLaunchKernelGGL(k14_sites, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, cand, n_cand, off, seg, t, min_baseq,
                     out, host_out);
}

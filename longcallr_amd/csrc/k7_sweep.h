// k7_sweep.h — what K7 (k7_ase.hip, per region) and the per-gene counts of K8 (k8_genes.hip, per region and gene) share: the sweep over the
// phase sets of a group of counting rows, and a row's parent-of-origin vote.  Device code only.
#pragma once
#include "lcr_dev.h"

struct K7Pick { uint32_t ps, n_sets, h1, h2; };   // the phase set with the most counting rows (0 = none), distinct sets, its rows per haplotype

// Called by every thread of one workgroup.  Over the rows [r0, r1) that `keep(r)` lets through: sweep k counts h1 / h2 of the k-th smallest
// phase set among the counting rows -- assignment 1 / 2 and a phase set -- and finds the next one (the first sweep, cur = 0, only finds the
// smallest: a counting row's phase set is not 0).  Every thread keeps its counts in registers, a wave adds them up with shuffles and its
// first lane does the three LDS atomics of the sweep: twelve per sweep and workgroup, whatever the depth.  "Most rows, ties to the smallest
// value" is a strict > against the best so far.  A group has a handful of phase sets; nothing bounds their number.  sh: three words of LDS;
// the result is the same in all threads.
template <class Keep>
__device__ __forceinline__ K7Pick k7_sweep_phase_sets(const lcr_read_record* __restrict__ rec, int r0, int r1, Keep keep, uint32_t* sh) {
  const int tid = threadIdx.x;
  uint32_t cur = 0;
  K7Pick best{0, 0, 0, 0};
  uint32_t best_tot = 0;
  for (;;) {   // (every value of the loop's state is the same in all threads)
    if (tid == 0) { sh[0] = 0xffffffffu; sh[1] = 0; sh[2] = 0; }
    __syncthreads();
    uint32_t c1 = 0, c2 = 0, nxt = 0xffffffffu;
    for (int r = r0 + tid; r < r1; r += LCR_BLOCK) {
      const lcr_read_record rr = rec[r];
      if ((rr.assignment != 1 && rr.assignment != 2) || rr.phase_set == 0 || !keep(r)) continue;
      if (rr.phase_set == cur) { if (rr.assignment == 1) c1++; else c2++; }
      else if (rr.phase_set > cur) nxt = min(nxt, rr.phase_set);
    }
    c1 = wave_sum_u32(c1); c2 = wave_sum_u32(c2); nxt = wave_min_u32(nxt);
    if ((tid & 63) == 0) {
      if (c1) atomicAdd(&sh[1], c1);
      if (c2) atomicAdd(&sh[2], c2);
      if (nxt != 0xffffffffu) atomicMin(&sh[0], nxt);
    }
    __syncthreads();
    const uint32_t next = sh[0], t1 = sh[1], t2 = sh[2];
    __syncthreads();
    if (cur != 0) {
      best.n_sets++;
      if (t1 + t2 > best_tot) { best_tot = t1 + t2; best.ps = cur; best.h1 = t1; best.h2 = t2; }
    }
    if (next == 0xffffffffu) break;
    cur = next;
  }
  return best;
}

constexpr int K7_GROUP = 8;   // lanes per row in the vote kernels: rows of the gene workloads hold a handful of entries, tens at most

// The vote of one row by the K7_GROUP lanes of its group (lane l of them): entries [e0, e1) of the CSR; site_of(candidate) gives the site
// byte -- bit0 eligible, bits1-2 pat code, bits3-4 mat code -- of an entry's candidate.  A row with more than eight entries takes further
// rounds; every lane of a group takes the same branches; the counts are added up inside the group with three xor shuffles.
// -> +1 paternal, -1 maternal, 0 no vote (the same in every lane of the group).
template <class SiteOf>
__device__ __forceinline__ int k7_row_vote(int64_t e0, int64_t e1, int l, const int32_t* __restrict__ col, const uint8_t* __restrict__ val,
                                           uint32_t min_baseq, SiteOf site_of) {
  int np = 0, nm = 0;
  for (int64_t e = e0 + l; e < e1; e += K7_GROUP) {
    const uint8_t sb = site_of(col[e]), v = val[e];
    if (!(sb & 1) || (uint32_t)(v & 31) < min_baseq) continue;
    const int code = v >> 6;
    if (code == ((sb >> 1) & 3)) np++;
    else if (code == ((sb >> 3) & 3)) nm++;
  }
#pragma unroll
  for (int d = K7_GROUP / 2; d >= 1; d >>= 1) { np += __shfl_xor(np, d, 64); nm += __shfl_xor(nm, d, 64); }
  return np > nm ? 1 : np < nm ? -1 : 0;
}

__device__ __forceinline__ int k7_code(uint8_t b) {   // upper-case ACGT only: a parental allele is a VCF's REF / ALT byte
  return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : -1;
}

// lcr_ase's eligibility (1), (2) and (4) of a candidate -- what does not depend on the region's (or pair's) phase set: the VCF writer would
// print it PASS with a phased het GT (vcf.format_records: the RDS=select branch with phase_score >= min_phase_score and variant_type 1
// prints 0|1 / 1|0 and PASS, and the record is written when one of the two alleles is an ALT), it has a phase set, and its position is a
// parental one (binary search).  -> the site byte without bit0 decided: 0 when not eligible, else 1 | pat << 1 | mat << 3.
__device__ __forceinline__ uint8_t k7_site_byte(const lcr_candidate* __restrict__ s, double min_phase_score, const int64_t* __restrict__ pos0,
                                                const uint8_t* __restrict__ pat, const uint8_t* __restrict__ mat, int32_t n_sites) {
  const uint32_t fl = s->flags;
  const bool ok = !(fl & (LCR_F_DENSE | LCR_F_NON_SELECTED)) && s->variant_type == 1 && s->phase_score >= min_phase_score &&
                  (s->allele1 != s->ref_base || s->allele2 != s->ref_base) && s->phase_set != 0;
  if (!ok) return 0;
  const int64_t p = s->pos;
  int lo = 0, hi = n_sites;   // first site with pos0 >= p
  while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (pos0[mid] < p) lo = mid + 1; else hi = mid; }
  if (lo < n_sites && pos0[lo] == p) return (uint8_t)(1 | (k7_code(pat[lo]) << 1) | (k7_code(mat[lo]) << 3));
  return 0;
}

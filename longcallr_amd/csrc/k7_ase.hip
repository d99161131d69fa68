// k7_ase.hip — K7: haplotype and parent-of-origin counts per region over the phased rows (lcr_ase; DESIGN.md "Allele-specific expression").
//
// The contract (include/lcr.h) per region g, over the COUNTING rows -- fragment rows with assignment 1 / 2 and a phase set:
//   k7_check   the caller's parental sites: ascending unique positions, pat / mat in ACGT and different      -> verdict (pinned host memory)
//   k7_pick    one workgroup per region: the phase sets of its counting rows in ascending order, one sweep each; the one with the most
//              rows (a strict >: ties to the smallest value), its h1 / h2, the number of sets; with sites, one more sweep tags the rows
//              of the chosen set {region, haplotype}                                                         -> record, row_tag
//   k7_sites   per candidate: would the VCF writer print it PASS with a phased het GT, is its phase set the region's, is its position a
//              parental one (binary search)                                                                   -> site byte, n_sites
//   k7_votes   eight lanes per tagged row over its CSR entries: bases that equal pat / mat at eligible sites, reduced inside the group,
//              one integer atomic per voting row into the region's four cells
//   k7_export  the finished records to pinned host memory (without sites k7_pick writes them itself)
// All arithmetic is integer adds; nothing depends on the order in which atomics land.
#include <algorithm>

#include "lcr_dev.h"

namespace {

constexpr int K7_GROUP = 8;   // lanes per row in k7_votes: rows of the gene workloads hold a handful of entries, tens at most

__device__ __forceinline__ int k7_code(uint8_t b) {   // upper-case ACGT only: a parental allele is a VCF's REF / ALT byte
  return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : -1;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, 64));
  return v;
}

__global__ void __launch_bounds__(LCR_BLOCK) k7_check(const int64_t* __restrict__ pos0, const uint8_t* __restrict__ pat,
                                                       const uint8_t* __restrict__ mat, int32_t n_sites, int32_t* __restrict__ bad) {
  const int32_t i = (int32_t)(blockIdx.x * LCR_BLOCK + threadIdx.x);
  if (i >= n_sites) return;
  const int p = k7_code(pat[i]), m = k7_code(mat[i]);
  if (p < 0 || m < 0 || p == m || (i > 0 && pos0[i - 1] >= pos0[i])) *bad = 1;   // (every writer stores the same value: a plain store)
}

// One workgroup per region.  Sweep k counts h1 / h2 of the k-th smallest phase set among the counting rows and finds the next one (the
// first sweep, cur = 0, only finds the smallest: a counting row's phase set is not 0).  Every thread keeps its counts in registers, a
// wave adds them up with shuffles and its first lane does the three LDS atomics of the sweep: twelve per sweep and workgroup, whatever
// the region's depth.  A region has a handful of phase sets; nothing bounds their number.
__global__ void __launch_bounds__(LCR_BLOCK) k7_pick(const int32_t* __restrict__ row_region_off, const lcr_read_record* __restrict__ rec,
                                                      int32_t ng, lcr_ase_region* __restrict__ out, lcr_ase_region* __restrict__ host_out,
                                                      int32_t* __restrict__ row_tag) {
  __shared__ uint32_t sh_next, sh_c1, sh_c2;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g >= ng) return;
  const int r0 = row_region_off[g], r1 = row_region_off[g + 1];
  uint32_t cur = 0, n_sets = 0, best_ps = 0, best_tot = 0, best1 = 0, best2 = 0;
  for (;;) {   // (every value of the loop's state is the same in all threads)
    if (tid == 0) { sh_next = 0xffffffffu; sh_c1 = 0; sh_c2 = 0; }
    __syncthreads();
    uint32_t c1 = 0, c2 = 0, nxt = 0xffffffffu;
    for (int r = r0 + tid; r < r1; r += LCR_BLOCK) {
      const lcr_read_record rr = rec[r];
      if ((rr.assignment != 1 && rr.assignment != 2) || rr.phase_set == 0) continue;
      if (rr.phase_set == cur) { if (rr.assignment == 1) c1++; else c2++; }
      else if (rr.phase_set > cur) nxt = min(nxt, rr.phase_set);
    }
    c1 = wave_sum(c1); c2 = wave_sum(c2); nxt = wave_min(nxt);
    if ((tid & 63) == 0) {
      if (c1) atomicAdd(&sh_c1, c1);
      if (c2) atomicAdd(&sh_c2, c2);
      if (nxt != 0xffffffffu) atomicMin(&sh_next, nxt);
    }
    __syncthreads();
    const uint32_t next = sh_next, t1 = sh_c1, t2 = sh_c2;
    __syncthreads();
    if (cur != 0) {
      n_sets++;
      if (t1 + t2 > best_tot) { best_tot = t1 + t2; best_ps = cur; best1 = t1; best2 = t2; }
    }
    if (next == 0xffffffffu) break;
    cur = next;
  }
  if (row_tag)   // the rows that vote: region and haplotype in one word, 0 for every other row
    for (int r = r0 + tid; r < r1; r += LCR_BLOCK) {
      const lcr_read_record rr = rec[r];
      const bool sel = best_ps != 0 && rr.phase_set == best_ps && (rr.assignment == 1 || rr.assignment == 2);
      row_tag[r] = sel ? (g << 2) | rr.assignment : 0;
    }
  if (tid == 0) {
    lcr_ase_region o{};
    o.region = g; o.phase_set = best_ps; o.n_phase_sets = n_sets; o.h1 = best1; o.h2 = best2;
    out[g] = o;
    if (host_out) host_out[g] = o;
  }
}

// site byte: bit0 eligible, bits1-2 pat code, bits3-4 mat code
__global__ void __launch_bounds__(LCR_BLOCK) k7_sites(const lcr_candidate* __restrict__ cand, int32_t n_cand, double min_phase_score,
                                                       const int64_t* __restrict__ pos0, const uint8_t* __restrict__ pat,
                                                       const uint8_t* __restrict__ mat, int32_t n_sites, lcr_ase_region* __restrict__ ase,
                                                       uint8_t* __restrict__ site) {
  const int32_t i = (int32_t)(blockIdx.x * LCR_BLOCK + threadIdx.x);
  if (i >= n_cand) return;
  const lcr_candidate* __restrict__ s = cand + i;
  uint8_t b = 0;
  const uint32_t fl = s->flags, ps = s->phase_set;
  const int g = s->region;
  // vcf.format_records: the RDS=select branch with phase_score >= min_phase_score and variant_type 1 prints 0|1 / 1|0 and PASS, and the
  // record is written when one of the two alleles is an ALT
  bool ok = !(fl & (LCR_F_DENSE | LCR_F_NON_SELECTED)) && s->variant_type == 1 && s->phase_score >= min_phase_score &&
            (s->allele1 != s->ref_base || s->allele2 != s->ref_base) && ps != 0;
  if (ok) ok = ps == ase[g].phase_set;
  if (ok) {
    const int64_t p = s->pos;
    int lo = 0, hi = n_sites;   // first site with pos0 >= p
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (pos0[mid] < p) lo = mid + 1; else hi = mid; }
    if (lo < n_sites && pos0[lo] == p) {
      b = (uint8_t)(1 | (k7_code(pat[lo]) << 1) | (k7_code(mat[lo]) << 3));
      atomicAdd(&ase[g].n_sites, 1u);
    }
  }
  site[i] = b;
}

// Eight lanes per row (eight rows per wave64); a row with more than eight entries takes further rounds.  Every lane of a group takes
// the same branches; the counts are added up inside the group with three xor shuffles.
__global__ void __launch_bounds__(LCR_BLOCK) k7_votes(const int32_t* __restrict__ row_tag, int32_t n_rows, const int64_t* __restrict__ row_ptr,
                                                       const int32_t* __restrict__ col, const uint8_t* __restrict__ val,
                                                       const uint8_t* __restrict__ site, uint32_t min_baseq, lcr_ase_region* __restrict__ ase) {
  const int l = threadIdx.x & (K7_GROUP - 1);
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) / K7_GROUP;
  if (rl >= n_rows) return;   // (a whole group leaves)
  const int r = (int)rl;
  const int tag = row_tag[r];
  if (tag == 0) return;
  const int64_t e0 = row_ptr[r], e1 = row_ptr[r + 1];
  int np = 0, nm = 0;
  for (int64_t e = e0 + l; e < e1; e += K7_GROUP) {
    const uint8_t sb = site[col[e]], v = val[e];
    if (!(sb & 1) || (uint32_t)(v & 31) < min_baseq) continue;
    const int code = v >> 6;
    if (code == ((sb >> 1) & 3)) np++;
    else if (code == ((sb >> 3) & 3)) nm++;
  }
#pragma unroll
  for (int d = K7_GROUP / 2; d >= 1; d >>= 1) { np += __shfl_xor(np, d, 64); nm += __shfl_xor(nm, d, 64); }
  if (l != 0 || np == nm) return;
  lcr_ase_region* o = ase + (tag >> 2);
  const bool h1 = (tag & 3) == 1;
  atomicAdd(np > nm ? (h1 ? &o->h1_pat : &o->h2_pat) : (h1 ? &o->h1_mat : &o->h2_mat), 1u);
}

__global__ void k7_export(const lcr_ase_region* __restrict__ ase, int32_t ng, lcr_ase_region* __restrict__ host_out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < ng) host_out[g] = ase[g];
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_k7_check(const int64_t* pos0, const uint8_t* pat, const uint8_t* mat, int32_t n_sites, int32_t* bad, hipStream_t s) {
  if (n_sites > 0) hipLaunchKernelGGL(k7_check, dim3((n_sites + LCR_BLOCK - 1) / LCR_BLOCK), dim3(LCR_BLOCK), 0, s, pos0, pat, mat, n_sites, bad);
}
void launch_k7_pick(const int32_t* row_region_off, const lcr_read_record* rec, int32_t ng, lcr_ase_region* out, lcr_ase_region* host_out,
                    int32_t* row_tag, hipStream_t s) {
  if (ng > 0) hipLaunchKernelGGL(k7_pick, dim3(ng), dim3(LCR_BLOCK), 0, s, row_region_off, rec, ng, out, host_out, row_tag);
}
void launch_k7_sites(const lcr_candidate* cand, int32_t n_cand, double min_phase_score, const int64_t* pos0, const uint8_t* pat,
                     const uint8_t* mat, int32_t n_sites, lcr_ase_region* ase, uint8_t* site, hipStream_t s) {
  if (n_cand > 0) hipLaunchKernelGGL(k7_sites, dim3((n_cand + LCR_BLOCK - 1) / LCR_BLOCK), dim3(LCR_BLOCK), 0, s, cand, n_cand, min_phase_score, pos0, pat, mat,
                                     n_sites, ase, site);
}
void launch_k7_votes(const int32_t* row_tag, int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, const uint8_t* site,
                     uint32_t min_baseq, lcr_ase_region* ase, hipStream_t s) {
  if (n_rows <= 0) return;
  const long long threads = (long long)n_rows * K7_GROUP;
  hipLaunchKernelGGL(k7_votes, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, row_tag, n_rows, row_ptr, col, val, site,
                     min_baseq, ase);
}
void launch_k7_export(const lcr_ase_region* ase, int32_t ng, lcr_ase_region* host_out, hipStream_t s) {
  if (ng > 0) hipLaunchKernelGGL(k7_export, dim3((ng + 255) / 256), dim3(256), 0, s, ase, ng, host_out);
}

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

#include "k7_sweep.h"

namespace {

__global__ void __launch_bounds__(LCR_BLOCK) k7_check(const int64_t* __restrict__ pos0, const uint8_t* __restrict__ pat,
                                                       const uint8_t* __restrict__ mat, int32_t n_sites, int32_t* __restrict__ bad) {
  const int32_t i = (int32_t)(blockIdx.x * LCR_BLOCK + threadIdx.x);
  if (i >= n_sites) return;
  const int p = k7_code(pat[i]), m = k7_code(mat[i]);
  if (p < 0 || m < 0 || p == m || (i > 0 && pos0[i - 1] >= pos0[i])) *bad = 1;   // (every writer stores the same value: a plain store)
}

// One workgroup per region: the sweep over the phase sets of its counting rows (k7_sweep.h), then the tags of the rows that vote.
__global__ void __launch_bounds__(LCR_BLOCK) k7_pick(const int32_t* __restrict__ row_region_off, const lcr_read_record* __restrict__ rec,
                                                      int32_t ng, lcr_ase_region* __restrict__ out, lcr_ase_region* __restrict__ host_out,
                                                      int32_t* __restrict__ row_tag) {
  __shared__ uint32_t sh[3];
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g >= ng) return;
  const int r0 = row_region_off[g], r1 = row_region_off[g + 1];
  const K7Pick best = k7_sweep_phase_sets(rec, r0, r1, [](int) { return true; }, sh);
  const uint32_t best_ps = best.ps;
  if (row_tag)   // the rows that vote: region and haplotype in one word, 0 for every other row
    for (int r = r0 + tid; r < r1; r += LCR_BLOCK) {
      const lcr_read_record rr = rec[r];
      const bool sel = best_ps != 0 && rr.phase_set == best_ps && (rr.assignment == 1 || rr.assignment == 2);
      row_tag[r] = sel ? (g << 2) | rr.assignment : 0;
    }
  if (tid == 0) {
    lcr_ase_region o{};
    o.region = g; o.phase_set = best.ps; o.n_phase_sets = best.n_sets; o.h1 = best.h1; o.h2 = best.h2;
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
  const int g = s->region;
  uint8_t b = 0;
  if (s->phase_set != 0 && s->phase_set == ase[g].phase_set) b = k7_site_byte(s, min_phase_score, pos0, pat, mat, n_sites);
  if (b) atomicAdd(&ase[g].n_sites, 1u);
  site[i] = b;
}

// Eight lanes per row (eight rows per wave64): k7_row_vote (k7_sweep.h).
__global__ void __launch_bounds__(LCR_BLOCK) k7_votes(const int32_t* __restrict__ row_tag, int32_t n_rows, const int64_t* __restrict__ row_ptr,
                                                       const int32_t* __restrict__ col, const uint8_t* __restrict__ val,
                                                       const uint8_t* __restrict__ site, uint32_t min_baseq, lcr_ase_region* __restrict__ ase) {
  const int l = threadIdx.x & (K7_GROUP - 1);
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) / K7_GROUP;
  if (rl >= n_rows) return;   // (a whole group leaves)
  const int r = (int)rl;
  const int tag = row_tag[r];
  if (tag == 0) return;
  const int vote = k7_row_vote(row_ptr[r], row_ptr[r + 1], l, col, val, min_baseq, [&](int i) { return site[i]; });
  if (l != 0 || vote == 0) return;
  lcr_ase_region* o = ase + (tag >> 2);
  const bool h1 = (tag & 3) == 1;
  atomicAdd(vote > 0 ? (h1 ? &o->h1_pat : &o->h2_pat) : (h1 ? &o->h1_mat : &o->h2_mat), 1u);
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

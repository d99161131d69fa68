// k19_site_pairs.hip — K19: base x base counts of nearby site pairs over the fragment matrix (lcr_site_pairs).
//
// The contract (include/lcr.h): the eligible candidates of a region in candidate order, pairs of eligible rank difference 1..max_partners
// within max_dist, and per pair the rows that hold an entry at both sites, by the two bases.
//   k19_elig       a flag per candidate: eligible in the call's mode                                                            -> elig
//   (scan)         the flags to eligible ranks, their sum to n_eligible (launch_scan_i32)                                        -> rank, ctl[0]
//   k19_list       rank -> candidate; per candidate its rank, or -1 where it is not eligible                                    -> list, erank
//   k19_count      per candidate the number m <= max_partners of its pairs as first site: existence is monotone in the rank
//                  difference (positions ascend inside a region), so the first partner that fails ends the walk                  -> m
//   (scan)         m to pair_off (n_cand + 1), its sum to n_pairs                                                                -> off
//   k19_init       a thread per (candidate, k): the record of an existing pair gets its two sites and zeros                      -> pair
//   k19_rows       a lane group per row of the CSR (colseg_count's shape): every lane takes an entry at an eligible candidate and walks
//                  the row's following entries up to rank difference m of its candidate; one integer atomic per joint row, straight on
//                  the record's cell -- pair (c, k) is record off[c] + k - 1, known before the pass, so there is no dense slot table and
//                  no compaction behind it
//   k19_export     a thread per record: n_rows = the sixteen cells + n_lowq; the record to HBM and to pinned host memory; pair_off and
//                  {n_eligible, n_pairs} to pinned host memory
// All arithmetic is integer adds; nothing depends on the order in which atomics land.  The grids of k19_init / k19_export are sized from
// n_cand x max_partners, which the host knows; the threads beyond n_pairs leave.
#include "k7_sweep.h"

namespace {

__global__ void __launch_bounds__(LCR_BLOCK) k19_elig(const lcr_candidate* __restrict__ cand, int32_t n_cand, uint32_t mode, int32_t* __restrict__ elig) {
  const int c = blockIdx.x * LCR_BLOCK + threadIdx.x;
  if (c >= n_cand) return;
  const lcr_candidate& k = cand[c];
  bool ok = !(k.flags & LCR_F_DENSE);
  if (mode == LCR_PAIRS_PHASED) ok = ok && k.variant_type == 1 && k.haplotype != 0 && k.phase_set != 0;
  elig[c] = ok;
}

__global__ void __launch_bounds__(LCR_BLOCK) k19_list(const int32_t* __restrict__ elig, const int32_t* __restrict__ rank, int32_t n_cand,
                                                       int32_t* __restrict__ list, int32_t* __restrict__ erank) {
  const int c = blockIdx.x * LCR_BLOCK + threadIdx.x;
  if (c >= n_cand) return;
  const bool ok = elig[c] != 0;
  const int32_t r = rank[c];
  erank[c] = ok ? r : -1;
  if (ok) list[r] = c;   // (r < n_eligible <= n_cand)
}

__global__ void __launch_bounds__(LCR_BLOCK) k19_count(const lcr_candidate* __restrict__ cand, int32_t n_cand, const int32_t* __restrict__ erank,
                                                        const int32_t* __restrict__ list, const int32_t* __restrict__ n_elig, uint32_t max_partners,
                                                        uint32_t max_dist, int32_t* __restrict__ m) {
  const int c = blockIdx.x * LCR_BLOCK + threadIdx.x;
  if (c >= n_cand) return;
  const int32_t r = erank[c];
  int32_t n = 0;
  if (r >= 0) {
    const int32_t ne = *n_elig;
    const int32_t region = cand[c].region;
    const int64_t pos = cand[c].pos;
    for (int32_t k = 1; k <= (int32_t)max_partners && r + k < ne; k++) {
      const lcr_candidate& b = cand[list[r + k]];
      if (b.region != region || (max_dist != 0 && b.pos - pos > (int64_t)max_dist)) break;
      n = k;
    }
  }
  m[c] = n;
}

__global__ void __launch_bounds__(LCR_BLOCK) k19_init(int32_t n_cand, uint32_t max_partners, const int32_t* __restrict__ erank,
                                                       const int32_t* __restrict__ list, const int32_t* __restrict__ off, lcr_site_pair* __restrict__ pair) {
  const long long t = (long long)blockIdx.x * LCR_BLOCK + threadIdx.x;
  if (t >= (long long)n_cand * max_partners) return;
  const int c = (int)(t / max_partners), k = (int)(t % max_partners) + 1;
  const int32_t p0 = off[c];
  if (k > off[c + 1] - p0) return;   // (covers the candidates that are not eligible: they have no pair)
  lcr_site_pair o;
  o.a = c; o.b = list[erank[c] + k]; o.n_rows = 0; o.n_lowq = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) o.n[j >> 2][j & 3] = 0;
  pair[p0 + k - 1] = o;
}

__global__ void __launch_bounds__(LCR_BLOCK) k19_rows(int32_t n_rows, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                       const uint8_t* __restrict__ val, int32_t n_cand, const int32_t* __restrict__ erank,
                                                       const int32_t* __restrict__ off, uint32_t min_baseq, lcr_site_pair* __restrict__ pair) {
  const int l = threadIdx.x & (K7_GROUP - 1);
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) / K7_GROUP;
  if (rl >= n_rows) return;
  const int64_t e1 = row_ptr[rl + 1];
  for (int64_t e = row_ptr[rl] + l; e < e1; e += K7_GROUP) {   // (a row longer than its lane group loops)
    const int32_t a = col[e];
    if ((uint32_t)a >= (uint32_t)n_cand) continue;
    const int32_t ra = erank[a];
    if (ra < 0) continue;
    const int32_t p0 = off[a], m = off[a + 1] - p0;
    if (m <= 0) continue;
    const uint32_t va = val[e];
    for (int64_t f = e + 1; f < e1; f++) {
      const int32_t b = col[f];
      if ((uint32_t)b >= (uint32_t)n_cand) continue;
      const int32_t rb = erank[b];
      if (rb < 0) continue;           // (an entry at a candidate that is not eligible takes no partner slot)
      const int32_t k = rb - ra;
      if (k > m) break;               // (ranks ascend along a row: nothing further is a partner)
      if (k < 1) continue;            // (cannot happen in a CSR whose rows are in candidate order: keeps the index below inside the record list)
      const uint32_t vb = val[f];
      lcr_site_pair* o = &pair[p0 + k - 1];
      if ((va & 31) < min_baseq || (vb & 31) < min_baseq) atomicAdd(&o->n_lowq, 1u);
      else atomicAdd(&o->n[va >> 6][vb >> 6], 1u);
    }
  }
}

__global__ void __launch_bounds__(LCR_BLOCK) k19_export(int32_t n_cand, long long bound, const int32_t* __restrict__ n_elig, const int32_t* __restrict__ off,
                                                         lcr_site_pair* __restrict__ pair, lcr_site_pair* __restrict__ host_pair,
                                                         int32_t* __restrict__ host_off, int32_t* __restrict__ host_ctl) {
  const long long t = (long long)blockIdx.x * LCR_BLOCK + threadIdx.x;
  const int32_t np = off[n_cand];
  if (t == 0) { host_ctl[0] = *n_elig; host_ctl[1] = np; }
  if (t <= n_cand) host_off[t] = off[t];
  if (t >= bound || t >= np) return;
  lcr_site_pair o = pair[t];
  uint32_t s = o.n_lowq;
#pragma unroll
  for (int j = 0; j < 16; j++) s += o.n[j >> 2][j & 3];
  o.n_rows = s;
  pair[t].n_rows = s;
  host_pair[t] = o;
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
static inline unsigned k19_blocks(long long threads) { return (unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK); }

void launch_k19_elig(const lcr_candidate* cand, int32_t n_cand, uint32_t mode, int32_t* elig, hipStream_t s) {
  if (n_cand <= 0) return;
  hipLaunchKernelGGL(k19_elig, dim3(k19_blocks(n_cand)), dim3(LCR_BLOCK), 0, s, cand, n_cand, mode, elig);
}
void launch_k19_list(const int32_t* elig, const int32_t* rank, int32_t n_cand, int32_t* list, int32_t* erank, hipStream_t s) {
  if (n_cand <= 0) return;
  hipLaunchKernelGGL(k19_list, dim3(k19_blocks(n_cand)), dim3(LCR_BLOCK), 0, s, elig, rank, n_cand, list, erank);
}
void launch_k19_count(const lcr_candidate* cand, int32_t n_cand, const int32_t* erank, const int32_t* list, const int32_t* n_elig, uint32_t max_partners,
                      uint32_t max_dist, int32_t* m, hipStream_t s) {
  if (n_cand <= 0) return;
  hipLaunchKernelGGL(k19_count, dim3(k19_blocks(n_cand)), dim3(LCR_BLOCK), 0, s, cand, n_cand, erank, list, n_elig, max_partners, max_dist, m);
}
void launch_k19_init(int32_t n_cand, uint32_t max_partners, const int32_t* erank, const int32_t* list, const int32_t* off, lcr_site_pair* pair, hipStream_t s) {
  if (n_cand <= 0) return;
  hipLaunchKernelGGL(k19_init, dim3(k19_blocks((long long)n_cand * max_partners)), dim3(LCR_BLOCK), 0, s, n_cand, max_partners, erank, list, off, pair);
}
void launch_k19_rows(int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, int32_t n_cand, const int32_t* erank,
                     const int32_t* off, uint32_t min_baseq, lcr_site_pair* pair, hipStream_t s) {
  if (n_rows <= 0 || n_cand <= 0) return;
  hipLaunchKernelGGL(k19_rows, dim3(k19_blocks((long long)n_rows * K7_GROUP)), dim3(LCR_BLOCK), 0, s, n_rows, row_ptr, col, val, n_cand, erank, off,
                     min_baseq, pair);
}
void launch_k19_export(int32_t n_cand, uint32_t max_partners, const int32_t* n_elig, const int32_t* off, lcr_site_pair* pair, lcr_site_pair* host_pair,
                       int32_t* host_off, int32_t* host_ctl, hipStream_t s) {
  const long long bound = (long long)std::max(n_cand, 0) * max_partners;
  hipLaunchKernelGGL(k19_export, dim3(k19_blocks(std::max<long long>(bound, (long long)n_cand + 1))), dim3(LCR_BLOCK), 0, s, n_cand, bound, n_elig, off,
                     pair, host_pair, host_off, host_ctl);
}

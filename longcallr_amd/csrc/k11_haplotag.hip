// k11_haplotag.hip — K11: the rows of the fragment matrix against the caller's phased sites (lcr_haplotag; DESIGN.md "Haplotagging against a
// phased VCF").  It stands where the phase stage stands and writes what k4_post writes: the candidate records, the per-row results in pinned
// host memory and as read records in HBM.
//
// The contract (include/lcr.h), four launches whatever the number of regions:
//   k11_check    the caller's sites: ascending unique positions, h1 / h2 in ACGT and different, phase set non-zero   -> verdict (pinned host memory)
//   k11_sites    a thread per candidate: is it usable (het, for phasing, not dense, not an RNA edit, its position one of the sites' -- binary
//                search --, its reference base one of the two alleles)                -> site byte (usable | h1 code << 1 | h2 code << 3), the
//                site's phase set, the candidate's haplotype / phase_set or its NON_SELECTED bit; clears the site accumulators
//   k11_rows     eight lanes per row (eight rows per wave64) over its CSR entries: the row's phase set by ascending-value sweeps (the rule of
//                k7_sweep_phase_sets: most entries, a strict > keeps the smallest value on a tie; no bound on the number of sets), A1 / A2 of
//                that set's entries from the fixed-point table in LDS, folded with three xor shuffles of 64-bit integers; the group's first
//                lane decides and writes; the lanes of an assigned row add their entries into the site accumulators
//   k11_finish   a thread per candidate: phase_score from the accumulators, the records to HBM and to pinned host memory
// Every decision is an integer compare, or one f64 product of exactly converted integers (the cutoff test; -ffp-contract=off); the
// accumulators are 64-bit and 32-bit integer atomics: nothing depends on the order in which they land.  The sums stay below 2^53 for rows and
// sites of up to about 2 000 entries (every term is below 2^41 in magnitude), so the int64 -> double conversions are exact there.
#include "k7_sweep.h"

namespace {

constexpr int K11_GROUP = 8;   // lanes per row

__global__ void __launch_bounds__(LCR_BLOCK) k11_check(K11Sites st, int32_t* __restrict__ bad) {
  const int32_t i = (int32_t)(blockIdx.x * LCR_BLOCK + threadIdx.x);
  if (i >= st.n) return;
  const int a = k7_code(st.h1[i]), b = k7_code(st.h2[i]);
  if (a < 0 || b < 0 || a == b || st.ps[i] == 0 || (i > 0 && st.pos0[i - 1] >= st.pos0[i])) *bad = 1;   // (every writer stores the same value: a plain store)
}

__global__ void __launch_bounds__(LCR_BLOCK) k11_sites(lcr_candidate* __restrict__ cand, int32_t n_cand, K11Sites st, uint8_t* __restrict__ site,
                                                        uint32_t* __restrict__ site_ps, lcr_haplotag_site* __restrict__ acc) {
  const int32_t i = (int32_t)(blockIdx.x * LCR_BLOCK + threadIdx.x);
  if (i >= n_cand) return;
  lcr_candidate* __restrict__ s = cand + i;
  const uint32_t fl = s->flags;
  uint8_t b = 0;
  uint32_t ps = 0;
  int hap = 0;
  if (s->variant_type == 1 && (fl & (LCR_F_HET | LCR_F_FOR_PHASING)) == (LCR_F_HET | LCR_F_FOR_PHASING) && !(fl & (LCR_F_DENSE | LCR_F_RNA_EDIT))) {
    const int64_t p = s->pos;
    int lo = 0, hi = st.n;   // first site with pos0 >= p
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (st.pos0[mid] < p) lo = mid + 1; else hi = mid; }
    if (lo < st.n && st.pos0[lo] == p) {
      const uint8_t h1 = st.h1[lo], h2 = st.h2[lo];
      uint8_t r = s->ref_base;
      if (r >= 'a' && r <= 'z') r = (uint8_t)(r - 32);
      hap = r == h1 ? 1 : r == h2 ? -1 : 0;
      if (hap != 0) { b = (uint8_t)(1 | (k7_code(h1) << 1) | (k7_code(h2) << 3)); ps = st.ps[lo]; }
    }
  }
  if (b) { s->haplotype = hap; s->phase_set = ps; }
  else s->flags = fl | LCR_F_NON_SELECTED;
  site[i] = b; site_ps[i] = ps;
  acc[i] = lcr_haplotag_site{0, 0, 0, 0, 0, 0};
}

__device__ __forceinline__ uint32_t k11_group_sum(uint32_t v) {
#pragma unroll
  for (int d = K11_GROUP / 2; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}
__device__ __forceinline__ uint32_t k11_group_min(uint32_t v) {
#pragma unroll
  for (int d = K11_GROUP / 2; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}
__device__ __forceinline__ uint32_t k11_group_max(uint32_t v) {
#pragma unroll
  for (int d = K11_GROUP / 2; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}
__device__ __forceinline__ long long k11_group_sum64(long long v) {
#pragma unroll
  for (int d = K11_GROUP / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// a CSR entry's site byte when the entry is usable (its base is one of the site's two alleles), else 0
__device__ __forceinline__ uint8_t k11_usable(uint8_t sb, uint8_t v) {
  const int code = v >> 6;
  return ((sb & 1) && (code == ((sb >> 1) & 3) || code == ((sb >> 3) & 3))) ? sb : (uint8_t)0;
}

// Eight lanes per row; every value a branch depends on is the same in the lanes of a group, so a group's lanes stay together through
// the loops and the shuffles between them.
__global__ void __launch_bounds__(LCR_BLOCK) k11_rows(int32_t n_rows, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                       const uint8_t* __restrict__ val, const uint8_t* __restrict__ site,
                                                       const uint32_t* __restrict__ site_ps, PhaseLutDev lut, uint32_t min_linkers,
                                                       double cutoff, K11Rows out, lcr_haplotag_site* __restrict__ acc) {
  __shared__ long long s_lut[62];   // fe[0..30] | f1e[0..30]
  if (threadIdx.x < 31) { s_lut[threadIdx.x] = lut.fe[threadIdx.x]; s_lut[31 + threadIdx.x] = lut.f1e[threadIdx.x]; }
  __syncthreads();
  const int l = threadIdx.x & (K11_GROUP - 1);
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) / K11_GROUP;
  if (rl >= n_rows) return;   // (a whole group leaves)
  const int r = (int)rl;
  const int64_t e0 = row_ptr[r], e1 = row_ptr[r + 1];
  // pass 1: usable entries, the smallest and the largest phase set among them
  uint32_t n = 0, mn = 0xffffffffu, mx = 0;
  for (int64_t e = e0 + l; e < e1; e += K11_GROUP) {
    const int c = col[e];
    if (!k11_usable(site[c], val[e])) continue;
    const uint32_t ps = site_ps[c];
    n++; mn = min(mn, ps); mx = max(mx, ps);
  }
  n = k11_group_sum(n); mn = k11_group_min(mn); mx = k11_group_max(mx);
  uint32_t best = 0, cnt = 0;
  if (n != 0 && mn == mx) { best = mn; cnt = n; }   // one phase set: the usual row
  else if (n != 0) {
    // the sets in ascending order, one sweep each: count the current one, find the next; a strict > keeps the smallest value on a tie
    uint32_t cur = mn;
    for (;;) {
      uint32_t k = 0, nxt = 0xffffffffu;
      for (int64_t e = e0 + l; e < e1; e += K11_GROUP) {
        const int c = col[e];
        if (!k11_usable(site[c], val[e])) continue;
        const uint32_t ps = site_ps[c];
        if (ps == cur) k++;
        else if (ps > cur) nxt = min(nxt, ps);
      }
      k = k11_group_sum(k); nxt = k11_group_min(nxt);
      if (k > cnt) { cnt = k; best = cur; }
      if (nxt == 0xffffffffu) break;
      cur = nxt;
    }
  }
  // pass 2: A1 / A2 over the entries of the row's phase set
  long long a1 = 0, a2 = 0;
  if (cnt != 0)
    for (int64_t e = e0 + l; e < e1; e += K11_GROUP) {
      const int c = col[e];
      const uint8_t v = val[e], sb = k11_usable(site[c], v);
      if (!sb || site_ps[c] != best) continue;
      const int q = v & 31;   // (the fragment matrix clamps q to 30)
      const long long fe = s_lut[q], f1e = s_lut[31 + q];
      const bool is_h1 = (v >> 6) == ((sb >> 1) & 3);
      a1 += is_h1 ? f1e : fe; a2 += is_h1 ? fe : f1e;
    }
  a1 = k11_group_sum64(a1); a2 = k11_group_sum64(a2);
  int asg = 0;
  if (cnt != 0 && cnt >= min_linkers && a1 != a2 && fabs((double)(a1 - a2)) >= cutoff * fabs((double)(a1 + a2))) asg = a1 > a2 ? 1 : 2;
  if (l == 0) {
    const int tag = asg == 1 ? 1 : asg == 2 ? -1 : 0;
    const uint32_t ps = asg ? best : 0u;
    out.haplotag[r] = (int8_t)tag; out.assignment[r] = (uint8_t)asg; out.phase_set[r] = ps;
    out.d_rec[3 * (size_t)r] = (uint32_t)r;
    out.d_rec[3 * (size_t)r + 1] = (uint32_t)(uint8_t)(int8_t)tag | ((uint32_t)asg << 8);
    out.d_rec[3 * (size_t)r + 2] = ps;
  }
  if (!asg) return;
  // pass 3: the assigned row's counted entries into the site accumulators (integer atomics: order-free)
  for (int64_t e = e0 + l; e < e1; e += K11_GROUP) {
    const int c = col[e];
    const uint8_t v = val[e], sb = k11_usable(site[c], v);
    if (!sb || site_ps[c] != best) continue;
    const int q = v & 31;
    const long long fe = s_lut[q], f1e = s_lut[31 + q];
    const bool is_h1 = (v >> 6) == ((sb >> 1) & 3);
    const bool match = is_h1 == (asg == 1);
    lcr_haplotag_site* a = acc + c;
    atomicAdd(asg == 1 ? &a->n_h1 : &a->n_h2, 1u);
    if (match) atomicAdd(asg == 1 ? &a->n_h1_match : &a->n_h2_match, 1u);
    atomicAdd((unsigned long long*)&a->total_fx, (unsigned long long)(fe + f1e));   // (two's complement: the wrapped unsigned sum is the signed one)
    atomicAdd((unsigned long long*)&a->match_fx, (unsigned long long)(match ? f1e : fe));
  }
}

__global__ void __launch_bounds__(LCR_BLOCK) k11_finish(lcr_candidate* __restrict__ cand, int32_t n_cand, const uint8_t* __restrict__ site,
                                                         const lcr_haplotag_site* __restrict__ acc, lcr_candidate* __restrict__ host_cand,
                                                         lcr_haplotag_site* __restrict__ host_acc) {
  const int32_t i = (int32_t)(blockIdx.x * LCR_BLOCK + threadIdx.x);
  if (i >= n_cand) return;
  const lcr_haplotag_site a = acc[i];
  lcr_candidate s = cand[i];
  if (site[i] & 1) {
    // cal_phase_score_log at the fixed delta (phase.rs:238-255): 1 - q1 / (q2 + q3) with q1 the sum of the mismatch terms = the match terms' share
    s.phase_score = (a.n_h1 >= 1 && a.n_h2 >= 1) ? -10.0 * log10((double)a.match_fx / (double)a.total_fx) : 0.19940219;
    cand[i].phase_score = s.phase_score;
  }
  host_cand[i] = s;
  host_acc[i] = a;
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_k11_check(const K11Sites& st, int32_t* bad, hipStream_t s) {
  if (st.n > 0) hipLaunchKernelGGL(k11_check, dim3((st.n + LCR_BLOCK - 1) / LCR_BLOCK), dim3(LCR_BLOCK), 0, s, st, bad);
}
void launch_k11_sites(lcr_candidate* cand, int32_t n_cand, const K11Sites& st, uint8_t* site, uint32_t* site_ps, lcr_haplotag_site* acc, hipStream_t s) {
  if (n_cand > 0) hipLaunchKernelGGL(k11_sites, dim3((n_cand + LCR_BLOCK - 1) / LCR_BLOCK), dim3(LCR_BLOCK), 0, s, cand, n_cand, st, site, site_ps, acc);
}
void launch_k11_rows(int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, const uint8_t* site, const uint32_t* site_ps,
                     const PhaseLutDev& lut, uint32_t min_linkers, double cutoff, const K11Rows& out, lcr_haplotag_site* acc, hipStream_t s) {
  if (n_rows <= 0) return;
  const long long threads = (long long)n_rows * K11_GROUP;
  hipLaunchKernelGGL(k11_rows, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, n_rows, row_ptr, col, val, site, site_ps, lut,
                     min_linkers, cutoff, out, acc);
}
void launch_k11_finish(lcr_candidate* cand, int32_t n_cand, const uint8_t* site, const lcr_haplotag_site* acc, lcr_candidate* host_cand,
                       lcr_haplotag_site* host_acc, hipStream_t s) {
  if (n_cand > 0) hipLaunchKernelGGL(k11_finish, dim3((n_cand + LCR_BLOCK - 1) / LCR_BLOCK), dim3(LCR_BLOCK), 0, s, cand, n_cand, site, acc, host_cand, host_acc);
}

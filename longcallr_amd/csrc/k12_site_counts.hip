// k12_site_counts.hip — K12: allele x haplotype counts per candidate over the fragment matrix (lcr_site_counts).
//
// The contract (include/lcr.h) per candidate c, over the CSR entries with col == c, grouped into per-candidate segments (col_segments.h):
//   colseg_count            one integer atomic per entry on its candidate's counter; its body lives here, K14 launches it too     -> cnt
//   (scan)                  the counters to 64-bit segment offsets (launch_scan_i32_to_i64)                                       -> off
//   colseg_fill<K12Entry>   one word per entry into its candidate's segment: beside the row's part the base code and the low-quality bit -> seg
//   k12_sites               a wave64 per candidate, looping over its segment: colseg_pick (low-quality entries, the phase set with the most
//                           counted entries, the number of sets), then the twelve cells.  The first lane writes the record to HBM and to
//                           pinned host memory.
// All arithmetic is integer adds; nothing depends on the order in which atomics land.
#include "col_segments.h"

namespace {

// the unit's bits of an entry's word: 34-35 base code, 36 quality below the threshold
constexpr int K12_BASE = COLSEG_OWN, K12_LOWQ = COLSEG_OWN + 2;

struct K12Entry {
  uint32_t min_baseq;
  __device__ uint64_t operator()(int32_t, uint8_t v) const {
    return ((uint64_t)(v >> 6) << K12_BASE) | ((uint64_t)((uint32_t)(v & 31) < min_baseq) << K12_LOWQ);
  }
};

__global__ void __launch_bounds__(LCR_BLOCK) colseg_count(int32_t n_rows, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
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
  const ColPick pick = colseg_pick(seg, e0, e1, lane, [](uint64_t w) { return !((w >> K12_LOWQ) & 1); });
  const uint32_t site_ps = own != 0 ? own : pick.best_ps;
  // the twelve cells: k = the row's haplotype when it counts and is in the site's set, else 0
  uint32_t n[12];
#pragma unroll
  for (int j = 0; j < 12; j++) n[j] = 0;
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const uint64_t w = seg[e];
    if ((w >> K12_LOWQ) & 1) continue;
    const uint32_t ps = (uint32_t)w;
    const int k = (ps != 0 && ps == site_ps) ? (int)((w >> COLSEG_HAP) & 3) : 0;
    const int cell = k * 4 + (int)((w >> K12_BASE) & 3);
#pragma unroll
    for (int j = 0; j < 12; j++) n[j] += (cell == j);
  }
#pragma unroll
  for (int j = 0; j < 12; j++) n[j] = wave_sum_u32(n[j]);
  if (lane != 0) return;
  lcr_site_count o;
  o.phase_set = site_ps; o.n_phase_sets = pick.n_sets; o.n_entries = (uint32_t)(e1 - e0); o.n_lowq = pick.lowq;
#pragma unroll
  for (int j = 0; j < 12; j++) o.n[j >> 2][j & 3] = n[j];
  out[c] = o;
  host_out[c] = o;
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_colseg_count(int32_t n_rows, const int64_t* row_ptr, const int32_t* col, int32_t n_cand, uint32_t* cnt, hipStream_t s) {
  if (n_rows <= 0 || n_cand <= 0) return;
  const long long threads = (long long)n_rows * K7_GROUP;
  hipLaunchKernelGGL(colseg_count, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, n_rows, row_ptr, col, n_cand, cnt);
}
void launch_k12_fill(int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, const lcr_read_record* rec, uint32_t min_baseq,
                     int32_t n_cand, uint32_t* cnt, const int64_t* off, uint64_t* seg, hipStream_t s) {
  launch_colseg_fill(n_rows, row_ptr, col, val, rec, K12Entry{min_baseq}, n_cand, cnt, off, seg, s);
}
void launch_k12_sites(const lcr_candidate* cand, int32_t n_cand, const int64_t* off, const uint64_t* seg, lcr_site_count* out, lcr_site_count* host_out,
                      hipStream_t s) {
  if (n_cand <= 0) return;
  const long long threads = (long long)n_cand * 64;
  hipLaunchKernelGGL(k12_sites, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, cand, n_cand, off, seg, out, host_out);
}

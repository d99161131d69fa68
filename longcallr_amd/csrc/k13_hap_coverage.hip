// k13_hap_coverage.hip — K13: covered depth per haplotype class at every window column, run-length encoded (lcr_hap_coverage; DESIGN.md
// section 1k).
//
// The contract (include/lcr.h) per region g, over ALL its reads -- class 1 / 2 for a read whose fragment row is assigned, 0 for every other:
//   k13_blocks   sixteen lanes per read over its CIGAR (k6_walk's layout).  A read's covered set is a union of intervals that only an N op
//                of length >= 1 breaks, so the walk emits one +1 where a covered run starts and one -1 where it ends -- not two per op --,
//                clipped to the window, into the difference plane of the read's class.  u32 adds that wrap; start and end adds commute.
//                What a wave sends to one address is summed in the wave first (k13_grouped_add)                                  -> planes
//   k13_scan     one workgroup per region: the inclusive scan of the three planes in steps of K13_TILE columns, in place (the planes
//                hold depths afterwards), and in the same pass the region's sums, maxima, reads per class and run starts       -> reg, nseg
//   (scan)       the run starts to segment offsets (launch_scan_i32); k13_offsets hands them and the region records to pinned memory
//   k13_emit     one workgroup per region, the same steps: a column starts a run when its triple is not (0, 0, 0) and differs from the
//                previous column's (the column in front of a window counts as (0, 0, 0)), and ends one when the next column's differs.
//                The i-th start and the i-th end of a region belong to one run: starts write the record, ends its end column   -> seg, send
//   k13_finish   a thread per segment: the length, and the record's copy in pinned memory
// Dense form: 12 bytes per window column.  All arithmetic is integer adds; nothing depends on the order in which atomics land.
#include "lcr_dev.h"
#include "k13_hap_coverage.h"

namespace {

static_assert(K13_TILE == 4 * LCR_BLOCK, "a step is four consecutive columns per thread");

// class of read r of region g: row k of a region is its k-th read (fragment.rs:293-307); a read behind the rows is no row
__device__ __forceinline__ int k13_class(const BatchView& b, const int32_t* __restrict__ row_region_off, const lcr_read_record* __restrict__ rec, int r, int g) {
  const int k = r - b.read_begin[g], row0 = row_region_off[g];
  if (k < 0 || k >= row_region_off[g + 1] - row0) return 0;
  const int a = rec[row0 + k].assignment;
  return (a == 1 || a == 2) ? a : 0;
}

// Every lane of the wave calls.  The active lanes' adds (delta = 1 or 0xffffffff) are grouped by address: one atomic per distinct
// address and wave, none where the group's sum is 0.
__device__ __forceinline__ void k13_grouped_add(bool active, uint32_t* addr, uint32_t delta) {
  const int lane = threadIdx.x & 63;
  unsigned long long pend = __ballot(active);
  while (pend) {   // (wave-uniform)
    const int leader = __ffsll((long long)pend) - 1;
    const unsigned long long la = __shfl((unsigned long long)(uintptr_t)addr, leader, 64);
    const bool same = active && (unsigned long long)(uintptr_t)addr == la;
    const unsigned long long mp = __ballot(same && delta == 1u), mm = __ballot(same && delta != 1u);
    const uint32_t sum = (uint32_t)__popcll(mp) - (uint32_t)__popcll(mm);
    if (lane == leader && sum != 0) atomicAdd(addr, sum);
    pend &= ~(mp | mm);
  }
}

// kind of an op for the walk: 0 neither covers nor advances (I S H P, zero length, padding), 1 covers (M = X D), 2 gap (N)
__global__ void __launch_bounds__(LCR_BLOCK) k13_blocks(BatchView b, const int32_t* __restrict__ row_region_off, const lcr_read_record* __restrict__ rec,
                                                         int64_t n_cols, uint32_t* __restrict__ planes) {
  const int lane = threadIdx.x & 63, l16 = lane & 15, rbase = lane & 48;
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) >> 4;
  const bool live = rl < b.n_reads;   // (rows without a read stay: the wave's adds are combined by all its lanes)
  const int r = live ? (int)rl : 0;
  uint32_t ncig = 0;
  const uint32_t* __restrict__ cg = b.cigar;
  uint32_t* plane = planes;
  int wlen = 0;
  long long ref_cur = 0;   // window-relative
  if (live) {
    const int g = region_of_read(b, r);
    ncig = b.n_cig[r];
    cg = b.cigar + b.cig_off[r];
    wlen = b.len[g];
    ref_cur = (long long)b.pos[r] - b.start0[g];
    plane = planes + (long long)k13_class(b, row_region_off, rec, r, g) * n_cols + b.col_off[g];
  }
  int prev_kind = 2;   // of the last covering / gap op in front of this round (row-uniform); nothing yet counts as a gap
  for (uint32_t c0 = 0; __ballot(c0 < ncig) != 0; c0 += 16) {   // (wave-uniform: a row whose CIGAR is through sees padding)
    const uint32_t w = c0 + l16 < ncig ? cg[c0 + l16] : 0u;
    const int op = w & 15, len = (int)(w >> 4);
    const bool cov = len >= 1 && (op == 0 || op == 2 || op == 7 || op == 8);
    const bool gap = len >= 1 && op == 3;
    const int dr = (cov || gap) ? len : 0;
    const int ir = row16_incl_scan(dr);
    const unsigned int mc = (unsigned int)(__ballot(cov) >> rbase) & 0xffffu;
    const unsigned int mg = (unsigned int)(__ballot(gap) >> rbase) & 0xffffu;
    const unsigned int before = (mc | mg) & ((1u << l16) - 1u);
    const int pk = before ? (((mc >> (31 - __clz((int)before))) & 1u) ? 1 : 2) : prev_kind;
    const long long s = ref_cur + ir - dr;                   // the op's first column
    const bool start = cov && pk == 2, end = gap && pk == 1;  // a run starts behind a gap, and ends where a gap begins
    const bool active = (start || end) && s < wlen;           // (a run wholly left of the window: +1 and -1 meet at column 0)
    k13_grouped_add(active, plane + (s > 0 ? s : 0), start ? 1u : 0xffffffffu);
    const unsigned int all = mc | mg;
    if (all) prev_kind = ((mc >> (31 - __clz((int)all))) & 1u) ? 1 : 2;
    ref_cur += __shfl(ir, rbase + 15, 64);
  }
  // the read's last run ends with the read; an end on the window's end is not written
  const bool active = live && l16 == 0 && prev_kind == 1 && ref_cur < wlen;
  k13_grouped_add(active, plane + (ref_cur > 0 ? ref_cur : 0), 0xffffffffu);
}

// One workgroup per region.  Step by step: four consecutive columns per thread, their running sums, the workgroup's exclusive scan of the
// threads' totals, the carry of the steps before.  The exclusive value in front of a thread's first column IS the depth of the column
// before it (0 in front of the window), so a run start needs no second load.
__global__ void __launch_bounds__(LCR_BLOCK) k13_scan(BatchView b, const int32_t* __restrict__ row_region_off, const lcr_read_record* __restrict__ rec,
                                                       int64_t n_cols, uint32_t* __restrict__ planes, lcr_hap_cov_region* __restrict__ reg,
                                                       int32_t* __restrict__ nseg) {
  __shared__ uint32_t s_w[3][4];
  __shared__ unsigned long long s_sum[3][4];
  __shared__ uint32_t s_max[3][4], s_nr[3][4], s_st[4];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wlen = b.len[g];
  uint32_t* const p0 = planes + b.col_off[g];
  uint32_t carry[3] = {0, 0, 0}, mx[3] = {0, 0, 0}, starts = 0;
  unsigned long long sum[3] = {0, 0, 0};
  for (long long c0 = 0; c0 < wlen; c0 += K13_TILE) {   // (workgroup-uniform)
    const long long c = c0 + 4 * tid;
    uint32_t d[3][4], ex[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
      for (int j = 0; j < 4; j++) d[k][j] = c + j < wlen ? p0[k * n_cols + c + j] : 0u;
      d[k][1] += d[k][0]; d[k][2] += d[k][1]; d[k][3] += d[k][2];
      const uint32_t inc = (uint32_t)wave_incl_scan((int)d[k][3]);
      ex[k] = inc - d[k][3];
      if (lane == 63) s_w[k][wv] = inc;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; k++) {
      uint32_t tot = 0;
#pragma unroll
      for (int w = 0; w < 4; w++) { if (w < wv) ex[k] += s_w[k][w]; tot += s_w[k][w]; }
      ex[k] += carry[k];
      carry[k] += tot;
    }
    uint32_t q0 = ex[0], q1 = ex[1], q2 = ex[2];   // the triple of the column before
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (c + j >= wlen) break;
      const uint32_t v0 = ex[0] + d[0][j], v1 = ex[1] + d[1][j], v2 = ex[2] + d[2][j];
      p0[c + j] = v0; p0[n_cols + c + j] = v1; p0[2 * n_cols + c + j] = v2;
      sum[0] += v0; sum[1] += v1; sum[2] += v2;
      mx[0] = max(mx[0], v0); mx[1] = max(mx[1], v1); mx[2] = max(mx[2], v2);
      starts += ((v0 | v1 | v2) != 0 && (v0 != q0 || v1 != q1 || v2 != q2)) ? 1u : 0u;
      q0 = v0; q1 = v1; q2 = v2;
    }
    __syncthreads();   // (s_w is rewritten by the next step)
  }
  // the region's reads per class, whether or not a block of theirs lies inside the window
  uint32_t nr[3] = {0, 0, 0};
  for (int r = b.read_begin[g] + tid; r < b.read_begin[g + 1]; r += LCR_BLOCK) {
    const int k = k13_class(b, row_region_off, rec, r, g);
    nr[0] += k == 0; nr[1] += k == 1; nr[2] += k == 2;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const unsigned long long s = wave_sum_u64(sum[k]);
    const uint32_t m = wave_max_u32(mx[k]), n = wave_sum_u32(nr[k]);
    if (lane == 0) { s_sum[k][wv] = s; s_max[k][wv] = m; s_nr[k][wv] = n; }
  }
  starts = wave_sum_u32(starts);
  if (lane == 0) s_st[wv] = starts;
  __syncthreads();
  if (tid != 0) return;
  lcr_hap_cov_region o;
  o.region = g; o.pad_ = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    o.bases[k] = s_sum[k][0] + s_sum[k][1] + s_sum[k][2] + s_sum[k][3];
    o.max_depth[k] = max(max(s_max[k][0], s_max[k][1]), max(s_max[k][2], s_max[k][3]));
    o.n_reads[k] = s_nr[k][0] + s_nr[k][1] + s_nr[k][2] + s_nr[k][3];
  }
  reg[g] = o;
  nseg[g] = (int32_t)(s_st[0] + s_st[1] + s_st[2] + s_st[3]);
}

__global__ void k13_offsets(int32_t ng, const int32_t* __restrict__ off, const lcr_hap_cov_region* __restrict__ reg, int32_t* __restrict__ host_off,
                            lcr_hap_cov_region* __restrict__ host_reg) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > ng) return;
  host_off[g] = off[g];
  if (g < ng) host_reg[g] = reg[g];
}

// One workgroup per region over the depths k13_scan left.  Starts and ends are counted in one word (low / high half: at most K13_TILE of
// each per step) and ranked by one workgroup scan; the ranks run on from step to step.
__global__ void __launch_bounds__(LCR_BLOCK) k13_emit(BatchView b, int64_t n_cols, const uint32_t* __restrict__ planes, const int32_t* __restrict__ off,
                                                       lcr_hap_cov_segment* __restrict__ seg, int32_t* __restrict__ send) {
  __shared__ uint32_t s_w[4];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n0 = off[g], n1 = off[g + 1];
  if (n1 <= n0) return;   // (the whole workgroup leaves)
  const int wlen = b.len[g];
  const int64_t s0 = b.start0[g];
  const uint32_t* const p0 = planes + b.col_off[g];
  uint32_t run_s = 0, run_e = 0;   // starts / ends of the steps before (two words: over a window they can pass 2^16)
  for (long long c0 = 0; c0 < wlen; c0 += K13_TILE) {
    const long long c = c0 + 4 * tid;
    uint32_t v[3][6];   // columns c - 1 .. c + 4; outside the window: 0
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int j = 0; j < 6; j++) {
        const long long cc = c + j - 1;
        v[k][j] = (cc >= 0 && cc < wlen) ? p0[k * n_cols + cc] : 0u;
      }
    uint32_t st = 0, en = 0;   // bit j: column c + j
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (c + j >= wlen) break;
      const bool nz = (v[0][j + 1] | v[1][j + 1] | v[2][j + 1]) != 0;
      const bool dp = v[0][j + 1] != v[0][j] || v[1][j + 1] != v[1][j] || v[2][j + 1] != v[2][j];
      const bool dn = v[0][j + 1] != v[0][j + 2] || v[1][j + 1] != v[1][j + 2] || v[2][j + 1] != v[2][j + 2];
      st |= (nz && dp) ? 1u << j : 0u;
      en |= (nz && dn) ? 1u << j : 0u;
    }
    const uint32_t cnt = (uint32_t)__popc(st) | ((uint32_t)__popc(en) << 16);
    const uint32_t inc = (uint32_t)wave_incl_scan((int)cnt);
    uint32_t ex = inc - cnt;
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t tot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) { if (w < wv) ex += s_w[w]; tot += s_w[w]; }
    long long is = (long long)n0 + run_s + (ex & 0xffffu), ie = (long long)n0 + run_e + (ex >> 16);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if ((st >> j) & 1u) {
        if (is < n1) {   // (always, while both passes see the same depths)
          lcr_hap_cov_segment o;
          o.region = g; o.len = 0; o.start0 = s0 + c + j;
          o.n[0] = v[0][j + 1]; o.n[1] = v[1][j + 1]; o.n[2] = v[2][j + 1]; o.pad_ = 0;
          seg[is] = o;
        }
        is++;
      }
      if ((en >> j) & 1u) {
        if (ie < n1) send[ie] = (int32_t)(c + j + 1);
        ie++;
      }
    }
    run_s += tot & 0xffffu; run_e += tot >> 16;
    __syncthreads();
  }
}

__global__ void k13_finish(int32_t n_seg, int32_t ng, const int64_t* __restrict__ start0, const int32_t* __restrict__ send,
                           lcr_hap_cov_segment* __restrict__ seg, lcr_hap_cov_segment* __restrict__ host_seg) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_seg) return;
  lcr_hap_cov_segment o = seg[j];
  if ((uint32_t)o.region >= (uint32_t)ng) return;   // (cannot happen: k13_emit wrote every record of every region)
  o.len = send[j] - (int32_t)(o.start0 - start0[o.region]);
  seg[j] = o;
  host_seg[j] = o;
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_k13_blocks(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, int64_t n_cols, uint32_t* planes, hipStream_t s) {
  if (b.n_reads <= 0 || n_cols <= 0) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k13_blocks, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, row_region_off, rec, n_cols, planes);
}
void launch_k13_scan(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, int64_t n_cols, uint32_t* planes,
                     lcr_hap_cov_region* reg, int32_t* nseg, hipStream_t s) {
  if (b.n_regions <= 0) return;
  hipLaunchKernelGGL(k13_scan, dim3((unsigned)b.n_regions), dim3(LCR_BLOCK), 0, s, b, row_region_off, rec, n_cols, planes, reg, nseg);
}
void launch_k13_offsets(int32_t ng, const int32_t* off, const lcr_hap_cov_region* reg, int32_t* host_off, lcr_hap_cov_region* host_reg, hipStream_t s) {
  if (ng < 0) return;
  hipLaunchKernelGGL(k13_offsets, dim3((unsigned)(ng / LCR_BLOCK + 1)), dim3(LCR_BLOCK), 0, s, ng, off, reg, host_off, host_reg);
}
void launch_k13_emit(const BatchView& b, int64_t n_cols, const uint32_t* planes, const int32_t* off, lcr_hap_cov_segment* seg, int32_t* send, hipStream_t s) {
  if (b.n_regions <= 0) return;
  hipLaunchKernelGGL(k13_emit, dim3((unsigned)b.n_regions), dim3(LCR_BLOCK), 0, s, b, n_cols, planes, off, seg, send);
}
void launch_k13_finish(int32_t n_seg, int32_t ng, const int64_t* start0, const int32_t* send, lcr_hap_cov_segment* seg, lcr_hap_cov_segment* host_seg, hipStream_t s) {
  if (n_seg <= 0) return;
  hipLaunchKernelGGL(k13_finish, dim3((unsigned)((n_seg + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, n_seg, ng, start0, send, seg, host_seg);
}

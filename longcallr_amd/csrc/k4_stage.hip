// k4_stage.hip — K4, staging: the phase matrices of every region from K3's fragment CSR (reference src/fragment.rs:144-146,253-255;
// the per-SNP constants of cross_optimize, phase.rs:810-976).  Two kernels from one set of steps: k4_stage, one workgroup per region,
// and k4_stage_grid, all CUs on one large region behind grid barriers.  Host control: k4_phase.hip.
//
// For every region: the rows with >= min_linkers linked SNPs (fragment.rs:253-255; with down-sampling, the sampled ones) restricted to
// the phase sites (for_phasing candidates, fragment.rs:144-146) as CSR + CSC mirror, the per-SNP constants of cross_optimize and the
// region descriptor.  Slices sit at offsets derived from K3's own offsets (rows: r0 + g, SNPs: c0 + g, entries: row_ptr[r0]) so no
// cross-region scan is needed.  The CSC fill order inside a column is whatever the atomics give: every consumer only sums over a
// column (the chain kernel builds its own row-ordered index).
#include <climits>
#include "k4_dev.h"
#include "k4_grid.h"
#include "k4_kernels.h"

namespace {

// ---- the region: its slices of K3's matrix and the descriptor (R, f_total and F_all are filled in by write_region)
struct StageRegion { int g, r0, nrow, c0, S; int64_t e_base, E_all; RegionDev rd; };
__device__ __forceinline__ StageRegion stage_region(const StageIn& in, int g) {
  StageRegion q{};
  q.g = g; q.r0 = in.row_region_off[g]; q.nrow = in.row_region_off[g + 1] - q.r0;
  q.c0 = in.cand_off[g]; q.S = in.cand_off[g + 1] - q.c0;
  q.e_base = in.row_ptr[q.r0]; q.E_all = in.row_ptr[q.r0 + q.nrow] - q.e_base;
  q.rd.S = q.S; q.rd.rp_off = q.r0 + g; q.rd.cp_off = q.c0 + g; q.rd.e_off = q.e_base; q.rd.sig_off = q.r0; q.rd.snp_off = q.c0;
  q.rd.seed = region_seed(in.seed, in.start0[g]);
  return q;
}
__device__ __forceinline__ void write_region(const StageIn& in, const StageOut& out, const StageRegion& q, int R, int E, int Fa, long long f_total,
                                             int part_entries, int part_rows, int64_t e_all, int band) {
  RegionDev rd = q.rd;
  rd.R = R; rd.f_total = f_total; rd.F_all = in.sampled ? Fa : R;
  out.reg[q.g] = rd;
  out.stat[q.g] = StageStat{R, E, part_entries, part_rows, (int)std::min<int64_t>(e_all, INT_MAX), band};
}
__device__ __forceinline__ void load_stage_lut(const PhaseLutDev& lut, long long* s_fe, long long* s_f1e) {
  if (threadIdx.x < 32) { const int t = threadIdx.x; s_fe[t] = t < 31 ? lut.fe[t] : 0; s_f1e[t] = t < 31 ? lut.f1e[t] : 0; }
}

// ---- row sources: where a step reads the region's fragment rows (region-relative rows, entries and columns) and keeps its column cursors.
// bit 0: phasing row (enough links, and sampled when the region is down-sampled), bit 1: enough links (the rows that draw)
__device__ __forceinline__ int row_bits(const StageIn& in, int row) {
  const int isl = in.links[row] >= in.min_linkers ? 1 : 0;
  return (isl && (!in.sampled || in.sampled[row]) ? 1 : 0) | (isl << 1);
}
struct GlobalRows {   // global memory: k4_stage beyond its LDS image, k4_stage_grid
  const StageIn& in; const StageOut& out; int r0, c0; int64_t e_base;
  __device__ void init_snp(int i, uint8_t) const { out.cursor[c0 + i] = 0; }
  __device__ void load(const StageRegion&) const {}
  __device__ int bits(int r) const { return row_bits(in, r0 + r); }
  __device__ int rp(int r) const { return (int)(in.row_ptr[r0 + r] - e_base); }
  __device__ int col(int e) const { return in.col[e_base + e] - c0; }
  __device__ uint8_t val(int e) const { return in.val[e_base + e]; }
  __device__ bool fp(int i) const { return out.snp_fp[c0 + i] != 0; }
  __device__ int& cur(int i) const { return out.cursor[c0 + i]; }
};
// The region's slice of the fragment matrix brought into LDS with coalesced loads when it fits (any realistic region does): the per-row
// entry loops are chains of dependent loads, a microsecond per link from HBM, and there are four of them per row.
struct LdsRows {
  const StageIn& in; uint16_t* s_col; uint8_t* s_val; uint16_t* s_rp; uint8_t* s_isp; uint8_t* s_fp; int* s_cur;
  __device__ void init_snp(int i, uint8_t fp) const { s_fp[i] = fp; s_cur[i] = 0; }
  __device__ void load(const StageRegion& q) const {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int e = tid; e < (int)q.E_all; e += nt) { s_col[e] = (uint16_t)(in.col[q.e_base + e] - q.c0); s_val[e] = in.val[q.e_base + e]; }
    for (int r = tid; r <= q.nrow; r += nt) s_rp[r] = (uint16_t)(in.row_ptr[q.r0 + r] - q.e_base);
    for (int r = tid; r < q.nrow; r += nt) s_isp[r] = (uint8_t)row_bits(in, q.r0 + r);
  }
  __device__ int bits(int r) const { return s_isp[r]; }
  __device__ int rp(int r) const { return s_rp[r]; }
  __device__ int col(int e) const { return s_col[e]; }
  __device__ uint8_t val(int e) const { return s_val[e]; }
  __device__ bool fp(int i) const { return s_fp[i] != 0; }
  __device__ int& cur(int i) const { return s_cur[i]; }
};

// ---- per-SNP flags, conserved bytes and column cursors
template <class SC, class SRC>
__device__ __forceinline__ void snp_init(SC& sc, const StageIn& in, const StageOut& out, const StageRegion& q, const SRC& src) {
  for (int i = sc.tid(); i < q.S; i += sc.nt()) {
    const lcr_candidate& c = in.cand[q.c0 + i];
    const uint8_t fp = (c.flags & LCR_F_FOR_PHASING) ? 1 : 0;
    out.snp_fp[q.c0 + i] = fp; out.snp_vt[q.c0 + i] = (int8_t)c.variant_type; out.snp_cons[q.c0 + i] = 0;
    src.init_snp(i, fp);
  }
}

// ---- one fragment row: its bits, entry range, phase-site entries (0 unless it is a phasing row) and the distance between its first and
// last phase site (every fragment row counts for the LD pair table, fragment.rs:208-240: the band width)
struct RowInfo { int isp, isl, cnt, span, eb, ee; };
template <class SRC>
__device__ __forceinline__ RowInfo row_scan(const SRC& src, int r) {
  const int bits = src.bits(r);
  RowInfo ri{bits & 1, bits >> 1, 0, 0, src.rp(r), src.rp(r + 1)};
  int first = -1, last = -1;
  for (int e = ri.eb; e < ri.ee; e++) { const int ci = src.col(e); if (src.fp(ci)) { ri.cnt++; if (first < 0) first = ci; last = ci; } }
  if (last > first) ri.span = last - first;
  if (!ri.isp) ri.cnt = 0;   // (the span counts for every row, the entries only for a phasing row)
  return ri;
}

// ---- CSR of the fragment rows [lo, hi) in row order behind a block scan, column counts into the cursors.  R, E, Fa: phasing rows, phase
// entries and rows that draw in front of `lo` on entry, in front of `hi` on return.  Returns the largest span this thread saw.
template <int NW, class SRC>
__device__ __forceinline__ int emit_csr(const StageIn& in, const StageOut& out, const StageRegion& q, const SRC& src, int lo, int hi,
                                        int& R, int& E, int& Fa, int (*sm)[16]) {
  int32_t* prp = out.prow_ptr + q.rd.rp_off;
  int span = 0;
  for (int base = lo; base < hi; base += NW * 64) {
    const int r = base + (int)threadIdx.x;
    RowInfo ri{};
    if (r < hi) ri = row_scan(src, r);
    span = max(span, ri.span);
    int k, eo, tk, te;
    block_scan2n<NW, 16>(ri.isp, ri.cnt, k, eo, tk, te, sm);
    if (in.sampled) {   // (uniform) draw ordinals: the rank among the rows with enough links
      int ord, d0, tl, d1;
      block_scan2n<NW, 16>(ri.isl, 0, ord, d0, tl, d1, sm);
      if (ri.isp) out.prow_ord[q.r0 + R + k] = Fa + ord;
      Fa += tl;
    }
    if (ri.isp) {
      k += R; eo += E;
      prp[k] = eo; out.prow_src[q.r0 + k] = r;
      for (int e = ri.eb; e < ri.ee; e++) {
        const int ci = src.col(e);
        if (!src.fp(ci)) continue;
        out.pcol[q.e_base + eo] = ci; out.pval[q.e_base + eo] = src.val(e) & 63;
        atomicAdd(&src.cur(ci), 1);
        eo++;
      }
    }
    R += tk; E += te;
  }
  return span;
}

// ---- column offsets from the column counts, by one workgroup; the cursors restart at the offsets
template <int NW, class SRC>
__device__ __forceinline__ void column_offsets(const SRC& src, int S, int32_t* pcp, int (*sm)[16]) {
  const int tid = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < S; base += NW * 64) {
    const int i = base + tid;
    const int v = i < S ? src.cur(i) : 0;
    int ex, d0, tot, d1;
    block_scan2n<NW, 16>(v, 0, ex, d0, tot, d1, sm);
    if (i < S) { pcp[i] = carry + ex; src.cur(i) = carry + ex; }
    carry += tot;
  }
  if (tid == 0) pcp[S] = carry;
}

// ---- per-SNP constants, one wave per SNP: F = sum fe, W = sum w, Cref = sum (p==+1 ? f1e : fe), Cvar = sum (p==-1 ? f1e : fe).
// Returns this thread's share of the region's f_total (lane 0 of a wave carries the wave's).
template <class SC>
__device__ __forceinline__ long long snp_constants(SC& sc, const StageOut& out, const StageRegion& q, const long long* s_fe, const long long* s_f1e) {
  const int lane = threadIdx.x & 63;
  const int32_t* pcp = out.ccol_ptr + q.rd.cp_off;
  long long ft = 0;
  for (int i = sc.wave(); i < q.S; i += sc.nwaves()) {
    long long F = 0, W = 0, Cr = 0, Cv = 0;
    for (int e = pcp[i] + lane; e < pcp[i + 1]; e += 64) {
      const uint8_t v = out.cval[q.e_base + e];
      const long long fe = s_fe[v & 31], f1 = s_f1e[v & 31];
      F += fe; W += f1 - fe;
      Cr += (v & 32) ? f1 : fe; Cv += (v & 32) ? fe : f1;
    }
    F = wave_sum_ll_dpp(F); W = wave_sum_ll_dpp(W); Cr = wave_sum_ll_dpp(Cr); Cv = wave_sum_ll_dpp(Cv);
    if (lane == 0) { long long* sc4 = out.snp_const + 4ll * (q.c0 + i); sc4[0] = F; sc4[1] = W; sc4[2] = Cr; sc4[3] = Cv; ft += F; }
  }
  return ft;
}

// ---------------------------------------------------------------------------------------------
// k4_stage: one workgroup per region.  The CSC mirror comes from a second scan over the source rows, so the LDS form never reads back
// what it just wrote to HBM.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(STAGE_THREADS) k4_stage(StageIn in, StageOut out, PhaseLutDev lut) {
  constexpr int NW = STAGE_THREADS / 64;
  __shared__ int sm[2][16];
  __shared__ int s_max[3];   // [0], [1]: k4_enum_reg's largest lane share in entries / rows, [2]: the LD band width
  __shared__ long long s_ft[NW];
  __shared__ long long s_fe[32], s_f1e[32];
  __shared__ uint16_t s_col[STG_E];
  __shared__ uint8_t s_val[STG_E];
  __shared__ uint16_t s_rp[STG_R + 1];
  __shared__ uint8_t s_isp[STG_R];
  __shared__ uint8_t s_fp[STG_S];
  __shared__ int s_cur[STG_S];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const StageRegion q = stage_region(in, blockIdx.x);
  const int S = q.S, nrow = q.nrow;
  if (S == 0) {
    if (tid == 0) { write_region(in, out, q, 0, 0, 0, 0, 0, 0, 0, 0); out.prow_ptr[q.rd.rp_off] = 0; out.ccol_ptr[q.rd.cp_off] = 0; }
    return;
  }
  if (q.E_all >= in.grid_min) return;   // k4_stage_grid stages this region with all CUs
  load_stage_lut(lut, s_fe, s_f1e);
  if (tid < 3) s_max[tid] = 0;
  WgScope sc{s_ft, nullptr};
  int32_t* prp = out.prow_ptr + q.rd.rp_off;
  int R = 0, E = 0, Fa = 0;
  auto build = [&](const auto& src) {
    snp_init(sc, in, out, q, src);
    src.load(q);
    __syncthreads();
    // ---- pass 1: phasing rows and their phase-site entries (CSR), column counts
    const int span = emit_csr<NW>(in, out, q, src, 0, nrow, R, E, Fa, sm);
    if (span) atomicMax(&s_max[2], span);
    if (tid == 0) prp[R] = E;
    __syncthreads();
    column_offsets<NW>(src, S, out.ccol_ptr + q.rd.cp_off, sm);
    __syncthreads();
    // ---- pass 2: CSC mirror (phasing-row index, value)
    int Rk = 0;
    for (int base = 0; base < nrow; base += STAGE_THREADS) {
      const int r = base + tid;
      const int isp = r < nrow ? src.bits(r) & 1 : 0;
      int k, d0, tk, d1;
      block_scan2n<NW, 16>(isp, 0, k, d0, tk, d1, sm);
      if (isp) {
        k += Rk;
        const int ee = src.rp(r + 1);
        for (int e = src.rp(r); e < ee; e++) {
          const int ci = src.col(e);
          if (!src.fp(ci)) continue;
          const int pos = atomicAdd(&src.cur(ci), 1);
          out.crow[q.e_base + pos] = k; out.cval[q.e_base + pos] = src.val(e) & 63;
        }
      }
      Rk += tk;
    }
    __syncthreads();
  };
  if (nrow <= STG_R && q.E_all <= STG_E && S <= STG_S) build(LdsRows{in, s_col, s_val, s_rp, s_isp, s_fp, s_cur});
  else build(GlobalRows{in, out, q.r0, q.c0, q.e_base});
  const long long ft = snp_constants(sc, out, q, s_fe, s_f1e);
  if (lane == 0) s_ft[wave] = ft;
  // ---- per-lane share of k4_enum_reg's row partition (enumeration regions only)
  if (S <= (int)in.max_enum_snps && tid < 64) {
    const uint32_t c = enum_chunk((uint32_t)E);
    auto lower = [&](uint32_t target) { int lo = 0, hi = R; while (lo < hi) { const int mid = (lo + hi) >> 1; if ((uint32_t)prp[mid] < target) lo = mid + 1; else hi = mid; } return lo; };
    const int f0 = lower((uint32_t)tid * c), f1 = lower((uint32_t)(tid + 1) * c);
    atomicMax(&s_max[0], prp[f1] - prp[f0]);
    atomicMax(&s_max[1], f1 - f0);
  }
  __syncthreads();
  if (tid == 0) {
    long long ftot = 0;
    for (int w = 0; w < NW; w++) ftot += s_ft[w];
    write_region(in, out, q, R, E, Fa, ftot, max(s_max[0], (int)enum_chunk((uint32_t)E)), s_max[1], q.E_all, s_max[2]);
  }
}

// ---------------------------------------------------------------------------------------------
// k4_stage_grid: ONE large region with all CUs.  Workgroup b owns a contiguous slab of fragment rows; slab totals give every slab its
// offsets, so the CSR comes out in row order.  The CSC mirror walks the CSR just written.
// blk_tot: per slab {phasing rows, phase entries} | the band width | per slab the rows that draw.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(K4_GRID_THREADS) k4_stage_grid(StageIn in, StageOut out, PhaseLutDev lut, int32_t g, GridCtl* ctl, int32_t* blk_tot) {
  constexpr int NW = K4_GRID_THREADS / 64;
  __shared__ long long red[NW];
  __shared__ unsigned long long bc[2];
  __shared__ int sm[2][16];
  __shared__ int s_sum[7];   // [5], [6]: rows with enough links (the rows that draw) in front of this slab / in the region
  __shared__ long long s_fe[32], s_f1e[32];
  GridScope sc{ctl, red, bc, 0u};
  const int tid = threadIdx.x, b = blockIdx.x, nb = gridDim.x;
  const StageRegion q = stage_region(in, g);
  const int nrow = q.nrow, c0 = q.c0;
  const int64_t e_base = q.e_base;
  const GlobalRows src{in, out, q.r0, c0, e_base};
  load_stage_lut(lut, s_fe, s_f1e);
  int32_t* wmax = blk_tot + 2 * nb;
  int32_t* blk_lnk = blk_tot + 2 * nb + 1;   // per slab: rows with enough links (down-sampling: the draw ordinals count them)
  snp_init(sc, in, out, q, src);
  if (sc.tid() == 0) *wmax = 0;
  sc.sync();
  const int rs = (((nrow + nb - 1) / nb) + 63) & ~63;         // rows per slab
  const int s0 = min(nrow, b * rs), s1 = min(nrow, s0 + rs);
  // ---- slab totals
  if (tid < 7) s_sum[tid] = 0;
  __syncthreads();
  int rows = 0, ents = 0, w = 0, lnk = 0;
  for (int r = s0 + tid; r < s1; r += K4_GRID_THREADS) { const RowInfo ri = row_scan(src, r); rows += ri.isp; ents += ri.cnt; w = max(w, ri.span); lnk += ri.isl; }
  atomicAdd(&s_sum[0], rows); atomicAdd(&s_sum[1], ents); atomicMax(&s_sum[2], w); atomicAdd(&s_sum[5], lnk);
  __syncthreads();
  if (tid == 0) { blk_tot[2 * b] = s_sum[0]; blk_tot[2 * b + 1] = s_sum[1]; blk_lnk[b] = s_sum[5]; if (s_sum[2]) atomicMax(wmax, s_sum[2]); }
  sc.sync();
  // ---- offsets of this slab, totals of the region
  if (tid < 7) s_sum[tid] = 0;
  __syncthreads();
  for (int k = tid; k < nb; k += K4_GRID_THREADS) {
    const int rr = blk_tot[2 * k], ee = blk_tot[2 * k + 1], ll = blk_lnk[k];
    if (k < b) { atomicAdd(&s_sum[0], rr); atomicAdd(&s_sum[1], ee); atomicAdd(&s_sum[5], ll); }
    atomicAdd(&s_sum[3], rr); atomicAdd(&s_sum[4], ee); atomicAdd(&s_sum[6], ll);
  }
  __syncthreads();
  int R = s_sum[0], E = s_sum[1], Fa = s_sum[5];
  const int R_tot = s_sum[3], E_tot = s_sum[4], F_tot = s_sum[6];
  int32_t* prp = out.prow_ptr + q.rd.rp_off;
  // ---- CSR of the slab (row order), column counts
  emit_csr<NW>(in, out, q, src, s0, s1, R, E, Fa, sm);
  if (b == nb - 1 && tid == 0) prp[R_tot] = E_tot;
  sc.sync();
  if (b == 0) column_offsets<NW>(src, q.S, out.ccol_ptr + q.rd.cp_off, sm);
  sc.sync();
  // ---- CSC mirror (phasing-row index, value)
  for (int k = sc.tid(); k < R_tot; k += sc.nt())
    for (int e = prp[k]; e < prp[k + 1]; e++) {
      const int pos = atomicAdd(&out.cursor[c0 + out.pcol[e_base + e]], 1);
      out.crow[e_base + pos] = k; out.cval[e_base + pos] = out.pval[e_base + e];
    }
  sc.sync();
  const long long ftot = sc.sync_sum(snp_constants(sc, out, q, s_fe, s_f1e));
  if (sc.tid() == 0) write_region(in, out, q, R_tot, E_tot, F_tot, ftot, INT_MAX, INT_MAX, q.E_all, *wmax);
}

}  // namespace

void launch_k4_stage(int32_t n_regions, hipStream_t s, const StageIn& in, const StageOut& out, const PhaseLutDev& lut) {
  if (n_regions > 0) hipLaunchKernelGGL(k4_stage, dim3((unsigned)n_regions), dim3(STAGE_THREADS), 0, s, in, out, lut);
}

hipError_t k4_stage_launch_grid(const StageIn& in, const StageOut& out, const PhaseLutDev& lut, int g, GridCtl* ctl, int32_t* blk_tot, hipStream_t s) {
  const int nb = k4_grid_blocks();
  if (nb <= 0) return hipErrorInvalidDevice;
  hipError_t e = hipMemsetAsync(ctl, 0, sizeof(GridCtl), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k4_stage_grid, dim3((unsigned)nb), dim3(K4_GRID_THREADS), 0, s, in, out, lut, (int32_t)g, ctl, blk_tot);
  return hipGetLastError();
}

// k4_post.hip — K4, post-phase steps (reference src/thread.rs:168-201, snpfrags.rs:191-733): k4_post, one workgroup per region with the
// region image in LDS, and k4_gpost, all CUs on one large region with the image in HBM.  Both set up the same state (post_init) and run
// k4_post.h's post_run; they differ in how the row-ordered column index is built.  Host control: k4_phase.hip.
#include <climits>
#include "k4_dev.h"
#include "k4_grid.h"
#include "k4_kernels.h"
#include "k4_post.h"

namespace {

// What both kernels set up before post_run: the LUT, the SNPs' state, the fragment rows' offsets and flags, the optimiser's haplotags.
template <class SC, class IDX>
__device__ __forceinline__ void post_init(SC& sc, const PostIn& in, const PostLut& lut, PostView<IDX>& v, int64_t e_base) {
  const int r0 = v.r0, c0 = v.c0;
  if (threadIdx.x < 31) { v.le[threadIdx.x] = lut.le[threadIdx.x]; v.l1e[threadIdx.x] = lut.l1e[threadIdx.x]; }
  for (int i = sc.tid(); i < v.S; i += sc.nt()) {
    v.sflags[i] = v.soflags[i] = v.cand[i].flags;
    v.shap[i] = in.st_delta[c0 + i]; v.sgt[i] = in.st_eta[c0 + i]; v.svt[i] = (int8_t)v.cand[i].variant_type;
    v.sps[i] = v.cand[i].phase_score;
    v.parent[i] = 0;
  }
  for (int r = sc.tid(); r < v.nrow; r += sc.nt()) {
    const int isp = in.links[r0 + r] >= in.min_linkers ? 1 : 0;
    v.rptr[r] = (IDX)(in.row_ptr[r0 + r] - e_base);
    v.lok[r] = (uint8_t)isp; v.fp[r] = (uint8_t)isp; v.asg[r] = 0; v.tag[r] = (int8_t)(isp && v.smp && !v.smp[r] ? 1 : 0);   // (an unsampled row's init_assignment tag: its sign is never read)
  }
  if (sc.tid() == 0) v.rptr[v.nrow] = (IDX)v.E;
  sc.sync();
  for (int k = sc.tid(); k < v.F; k += sc.nt()) v.tag[in.prow_src[r0 + k]] = in.st_sigma[r0 + k];   // the optimiser's haplotags
}

// ---------------------------------------------------------------------------------------------
// k4_post: the post-phase sequence of thread.rs:168-201, one workgroup per region with the region's fragment rows
// staged in LDS and a row-ordered column index (stable counting sort by one wave per row part).
// ---------------------------------------------------------------------------------------------
template <int NT>
__global__ void __launch_bounds__(NT) k4_post(PostIn in, const int32_t* __restrict__ slots, int32_t n_slots, PostLut lut) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  constexpr int NW = NT / 64;
  __shared__ int sm[2][16];
  __shared__ long long red[NW];
  __shared__ int wg_bc;
  __shared__ double stage[NW * 4 * POST_SSTR];
  if ((int)blockIdx.x >= n_slots) return;
  const int g = slots[blockIdx.x], tid = threadIdx.x, lane = tid & 63;
  const int r0 = in.row_region_off[g], nrow = in.row_region_off[g + 1] - r0;
  const int c0 = in.cand_off[g], S = in.cand_off[g + 1] - c0;
  if (S == 0) return;
  const int64_t e_base = in.row_ptr[r0];
  const int E = (int)(in.row_ptr[r0 + nrow] - e_base);
  const PostLayout L = post_layout(nrow, E, S);
  PostView<uint16_t> v;
  v.g = g; v.S = S; v.nrow = nrow; v.E = E; v.F = in.reg[g].R; v.FA = in.reg[g].F_all; v.r0 = r0; v.c0 = c0;
  v.smp = in.sampled ? in.sampled + r0 : nullptr;
  v.le = (double*)lds; v.l1e = v.le + 32;
  v.sps = (double*)(lds + L.sps); v.rpa = (double*)(lds + L.rpa); v.rpb = (double*)(lds + L.rpb);
  v.sflags = (uint32_t*)(lds + L.sflags); v.soflags = (uint32_t*)(lds + L.soflags);
  v.parent = (int32_t*)(lds + L.parent);
  v.rptr = (uint16_t*)(lds + L.rptr); v.ecol = (uint16_t*)(lds + L.ecol);
  v.erow = (uint16_t*)(lds + L.erow); v.cent = (uint16_t*)(lds + L.cent);
  v.ccptr = (uint16_t*)(lds + L.ccptr);
  v.ev = lds + L.eval;
  v.tag = (int8_t*)(lds + L.tag); v.asg = lds + L.asg; v.fp = lds + L.fp; v.lok = lds + L.lok;
  v.dirty = lds + L.dirty;
  v.shap = (int8_t*)(lds + L.shap); v.sgt = (int8_t*)(lds + L.sgt); v.svt = (int8_t*)(lds + L.svt);
  v.rcode = lds + L.rcode;
  v.cand = in.cand + c0;
  v.stage = stage;
  uint16_t* rptr = v.rptr; uint16_t* ecol = v.ecol; uint16_t* erow = v.erow; uint16_t* cent = v.cent; uint16_t* ccptr = v.ccptr;

  int n_mark = 0;
  auto mark = [&]() { if (in.dbg_clk && tid == 0) in.dbg_clk[(size_t)g * 16 + n_mark] = (long long)wall_clock64(); n_mark++; };
  mark();
  // ---- stage: LUT, SNP state, rows; then entries and the row-ordered column index
  WgScope sc{red, &wg_bc};
  post_init(sc, in, lut, v, e_base);
  mark();
  // row-ordered column index: wave q fills the entries of the q-th part of the rows (stable inside a
  // part: 64 entries at a time in (row, column) order, equal columns keep their order), the parts'
  // slots inside a column follow each other
  int32_t* qcnt = (int32_t*)(lds + L.qcnt);
  const int rq = (nrow + NW - 1) / NW;   // rows per part (one part per wave)
  for (int i = tid; i < NW * S; i += NT) qcnt[i] = 0;
  __syncthreads();
  for (int r = tid; r < nrow; r += NT)
    for (int e = rptr[r]; e < rptr[r + 1]; e++) {
      const int ci = in.col[e_base + e] - c0;
      ecol[e] = (uint16_t)ci; erow[e] = (uint16_t)r; v.ev[e] = in.val[e_base + e];
      atomicAdd(&qcnt[(r / rq) * S + ci], 1);
    }
  __syncthreads();
  {
    int carry = 0;
    for (int base = 0; base < S; base += NT) {
      const int i = base + tid;
      int x = 0;
      if (i < S) for (int q = 0; q < NW; q++) x += qcnt[q * S + i];
      int ex, d0, tot, d1;
      block_scan2n<NW, 16>(x, 0, ex, d0, tot, d1, sm);
      if (i < S) {
        int at = carry + ex;
        ccptr[i] = (uint16_t)at;
        for (int q = 0; q < NW; q++) { const int n = qcnt[q * S + i]; qcnt[q * S + i] = at; at += n; }
      }
      carry += tot;
    }
    if (tid == 0) ccptr[S] = (uint16_t)carry;
  }
  __syncthreads();
  {
    const int q = tid >> 6;
    int32_t* cur = qcnt + q * S;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int e_lo = rptr[min(q * rq, nrow)], e_hi = rptr[min((q + 1) * rq, nrow)];
    for (int base = e_lo; base < e_hi; base += 64) {
      const int e = base + lane;
      const bool valid = e < e_hi;
      const int c = valid ? (int)ecol[e] : -1;
      unsigned long long rem = __ballot(valid);
      while (rem) {
        const int cc = __shfl(c, __ffsll((long long)rem) - 1, 64);
        const unsigned long long m = __ballot(c == cc);
        const int at = cur[cc];
        if (c == cc) cent[at + __popcll(m & below)] = (uint16_t)e;
        wave_lds_sync();
        if (lane == 0) cur[cc] = at + __popcll(m);
        rem &= ~m;
      }
      wave_lds_sync();
    }
  }
  __syncthreads();
  mark();
  post_run(sc, in, lut, v, mark);
}

// ------------------------------------------------------------------------------------------------------------
// k4_gpost: the post-phase sequence (k4_post.h) with all CUs on ONE region, the region image in HBM
// ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(K4_GRID_THREADS) k4_gpost(PostIn in, PostScratch ps, int32_t g, PostLut lut) {
  __shared__ long long red[K4_GRID_THREADS / 64];
  __shared__ unsigned long long bc[2];
  __shared__ int sm[2][16];
  __shared__ double s_lut[64];
  __shared__ double stage[(K4_GRID_THREADS / 64) * 4 * POST_SSTR];
  GridScope sc{ps.ctl, red, bc, 0u};
  const int r0 = in.row_region_off[g], nrow = in.row_region_off[g + 1] - r0;
  const int c0 = in.cand_off[g], S = in.cand_off[g + 1] - c0;
  const int64_t e_base = in.row_ptr[r0];
  const int E = (int)(in.row_ptr[r0 + nrow] - e_base);
  PostView<int32_t> v;
  v.g = g; v.S = S; v.nrow = nrow; v.E = E; v.F = in.reg[g].R; v.FA = in.reg[g].F_all; v.r0 = r0; v.c0 = c0;
  v.smp = in.sampled ? in.sampled + r0 : nullptr;
  v.le = s_lut; v.l1e = s_lut + 32;
  v.sps = ps.sps; v.rpa = ps.rpa; v.rpb = ps.rpb; v.sflags = ps.sflags; v.soflags = ps.soflags; v.parent = ps.parent;
  v.rptr = ps.rptr; v.ecol = ps.ecol; v.erow = ps.erow; v.cent = ps.cent; v.ccptr = ps.ccptr; v.ev = ps.ev;
  v.tag = ps.tag; v.asg = ps.asg; v.fp = ps.fp; v.lok = ps.lok; v.dirty = ps.dirty;
  v.shap = ps.shap; v.sgt = ps.sgt; v.svt = ps.svt; v.rcode = ps.rcode;
  v.fdirt = ps.fdirt; v.minf = ps.minf; v.ndraw = ps.ndraw; v.gwords = ps.gwords;
  v.cand = in.cand + c0;
  v.stage = stage;
  int n_mark = 0;
  auto mark = [&]() { if (in.dbg_clk && sc.tid() == 0) in.dbg_clk[(size_t)g * 16 + n_mark] = (long long)wall_clock64(); n_mark++; };
  mark();
  for (int e = sc.tid(); e < E; e += sc.nt()) { v.ecol[e] = in.col[e_base + e] - c0; v.ev[e] = in.val[e_base + e]; }   // (visible behind post_init's barrier)
  post_init(sc, in, lut, v, e_base);
  mark();
  ordered_index(sc, nrow, S, v.rptr, v.ecol, nullptr, v.ccptr, v.erow, v.cent, ps.pcnt, ps.n_parts, sm);
  mark();
  post_run(sc, in, lut, v, mark);
}
}  // namespace

hipError_t launch_k4_post(int threads, unsigned n_blocks, size_t dyn_lds, hipStream_t s, const PostIn& in, const int32_t* slots, int32_t n_slots,
                          const PostLut& lut) {
  // 33 KB of static stage buffers + up to 64 KB of region image
  hipError_t e = hipSuccess;
  if (threads == CHAIN_THREADS) {
    if ((e = k4_set_dyn_lds_once(reinterpret_cast<const void*>(&k4_post<CHAIN_THREADS>), 96 * 1024, 4)) != hipSuccess) return e;
    hipLaunchKernelGGL(k4_post<CHAIN_THREADS>, dim3(n_blocks), dim3(CHAIN_THREADS), dyn_lds, s, in, slots, n_slots, lut);
  } else {   // CHAIN_THREADS / 2 == 2 * LCR_BLOCK
    if ((e = k4_set_dyn_lds_once(reinterpret_cast<const void*>(&k4_post<CHAIN_THREADS / 2>), 96 * 1024, 5)) != hipSuccess) return e;
    hipLaunchKernelGGL(k4_post<CHAIN_THREADS / 2>, dim3(n_blocks), dim3(CHAIN_THREADS / 2), dyn_lds, s, in, slots, n_slots, lut);
  }
  return hipSuccess;
}

hipError_t k4_post_launch_grid(const PostIn& post_in, const PostScratch& ps, int g, const PostLut& lut, hipStream_t s) {
  const int nb = k4_grid_blocks();
  if (nb <= 0) return hipErrorInvalidDevice;
  hipError_t e = hipMemsetAsync(ps.ctl, 0, sizeof(GridCtl), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k4_gpost, dim3((unsigned)nb), dim3(K4_GRID_THREADS), 0, s, post_in, ps, (int32_t)g, lut);
  return hipGetLastError();
}

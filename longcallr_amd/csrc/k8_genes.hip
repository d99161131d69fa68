// k8_genes.hip — K8: read -> gene over the bound batch (lcr_assign_genes) and the per-gene form of K7's counts on top of it
// (lcr_ase_genes); DESIGN.md "Per-gene expression".
//
// The contract (include/lcr.h), all coordinates 0-based half-open.  Read -> gene:
//   k8_check      the caller's annotation: spans sorted by (start, end), every gene's exons non-empty, ascending, disjoint, from the span's
//                 start to its end                                                                        -> verdict (pinned host memory)
//   k8_prefix_max the running maximum of the spans' ends: the first gene that can still reach a position is a binary search on it.  A
//                 read behind every long gene starts at its own genes; a read INSIDE a long gene starts at that gene and pays one
//                 span_end0 load and a skip for every gene between it and the read         -> pmax (gene-scale, one workgroup)
//   k8_assign     sixteen lanes per read: rend, the candidate range [lo, hi), then per candidate one walk over the CIGAR -- ops over the
//                 lanes, a row scan, a carry between rounds of 16 ops; every lane whose op is an N closes the block in front of it,
//                 searches the gene's exons and walks the few the block meets -- folded with xor shuffles; the running best under the
//                 strict > rule                                                                           -> gene, overlap per read
// Per-gene counts, over the fragment rows of region g whose read went to gene k (the pair (g, k)):
//   k8_pairs<false>  one workgroup per region: its genes in ascending order, one sweep each                -> pairs per region (a scan follows)
//   k8_pairs<true>   the same sweeps; per gene the phase-set sweep of K7 (k7_sweep.h) over the pair's rows -> record, row_tag
//   k8_sites      per candidate: the pair-independent part of eligibility -> site byte, the candidate's phase set; n_sites of every pair
//                 of its region whose phase set it is
//   k8_votes      eight lanes per tagged row; an entry counts when its site's phase set is the pair's     -> the pair's four cells
//   k8_export     the finished records to pinned host memory (without sites k8_pairs<true> writes them itself)
// All arithmetic is integer adds; nothing depends on the order in which atomics land.
#include <algorithm>

#include "k7_sweep.h"

namespace {

struct GeneView {
  int32_t n_genes, n_exons;
  const int64_t *span_start0, *span_end0;
  const int32_t* exon_off;
  const int64_t *exon_start0, *exon_end0;
};

__global__ void __launch_bounds__(LCR_BLOCK) k8_check(GeneView a, int32_t* __restrict__ bad) {
  const int32_t k = (int32_t)(blockIdx.x * LCR_BLOCK + threadIdx.x);
  if (k >= a.n_genes) return;
  bool ok = true;
  if (k == 0 && a.exon_off[0] != 0) ok = false;
  if (k == a.n_genes - 1 && a.exon_off[a.n_genes] != a.n_exons) ok = false;
  const int32_t x0 = a.exon_off[k], x1 = a.exon_off[k + 1];
  const int64_t s = a.span_start0[k], e = a.span_end0[k];
  if (k > 0) {
    const int64_t ps = a.span_start0[k - 1], pe = a.span_end0[k - 1];
    if (ps > s || (ps == s && pe > e)) ok = false;
  }
  if (x0 < 0 || x1 <= x0 || x1 > a.n_exons) ok = false;   // (no exon is read through a bad offset)
  if (ok) {
    if (a.exon_start0[x0] != s || a.exon_end0[x1 - 1] != e) ok = false;
    int64_t prev_end = s;
    for (int32_t i = x0; i < x1 && ok; i++) {
      const int64_t x = a.exon_start0[i], y = a.exon_end0[i];
      if (x >= y || x < prev_end) ok = false;
      prev_end = y;
    }
  }
  if (!ok) *bad = 1;   // (every writer stores the same value: a plain store)
}

// one workgroup: chunks of LCR_BLOCK genes, a Hillis-Steele maximum scan in LDS, the carry of the chunks in front
__global__ void __launch_bounds__(LCR_BLOCK) k8_prefix_max(const int64_t* __restrict__ span_end0, int32_t n_genes, int64_t* __restrict__ pmax) {
  __shared__ int64_t sh[LCR_BLOCK];
  const int tid = threadIdx.x;
  int64_t carry = INT64_MIN;
  for (int32_t base = 0; base < n_genes; base += LCR_BLOCK) {
    const int32_t k = base + tid;
    int64_t v = k < n_genes ? span_end0[k] : INT64_MIN;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < LCR_BLOCK; d <<= 1) {
      const int64_t o = tid >= d ? sh[tid - d] : INT64_MIN;
      __syncthreads();
      v = max(v, o);
      sh[tid] = v;
      __syncthreads();
    }
    v = max(v, carry);
    if (k < n_genes) pmax[k] = v;
    carry = max(carry, sh[LCR_BLOCK - 1]);
    __syncthreads();
  }
}

__device__ __forceinline__ bool k8_ref_op(int op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }   // M D N = X

// the overlap of the block [s, e) with gene exons [x0, x1): the script's interval-tree query with the block's inclusive end passed as
// an exclusive one -- nothing for e - s < 2; an exon [x, y) counts iff y > s && x < e - 1
__device__ __forceinline__ uint32_t k8_block_overlap(long long s, long long e, const int64_t* __restrict__ ex, const int64_t* __restrict__ ey,
                                                     int32_t x0, int32_t x1) {
  if (e - s < 2) return 0;
  int32_t lo = x0, hi = x1;   // first exon with y > s (exons are ascending and disjoint: so are their ends)
  while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (ey[mid] > s) hi = mid; else lo = mid + 1; }
  uint32_t ov = 0;
  for (int32_t i = lo; i < x1; i++) {
    const long long x = ex[i];
    if (!(x < e - 1)) break;
    const long long y = ey[i];
    ov += (uint32_t)(min(e, y) - max(s, x));
  }
  return ov;
}

// Sixteen lanes per read (one DPP row; four reads per wave64).  Every lane of a row takes the same branches outside k8_block_overlap,
// which holds no shuffle.
__global__ void __launch_bounds__(LCR_BLOCK) k8_assign(BatchView b, GeneView a, const int64_t* __restrict__ pmax, int32_t* __restrict__ gene,
                                                        uint32_t* __restrict__ overlap) {
  const int lane = threadIdx.x & 63, l16 = lane & 15, rbase = lane & 48;
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) >> 4;
  if (rl >= b.n_reads) return;   // (a whole row leaves)
  const int r = (int)rl;
  const uint32_t ncig = b.n_cig[r];
  const uint32_t* __restrict__ cg = b.cigar + b.cig_off[r];
  const long long pos = b.pos[r];
  // rend
  long long span = 0;
  for (uint32_t c = l16; c < ncig; c += 16) { const uint32_t w = cg[c]; if (k8_ref_op(w & 15)) span += (long long)(w >> 4); }
#pragma unroll
  for (int d = 8; d >= 1; d >>= 1) span += __shfl_xor(span, d, 64);
  const long long rend = pos + span;
  // candidates: span_start0 < rend bounds them above; below, the genes in front of the first one whose running maximum of ends exceeds pos all end at or before pos
  int32_t hi, lo;
  { int32_t p = 0, q = a.n_genes; while (p < q) { const int32_t mid = p + ((q - p) >> 1); if (a.span_start0[mid] < rend) p = mid + 1; else q = mid; } hi = p; }
  { int32_t p = 0, q = hi; while (p < q) { const int32_t mid = p + ((q - p) >> 1); if (pmax[mid] > pos) q = mid; else p = mid + 1; } lo = p; }
  int32_t best_gene = -1; uint32_t best_ov = 0;
  for (int32_t k = lo; k < hi; k++) {
    if (!(a.span_end0[k] > pos)) continue;   // (row-uniform)
    const int32_t x0 = a.exon_off[k], x1 = a.exon_off[k + 1];
    long long ref_cur = pos, blk_start = pos;
    uint32_t ov = 0;
    for (uint32_t c0 = 0; c0 < ncig; c0 += 16) {
      const uint32_t w = c0 + l16 < ncig ? cg[c0 + l16] : 0u;   // (a padding word is a 0-length M)
      const int op = w & 15, len = (int)(w >> 4);
      const int dr = k8_ref_op(op) ? len : 0;
      const int ir = row16_incl_scan(dr);
      const bool is_n = op == 3;                                 // (of any length, 0 included)
      const unsigned int m = (unsigned int)(__ballot(is_n) >> rbase) & 0xffffu;
      const long long rs = ref_cur + ir - dr;                    // the op's first reference column
      const long long after = rs + len;                          // (an N lane: the first column behind the gap)
      // the block an N closes begins behind the previous N of this round, or where the rounds in front left off
      const unsigned int below = m & ((1u << l16) - 1u);
      const int prev = below ? 31 - __clz((int)below) : 0;
      const long long prev_after = __shfl(after, rbase + prev, 64);
      if (is_n) ov += k8_block_overlap(below ? prev_after : blk_start, rs, a.exon_start0, a.exon_end0, x0, x1);
      if (m) blk_start = __shfl(after, rbase + (31 - __clz((int)m)), 64);
      ref_cur += __shfl(ir, rbase + 15, 64);
    }
    if (l16 == 0) ov += k8_block_overlap(blk_start, ref_cur, a.exon_start0, a.exon_end0, x0, x1);   // the block behind the last N
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) ov += __shfl_xor(ov, d, 64);
    if (best_gene < 0 || ov > best_ov) { best_gene = k; best_ov = ov; }
  }
  if (l16 == 0) { gene[r] = best_gene; overlap[r] = best_ov; }
}

// ---- per-gene counts ------------------------------------------------------------------------------------------------------------------

// One workgroup per region.  Row r of region g is the region's (r - r0)-th read (fragment.rs:293-307), so its gene is
// gene[read_begin[g] + r - r0].  The genes of the region's rows are visited in ascending order: every sweep finds the smallest gene index
// above the current one.  EMIT: per gene the phase-set sweep over the pair's rows, the record, and the tags of the rows that vote --
// pair and haplotype in one word, 0 for every other row.
template <bool EMIT>
__global__ void __launch_bounds__(LCR_BLOCK) k8_pairs(const int32_t* __restrict__ read_begin, const int32_t* __restrict__ row_region_off,
                                                       const lcr_read_record* __restrict__ rec, const int32_t* __restrict__ gene, int32_t ng,
                                                       int32_t* __restrict__ n_pairs, const int32_t* __restrict__ pair_off,
                                                       lcr_ase_gene* __restrict__ out, lcr_ase_gene* __restrict__ host_out,
                                                       int32_t* __restrict__ row_tag) {
  __shared__ int32_t sh_next;
  __shared__ uint32_t sh[3];
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g >= ng) return;
  const int r0 = row_region_off[g], r1 = row_region_off[g + 1];
  const int32_t* __restrict__ rg = gene + read_begin[g] - r0;   // rg[r] = gene of row r
  if (EMIT && row_tag)
    for (int r = r0 + tid; r < r1; r += LCR_BLOCK) if (rg[r] < 0) row_tag[r] = 0;
  int32_t cur = -1, j = 0;
  for (;;) {   // (every value of the loop's state is the same in all threads)
    if (tid == 0) sh_next = INT_MAX;
    __syncthreads();
    int32_t nxt = INT_MAX;
    for (int r = r0 + tid; r < r1; r += LCR_BLOCK) { const int32_t k = rg[r]; if (k > cur) nxt = min(nxt, k); }
    nxt = (int32_t)wave_min_u32((uint32_t)nxt);   // (gene indices above cur >= -1 are not negative)
    if ((tid & 63) == 0 && nxt != INT_MAX) atomicMin(&sh_next, nxt);
    __syncthreads();
    const int32_t k = sh_next;
    __syncthreads();
    if (k == INT_MAX) break;
    if (EMIT) {
      const int32_t p = pair_off[g] + j;
      const K7Pick best = k7_sweep_phase_sets(rec, r0, r1, [&](int r) { return rg[r] == k; }, sh);
      if (row_tag)
        for (int r = r0 + tid; r < r1; r += LCR_BLOCK) {
          if (rg[r] != k) continue;
          const lcr_read_record rr = rec[r];
          const bool sel = best.ps != 0 && rr.phase_set == best.ps && (rr.assignment == 1 || rr.assignment == 2);
          row_tag[r] = sel ? (p << 2) | rr.assignment : 0;
        }
      if (tid == 0) {
        lcr_ase_gene o{};
        o.region = g; o.gene = k; o.phase_set = best.ps; o.n_phase_sets = best.n_sets; o.h1 = best.h1; o.h2 = best.h2;
        out[p] = o;
        if (host_out) host_out[p] = o;
      }
    }
    cur = k; j++;
  }
  if (!EMIT && tid == 0) n_pairs[g] = j;
}

__global__ void k8_pair_offsets(const int32_t* __restrict__ pair_off, int32_t ng, int32_t* __restrict__ host_off, int32_t* __restrict__ host_ctl) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > ng) return;
  const int v = pair_off[g];
  host_off[g] = v;
  if (g == ng) host_ctl[0] = v;
}

// site byte as in K7 with bit0 = eligible apart from the phase set; site_ps = the candidate's phase set where bit0 is set, else 0
__global__ void __launch_bounds__(LCR_BLOCK) k8_sites(const lcr_candidate* __restrict__ cand, int32_t n_cand, double min_phase_score,
                                                       const int64_t* __restrict__ pos0, const uint8_t* __restrict__ pat,
                                                       const uint8_t* __restrict__ mat, int32_t n_sites, const int32_t* __restrict__ pair_off,
                                                       lcr_ase_gene* __restrict__ pairs, uint8_t* __restrict__ site, uint32_t* __restrict__ site_ps) {
  const int32_t i = (int32_t)(blockIdx.x * LCR_BLOCK + threadIdx.x);
  if (i >= n_cand) return;
  const lcr_candidate* __restrict__ s = cand + i;
  const uint8_t b = k7_site_byte(s, min_phase_score, pos0, pat, mat, n_sites);
  site[i] = b;
  site_ps[i] = b ? s->phase_set : 0u;
  if (!b) return;
  const int g = s->region;
  for (int32_t p = pair_off[g]; p < pair_off[g + 1]; p++)
    if (pairs[p].phase_set == s->phase_set) atomicAdd(&pairs[p].n_sites, 1u);
}

__global__ void __launch_bounds__(LCR_BLOCK) k8_votes(const int32_t* __restrict__ row_tag, int32_t n_rows, const int64_t* __restrict__ row_ptr,
                                                       const int32_t* __restrict__ col, const uint8_t* __restrict__ val,
                                                       const uint8_t* __restrict__ site, const uint32_t* __restrict__ site_ps, uint32_t min_baseq,
                                                       lcr_ase_gene* __restrict__ pairs) {
  const int l = threadIdx.x & (K7_GROUP - 1);
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) / K7_GROUP;
  if (rl >= n_rows) return;   // (a whole group leaves)
  const int r = (int)rl;
  const int tag = row_tag[r];
  if (tag == 0) return;
  lcr_ase_gene* o = pairs + (tag >> 2);
  const uint32_t ps = o->phase_set;   // (written by k8_pairs<true>; the kernels between change n_sites and the vote cells only)
  const int vote = k7_row_vote(row_ptr[r], row_ptr[r + 1], l, col, val, min_baseq,
                               [&](int i) { return site_ps[i] == ps ? site[i] : (uint8_t)0; });
  if (l != 0 || vote == 0) return;
  const bool h1 = (tag & 3) == 1;
  atomicAdd(vote > 0 ? (h1 ? &o->h1_pat : &o->h2_pat) : (h1 ? &o->h1_mat : &o->h2_mat), 1u);
}

__global__ void k8_export(const lcr_ase_gene* __restrict__ pairs, int32_t n, lcr_ase_gene* __restrict__ host_out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n) host_out[p] = pairs[p];
}

GeneView gene_view(const lcr_gene_annotation& a) {
  return GeneView{a.n_genes, a.n_exons, a.span_start0, a.span_end0, a.exon_off, a.exon_start0, a.exon_end0};
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_k8_check(const lcr_gene_annotation& a, int32_t* bad, hipStream_t s) {
  if (a.n_genes > 0) hipLaunchKernelGGL(k8_check, dim3((a.n_genes + LCR_BLOCK - 1) / LCR_BLOCK), dim3(LCR_BLOCK), 0, s, gene_view(a), bad);
}
void launch_k8_prefix_max(const lcr_gene_annotation& a, int64_t* pmax, hipStream_t s) {
  if (a.n_genes > 0) hipLaunchKernelGGL(k8_prefix_max, dim3(1), dim3(LCR_BLOCK), 0, s, a.span_end0, a.n_genes, pmax);
}
void launch_k8_assign(const BatchView& b, const lcr_gene_annotation& a, const int64_t* pmax, int32_t* gene, uint32_t* overlap, hipStream_t s) {
  if (b.n_reads <= 0) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k8_assign, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, gene_view(a), pmax, gene, overlap);
}
void launch_k8_pair_count(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, const int32_t* gene, int32_t* n_pairs, hipStream_t s) {
  if (b.n_regions > 0)
    hipLaunchKernelGGL(k8_pairs<false>, dim3(b.n_regions), dim3(LCR_BLOCK), 0, s, b.read_begin, row_region_off, rec, gene, b.n_regions, n_pairs,
                       (const int32_t*)nullptr, (lcr_ase_gene*)nullptr, (lcr_ase_gene*)nullptr, (int32_t*)nullptr);
}
void launch_k8_pair_offsets(const int32_t* pair_off, int32_t ng, int32_t* host_off, int32_t* host_ctl, hipStream_t s) {
  hipLaunchKernelGGL(k8_pair_offsets, dim3((ng + 1 + 255) / 256), dim3(256), 0, s, pair_off, ng, host_off, host_ctl);
}
void launch_k8_pair_emit(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, const int32_t* gene, const int32_t* pair_off,
                         lcr_ase_gene* out, lcr_ase_gene* host_out, int32_t* row_tag, hipStream_t s) {
  if (b.n_regions > 0)
    hipLaunchKernelGGL(k8_pairs<true>, dim3(b.n_regions), dim3(LCR_BLOCK), 0, s, b.read_begin, row_region_off, rec, gene, b.n_regions, (int32_t*)nullptr,
                       pair_off, out, host_out, row_tag);
}
void launch_k8_sites(const lcr_candidate* cand, int32_t n_cand, double min_phase_score, const int64_t* pos0, const uint8_t* pat, const uint8_t* mat,
                     int32_t n_sites, const int32_t* pair_off, lcr_ase_gene* pairs, uint8_t* site, uint32_t* site_ps, hipStream_t s) {
  if (n_cand > 0) hipLaunchKernelGGL(k8_sites, dim3((n_cand + LCR_BLOCK - 1) / LCR_BLOCK), dim3(LCR_BLOCK), 0, s, cand, n_cand, min_phase_score, pos0, pat, mat,
                                     n_sites, pair_off, pairs, site, site_ps);
}
void launch_k8_votes(const int32_t* row_tag, int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, const uint8_t* site,
                     const uint32_t* site_ps, uint32_t min_baseq, lcr_ase_gene* pairs, hipStream_t s) {
  if (n_rows <= 0) return;
  const long long threads = (long long)n_rows * K7_GROUP;
  hipLaunchKernelGGL(k8_votes, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, row_tag, n_rows, row_ptr, col, val, site, site_ps,
                     min_baseq, pairs);
}
void launch_k8_export(const lcr_ase_gene* pairs, int32_t n, lcr_ase_gene* host_out, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k8_export, dim3((n + 255) / 256), dim3(256), 0, s, pairs, n, host_out);
}

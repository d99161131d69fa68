// k10_asj_modes.hip — K10: what lcr_asj_genes adds to K9's per-gene junction table (k9_gene_junctions.hip; DESIGN.md "Per-gene junctions:
// exons, DNA filter, coverage").  The junction table itself is built by K9's launchers on K10's buffers; the kernels here run beside them:
//   k10_dna_check     the caller's DNA sites: ascending unique positions                                   -> verdict (pinned host memory)
//   k10_walk<false>   sixteen lanes per read with a gene: its junctions and its INTERIOR blocks            -> nblk (participating rows),
//                     gene_reads[gene] += 1 for every read with more than min_junctions junctions             one scan follows
//   k10_pair_blocks   per participating read nblk into its pair's sum (integer atomics)                    -> pair_blk
//   (k9_sizes: per pair the slots of its segment of the EXON hash table, one scan follows)
//   k10_walk<true>    the same walk: every interior block's key start << 32 | len into the pair's segment
//   (k6's flag kernel, one scan, k9_offsets: kept exons in front of every region)
//   k10_compact, k10_rank   the kept slots pair after pair, then every kept exon to its rank among the pair's kept keys
//   k10_support       per candidate: PASS + phased het + phase set (k7_site_byte's test without the parental join) and pos in dna_pos0
//                     -> its phase set or 0
//   k10_support_uniq  one workgroup per region: the distinct supported phase sets, ascending (the sweep of k7_sweep.h)
//   k10_filter        per participating row: phase set not among its region's supported ones -> the row's "counted" bit is cleared, in
//                     front of k9_tables
// A second table, not tagged keys in K9's: K9's launchers then run unchanged on unchanged data, so flags cannot move a junction record.
// Blocks: an N op of length >= 1 closes the block in front of it, [end of the previous such N (or pos), its own start); a closed block
// with bases that is not the read's first one with bases is interior; the last block is never closed, so it is never seen.  All integer;
// nothing depends on the order in which atomics land.
#include <algorithm>

#include "k7_sweep.h"

namespace {

constexpr unsigned long long K10_EMPTY = ~0ull;   // no key (the fill of the table; a block's start is below 2^31)

__device__ __forceinline__ uint32_t k10_hash(unsigned long long key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32); }

__global__ void __launch_bounds__(LCR_BLOCK) k10_dna_check(const int64_t* __restrict__ pos0, int32_t n, int32_t* __restrict__ bad) {
  const int32_t i = (int32_t)(blockIdx.x * LCR_BLOCK + threadIdx.x);
  if (i >= n) return;
  if (i > 0 && pos0[i - 1] >= pos0[i]) *bad = 1;   // (every writer stores the same value: a plain store)
}

// Sixteen lanes per read (one DPP row; four reads per wave64), k9_walk's walk.  The carry between rounds of sixteen ops: the reference
// cursor, the open block's start, "a block with bases was closed before".  Every lane of a row takes the same branches outside the
// table insertion, which holds no shuffle.
template <bool EMIT>
__global__ void __launch_bounds__(LCR_BLOCK) k10_walk(BatchView b, const int32_t* __restrict__ gene, const int32_t* __restrict__ part_flag,
                                                       uint32_t min_junctions, int32_t* __restrict__ nblk, int32_t* __restrict__ gene_reads,
                                                       const int32_t* __restrict__ read_pair, const int32_t* __restrict__ xtbl_off,
                                                       unsigned long long* __restrict__ xtbl_key, uint32_t* __restrict__ xtbl_cnt) {
  const int lane = threadIdx.x & 63, l16 = lane & 15, rbase = lane & 48;
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) >> 4;
  if (rl >= b.n_reads) return;   // (a whole row leaves)
  const int r = (int)rl;
  const int32_t k = EMIT ? 0 : gene[r];
  const bool part = part_flag[r] != 0;   // (K9's: a fragment row with assignment 1 / 2, a gene and more than min_junctions junctions)
  if (!EMIT) {
    if (k < 0 || (!gene_reads && !part)) { if (l16 == 0 && nblk) nblk[r] = 0; return; }
  } else {
    if (!part || nblk[r] == 0) return;
  }
  const uint32_t ncig = b.n_cig[r];
  const uint32_t* __restrict__ cg = b.cigar + b.cig_off[r];
  const int p = EMIT ? read_pair[r] : 0;
  const int t0 = EMIT ? xtbl_off[p] : 0;
  const uint32_t mask = EMIT ? (uint32_t)(xtbl_off[p + 1] - t0) - 1u : 0u;   // (no pair's segment is empty: k9_sizes gives two slots at least)
  const uint32_t below = (1u << l16) - 1u;
  int ref_cur = b.pos[r], blk_start = ref_cur, n_n = 0, n_int = 0;
  bool closed = false;
  for (uint32_t c0 = 0; c0 < ncig; c0 += 16) {
    const uint32_t w = c0 + l16 < ncig ? cg[c0 + l16] : 0u;   // (a padding word is a 0-length M)
    const int op = w & 15, len = (int)(w >> 4);
    const int dr = (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? len : 0;   // I S H P consume no reference
    const int ir = row16_incl_scan(dr);
    const bool is_n = op == 3 && len >= 1;
    const unsigned int m = (unsigned int)(__ballot(is_n) >> rbase) & 0xffffu;
    const int e = ref_cur + ir, s = e - dr;   // the op's reference columns [s, e)
    // the block this N closes starts behind the previous N of the round, or at the carried start
    const unsigned int lower = m & below;
    const int prev_end = __shfl(e, rbase + (lower ? 31 - __clz((int)lower) : 0), 64);
    const int bs = lower ? prev_end : blk_start;
    const bool full = is_n && s > bs;   // it holds a base
    const unsigned int mf = (unsigned int)(__ballot(full) >> rbase) & 0xffffu;
    const bool interior = full && (closed || (mf & below) != 0u);
    if (!EMIT) {
      n_int += __popc((unsigned int)(__ballot(interior) >> rbase) & 0xffffu);
    } else if (interior) {
      const unsigned long long key = ((unsigned long long)(uint32_t)bs << 32) | (uint32_t)(s - bs);
      // the segment has at least twice the pair's interior blocks in slots: an empty one is met before the probe comes round
      uint32_t h = k10_hash(key) & mask;
      for (uint32_t i = 0; i <= mask; i++, h = (h + 1) & mask) {
        const unsigned long long prev = atomicCAS(&xtbl_key[t0 + h], K10_EMPTY, key);
        if (prev == K10_EMPTY || prev == key) { atomicAdd(&xtbl_cnt[t0 + h], 1u); break; }   // (a read holds a block once: starts rise along it)
      }
    }
    const int last_end = __shfl(e, rbase + (m ? 31 - __clz((int)m) : 0), 64);
    if (m) blk_start = last_end;
    if (mf) closed = true;
    n_n += __popc(m);
    ref_cur += __shfl(ir, rbase + 15, 64);
  }
  if (EMIT || l16 != 0) return;
  if (nblk) nblk[r] = part ? n_int : 0;
  if (gene_reads && (uint32_t)n_n > min_junctions) atomicAdd(&gene_reads[k], 1);
}

__global__ void k10_pair_blocks(int32_t nr, const int32_t* __restrict__ part_flag, const int32_t* __restrict__ nblk,
                                const int32_t* __restrict__ read_pair, int32_t* __restrict__ pair_blk) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nr || !part_flag[r]) return;
  const int32_t n = nblk[r];
  if (n) atomicAdd(&pair_blk[read_pair[r]], n);
}

__global__ void k10_compact(const unsigned long long* __restrict__ tbl_key, const uint32_t* __restrict__ tbl_cnt, const int32_t* __restrict__ flag,
                            const int32_t* __restrict__ koff, const int32_t* __restrict__ tbl_off, const int32_t* __restrict__ pair_off, int32_t ng,
                            int32_t n_slots, unsigned long long* __restrict__ ck, uint32_t* __restrict__ cc, int32_t* __restrict__ cp) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots || !flag[t]) return;
  int lo = 0, hi = pair_off[ng];   // the pair whose segment holds slot t: the last p with tbl_off[p] <= t (no pair's segment is empty)
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tbl_off[mid] <= t) lo = mid; else hi = mid; }
  const int j = koff[t];
  ck[j] = tbl_key[t]; cc[j] = tbl_cnt[t]; cp[j] = lo;
}

// k9_rank's argument: a pair keeps tens of exons.  The pair's kept exons are [koff[tbl_off[p]], koff[tbl_off[p + 1]]).
__global__ void k10_rank(const unsigned long long* __restrict__ ck, const uint32_t* __restrict__ cc, const int32_t* __restrict__ cp,
                         const int32_t* __restrict__ koff, const int32_t* __restrict__ tbl_off, const int32_t* __restrict__ pair_region,
                         const int32_t* __restrict__ pair_gene, int32_t n_kept, lcr_exon_gene* __restrict__ out, lcr_exon_gene* __restrict__ host_out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_kept) return;
  const int p = cp[j], lo = koff[tbl_off[p]], hi = koff[tbl_off[p + 1]];
  const unsigned long long key = ck[j];
  int rank = 0;
  for (int q = lo; q < hi; q++) rank += ck[q] < key ? 1 : 0;
  lcr_exon_gene o{};
  o.region = pair_region[p]; o.gene = pair_gene[p]; o.start0 = (int64_t)(key >> 32); o.len = (int32_t)(key & 0xffffffffu); o.n_reads = cc[j];
  out[lo + rank] = o; host_out[lo + rank] = o;
}

__global__ void __launch_bounds__(LCR_BLOCK) k10_support(const lcr_candidate* __restrict__ cand, int32_t n_cand, double min_phase_score,
                                                          const int64_t* __restrict__ pos0, int32_t n_dna, uint32_t* __restrict__ sup) {
  const int32_t i = (int32_t)(blockIdx.x * LCR_BLOCK + threadIdx.x);
  if (i >= n_cand) return;
  const lcr_candidate* s = cand + i;
  const uint32_t fl = s->flags;
  const bool ok = !(fl & (LCR_F_DENSE | LCR_F_NON_SELECTED)) && s->variant_type == 1 && s->phase_score >= min_phase_score &&
                  (s->allele1 != s->ref_base || s->allele2 != s->ref_base) && s->phase_set != 0;   // k7_site_byte's (1) - (2)
  uint32_t v = 0;
  if (ok) {
    const int64_t p = s->pos;
    int lo = 0, hi = n_dna;   // first site with pos0 >= p
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (pos0[mid] < p) lo = mid + 1; else hi = mid; }
    if (lo < n_dna && pos0[lo] == p) v = s->phase_set;
  }
  sup[i] = v;
}

// One workgroup per region: sweep j finds the j-th smallest supported phase set of the region's candidates (0 = not supporting).
__global__ void __launch_bounds__(LCR_BLOCK) k10_support_uniq(const int32_t* __restrict__ cand_off, const uint32_t* __restrict__ sup, int32_t ng,
                                                               uint32_t* __restrict__ uniq, int32_t* __restrict__ n_uniq) {
  __shared__ uint32_t sh_next;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g >= ng) return;
  const int c0 = cand_off[g], c1 = cand_off[g + 1];
  uint32_t cur = 0;
  int32_t j = 0;
  for (;;) {   // (every value of the loop's state is the same in all threads)
    if (tid == 0) sh_next = 0xffffffffu;
    __syncthreads();
    uint32_t nxt = 0xffffffffu;
    for (int c = c0 + tid; c < c1; c += LCR_BLOCK) { const uint32_t v = sup[c]; if (v > cur) nxt = min(nxt, v); }
    nxt = wave_min_u32(nxt);
    if ((tid & 63) == 0 && nxt != 0xffffffffu) atomicMin(&sh_next, nxt);
    __syncthreads();
    const uint32_t next = sh_next;
    __syncthreads();
    if (next == 0xffffffffu) break;
    if (tid == 0) uniq[c0 + j] = next;   // (at most one distinct value per candidate: j < c1 - c0)
    cur = next; j++;
  }
  if (tid == 0) n_uniq[g] = j;
}

__global__ void k10_filter(BatchView b, const int32_t* __restrict__ part_flag, const int32_t* __restrict__ row_slot,
                           const int32_t* __restrict__ cand_off, const uint32_t* __restrict__ uniq, const int32_t* __restrict__ n_uniq,
                           K9Row* __restrict__ rows) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= b.n_reads || !part_flag[r]) return;
  const int g = region_of_read(b, r);
  K9Row* row = rows + row_slot[r];
  const uint32_t ps = row->ps;
  bool ok = false;
  if (ps != 0) {
    int lo = cand_off[g], hi = lo + n_uniq[g];   // ascending: first value >= ps
    const int end = hi;
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (uniq[mid] < ps) lo = mid + 1; else hi = mid; }
    ok = lo < end && uniq[lo] == ps;
  }
  if (!ok) row->hap &= ~4;
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_k10_dna_check(const int64_t* dna_pos0, int32_t n_dna, int32_t* bad, hipStream_t s) {
  if (n_dna > 0) hipLaunchKernelGGL(k10_dna_check, dim3((n_dna + LCR_BLOCK - 1) / LCR_BLOCK), dim3(LCR_BLOCK), 0, s, dna_pos0, n_dna, bad);
}
void launch_k10_count(const BatchView& b, const int32_t* gene, const int32_t* part_flag, uint32_t min_junctions, int32_t* nblk, int32_t* gene_reads,
                      hipStream_t s) {
  if (b.n_reads <= 0 || (!nblk && !gene_reads)) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k10_walk<false>, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, gene, part_flag, min_junctions, nblk,
                     gene_reads, (const int32_t*)nullptr, (const int32_t*)nullptr, (unsigned long long*)nullptr, (uint32_t*)nullptr);
}
void launch_k10_pair_blocks(const BatchView& b, const int32_t* part_flag, const int32_t* nblk, const int32_t* read_pair, int32_t* pair_blk, hipStream_t s) {
  if (b.n_reads > 0) hipLaunchKernelGGL(k10_pair_blocks, dim3((b.n_reads + 255) / 256), dim3(256), 0, s, b.n_reads, part_flag, nblk, read_pair, pair_blk);
}
void launch_k10_emit(const BatchView& b, const int32_t* part_flag, const int32_t* nblk, const int32_t* read_pair, const int32_t* xtbl_off, uint64_t* xtbl_key,
                     uint32_t* xtbl_cnt, hipStream_t s) {
  if (b.n_reads <= 0) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k10_walk<true>, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, (const int32_t*)nullptr, part_flag, 0u,
                     const_cast<int32_t*>(nblk), (int32_t*)nullptr, read_pair, xtbl_off, (unsigned long long*)xtbl_key, xtbl_cnt);
}
void launch_k10_place(const uint64_t* xtbl_key, const uint32_t* xtbl_cnt, const int32_t* flag, const int32_t* koff, const int32_t* xtbl_off,
                      const int32_t* pair_off, const K9Pairs& pr, int32_t ng, int32_t n_slots, int32_t n_kept, uint64_t* ck, uint32_t* cc, int32_t* cp,
                      lcr_exon_gene* exon, lcr_exon_gene* host_exon, hipStream_t s) {
  if (n_slots <= 0 || n_kept <= 0) return;
  hipLaunchKernelGGL(k10_compact, dim3((n_slots + 255) / 256), dim3(256), 0, s, (const unsigned long long*)xtbl_key, xtbl_cnt, flag, koff, xtbl_off, pair_off, ng,
                     n_slots, (unsigned long long*)ck, cc, cp);
  hipLaunchKernelGGL(k10_rank, dim3((n_kept + 255) / 256), dim3(256), 0, s, (const unsigned long long*)ck, (const uint32_t*)cc, (const int32_t*)cp, koff, xtbl_off,
                     (const int32_t*)pr.region, (const int32_t*)pr.gene, n_kept, exon, host_exon);
}
void launch_k10_support(const lcr_candidate* cand, int32_t n_cand, const int32_t* cand_off, int32_t ng, double min_phase_score, const int64_t* dna_pos0,
                        int32_t n_dna, uint32_t* sup, uint32_t* sup_uniq, int32_t* sup_n, hipStream_t s) {
  if (n_cand > 0) hipLaunchKernelGGL(k10_support, dim3((n_cand + LCR_BLOCK - 1) / LCR_BLOCK), dim3(LCR_BLOCK), 0, s, cand, n_cand, min_phase_score, dna_pos0, n_dna, sup);
  if (ng > 0) hipLaunchKernelGGL(k10_support_uniq, dim3(ng), dim3(LCR_BLOCK), 0, s, cand_off, (const uint32_t*)sup, ng, sup_uniq, sup_n);
}
void launch_k10_filter(const BatchView& b, const int32_t* part_flag, const int32_t* row_slot, const int32_t* cand_off, const uint32_t* sup_uniq,
                       const int32_t* sup_n, void* rows, hipStream_t s) {
  if (b.n_reads > 0) hipLaunchKernelGGL(k10_filter, dim3((b.n_reads + 255) / 256), dim3(256), 0, s, b, part_flag, row_slot, cand_off, sup_uniq, sup_n, (K9Row*)rows);
}

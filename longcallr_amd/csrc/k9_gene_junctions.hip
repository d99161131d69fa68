// k9_gene_junctions.hip — K9: haplotype x junction counts per (region, gene) pair over the phased rows (lcr_junctions_genes;
// DESIGN.md "Per-gene junctions").  K6 (k6_junctions.hip) with the gene of K8 as a second grouping key, plus the script's exon-overlap
// filter as one more test per read.
//
// The contract (include/lcr.h) per pair (g, k), over the PARTICIPATING rows -- fragment rows of region g with assignment 1 / 2 whose read
// went to gene k >= 0 and has more than min_junctions N ops of length >= 1:
//   k9_walk<false>   sixteen lanes per read count the read's junctions                       -> part_flag, nocc   (two scans follow)
//   k9_pairs<false>  one workgroup per region: the genes of its participating reads, ascending -> pairs per region (one scan follows)
//   k9_pairs<true>   the same sweeps; per gene a running count over the region's reads in read order gives every participating read its
//                    pair and its slot among the row records -- a pair's rows are contiguous and keep the reads' order, which is by pos --
//                    and the pair its region, gene, first row, rows and junction occurrences
//   k9_sizes         per pair the slots of its segment of the junction hash table            -> tsz               (one scan follows)
//   k9_walk<true>    the same walk again: per junction the key s << 32 | l and its insertion into the PAIR's table segment (the key has
//                    no room for a gene: the gene is the segment); per M / = / X / D op the test "one of its bases lies in a merged exon
//                    of gene k" (a binary search on the exons' ends, then exon_start < the op's end); the row's record
//                    {pos, rend, ps, first key, keys, hap | counted}
//   (k6's flag kernel: slot kept = occupied && n_reads >= min_count, one scan follows)
//   k9_offsets       junctions in front of every region, to HBM and to pinned host memory
//   k9_compact       the kept slots, pair after pair (in slot order)
//   k9_rank          every kept junction to its rank among the pair's kept keys (= order by s, then l) + the motif
//   k9_tables        one workgroup per kept junction: over the pair's COUNTED rows the overlap, presence, the phase set with the most
//                    rows, the four counters
// Pairs come out ordered by region and then gene, so the records are ordered by region, gene, s, l.  All arithmetic is integer adds, and
// nothing depends on the order in which atomics land: a slot's position inside its segment does, the sorted output does not; row slots
// come from counts in read order, not from arrival.
#include <algorithm>

#include "k6_walk.h"

namespace {

constexpr unsigned long long K9_EMPTY = ~0ull;   // no key (the fill of K6's table: l < 2^28 keeps every key below it)

struct K9Exons { const int32_t* exon_off; const int64_t *exon_start0, *exon_end0; };

__device__ __forceinline__ uint32_t k9_hash(unsigned long long key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32); }

// does [s, e), s < e, share a base with one of the ascending, disjoint exons [x0, x1)?  The first exon that ends behind s is the only
// one that can be the first to meet it
__device__ __forceinline__ bool k9_shares_base(long long s, long long e, const int64_t* __restrict__ ex, const int64_t* __restrict__ ey,
                                               int32_t x0, int32_t x1) {
  int32_t lo = x0, hi = x1;   // first exon with y > s
  while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (ey[mid] > s) hi = mid; else lo = mid + 1; }
  return lo < x1 && ex[lo] < e;
}

// Sixteen lanes per read (one DPP row; four reads per wave64), the walk of k6_walk: ops spread over the lanes, reference offsets from a
// row scan of the reference-consuming lengths (M D N = X), a carry between rounds of 16 ops.  Every lane of a row takes the same branches
// outside k9_shares_base, which holds no shuffle.
template <bool EMIT>
__global__ void __launch_bounds__(LCR_BLOCK) k9_walk(BatchView b, const int32_t* __restrict__ row_region_off, const lcr_read_record* __restrict__ rec,
                                                      const int32_t* __restrict__ gene, uint32_t min_junctions, int32_t* __restrict__ part_flag,
                                                      int32_t* __restrict__ nocc, const int32_t* __restrict__ occ_off,
                                                      const int32_t* __restrict__ read_pair, const int32_t* __restrict__ row_slot,
                                                      const int32_t* __restrict__ tbl_off, K9Exons a, K9Row* __restrict__ rows,
                                                      unsigned long long* __restrict__ keys, unsigned long long* __restrict__ tbl_key,
                                                      uint32_t* __restrict__ tbl_cnt) {
  const int lane = threadIdx.x & 63, l16 = lane & 15, rbase = lane & 48;
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) >> 4;
  if (rl >= b.n_reads) return;   // (a whole row leaves)
  const int r = (int)rl;
  const int g = region_of_read(b, r);
  int hap = 0; uint32_t ps = 0;
  int32_t x0 = 0, x1 = 0;
  if (!EMIT) {
    // row k of region g is the region's k-th read (fragment.rs:293-307: the reads up to the last candidate); a read behind them is no row
    const int k = r - b.read_begin[g], row0 = row_region_off[g];
    bool cand = k < row_region_off[g + 1] - row0 && gene[r] >= 0;
    if (cand) { const int as = rec[row0 + k].assignment; cand = as == 1 || as == 2; }
    if (!cand) { if (l16 == 0) { part_flag[r] = 0; nocc[r] = 0; } return; }
  } else {
    if (!part_flag[r]) return;
    const lcr_read_record rr = rec[row_region_off[g] + (r - b.read_begin[g])];
    hap = rr.assignment; ps = rr.phase_set;
    const int32_t k = gene[r];
    x0 = a.exon_off[k]; x1 = a.exon_off[k + 1];
  }
  const uint32_t ncig = b.n_cig[r];
  const uint32_t* __restrict__ cg = b.cigar + b.cig_off[r];
  const int pos = b.pos[r];
  const int first = EMIT ? occ_off[r] : 0;
  const int p = EMIT ? read_pair[r] : 0;
  const int t0 = EMIT ? tbl_off[p] : 0;
  const uint32_t mask = EMIT ? (uint32_t)(tbl_off[p + 1] - t0) - 1u : 0u;   // (a participating row has an occurrence: the segment is not empty)
  int ref_cur = pos, n_n = 0;
  bool counted = false;
  for (uint32_t c0 = 0; c0 < ncig; c0 += 16) {
    const uint32_t w = c0 + l16 < ncig ? cg[c0 + l16] : 0u;   // (a padding word is a 0-length M)
    const int op = w & 15, len = (int)(w >> 4);
    const int dr = (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? len : 0;   // I S H P consume no reference
    const int ir = row16_incl_scan(dr);
    const bool is_n = op == 3 && len >= 1;
    const unsigned int m = (unsigned int)(__ballot(is_n) >> rbase) & 0xffffu;
    const int s = ref_cur + ir - dr;   // the op's first reference column
    if (EMIT) {
      if (is_n) {
        const unsigned long long key = ((unsigned long long)(uint32_t)s << 32) | (uint32_t)len;
        keys[first + n_n + __popc(m & ((1u << l16) - 1u))] = key;
        // the segment has at least twice the pair's occurrences in slots: an empty one is met before the probe comes round
        uint32_t h = k9_hash(key) & mask;
        for (uint32_t i = 0; i <= mask; i++, h = (h + 1) & mask) {
          const unsigned long long prev = atomicCAS(&tbl_key[t0 + h], K9_EMPTY, key);
          if (prev == K9_EMPTY || prev == key) { atomicAdd(&tbl_cnt[t0 + h], 1u); break; }   // (a read holds a key once: s rises along it)
        }
      }
      // the filter: the bases of an M / = / X / D op against the gene's merged exons, until one op of the read has met one
      const bool aligned = dr > 0 && op != 3;
      const bool hit = !counted && aligned && k9_shares_base(s, (long long)s + len, a.exon_start0, a.exon_end0, x0, x1);
      if (((unsigned int)(__ballot(hit) >> rbase) & 0xffffu) != 0u) counted = true;
    }
    n_n += __popc(m);
    ref_cur += __shfl(ir, rbase + 15, 64);
  }
  if (l16 != 0) return;
  if (!EMIT) {
    const int pf = (uint32_t)n_n > min_junctions ? 1 : 0;
    part_flag[r] = pf; nocc[r] = pf ? n_n : 0;
  } else {
    rows[row_slot[r]] = K9Row{pos, ref_cur, ps, first, n_n, hap | (counted ? 4 : 0)};
  }
}

// One workgroup per region.  The genes of the region's participating reads are visited in ascending order: every sweep finds the smallest
// gene index above the current one (k8_pairs' sweep, over reads in place of rows).  EMIT: per gene one more pass over the region's reads in
// read order with a running count -- a ballot per wave, the waves' totals through LDS -- that gives every read of the pair its slot.
template <bool EMIT>
__global__ void __launch_bounds__(LCR_BLOCK) k9_pairs(const int32_t* __restrict__ read_begin, const int32_t* __restrict__ gene,
                                                       const int32_t* __restrict__ part_flag, const int32_t* __restrict__ nocc, int32_t ng,
                                                       int32_t* __restrict__ n_pairs, const int32_t* __restrict__ pair_off,
                                                       const int32_t* __restrict__ part_off, int32_t* __restrict__ read_pair,
                                                       int32_t* __restrict__ row_slot, int32_t* __restrict__ pair_region,
                                                       int32_t* __restrict__ pair_gene, int32_t* __restrict__ pair_row0,
                                                       int32_t* __restrict__ pair_rows, int32_t* __restrict__ pair_occ) {
  __shared__ int32_t sh_next;
  __shared__ uint32_t sh_wave[LCR_BLOCK / 64], sh_occ;
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (g >= ng) return;
  const int r0 = read_begin[g], r1 = read_begin[g + 1];
  int32_t cur = -1, j = 0;
  int32_t base = EMIT ? part_off[r0] : 0;   // the first row slot of the region's next pair
  for (;;) {   // (every value of the loop's state is the same in all threads)
    if (tid == 0) { sh_next = INT_MAX; sh_occ = 0; }
    __syncthreads();
    int32_t nxt = INT_MAX;
    for (int r = r0 + tid; r < r1; r += LCR_BLOCK) { const int32_t k = gene[r]; if (part_flag[r] && k > cur) nxt = min(nxt, k); }
    nxt = (int32_t)wave_min_u32((uint32_t)nxt);   // (a participating read's gene is not negative)
    if (lane == 0 && nxt != INT_MAX) atomicMin(&sh_next, nxt);
    __syncthreads();
    const int32_t k = sh_next;
    if (k == INT_MAX) break;
    if (EMIT) {
      const int32_t p = pair_off[g] + j;
      int32_t n_rows = 0;
      uint32_t occ = 0;
      for (int c = r0; c < r1; c += LCR_BLOCK) {   // chunks of LCR_BLOCK reads in read order
        const int r = c + tid;
        const bool in = r < r1 && part_flag[r] && gene[r] == k;
        const unsigned long long bal = __ballot(in);
        if (lane == 0) sh_wave[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        int32_t before = 0, total = 0;
        for (int w = 0; w < LCR_BLOCK / 64; w++) { const int32_t t = (int32_t)sh_wave[w]; if (w < wv) before += t; total += t; }
        if (in) {
          read_pair[r] = p;
          row_slot[r] = base + n_rows + before + __popcll(bal & ((1ull << lane) - 1ull));
          occ += (uint32_t)nocc[r];
        }
        n_rows += total;
        __syncthreads();
      }
      occ = wave_sum_u32(occ);
      if (lane == 0 && occ) atomicAdd(&sh_occ, occ);
      __syncthreads();
      if (tid == 0) { pair_region[p] = g; pair_gene[p] = k; pair_row0[p] = base; pair_rows[p] = n_rows; pair_occ[p] = (int32_t)sh_occ; }
      base += n_rows;
    }
    __syncthreads();   // (sh_next and sh_occ are reset at the loop's head)
    cur = k; j++;
  }
  if (!EMIT && tid == 0) n_pairs[g] = j;
}

// per pair: slots of its table segment = 2 x occurrences rounded up to a power of two; 0 behind the last pair (the arrays are sized by
// the reads, an upper bound of the pairs the host does not wait for); the totals for the host
__global__ void k9_sizes(const int32_t* __restrict__ pair_off, int32_t ng, int32_t nr, const int32_t* __restrict__ part_off,
                         const int32_t* __restrict__ occ_off, const int32_t* __restrict__ pair_occ, int32_t* __restrict__ tsz,
                         int32_t* __restrict__ host_ctl) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int n_pairs = pair_off[ng];
  if (p == 0) { host_ctl[0] = part_off[nr]; host_ctl[1] = occ_off[nr]; host_ctl[3] = n_pairs; }
  if (p >= nr) return;
  int s = 0;
  if (p < n_pairs) { const int o = pair_occ[p]; s = 2; while (s < 2 * o) s <<= 1; }
  tsz[p] = s;
}

// koff: kept slots in front of every slot ([n_slots] = all of them; slots behind the last segment are never filled)
__global__ void k9_offsets(const int32_t* __restrict__ pair_off, const int32_t* __restrict__ tbl_off, const int32_t* __restrict__ koff, int32_t ng,
                           int32_t n_slots, int32_t* __restrict__ joff, int32_t* __restrict__ host_joff, int32_t* __restrict__ host_ctl) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) host_ctl[2] = koff[n_slots];
  if (g > ng) return;
  const int v = koff[tbl_off[pair_off[g]]];   // (tbl_off[all pairs] = the slots in use <= n_slots)
  joff[g] = v; host_joff[g] = v;
}

__global__ void k9_compact(const unsigned long long* __restrict__ tbl_key, const uint32_t* __restrict__ tbl_cnt, const int32_t* __restrict__ flag,
                           const int32_t* __restrict__ koff, const int32_t* __restrict__ tbl_off, const int32_t* __restrict__ pair_off, int32_t ng,
                           int32_t n_slots, unsigned long long* __restrict__ ck, uint32_t* __restrict__ cc, int32_t* __restrict__ cp) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots || !flag[t]) return;
  int lo = 0, hi = pair_off[ng];   // the pair whose segment holds slot t: the last p with tbl_off[p] <= t (no pair's segment is empty)
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tbl_off[mid] <= t) lo = mid; else hi = mid; }
  const int j = koff[t];
  ck[j] = tbl_key[t]; cc[j] = tbl_cnt[t]; cp[j] = lo;
}

// A kept junction's place is its rank among the pair's kept keys, found by counting the smaller ones (k6_rank's argument: tens to a few
// hundred kept junctions per gene).  The pair's kept junctions are [koff[tbl_off[p]], koff[tbl_off[p + 1]]).
__global__ void k9_rank(BatchView b, const unsigned long long* __restrict__ ck, const uint32_t* __restrict__ cc, const int32_t* __restrict__ cp,
                        const int32_t* __restrict__ koff, const int32_t* __restrict__ tbl_off, const int32_t* __restrict__ pair_region,
                        const int32_t* __restrict__ pair_gene, int32_t n_kept, lcr_junction_gene* __restrict__ out, int32_t* __restrict__ out_pair) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_kept) return;
  const int p = cp[j], lo = koff[tbl_off[p]], hi = koff[tbl_off[p + 1]];
  const int g = pair_region[p];
  const unsigned long long key = ck[j];
  int rank = 0;
  for (int k = lo; k < hi; k++) rank += ck[k] < key ? 1 : 0;
  const int32_t s = (int32_t)(key >> 32), l = (int32_t)(key & 0xffffffffu);
  lcr_junction_gene o{};
  o.region = g; o.motif = splice_motif(b, g, s, l); o.start0 = s; o.len = l; o.n_reads = cc[j]; o.gene = pair_gene[p];
  out[lo + rank] = o;
  out_pair[lo + rank] = p;
}

// One workgroup per kept junction: k6_tables over the pair's rows, its sweeps restricted to the counted ones.  The pair's rows are sorted
// by pos: those from the first with pos >= s + l on cannot overlap and are cut off by a binary search.
__global__ void __launch_bounds__(LCR_BLOCK) k9_tables(const int32_t* __restrict__ out_pair, const int32_t* __restrict__ pair_row0,
                                                        const int32_t* __restrict__ pair_rows, const K9Row* __restrict__ rows,
                                                        const unsigned long long* __restrict__ keys, int32_t n_kept,
                                                        lcr_junction_gene* __restrict__ junc, lcr_junction_gene* __restrict__ host_junc) {
  __shared__ int sh_end;
  const int j = blockIdx.x, tid = threadIdx.x;
  if (j >= n_kept) return;
  const lcr_junction_gene rec = junc[j];
  const int p = out_pair[j];
  const int32_t s = (int32_t)rec.start0, l = rec.len;
  const long long jend = (long long)s + l;
  const unsigned long long key = ((unsigned long long)(uint32_t)s << 32) | (uint32_t)l;
  const int p0 = pair_row0[p], p1 = p0 + pair_rows[p];
  if (tid == 0) {
    int lo = p0, hi = p1;   // first row in [p0, p1) with pos >= s + l
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if ((long long)rows[mid].pos >= jend) hi = mid; else lo = mid + 1; }
    sh_end = lo;
  }
  __syncthreads();
  const K6Cells best = sweep_phase_set_cells(
      rows, p0, sh_end,
      // counted (a shared base with the gene's exons) and overlap: pos < s + l && rend > s
      [&](const K9Row& row) { return (row.hap & 4) && (long long)row.pos < jend && row.rend > s; },
      [&](const K9Row& row) {
        int present = 0;
        for (int k = 0; k < row.n; k++) present |= keys[row.first + k] == key ? 1 : 0;
        return ((row.hap & 3) - 1) * 2 + present;
      });
  if (tid == 0) {
    lcr_junction_gene o = rec;
    o.phase_set = best.ps; o.n_phase_sets = best.n_sets;
    o.h1_absent = best.n[0]; o.h1_present = best.n[1]; o.h2_absent = best.n[2]; o.h2_present = best.n[3];
    junc[j] = o; host_junc[j] = o;
  }
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_k9_count(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, const int32_t* gene, uint32_t min_junctions,
                     int32_t* part_flag, int32_t* nocc, hipStream_t s) {
  if (b.n_reads <= 0) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k9_walk<false>, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, row_region_off, rec, gene, min_junctions,
                     part_flag, nocc, (const int32_t*)nullptr, (const int32_t*)nullptr, (const int32_t*)nullptr, (const int32_t*)nullptr, K9Exons{},
                     (K9Row*)nullptr, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (uint32_t*)nullptr);
}
void launch_k9_pair_count(const BatchView& b, const int32_t* gene, const int32_t* part_flag, int32_t* n_pairs, hipStream_t s) {
  if (b.n_regions > 0)
    hipLaunchKernelGGL(k9_pairs<false>, dim3(b.n_regions), dim3(LCR_BLOCK), 0, s, b.read_begin, gene, part_flag, (const int32_t*)nullptr, b.n_regions, n_pairs,
                       (const int32_t*)nullptr, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                       (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
}
void launch_k9_pair_emit(const BatchView& b, const int32_t* gene, const int32_t* part_flag, const int32_t* nocc, const int32_t* pair_off,
                         const int32_t* part_off, const K9Pairs& pr, hipStream_t s) {
  if (b.n_regions > 0)
    hipLaunchKernelGGL(k9_pairs<true>, dim3(b.n_regions), dim3(LCR_BLOCK), 0, s, b.read_begin, gene, part_flag, nocc, b.n_regions, (int32_t*)nullptr, pair_off,
                       part_off, pr.read_pair, pr.row_slot, pr.region, pr.gene, pr.row0, pr.rows, pr.occ);
}
void launch_k9_sizes(const BatchView& b, const int32_t* pair_off, const int32_t* part_off, const int32_t* occ_off, const int32_t* pair_occ, int32_t* tsz,
                     int32_t* host_ctl, hipStream_t s) {
  hipLaunchKernelGGL(k9_sizes, dim3((std::max(b.n_reads, 1) + 255) / 256), dim3(256), 0, s, pair_off, b.n_regions, b.n_reads, part_off, occ_off, pair_occ, tsz,
                     host_ctl);
}
size_t launch_k9_row_bytes() { return sizeof(K9Row); }
void launch_k9_emit(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, const int32_t* gene, const int32_t* part_flag,
                    const int32_t* occ_off, const K9Pairs& pr, const int32_t* tbl_off, const lcr_gene_annotation& a, void* rows, uint64_t* keys,
                    uint64_t* tbl_key, uint32_t* tbl_cnt, hipStream_t s) {
  if (b.n_reads <= 0) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k9_walk<true>, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, row_region_off, rec, gene, 0u,
                     const_cast<int32_t*>(part_flag), (int32_t*)nullptr, occ_off, (const int32_t*)pr.read_pair, (const int32_t*)pr.row_slot, tbl_off,
                     K9Exons{a.exon_off, a.exon_start0, a.exon_end0}, (K9Row*)rows, (unsigned long long*)keys, (unsigned long long*)tbl_key, tbl_cnt);
}
void launch_k9_offsets(const int32_t* pair_off, const int32_t* tbl_off, const int32_t* koff, int32_t ng, int32_t n_slots, int32_t* joff, int32_t* host_joff,
                       int32_t* host_ctl, hipStream_t s) {
  hipLaunchKernelGGL(k9_offsets, dim3((ng + 1 + 255) / 256), dim3(256), 0, s, pair_off, tbl_off, koff, ng, n_slots, joff, host_joff, host_ctl);
}
void launch_k9_place(const BatchView& b, const uint64_t* tbl_key, const uint32_t* tbl_cnt, const int32_t* flag, const int32_t* koff,
                     const int32_t* tbl_off, const int32_t* pair_off, const K9Pairs& pr, int32_t n_slots, int32_t n_kept, uint64_t* ck, uint32_t* cc,
                     int32_t* cp, lcr_junction_gene* junc, int32_t* junc_pair, hipStream_t s) {
  if (n_slots <= 0 || n_kept <= 0) return;
  hipLaunchKernelGGL(k9_compact, dim3((n_slots + 255) / 256), dim3(256), 0, s, (const unsigned long long*)tbl_key, tbl_cnt, flag, koff, tbl_off, pair_off,
                     b.n_regions, n_slots, (unsigned long long*)ck, cc, cp);
  hipLaunchKernelGGL(k9_rank, dim3((n_kept + 255) / 256), dim3(256), 0, s, b, (const unsigned long long*)ck, cc, cp, koff, tbl_off, (const int32_t*)pr.region,
                     (const int32_t*)pr.gene, n_kept, junc, junc_pair);
}
void launch_k9_tables(const int32_t* junc_pair, const K9Pairs& pr, const void* rows, const uint64_t* keys, int32_t n_kept, lcr_junction_gene* junc,
                      lcr_junction_gene* host_junc, hipStream_t s) {
  if (n_kept <= 0) return;
  hipLaunchKernelGGL(k9_tables, dim3(n_kept), dim3(LCR_BLOCK), 0, s, junc_pair, (const int32_t*)pr.row0, (const int32_t*)pr.rows, (const K9Row*)rows,
                     (const unsigned long long*)keys, n_kept, junc, host_junc);
}

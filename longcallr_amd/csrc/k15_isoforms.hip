// k15_isoforms.hip — K15: haplotype x intron-chain counts over the phased rows (lcr_isoforms; DESIGN.md "Allele-specific isoforms").
//
// The contract (include/lcr.h) per region g, over the PARTICIPATING rows -- fragment rows with assignment 1 / 2 whose read has at least
// min_junctions N ops of length >= 1 (counted by K6's launch_k6_count with min_junctions - 1: "more than" that is "at least" this):
//   k15_sizes     per region the slots of its segment of the chain table: 2 x its participating rows, a power of two   (one scan follows)
//   k15_walk      the junction walk again (k6_walk.h): the row's record, its keys s << 32 | l, and the 64-bit hash of its chain
//   k15_insert    a launch of its own behind the walk: a slot holds a representative row, claimed by atomicCAS; a row that meets an
//                 occupied slot compares its whole chain with the representative's -- rows and keys are the PREVIOUS launch's stores; inside
//                 this launch a workgroup learns from another only what an atomic returns -- and joins on equality, probes on otherwise
//   k15_flag      slot kept = occupied && n_h1 + n_h2 >= min_count, and the kept chain's length                        (two scans follow)
//   k15_offsets   kept chains and pool entries in front of every region, to HBM and to pinned host memory
//   k15_compact   the kept slots, region after region (in slot order)
//   k15_rank      every kept chain to its rank among the region's kept chains (lexicographic over the keys, a proper prefix first), its
//                 record without the table, its keys into the pool in record order
//   k15_rows      row -> slot -> record: row_isoform of the rows that hold a kept chain (the others keep the fill's -1)
//   k15_export    row_isoform, all of it, to pinned host memory: one coalesced copy instead of scattered stores across the link
//   k15_tables    one workgroup per kept chain: spanning, presence, the phase set with the most rows, the four cells
// Coordinates are the contig's; all arithmetic is integer, and nothing in the output depends on the order in which atomics land: which row
// represents a chain and where its slot lies do, the sorted records, the counts and row_isoform do not.
#include <algorithm>

#include "k6_walk.h"
#include "lcr_dev.h"

namespace {

struct K15Row {           // a participating row, in read order (= by pos inside a region)
  int32_t pos, rend;      // [pos, rend) on the contig
  uint32_t ps;            // phase set, 0 = none
  int32_t first, n;       // its junction keys are keys[first .. first + n), ascending
  int32_t hap;            // 1 / 2
  int32_t region, frow;   // its region; its row of the fragment matrix
};
static_assert(sizeof(K15Row) == 32, "K15Row is eight words");

// splitmix64's finaliser over the key and its index in the chain: the chain's hash is the sum of these, so the lanes of a row and the
// rounds of 16 ops add their shares in any order
__device__ __forceinline__ unsigned long long k15_mix(unsigned long long key, int idx) {
  unsigned long long x = key + (unsigned long long)(idx + 1) * 0x9E3779B97F4A7C15ull;
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__global__ void k15_sizes(const int32_t* __restrict__ read_begin, int32_t ng, int32_t nr, const int32_t* __restrict__ part_off,
                          const int32_t* __restrict__ pair_off, int32_t* __restrict__ tsz, int32_t* __restrict__ host_ctl) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) { host_ctl[0] = part_off[nr]; host_ctl[1] = pair_off[nr]; }
  if (g >= ng) return;
  const int p = part_off[read_begin[g + 1]] - part_off[read_begin[g]];
  int s = 0;
  if (p > 0) { s = 2; while (s < 2 * p) s <<= 1; }
  tsz[g] = s;
}

__global__ void __launch_bounds__(LCR_BLOCK) k15_walk(BatchView b, const int32_t* __restrict__ row_region_off, const lcr_read_record* __restrict__ rec,
                                                       const int32_t* __restrict__ part_flag, const int32_t* __restrict__ part_off,
                                                       const int32_t* __restrict__ pair_off, K15Row* __restrict__ rows,
                                                       unsigned long long* __restrict__ keys, unsigned long long* __restrict__ hash) {
  const int l16 = threadIdx.x & 15;
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) >> 4;
  if (rl >= b.n_reads) return;   // (a whole row leaves)
  const int r = (int)rl;
  if (!part_flag[r]) return;
  const int g = region_of_read(b, r);
  const int frow = row_region_off[g] + (r - b.read_begin[g]);
  const int first = pair_off[r];
  unsigned long long hs = 0;
  int n_n, rend;
  row16_walk_junctions(b, r, [&](int s, int len, int k) {
    const unsigned long long key = ((unsigned long long)(uint32_t)s << 32) | (uint32_t)len;
    keys[first + k] = key;
    hs += k15_mix(key, k);
  }, &n_n, &rend);
  for (int d = 8; d >= 1; d >>= 1) hs += __shfl_xor(hs, d, 64);   // (the partners are lanes of the same row)
  if (l16 != 0) return;
  const lcr_read_record rr = rec[frow];
  const int pi = part_off[r];
  rows[pi] = K15Row{b.pos[r], rend, rr.phase_set, first, n_n, (int32_t)rr.assignment, g, frow};
  hash[pi] = hs;
}

// One thread per participating row.  The segment has at least twice the region's rows in slots: an empty one is met before the probe
// comes round.  hash_mask keeps the bits of the hash that route (lcr_debug_set "iso_hash_bits"): identity is the comparison's alone.
__global__ void k15_insert(int32_t n_part, const K15Row* __restrict__ rows, const unsigned long long* __restrict__ keys,
                           const unsigned long long* __restrict__ hash, unsigned long long hash_mask, const int32_t* __restrict__ tbl_off,
                           int32_t* __restrict__ tbl_rep, uint32_t* __restrict__ tbl_cnt, int32_t* __restrict__ row_slot) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_part) return;
  const K15Row row = rows[p];
  const int t0 = tbl_off[row.region];
  const uint32_t mask = (uint32_t)(tbl_off[row.region + 1] - t0) - 1u;
  const unsigned long long hm = hash[p] & hash_mask;
  uint32_t h = (uint32_t)(hm ^ (hm >> 32)) & mask;
  for (uint32_t i = 0; i <= mask; i++, h = (h + 1) & mask) {
    const int prev = atomicCAS(&tbl_rep[t0 + h], -1, p);
    bool same = prev == -1 || prev == p;
    if (!same) {
      const K15Row o = rows[prev];
      same = o.n == row.n;
      for (int k = 0; same && k < row.n; k++) same = keys[o.first + k] == keys[row.first + k];
    }
    if (same) {
      atomicAdd(&tbl_cnt[2 * (size_t)(t0 + h) + (row.hap - 1)], 1u);
      row_slot[p] = t0 + h;
      break;
    }
  }
}

__global__ void k15_flag(const int32_t* __restrict__ tbl_rep, const uint32_t* __restrict__ tbl_cnt, const K15Row* __restrict__ rows, int32_t n_slots,
                         uint32_t min_count, int32_t* __restrict__ flag, int32_t* __restrict__ plen) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots) return;
  const int rep = tbl_rep[t];
  const bool kept = rep >= 0 && tbl_cnt[2 * (size_t)t] + tbl_cnt[2 * (size_t)t + 1] >= min_count;
  flag[t] = kept ? 1 : 0;
  plen[t] = kept ? rows[rep].n : 0;
}

// koff / poff: kept slots and their keys in front of every slot ([n_slots] = all of them; slots behind the last segment are never filled)
__global__ void k15_offsets(const int32_t* __restrict__ tbl_off, const int32_t* __restrict__ koff, const int32_t* __restrict__ poff, int32_t ng,
                            int32_t n_slots, int32_t* __restrict__ off, int32_t* __restrict__ host_off, int32_t* __restrict__ pbase,
                            int32_t* __restrict__ host_ctl) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) { host_ctl[2] = koff[n_slots]; host_ctl[3] = poff[n_slots]; }
  if (g > ng) return;
  const int t = tbl_off[g];
  off[g] = koff[t]; host_off[g] = koff[t]; pbase[g] = poff[t];
}

__global__ void k15_compact(const int32_t* __restrict__ flag, const int32_t* __restrict__ koff, int32_t n_slots, int32_t* __restrict__ cslot) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_slots && flag[t]) cslot[koff[t]] = t;
}

// chain A in front of chain B: the first differing key decides (s in the high word: s before l), a proper prefix comes first
__device__ __forceinline__ bool k15_less(const unsigned long long* __restrict__ a, int na, const unsigned long long* __restrict__ b, int nb) {
  const int n = na < nb ? na : nb;
  for (int q = 0; q < n; q++) {
    const unsigned long long x = a[q], y = b[q];
    if (x != y) return x < y;
  }
  return na < nb;
}

// A kept chain's place is its rank among the region's kept chains, found by counting the smaller ones (as k6_rank): kept chains per region
// are the isoforms of a gene with min_count reads each -- tens to a few hundred.  A region with more is still ordered correctly, only more
// slowly.  The keys of the smaller ones lie in front of its own in the pool.
__global__ void k15_rank(const K15Row* __restrict__ rows, const unsigned long long* __restrict__ keys, const int32_t* __restrict__ tbl_rep,
                         const uint32_t* __restrict__ tbl_cnt, const int32_t* __restrict__ cslot, const int32_t* __restrict__ off,
                         const int32_t* __restrict__ pbase, int32_t n_kept, lcr_isoform* __restrict__ iso, int32_t* __restrict__ crank,
                         unsigned long long* __restrict__ chain, unsigned long long* __restrict__ host_chain) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_kept) return;
  const int t = cslot[j];
  const K15Row row = rows[tbl_rep[t]];
  const int g = row.region, lo = off[g], hi = off[g + 1];
  const unsigned long long* __restrict__ mine = keys + row.first;
  int rank = 0, psum = 0;
  for (int k = lo; k < hi; k++) {
    if (k == j) continue;
    const K15Row o = rows[tbl_rep[cslot[k]]];
    if (k15_less(keys + o.first, o.n, mine, row.n)) { rank++; psum += o.n; }
  }
  const int cf = pbase[g] + psum;
  const unsigned long long last = mine[row.n - 1];
  lcr_isoform o{};
  o.region = g; o.n_junc = row.n;
  o.start0 = (int64_t)(mine[0] >> 32);
  o.end0 = (int64_t)(last >> 32) + (int64_t)(last & 0xffffffffull);
  o.chain_first = cf;
  o.n_h1 = tbl_cnt[2 * (size_t)t]; o.n_h2 = tbl_cnt[2 * (size_t)t + 1]; o.n_reads = o.n_h1 + o.n_h2;
  iso[lo + rank] = o;
  crank[j] = lo + rank;
  for (int q = 0; q < row.n; q++) { const unsigned long long v = mine[q]; chain[cf + q] = v; host_chain[cf + q] = v; }
}

__global__ void k15_rows(int32_t n_part, const K15Row* __restrict__ rows, const int32_t* __restrict__ row_slot, const int32_t* __restrict__ flag,
                         const int32_t* __restrict__ koff, const int32_t* __restrict__ crank, int32_t* __restrict__ row_iso) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_part) return;
  const int t = row_slot[p];
  if (flag[t]) row_iso[rows[p].frow] = crank[koff[t]];
}

__global__ void k15_export(int32_t n_rows, const int32_t* __restrict__ row_iso, int32_t* __restrict__ host_row_iso) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n_rows) host_row_iso[r] = row_iso[r];
}

// the row against a kept chain whose extent [a, e) it spans: its junctions that meet the extent (s < e && s + l > a: a run, since s and
// s + l both rise along a read) equal the chain, in order
__device__ __forceinline__ int k15_present(const unsigned long long* __restrict__ rk, int rn, const unsigned long long* __restrict__ ch, int k,
                                           long long a, long long e) {
  int lo = 0, hi = rn;   // first junction with s + l > a
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const unsigned long long v = rk[mid];
    if ((long long)(v >> 32) + (long long)(v & 0xffffffffull) > a) hi = mid; else lo = mid + 1;
  }
  if (lo + k > rn) return 0;
  for (int q = 0; q < k; q++) if (rk[lo + q] != ch[q]) return 0;
  if (lo + k < rn && (long long)(rk[lo + k] >> 32) < e) return 0;   // one more junction inside the extent
  return 1;
}

// One workgroup per kept chain.  The region's participating rows are sorted by pos: those from the first with pos > a on cannot span and
// are cut off by a binary search.  The spanning rows go through the four-cell sweep of k6_walk.h, as k6_tables' overlapping rows do.
__global__ void __launch_bounds__(LCR_BLOCK) k15_tables(BatchView b, const int32_t* __restrict__ part_off, const K15Row* __restrict__ rows,
                                                         const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ chain,
                                                         int32_t n_kept, lcr_isoform* __restrict__ iso, lcr_isoform* __restrict__ host_iso) {
  __shared__ int sh_end;
  const int j = blockIdx.x, tid = threadIdx.x;
  if (j >= n_kept) return;
  const lcr_isoform rec = iso[j];
  const int g = rec.region, k = rec.n_junc;
  const long long a = rec.start0, e = rec.end0;
  const unsigned long long* __restrict__ ch = chain + rec.chain_first;
  const int p0 = part_off[b.read_begin[g]], p1 = part_off[b.read_begin[g + 1]];
  if (tid == 0) {
    int lo = p0, hi = p1;   // first row in [p0, p1) with pos > a
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if ((long long)rows[mid].pos > a) hi = mid; else lo = mid + 1; }
    sh_end = lo;
  }
  __syncthreads();
  const K6Cells best = sweep_phase_set_cells(
      rows, p0, sh_end, [&](const K15Row& row) { return (long long)row.rend >= e; },   // spanning: pos <= a && rend >= e
      [&](const K15Row& row) { return (row.hap - 1) * 2 + k15_present(keys + row.first, row.n, ch, k, a, e); });
  if (tid == 0) {
    lcr_isoform o = rec;
    o.phase_set = best.ps; o.n_phase_sets = best.n_sets;
    o.h1_absent = best.n[0]; o.h1_present = best.n[1]; o.h2_absent = best.n[2]; o.h2_present = best.n[3];
    iso[j] = o; host_iso[j] = o;
  }
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_k15_sizes(const BatchView& b, const int32_t* part_off, const int32_t* pair_off, int32_t* tsz, int32_t* host_ctl, hipStream_t s) {
  hipLaunchKernelGGL(k15_sizes, dim3((std::max(b.n_regions, 1) + 255) / 256), dim3(256), 0, s, b.read_begin, b.n_regions, b.n_reads, part_off, pair_off, tsz, host_ctl);
}
size_t launch_k15_row_bytes() { return sizeof(K15Row); }
void launch_k15_walk(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, const int32_t* part_flag, const int32_t* part_off,
                     const int32_t* pair_off, void* rows, uint64_t* keys, uint64_t* hash, hipStream_t s) {
  if (b.n_reads <= 0) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k15_walk, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, row_region_off, rec, part_flag, part_off,
                     pair_off, (K15Row*)rows, (unsigned long long*)keys, (unsigned long long*)hash);
}
void launch_k15_insert(int32_t n_part, const void* rows, const uint64_t* keys, const uint64_t* hash, uint64_t hash_mask, const int32_t* tbl_off,
                       int32_t* tbl_rep, uint32_t* tbl_cnt, int32_t* row_slot, hipStream_t s) {
  if (n_part <= 0) return;
  hipLaunchKernelGGL(k15_insert, dim3((n_part + 255) / 256), dim3(256), 0, s, n_part, (const K15Row*)rows, (const unsigned long long*)keys,
                     (const unsigned long long*)hash, (unsigned long long)hash_mask, tbl_off, tbl_rep, tbl_cnt, row_slot);
}
void launch_k15_flag(const int32_t* tbl_rep, const uint32_t* tbl_cnt, const void* rows, int32_t n_slots, uint32_t min_count, int32_t* flag, int32_t* plen,
                     hipStream_t s) {
  if (n_slots > 0) hipLaunchKernelGGL(k15_flag, dim3((n_slots + 255) / 256), dim3(256), 0, s, tbl_rep, tbl_cnt, (const K15Row*)rows, n_slots, min_count, flag, plen);
}
void launch_k15_offsets(const int32_t* tbl_off, const int32_t* koff, const int32_t* poff, int32_t ng, int32_t n_slots, int32_t* off, int32_t* host_off,
                        int32_t* pbase, int32_t* host_ctl, hipStream_t s) {
  hipLaunchKernelGGL(k15_offsets, dim3((ng + 1 + 255) / 256), dim3(256), 0, s, tbl_off, koff, poff, ng, n_slots, off, host_off, pbase, host_ctl);
}
void launch_k15_place(const void* rows, const uint64_t* keys, const int32_t* tbl_rep, const uint32_t* tbl_cnt, const int32_t* flag, const int32_t* koff,
                      int32_t n_slots, const int32_t* off, const int32_t* pbase, int32_t n_kept, int32_t* cslot, int32_t* crank, lcr_isoform* iso,
                      uint64_t* chain, uint64_t* host_chain, hipStream_t s) {
  if (n_slots <= 0 || n_kept <= 0) return;
  hipLaunchKernelGGL(k15_compact, dim3((n_slots + 255) / 256), dim3(256), 0, s, flag, koff, n_slots, cslot);
  hipLaunchKernelGGL(k15_rank, dim3((n_kept + 255) / 256), dim3(256), 0, s, (const K15Row*)rows, (const unsigned long long*)keys, tbl_rep, tbl_cnt, cslot, off,
                     pbase, n_kept, iso, crank, (unsigned long long*)chain, (unsigned long long*)host_chain);
}
void launch_k15_rows(int32_t n_part, const void* rows, const int32_t* row_slot, const int32_t* flag, const int32_t* koff, const int32_t* crank,
                     int32_t* row_iso, hipStream_t s) {
  if (n_part <= 0) return;
  hipLaunchKernelGGL(k15_rows, dim3((n_part + 255) / 256), dim3(256), 0, s, n_part, (const K15Row*)rows, row_slot, flag, koff, crank, row_iso);
}
void launch_k15_export(int32_t n_rows, const int32_t* row_iso, int32_t* host_row_iso, hipStream_t s) {
  if (n_rows > 0) hipLaunchKernelGGL(k15_export, dim3((n_rows + 255) / 256), dim3(256), 0, s, n_rows, row_iso, host_row_iso);
}
void launch_k15_tables(const BatchView& b, const int32_t* part_off, const void* rows, const uint64_t* keys, const uint64_t* chain, int32_t n_kept,
                       lcr_isoform* iso, lcr_isoform* host_iso, hipStream_t s) {
  if (n_kept <= 0) return;
  hipLaunchKernelGGL(k15_tables, dim3(n_kept), dim3(LCR_BLOCK), 0, s, b, part_off, (const K15Row*)rows, (const unsigned long long*)keys,
                     (const unsigned long long*)chain, n_kept, iso, host_iso);
}

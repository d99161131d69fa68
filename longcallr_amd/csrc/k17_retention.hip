// k17_retention.hip — K17: haplotype x intron retention over the phased rows (lcr_intron_retention; DESIGN.md "Allele-specific intron retention").
//
// The contract (include/lcr.h) per region g, over the PARTICIPATING rows -- fragment rows with assignment 1 / 2, spliced or not:
//   k17_walk<false>  sixteen lanes per read count the read's junctions                     -> part_flag, npair  (two scans follow)
//   k17_sizes        per region the slots of its segment of the junction hash table        -> tsz               (one scan follows)
//   k17_walk<true>   the same walk again: the row's record {pos, rend, ps, first key, keys, hap, fragment row}, per junction the key
//                    s << 32 | l, and the key's insertion into the region's table segment (64-bit atomicCAS, atomicAdd of its count)
//   k17_flag         slot kept = occupied && count >= min_count                             -> flag              (one scan follows)
//   k17_offsets      introns in front of every region, to HBM and to pinned host memory
//   k17_compact      the kept slots, region after region (in slot order)
//   k17_rank         every kept intron to its rank among the region's kept keys (= order by s, then l) + the motif
//   k17_tables       one workgroup per kept intron: spliced / retained / other, row_retained, the phase set with the most rows, the four cells
//   k17_export       row_retained, all of it, and n_retained_total to pinned host memory
// Unlike K6 a participating row may hold no junction, and a region may have participating rows and an empty table segment: the walk asks
// for the segment's size before it probes.  k17_sizes / _flag / _offsets / _compact / _rank are K6's forms, kept as copies here (they
// differ in the record, the control words and the hash's routing mask; k6_junctions.hip is untouched).  Coordinates are the contig's; all
// arithmetic is integer adds, and nothing in the output depends on the order in which atomics land.
#include <algorithm>

#include "k6_walk.h"
#include "lcr_dev.h"

namespace {

constexpr unsigned long long K17_EMPTY = ~0ull;   // no key: l < 2^28 keeps every key below it

struct K17Row {           // a participating row, in read order (= by pos inside a region)
  int32_t pos, rend;      // [pos, rend) on the contig
  uint32_t ps;            // phase set, 0 = none
  int32_t first, n;       // its junction keys are keys[first .. first + n), ascending; n may be 0
  int32_t hap;            // 1 / 2
  int32_t frow;           // its row of the fragment matrix
};
static_assert(sizeof(K17Row) == 28, "K17Row is seven words");

__device__ __forceinline__ uint32_t k17_hash(unsigned long long key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32); }

// Sixteen lanes per read walk its junctions (k6_walk.h: row16_walk_junctions).
template <bool EMIT>
__global__ void __launch_bounds__(LCR_BLOCK) k17_walk(BatchView b, const int32_t* __restrict__ row_region_off, const lcr_read_record* __restrict__ rec,
                                                       uint32_t hmask, int32_t* __restrict__ part_flag, int32_t* __restrict__ npair,
                                                       const int32_t* __restrict__ part_off, const int32_t* __restrict__ pair_off,
                                                       const int32_t* __restrict__ tbl_off, K17Row* __restrict__ rows,
                                                       unsigned long long* __restrict__ keys, unsigned long long* __restrict__ tbl_key,
                                                       uint32_t* __restrict__ tbl_cnt) {
  const int l16 = threadIdx.x & 15;
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) >> 4;
  if (rl >= b.n_reads) return;   // (a whole row leaves)
  const int r = (int)rl;
  const int g = region_of_read(b, r);
  int hap = 0, frow = 0; uint32_t ps = 0;
  if (!EMIT) {
    // row k of region g is the region's k-th read (fragment.rs:293-307: the reads up to the last candidate); a read behind them is no row
    const int k = r - b.read_begin[g], row0 = row_region_off[g];
    bool part = k < row_region_off[g + 1] - row0;
    if (part) { const int a = rec[row0 + k].assignment; part = a == 1 || a == 2; }
    if (!part) { if (l16 == 0) { part_flag[r] = 0; npair[r] = 0; } return; }
  } else {
    if (!part_flag[r]) return;
    frow = row_region_off[g] + (r - b.read_begin[g]);
    const lcr_read_record rr = rec[frow];
    hap = rr.assignment; ps = rr.phase_set;
  }
  const int pos = b.pos[r];
  const int first = EMIT ? pair_off[r] : 0;
  const int t0 = EMIT ? tbl_off[g] : 0;
  const int tsz = EMIT ? tbl_off[g + 1] - t0 : 0;   // 0: no participating row of the region holds a junction, and the sink is never reached
  const uint32_t mask = (uint32_t)tsz - 1u;
  int ref_cur, n_n;
  row16_walk_junctions(b, r, [&](int s, int len, int k) {
    if (!EMIT || tsz <= 0) return;
    const unsigned long long key = ((unsigned long long)(uint32_t)s << 32) | (uint32_t)len;
    keys[first + k] = key;
    // the segment has at least twice the region's pairs in slots: an empty one is met before the probe comes round
    uint32_t h = k17_hash(key) & hmask & mask;
    for (uint32_t i = 0; i <= mask; i++, h = (h + 1) & mask) {
      const unsigned long long prev = atomicCAS(&tbl_key[t0 + h], K17_EMPTY, key);
      if (prev == K17_EMPTY || prev == key) { atomicAdd(&tbl_cnt[t0 + h], 1u); break; }   // (a read holds a key once: s rises along it)
    }
  }, &n_n, &ref_cur);
  if (l16 != 0) return;
  if (!EMIT) { part_flag[r] = 1; npair[r] = n_n; }
  else rows[part_off[r]] = K17Row{pos, ref_cur, ps, first, n_n, hap, frow};
}

// per region: slots of its table segment = 2 x pairs rounded up to a power of two (0 without pairs); the totals for the host
__global__ void k17_sizes(const int32_t* __restrict__ read_begin, int32_t ng, int32_t nr, const int32_t* __restrict__ part_off,
                          const int32_t* __restrict__ pair_off, int32_t* __restrict__ tsz, int32_t* __restrict__ host_ctl) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) { host_ctl[0] = part_off[nr]; host_ctl[1] = pair_off[nr]; }
  if (g >= ng) return;
  const int p = pair_off[read_begin[g + 1]] - pair_off[read_begin[g]];
  int s = 0;
  if (p > 0) { s = 2; while (s < 2 * p) s <<= 1; }
  tsz[g] = s;
}

__global__ void k17_flag(const unsigned long long* __restrict__ tbl_key, const uint32_t* __restrict__ tbl_cnt, int32_t n_slots,
                         uint32_t min_count, int32_t* __restrict__ flag) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_slots) flag[t] = (tbl_key[t] != K17_EMPTY && tbl_cnt[t] >= min_count) ? 1 : 0;
}

// koff: kept slots in front of every slot ([n_slots] = all of them; slots behind the last segment are never filled)
__global__ void k17_offsets(const int32_t* __restrict__ tbl_off, const int32_t* __restrict__ koff, int32_t ng, int32_t n_slots,
                            int32_t* __restrict__ off, int32_t* __restrict__ host_off, int32_t* __restrict__ host_ctl) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) host_ctl[2] = koff[n_slots];
  if (g > ng) return;
  const int v = koff[tbl_off[g]];   // (tbl_off[g] <= n_slots, and koff has n_slots + 1 words)
  off[g] = v; host_off[g] = v;
}

__global__ void k17_compact(const unsigned long long* __restrict__ tbl_key, const uint32_t* __restrict__ tbl_cnt, const int32_t* __restrict__ flag,
                            const int32_t* __restrict__ koff, const int32_t* __restrict__ tbl_off, int32_t ng, int32_t n_slots,
                            unsigned long long* __restrict__ ck, uint32_t* __restrict__ cc, int32_t* __restrict__ cgr) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots || !flag[t]) return;
  int lo = 0, hi = ng;   // the region whose segment holds slot t: the last g with tbl_off[g] <= t (empty segments share an offset)
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tbl_off[mid] <= t) lo = mid; else hi = mid; }
  const int j = koff[t];
  ck[j] = tbl_key[t]; cc[j] = tbl_cnt[t]; cgr[j] = lo;
}

// A kept intron's place is its rank among the region's kept keys, found by counting the smaller ones (as k6_rank: kept introns per region
// are tens to a few hundred).  n_spliced starts as the table's count; k17_tables counts it again.
__global__ void k17_rank(BatchView b, const unsigned long long* __restrict__ ck, const uint32_t* __restrict__ cc, const int32_t* __restrict__ cgr,
                         const int32_t* __restrict__ off, int32_t n_kept, lcr_retained_intron* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_kept) return;
  const int g = cgr[j], lo = off[g], hi = off[g + 1];
  const unsigned long long key = ck[j];
  int rank = 0;
  for (int k = lo; k < hi; k++) rank += ck[k] < key ? 1 : 0;
  const int32_t s = (int32_t)(key >> 32), l = (int32_t)(key & 0xffffffffu);
  lcr_retained_intron o{};
  o.region = g; o.motif = splice_motif(b, g, s, l); o.start0 = s; o.len = l; o.n_spliced = cc[j];
  out[lo + rank] = o;
}

// The class of a row that overlaps the intron [s, e) with the anchored span [lo_a, hi_a) = [s - a, e + a): 1 SPLICED (asked first),
// 2 RETAINED, 0 OTHER.  One scan of the row's own keys answers both questions.
__device__ __forceinline__ int k17_class(const K17Row& row, const unsigned long long* __restrict__ keys, unsigned long long key, long long lo_a,
                                         long long hi_a) {
  bool spliced = false, cut = false;
  for (int k = 0; k < row.n; k++) {
    const unsigned long long q = keys[row.first + k];
    const long long si = (long long)(int32_t)(q >> 32), ei = si + (long long)(uint32_t)q;
    spliced |= q == key;
    cut |= si < hi_a && ei > lo_a;
  }
  if (spliced) return 1;
  return (lo_a >= 0 && (long long)row.pos <= lo_a && (long long)row.rend >= hi_a && !cut) ? 2 : 0;
}

// One workgroup per kept intron.  The region's participating rows are sorted by pos: those from the first with pos >= e on cannot overlap
// and are cut off by a binary search.  One pass classes every overlapping row (a thread's counts in registers, a wave's sum, three LDS
// atomics per wave) and adds 1 to row_retained of a RETAINED row; then the four-cell sweep of k6_walk.h over the SPLICED and RETAINED rows.
__global__ void __launch_bounds__(LCR_BLOCK) k17_tables(BatchView b, const int32_t* __restrict__ part_off, const K17Row* __restrict__ rows,
                                                         const unsigned long long* __restrict__ keys, int32_t anchor, int32_t n_kept,
                                                         lcr_retained_intron* __restrict__ intron, lcr_retained_intron* __restrict__ host_intron,
                                                         int32_t* __restrict__ row_retained, unsigned long long* __restrict__ n_total) {
  __shared__ int sh_end;
  __shared__ uint32_t sh_n[3];
  const int j = blockIdx.x, tid = threadIdx.x;
  if (j >= n_kept) return;
  const lcr_retained_intron rec = intron[j];
  const int g = rec.region;
  const int32_t s = (int32_t)rec.start0, l = rec.len;
  const long long e = (long long)s + l, lo_a = (long long)s - anchor, hi_a = e + anchor;
  const unsigned long long key = ((unsigned long long)(uint32_t)s << 32) | (uint32_t)l;
  const int p0 = part_off[b.read_begin[g]], p1 = part_off[b.read_begin[g + 1]];
  if (tid == 0) {
    int lo = p0, hi = p1;   // first row in [p0, p1) with pos >= e
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if ((long long)rows[mid].pos >= e) hi = mid; else lo = mid + 1; }
    sh_end = lo;
    sh_n[0] = sh_n[1] = sh_n[2] = 0;
  }
  __syncthreads();
  const int p_end = sh_end;
  uint32_t n0 = 0, n1 = 0, n2 = 0;   // other, spliced, retained
  for (int p = p0 + tid; p < p_end; p += LCR_BLOCK) {
    const K17Row row = rows[p];
    if (!((long long)row.pos < e && row.rend > s)) continue;   // overlap: pos < e && rend > s
    const int cls = k17_class(row, keys, key, lo_a, hi_a);
    n0 += cls == 0; n1 += cls == 1; n2 += cls == 2;
    if (cls == 2) atomicAdd(&row_retained[row.frow], 1);
  }
  n0 = wave_sum_u32(n0); n1 = wave_sum_u32(n1); n2 = wave_sum_u32(n2);
  if ((tid & 63) == 0) {
    if (n0) atomicAdd(&sh_n[0], n0);
    if (n1) atomicAdd(&sh_n[1], n1);
    if (n2) atomicAdd(&sh_n[2], n2);
  }
  __syncthreads();
  const uint32_t n_other = sh_n[0], n_spliced = sh_n[1], n_retained = sh_n[2];
  const K6Cells best = sweep_phase_set_cells(
      rows, p0, p_end,
      [&](const K17Row& row) { return (long long)row.pos < e && row.rend > s && k17_class(row, keys, key, lo_a, hi_a) != 0; },
      [&](const K17Row& row) { return (row.hap - 1) * 2 + (k17_class(row, keys, key, lo_a, hi_a) == 2 ? 1 : 0); });
  if (tid == 0) {
    lcr_retained_intron o = rec;
    o.n_spliced = n_spliced; o.n_retained = n_retained; o.n_other = n_other;   // (n_spliced equals the table's count: both count the rows that hold the key)
    o.phase_set = best.ps; o.n_phase_sets = best.n_sets;
    o.h1_spliced = best.n[0]; o.h1_retained = best.n[1]; o.h2_spliced = best.n[2]; o.h2_retained = best.n[3];
    intron[j] = o; host_intron[j] = o;
    if (n_retained) atomicAdd(n_total, (unsigned long long)n_retained);
  }
}

__global__ void k17_export(int32_t n_rows, const int32_t* __restrict__ row_retained, int32_t* __restrict__ host_row_retained,
                           const unsigned long long* __restrict__ n_total, unsigned long long* __restrict__ host_n_total) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0) *host_n_total = *n_total;
  if (r < n_rows) host_row_retained[r] = row_retained[r];
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_k17_count(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, int32_t* part_flag, int32_t* npair, hipStream_t s) {
  if (b.n_reads <= 0) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k17_walk<false>, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, row_region_off, rec, 0u,
                     part_flag, npair, (const int32_t*)nullptr, (const int32_t*)nullptr, (const int32_t*)nullptr, (K17Row*)nullptr,
                     (unsigned long long*)nullptr, (unsigned long long*)nullptr, (uint32_t*)nullptr);
}
void launch_k17_sizes(const BatchView& b, const int32_t* part_off, const int32_t* pair_off, int32_t* tsz, int32_t* host_ctl, hipStream_t s) {
  hipLaunchKernelGGL(k17_sizes, dim3((std::max(b.n_regions, 1) + 255) / 256), dim3(256), 0, s, b.read_begin, b.n_regions, b.n_reads, part_off, pair_off, tsz, host_ctl);
}
size_t launch_k17_row_bytes() { return sizeof(K17Row); }
void launch_k17_emit(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, uint32_t hash_mask, const int32_t* part_flag,
                     const int32_t* part_off, const int32_t* pair_off, const int32_t* tbl_off, void* rows, uint64_t* keys, uint64_t* tbl_key,
                     uint32_t* tbl_cnt, hipStream_t s) {
  if (b.n_reads <= 0) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k17_walk<true>, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, row_region_off, rec, hash_mask,
                     const_cast<int32_t*>(part_flag), (int32_t*)nullptr, part_off, pair_off, tbl_off, (K17Row*)rows, (unsigned long long*)keys,
                     (unsigned long long*)tbl_key, tbl_cnt);
}
void launch_k17_flag(const uint64_t* tbl_key, const uint32_t* tbl_cnt, int32_t n_slots, uint32_t min_count, int32_t* flag, hipStream_t s) {
  if (n_slots > 0) hipLaunchKernelGGL(k17_flag, dim3((n_slots + 255) / 256), dim3(256), 0, s, (const unsigned long long*)tbl_key, tbl_cnt, n_slots, min_count, flag);
}
void launch_k17_offsets(const int32_t* tbl_off, const int32_t* koff, int32_t ng, int32_t n_slots, int32_t* off, int32_t* host_off, int32_t* host_ctl,
                        hipStream_t s) {
  hipLaunchKernelGGL(k17_offsets, dim3((ng + 1 + 255) / 256), dim3(256), 0, s, tbl_off, koff, ng, n_slots, off, host_off, host_ctl);
}
void launch_k17_place(const BatchView& b, const uint64_t* tbl_key, const uint32_t* tbl_cnt, const int32_t* flag, const int32_t* koff,
                      const int32_t* tbl_off, int32_t n_slots, const int32_t* off, int32_t n_kept, uint64_t* ck, uint32_t* cc, int32_t* cgr,
                      lcr_retained_intron* intron, hipStream_t s) {
  if (n_slots <= 0 || n_kept <= 0) return;
  hipLaunchKernelGGL(k17_compact, dim3((n_slots + 255) / 256), dim3(256), 0, s, (const unsigned long long*)tbl_key, tbl_cnt, flag, koff, tbl_off, b.n_regions,
                     n_slots, (unsigned long long*)ck, cc, cgr);
  hipLaunchKernelGGL(k17_rank, dim3((n_kept + 255) / 256), dim3(256), 0, s, b, (const unsigned long long*)ck, cc, cgr, off, n_kept, intron);
}
void launch_k17_tables(const BatchView& b, const int32_t* part_off, const void* rows, const uint64_t* keys, uint32_t anchor, int32_t n_kept,
                       lcr_retained_intron* intron, lcr_retained_intron* host_intron, int32_t* row_retained, uint64_t* n_total, hipStream_t s) {
  if (n_kept <= 0) return;
  hipLaunchKernelGGL(k17_tables, dim3(n_kept), dim3(LCR_BLOCK), 0, s, b, part_off, (const K17Row*)rows, (const unsigned long long*)keys, (int32_t)anchor,
                     n_kept, intron, host_intron, row_retained, (unsigned long long*)n_total);
}
void launch_k17_export(int32_t n_rows, const int32_t* row_retained, int32_t* host_row_retained, const uint64_t* n_total, uint64_t* host_n_total,
                       hipStream_t s) {
  hipLaunchKernelGGL(k17_export, dim3((std::max(n_rows, 1) + 255) / 256), dim3(256), 0, s, n_rows, row_retained, host_row_retained,
                     (const unsigned long long*)n_total, (unsigned long long*)host_n_total);
}

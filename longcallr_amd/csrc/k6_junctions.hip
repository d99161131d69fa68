// k6_junctions.hip — K6: haplotype x junction counts over the phased rows (lcr_junctions; DESIGN.md "Allele-specific junctions").
//
// The contract (include/lcr.h) per region g, over the PARTICIPATING rows -- fragment rows with assignment 1 / 2 whose read has more
// than min_junctions N ops of length >= 1:
//   k6_walk<false>   sixteen lanes per read count the read's junctions                     -> part_flag, npair  (two scans follow)
//   k6_sizes         per region the slots of its segment of the junction hash table        -> tsz               (one scan follows)
//   k6_walk<true>    the same walk again: the row's record {pos, rend, ps, hap, first pair, pairs}, per junction the key
//                    s << 32 | l, and the key's insertion into the region's table segment (64-bit atomicCAS, atomicAdd of n_reads)
//   k6_flag          slot kept = occupied && n_reads >= min_count                           -> flag              (one scan follows)
//   k6_offsets       junctions in front of every region, to HBM and to pinned host memory
//   k6_compact       the kept slots, region after region (in slot order)
//   k6_rank          every kept junction to its rank among the region's kept keys (= order by s, then l) + the motif
//   k6_tables        one workgroup per kept junction: overlap, presence, the phase set with the most rows, the four counters
// Coordinates are the contig's (pos, s and rend as the batch's int32 positions); all arithmetic is integer adds, and nothing
// depends on the order in which atomics land: a slot's position inside its segment does, the sorted output does not.
#include <algorithm>

#include "k6_walk.h"
#include "lcr_dev.h"

namespace {

constexpr unsigned long long K6_EMPTY = ~0ull;   // no key: l < 2^28 keeps every key below it

struct K6Row {            // a participating row, in read order (= by pos inside a region)
  int32_t pos, rend;      // [pos, rend) on the contig
  uint32_t ps;            // phase set, 0 = none
  int32_t first, n;       // its junction keys are keys[first .. first + n), ascending
  int32_t hap;            // 1 / 2
};
static_assert(sizeof(K6Row) == 24, "K6Row is six words");

__device__ __forceinline__ uint32_t k6_hash(unsigned long long key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32); }

// Sixteen lanes per read walk its junctions (k6_walk.h: row16_walk_junctions).
template <bool EMIT>
__global__ void __launch_bounds__(LCR_BLOCK) k6_walk(BatchView b, const int32_t* __restrict__ row_region_off, const lcr_read_record* __restrict__ rec,
                                                      uint32_t min_junctions, int32_t* __restrict__ part_flag, int32_t* __restrict__ npair,
                                                      const int32_t* __restrict__ part_off, const int32_t* __restrict__ pair_off,
                                                      const int32_t* __restrict__ tbl_off, K6Row* __restrict__ rows,
                                                      unsigned long long* __restrict__ keys, unsigned long long* __restrict__ tbl_key,
                                                      uint32_t* __restrict__ tbl_cnt) {
  const int l16 = threadIdx.x & 15;
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) >> 4;
  if (rl >= b.n_reads) return;   // (a whole row leaves)
  const int r = (int)rl;
  const int g = region_of_read(b, r);
  int hap = 0; uint32_t ps = 0;
  if (!EMIT) {
    // row k of region g is the region's k-th read (fragment.rs:293-307: the reads up to the last candidate); a read behind them is no row
    const int k = r - b.read_begin[g], row0 = row_region_off[g];
    bool cand = k < row_region_off[g + 1] - row0;
    if (cand) { const int a = rec[row0 + k].assignment; cand = a == 1 || a == 2; }
    if (!cand) { if (l16 == 0) { part_flag[r] = 0; npair[r] = 0; } return; }
  } else {
    if (!part_flag[r]) return;
    const lcr_read_record rr = rec[row_region_off[g] + (r - b.read_begin[g])];
    hap = rr.assignment; ps = rr.phase_set;
  }
  const int pos = b.pos[r];
  const int first = EMIT ? pair_off[r] : 0;
  const int t0 = EMIT ? tbl_off[g] : 0;
  const uint32_t mask = EMIT ? (uint32_t)(tbl_off[g + 1] - t0) - 1u : 0u;   // (a participating row has a pair: the segment is not empty)
  int ref_cur, n_n;
  row16_walk_junctions(b, r, [&](int s, int len, int k) {
    if (!EMIT) return;
    const unsigned long long key = ((unsigned long long)(uint32_t)s << 32) | (uint32_t)len;
    keys[first + k] = key;
    // the segment has at least twice the region's pairs in slots: an empty one is met before the probe comes round
    uint32_t h = k6_hash(key) & mask;
    for (uint32_t i = 0; i <= mask; i++, h = (h + 1) & mask) {
      const unsigned long long prev = atomicCAS(&tbl_key[t0 + h], K6_EMPTY, key);
      if (prev == K6_EMPTY || prev == key) { atomicAdd(&tbl_cnt[t0 + h], 1u); break; }   // (a read holds a key once: s rises along it)
    }
  }, &n_n, &ref_cur);
  if (l16 != 0) return;
  if (!EMIT) {
    const int p = (uint32_t)n_n > min_junctions ? 1 : 0;
    part_flag[r] = p; npair[r] = p ? n_n : 0;
  } else {
    rows[part_off[r]] = K6Row{pos, ref_cur, ps, first, n_n, hap};
  }
}

// per region: slots of its table segment = 2 x pairs rounded up to a power of two (0 without pairs); the totals for the host
__global__ void k6_sizes(const int32_t* __restrict__ read_begin, int32_t ng, int32_t nr, const int32_t* __restrict__ part_off,
                         const int32_t* __restrict__ pair_off, int32_t* __restrict__ tsz, int32_t* __restrict__ host_ctl) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) { host_ctl[0] = part_off[nr]; host_ctl[1] = pair_off[nr]; }
  if (g >= ng) return;
  const int p = pair_off[read_begin[g + 1]] - pair_off[read_begin[g]];
  int s = 0;
  if (p > 0) { s = 2; while (s < 2 * p) s <<= 1; }
  tsz[g] = s;
}

__global__ void k6_flag(const unsigned long long* __restrict__ tbl_key, const uint32_t* __restrict__ tbl_cnt, int32_t n_slots,
                        uint32_t min_count, int32_t* __restrict__ flag) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_slots) flag[t] = (tbl_key[t] != K6_EMPTY && tbl_cnt[t] >= min_count) ? 1 : 0;
}

// koff: kept slots in front of every slot ([n_slots] = all of them; slots behind the last segment are never filled)
__global__ void k6_offsets(const int32_t* __restrict__ tbl_off, const int32_t* __restrict__ koff, int32_t ng, int32_t n_slots,
                           int32_t* __restrict__ joff, int32_t* __restrict__ host_joff, int32_t* __restrict__ host_ctl) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) host_ctl[2] = koff[n_slots];
  if (g > ng) return;
  const int v = koff[tbl_off[g]];
  joff[g] = v; host_joff[g] = v;
}

__global__ void k6_compact(const unsigned long long* __restrict__ tbl_key, const uint32_t* __restrict__ tbl_cnt, const int32_t* __restrict__ flag,
                           const int32_t* __restrict__ koff, const int32_t* __restrict__ tbl_off, int32_t ng, int32_t n_slots,
                           unsigned long long* __restrict__ ck, uint32_t* __restrict__ cc, int32_t* __restrict__ cgr) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots || !flag[t]) return;
  int lo = 0, hi = ng;   // the region whose segment holds slot t: the last g with tbl_off[g] <= t (empty segments share an offset)
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tbl_off[mid] <= t) lo = mid; else hi = mid; }
  const int j = koff[t];
  ck[j] = tbl_key[t]; cc[j] = tbl_cnt[t]; cgr[j] = lo;
}

// A kept junction's place is its rank among the region's kept keys, found by counting the smaller ones: kept junctions per region are
// the splice sites of a gene with min_count reads each -- tens to a few hundred, next to thousands of rows -- so the quadratic count is
// a few thousand coalesced loads per junction.  A region with more is still ordered correctly, only more slowly.
__global__ void k6_rank(BatchView b, const unsigned long long* __restrict__ ck, const uint32_t* __restrict__ cc, const int32_t* __restrict__ cgr,
                        const int32_t* __restrict__ joff, int32_t n_kept, lcr_junction* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_kept) return;
  const int g = cgr[j], lo = joff[g], hi = joff[g + 1];
  const unsigned long long key = ck[j];
  int rank = 0;
  for (int k = lo; k < hi; k++) rank += ck[k] < key ? 1 : 0;
  const int32_t s = (int32_t)(key >> 32), l = (int32_t)(key & 0xffffffffu);
  lcr_junction o{};
  o.region = g; o.motif = splice_motif(b, g, s, l); o.start0 = s; o.len = l; o.n_reads = cc[j];
  out[lo + rank] = o;
}

// One workgroup per kept junction.  The region's participating rows are sorted by pos: those from the first with pos >= s + l on cannot
// overlap and are cut off by a binary search.  The overlapping rows go through the four-cell sweep of k6_walk.h; presence is a scan of
// the row's own keys.
__global__ void __launch_bounds__(LCR_BLOCK) k6_tables(BatchView b, const int32_t* __restrict__ part_off, const K6Row* __restrict__ rows,
                                                        const unsigned long long* __restrict__ keys, int32_t n_kept,
                                                        lcr_junction* __restrict__ junc, lcr_junction* __restrict__ host_junc) {
  __shared__ int sh_end;
  const int j = blockIdx.x, tid = threadIdx.x;
  if (j >= n_kept) return;
  const lcr_junction rec = junc[j];
  const int g = rec.region;
  const int32_t s = (int32_t)rec.start0, l = rec.len;
  const long long jend = (long long)s + l;
  const unsigned long long key = ((unsigned long long)(uint32_t)s << 32) | (uint32_t)l;
  const int p0 = part_off[b.read_begin[g]], p1 = part_off[b.read_begin[g + 1]];
  if (tid == 0) {
    int lo = p0, hi = p1;   // first row in [p0, p1) with pos >= s + l
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if ((long long)rows[mid].pos >= jend) hi = mid; else lo = mid + 1; }
    sh_end = lo;
  }
  __syncthreads();
  const K6Cells best = sweep_phase_set_cells(
      rows, p0, sh_end, [&](const K6Row& row) { return (long long)row.pos < jend && row.rend > s; },   // overlap: pos < s + l && rend > s
      [&](const K6Row& row) {
        int present = 0;
        for (int k = 0; k < row.n; k++) present |= keys[row.first + k] == key ? 1 : 0;
        return (row.hap - 1) * 2 + present;
      });
  if (tid == 0) {
    lcr_junction o = rec;
    o.phase_set = best.ps; o.n_phase_sets = best.n_sets;
    o.h1_absent = best.n[0]; o.h1_present = best.n[1]; o.h2_absent = best.n[2]; o.h2_present = best.n[3];
    junc[j] = o; host_junc[j] = o;
  }
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_k6_count(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, uint32_t min_junctions,
                     int32_t* part_flag, int32_t* npair, hipStream_t s) {
  if (b.n_reads <= 0) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k6_walk<false>, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, row_region_off, rec, min_junctions,
                     part_flag, npair, (const int32_t*)nullptr, (const int32_t*)nullptr, (const int32_t*)nullptr, (K6Row*)nullptr,
                     (unsigned long long*)nullptr, (unsigned long long*)nullptr, (uint32_t*)nullptr);
}
void launch_k6_sizes(const BatchView& b, const int32_t* part_off, const int32_t* pair_off, int32_t* tsz, int32_t* host_ctl, hipStream_t s) {
  hipLaunchKernelGGL(k6_sizes, dim3((std::max(b.n_regions, 1) + 255) / 256), dim3(256), 0, s, b.read_begin, b.n_regions, b.n_reads, part_off, pair_off, tsz, host_ctl);
}
size_t launch_k6_row_bytes() { return sizeof(K6Row); }
void launch_k6_emit(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, const int32_t* part_flag,
                    const int32_t* part_off, const int32_t* pair_off, const int32_t* tbl_off, void* rows, uint64_t* keys,
                    uint64_t* tbl_key, uint32_t* tbl_cnt, hipStream_t s) {
  if (b.n_reads <= 0) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k6_walk<true>, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, row_region_off, rec, 0u,
                     const_cast<int32_t*>(part_flag), (int32_t*)nullptr, part_off, pair_off, tbl_off, (K6Row*)rows, (unsigned long long*)keys,
                     (unsigned long long*)tbl_key, tbl_cnt);
}
void launch_k6_flag(const uint64_t* tbl_key, const uint32_t* tbl_cnt, int32_t n_slots, uint32_t min_count, int32_t* flag, hipStream_t s) {
  if (n_slots > 0) hipLaunchKernelGGL(k6_flag, dim3((n_slots + 255) / 256), dim3(256), 0, s, (const unsigned long long*)tbl_key, tbl_cnt, n_slots, min_count, flag);
}
void launch_k6_offsets(const int32_t* tbl_off, const int32_t* koff, int32_t ng, int32_t n_slots, int32_t* joff, int32_t* host_joff, int32_t* host_ctl,
                       hipStream_t s) {
  hipLaunchKernelGGL(k6_offsets, dim3((ng + 1 + 255) / 256), dim3(256), 0, s, tbl_off, koff, ng, n_slots, joff, host_joff, host_ctl);
}
void launch_k6_place(const BatchView& b, const uint64_t* tbl_key, const uint32_t* tbl_cnt, const int32_t* flag, const int32_t* koff,
                     const int32_t* tbl_off, int32_t n_slots, const int32_t* joff, int32_t n_kept, uint64_t* ck, uint32_t* cc, int32_t* cgr,
                     lcr_junction* junc, hipStream_t s) {
  if (n_slots <= 0 || n_kept <= 0) return;
  hipLaunchKernelGGL(k6_compact, dim3((n_slots + 255) / 256), dim3(256), 0, s, (const unsigned long long*)tbl_key, tbl_cnt, flag, koff, tbl_off, b.n_regions,
                     n_slots, (unsigned long long*)ck, cc, cgr);
  hipLaunchKernelGGL(k6_rank, dim3((n_kept + 255) / 256), dim3(256), 0, s, b, (const unsigned long long*)ck, cc, cgr, joff, n_kept, junc);
}
void launch_k6_tables(const BatchView& b, const int32_t* part_off, const void* rows, const uint64_t* keys, int32_t n_kept, lcr_junction* junc,
                      lcr_junction* host_junc, hipStream_t s) {
  if (n_kept <= 0) return;
  hipLaunchKernelGGL(k6_tables, dim3(n_kept), dim3(LCR_BLOCK), 0, s, b, part_off, (const K6Row*)rows, (const unsigned long long*)keys, n_kept, junc, host_junc);
}

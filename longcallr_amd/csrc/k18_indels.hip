// k18_indels.hip — K18: phased small indels over the fragment rows (lcr_indels; DESIGN.md "Phased small indels").
//
// The contract (include/lcr.h) per region g, over the PARTICIPATING rows -- every fragment row, whatever its assignment:
//   k18_walk<false>  sixteen lanes per read count the read's gaps and events (k18_walk.h)    -> part_flag, ngap, nev (three scans follow)
//   k18_sizes        per region the slots of its segment of the event hash table              -> tsz              (one scan follows)
//   k18_walk<true>   the same walk again: the row's record {pos, rend, ps, first gap, gaps, hap, fragment row}; per gap {s, Lr, key} with the
//                    key of an event's left-shifted form (the lane normalises it against the window's reference) or "no key"; and +1 / -1
//                    at the ends of the row's aligned blocks into the region's segment of the difference array (wlen + 1 words per region:
//                    both ends are clamped into [0, wlen], so a segment sums to 0 and one scan over all segments gives the depths)
//   k18_insert       a thread per gap: an event whose key no earlier gap of its row holds goes into the region's table segment (64-bit
//                    atomicCAS, atomicAdd of its count).  A row can hold a key twice -- two 1-base deletions in one homopolymer --, and cnt
//                    counts rows: the second occurrence is found by a look back over the row's gaps whose end is >= s_left
//   k18_flag         slot kept = occupied && cnt >= min_count && cnt * 1000 >= min_permille * depth(s_left - 1)   -> flag (one scan follows)
//   k18_offsets      events in front of every region, to HBM and to pinned host memory
//   k18_compact      the kept slots, region after region (in slot order)
//   k18_rank         every kept event to its rank among the region's kept keys + type, len, seq, shift, hrun, depth
//   k18_tables       one workgroup per kept event: present / absent / other, row_indels, the phase set with the most rows, the four cells
//   k18_export       row_indels, all of it, and n_present_total to pinned host memory
// Coordinates are the contig's; all arithmetic is integer adds, and nothing in the output depends on the order in which atomics land.
#include <algorithm>

#include "k6_walk.h"
#include "k18_walk.h"
#include "lcr_dev.h"

namespace {

constexpr unsigned long long K18_NOKEY = ~0ull;   // no key / an empty slot: s_left < 2^31 keeps every key below it

struct K18Gap {           // a gap of a participating row, in walk order: starts and ends both ascend
  int32_t s, lr;          // [s, s + lr) on the contig; lr = 0 for I
  unsigned long long key; // of an event, else K18_NOKEY
};
static_assert(sizeof(K18Gap) == 16, "K18Gap is four words");

struct K18Row {           // a participating row, in read order (= by pos inside a region)
  int32_t pos, rend;      // [pos, rend) on the contig
  uint32_t ps;            // phase set, 0 = none
  int32_t first, n;       // its gaps are gaps[first .. first + n)
  int32_t hap;            // 1 / 2, or another assignment: no cell
  int32_t frow;           // its row of the fragment matrix
};
static_assert(sizeof(K18Row) == 28, "K18Row is seven words");

__device__ __forceinline__ uint32_t k18_hash(unsigned long long key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32); }

// Is the gap an event?  *seq: the bases of an insertion, 2 bits each, first base lowest
__device__ __forceinline__ bool k18_event(const BatchView& b, int r, long long w0, long long w1, int s, int len, int op, int q, uint32_t max_ins,
                                          uint32_t max_del, uint32_t* seq) {
  *seq = 0;
  if (op == 2) return (uint32_t)len <= max_del && (long long)s >= w0 + 1 && (long long)s + len <= w1;
  if (op != 1 || (uint32_t)len > max_ins || !((long long)s >= w0 + 1 && (long long)s <= w1)) return false;
  if (q < 0 || (long long)q + len > (long long)b.seq_len[r]) return false;   // (a CIGAR that overruns its bases: no letters to read)
  const uint8_t* __restrict__ bs = b.bases + b.seq_off[r] + q;
  uint32_t v = 0;
  for (int k = 0; k < len; k++) {   // (len <= 12)
    const int a = k18_code(bs[k]);
    if (a < 0) return false;
    v |= (uint32_t)a << (2 * k);
  }
  *seq = v;
  return true;
}

template <bool EMIT>
__global__ void __launch_bounds__(LCR_BLOCK) k18_walk(BatchView b, const int32_t* __restrict__ row_region_off, const lcr_read_record* __restrict__ rec,
                                                       uint32_t max_ins, uint32_t max_del, int32_t* __restrict__ part_flag, int32_t* __restrict__ ngap,
                                                       int32_t* __restrict__ nev, const int32_t* __restrict__ part_off, const int32_t* __restrict__ gap_off,
                                                       K18Row* __restrict__ rows, K18Gap* __restrict__ gaps, int32_t* __restrict__ gap_read,
                                                       int32_t* __restrict__ diff) {
  const int l16 = threadIdx.x & 15;
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) >> 4;
  if (rl >= b.n_reads) return;   // (a whole row leaves)
  const int r = (int)rl;
  const int g = region_of_read(b, r);
  int hap = 0, frow = 0; uint32_t ps = 0;
  if (!EMIT) {
    // row k of region g is the region's k-th read (fragment.rs:293-307: the reads up to the last candidate); a read behind them is no row
    const int k = r - b.read_begin[g], row0 = row_region_off[g];
    if (!(k < row_region_off[g + 1] - row0)) { if (l16 == 0) { part_flag[r] = 0; ngap[r] = 0; nev[r] = 0; } return; }
  } else {
    if (!part_flag[r]) return;
    frow = row_region_off[g] + (r - b.read_begin[g]);
    const lcr_read_record rr = rec[frow];
    hap = rr.assignment; ps = rr.phase_set;
  }
  const long long w0 = b.start0[g], wlen = b.len[g], w1 = w0 + wlen;
  const uint8_t* __restrict__ wref = b.ref + b.col_off[g];
  const int first = EMIT ? gap_off[r] : 0;
  int32_t* const dseg = EMIT ? diff + (b.col_off[g] + g) : nullptr;
  int n_g, n_e, rend;
  row16_walk_gaps(b, r, [&](int s, int len, int op, int q, int k) {
    uint32_t seq;
    const bool ev = k18_event(b, r, w0, w1, s, len, op, q, max_ins, max_del, &seq);
    if (EMIT) {
      unsigned long long key = K18_NOKEY;
      if (ev) {
        const int type = op == 1 ? 1 : 0;
        const long long sl = k18_left_shift(wref, w0, type, s, len, &seq);
        key = ((unsigned long long)(uint32_t)sl << 32) | ((unsigned long long)type << 31) | (type ? ((uint32_t)len << 24) | seq : (uint32_t)len);
      }
      gaps[first + k] = K18Gap{s, op == 1 ? 0 : len, key};
      gap_read[first + k] = r;
    }
    return ev;
  }, [&](int col, int d) {
    if (!EMIT) return;
    const long long x = (long long)col - w0;
    atomicAdd(&dseg[x < 0 ? 0 : x > wlen ? wlen : x], d);
  }, &n_g, &n_e, &rend);
  if (l16 != 0) return;
  if (!EMIT) { part_flag[r] = 1; ngap[r] = n_g; nev[r] = n_e; }
  else rows[part_off[r]] = K18Row{b.pos[r], rend, ps, first, n_g, hap, frow};
}

// per region: slots of its table segment = 2 x event occurrences rounded up to a power of two (0 without events); the totals for the host
__global__ void k18_sizes(const int32_t* __restrict__ read_begin, int32_t ng, int32_t nr, const int32_t* __restrict__ part_off,
                          const int32_t* __restrict__ gap_off, const int32_t* __restrict__ ev_off, int32_t* __restrict__ tsz,
                          int32_t* __restrict__ host_ctl) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) { host_ctl[0] = part_off[nr]; host_ctl[1] = gap_off[nr]; host_ctl[3] = ev_off[nr]; }
  if (g >= ng) return;
  const int p = ev_off[read_begin[g + 1]] - ev_off[read_begin[g]];
  int s = 0;
  if (p > 0) { s = 2; while (s < 2 * p) s <<= 1; }
  tsz[g] = s;
}

__global__ void k18_insert(BatchView b, const K18Gap* __restrict__ gaps, const int32_t* __restrict__ gap_read, const int32_t* __restrict__ gap_off,
                           int32_t n_gaps, const int32_t* __restrict__ tbl_off, uint32_t hmask, unsigned long long* __restrict__ tbl_key,
                           uint32_t* __restrict__ tbl_cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_gaps) return;
  const unsigned long long key = gaps[i].key;
  if (key == K18_NOKEY) return;
  const int r = gap_read[i];
  const long long sl = (long long)(int32_t)(key >> 32);
  // an earlier gap of the row with the same key lies inside the event's extent, so its end is >= s_left; ends ascend along the row
  for (int j = i - 1; j >= gap_off[r]; j--) {
    const K18Gap q = gaps[j];
    if ((long long)q.s + q.lr < sl) break;
    if (q.key == key) return;
  }
  const int g = region_of_read(b, r);
  const int t0 = tbl_off[g], tsz = tbl_off[g + 1] - t0;
  if (tsz <= 0) return;   // (cannot happen: the segment is sized from this region's events)
  const uint32_t mask = (uint32_t)tsz - 1u;
  // the segment has at least twice the region's events in slots: an empty one is met before the probe comes round
  uint32_t h = k18_hash(key) & hmask & mask;
  for (uint32_t k = 0; k <= mask; k++, h = (h + 1) & mask) {
    const unsigned long long prev = atomicCAS(&tbl_key[t0 + h], K18_NOKEY, key);
    if (prev == K18_NOKEY || prev == key) { atomicAdd(&tbl_cnt[t0 + h], 1u); break; }
  }
}

// the region whose segment holds slot t: the last g with tbl_off[g] <= t (empty segments share an offset)
__device__ __forceinline__ int k18_slot_region(const int32_t* __restrict__ tbl_off, int ng, int t) {
  int lo = 0, hi = ng;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tbl_off[mid] <= t) lo = mid; else hi = mid; }
  return lo;
}

// depth(g, x) = dscan[col_off[g] + g + (x - w0) + 1]: the exclusive scan's value behind the column's own difference
__device__ __forceinline__ uint32_t k18_depth(const BatchView& b, const int32_t* __restrict__ dscan, int g, long long x) {
  return (uint32_t)dscan[b.col_off[g] + g + (x - b.start0[g]) + 1];
}

__global__ void k18_flag(BatchView b, const unsigned long long* __restrict__ tbl_key, const uint32_t* __restrict__ tbl_cnt, int32_t n_slots,
                         const int32_t* __restrict__ tbl_off, const int32_t* __restrict__ dscan, uint32_t min_count, uint32_t min_permille,
                         int32_t* __restrict__ flag) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots) return;
  const unsigned long long key = tbl_key[t];
  const uint32_t cnt = tbl_cnt[t];
  int keep = 0;
  if (key != K18_NOKEY && cnt >= min_count && t < tbl_off[b.n_regions]) {
    const int g = k18_slot_region(tbl_off, b.n_regions, t);
    const uint32_t depth = k18_depth(b, dscan, g, (long long)(int32_t)(key >> 32) - 1);   // (s_left >= w0 + 1: the anchor lies inside the window)
    keep = (unsigned long long)cnt * 1000ull >= (unsigned long long)min_permille * depth ? 1 : 0;
  }
  flag[t] = keep;
}

// koff: kept slots in front of every slot ([n_slots] = all of them; slots behind the last segment are never filled)
__global__ void k18_offsets(const int32_t* __restrict__ tbl_off, const int32_t* __restrict__ koff, int32_t ng, int32_t n_slots,
                            int32_t* __restrict__ off, int32_t* __restrict__ host_off, int32_t* __restrict__ host_ctl) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) host_ctl[2] = koff[n_slots];
  if (g > ng) return;
  const int v = koff[tbl_off[g]];   // (tbl_off[g] <= n_slots, and koff has n_slots + 1 words)
  off[g] = v; host_off[g] = v;
}

__global__ void k18_compact(const unsigned long long* __restrict__ tbl_key, const uint32_t* __restrict__ tbl_cnt, const int32_t* __restrict__ flag,
                            const int32_t* __restrict__ koff, const int32_t* __restrict__ tbl_off, int32_t ng, int32_t n_slots,
                            unsigned long long* __restrict__ ck, uint32_t* __restrict__ cc, int32_t* __restrict__ cgr) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots || !flag[t]) return;
  const int j = koff[t];
  ck[j] = tbl_key[t]; cc[j] = tbl_cnt[t]; cgr[j] = k18_slot_region(tbl_off, ng, t);
}

// A kept event's place is its rank among the region's kept keys, found by counting the smaller ones (as k17_rank).  The right shift and
// hrun are functions of the key and the window's reference; n_present starts as the table's count, k18_tables counts it again.
__global__ void k18_rank(BatchView b, const unsigned long long* __restrict__ ck, const uint32_t* __restrict__ cc, const int32_t* __restrict__ cgr,
                         const int32_t* __restrict__ off, const int32_t* __restrict__ dscan, int32_t n_kept, lcr_indel* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_kept) return;
  const int g = cgr[j], lo = off[g], hi = off[g + 1];
  const unsigned long long key = ck[j];
  int rank = 0;
  for (int k = lo; k < hi; k++) rank += ck[k] < key ? 1 : 0;
  const long long sl = (long long)(int32_t)(key >> 32), w0 = b.start0[g], w1 = w0 + b.len[g];
  const uint32_t low = (uint32_t)key;
  const int type = (int)(low >> 31);
  const int len = type ? (int)((low >> 24) & 0x7fu) : (int)(low & 0x7fffffffu);
  const uint32_t seq = type ? (low & 0xffffffu) : 0u;
  const uint8_t* __restrict__ wref = b.ref + b.col_off[g];
  const long long sr = k18_right_shift(wref, w0, w1, type, sl, len, seq);
  int hrun = 0;
  if (sl < w1) {
    const uint8_t c0 = wref[sl - w0] & 0xdfu;
    while (hrun < 255 && sl + hrun < w1 && (wref[sl + hrun - w0] & 0xdfu) == c0) hrun++;
  }
  lcr_indel o{};
  o.region = g; o.type = (uint8_t)type; o.hrun = (uint8_t)hrun; o.shift = (uint16_t)(sr - sl); o.start0 = sl; o.len = len; o.seq = seq;
  o.depth = k18_depth(b, dscan, g, sl - 1); o.n_present = cc[j];
  out[lo + rank] = o;
}

// The class of a looked-at row at the event `key` with the flanked extent [lo_f, hi_f]: 1 PRESENT (asked first), 2 ABSENT, 0 OTHER.  The
// gaps that touch the extent are those from the first whose end is >= lo_f (a binary search: ends ascend) while the start is <= hi_f.
__device__ __forceinline__ int k18_class(const K18Row& row, const K18Gap* __restrict__ gaps, unsigned long long key, long long lo_f, long long hi_f) {
  int lo = row.first, hi = row.first + row.n;
  const int end = hi;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const K18Gap q = gaps[mid];
    if ((long long)q.s + q.lr >= lo_f) hi = mid; else lo = mid + 1;
  }
  bool present = false, touch = false;
  for (int j = lo; j < end; j++) {
    const K18Gap q = gaps[j];
    if ((long long)q.s > hi_f) break;
    touch = true;
    present |= q.key == key;
  }
  if (present) return 1;
  return ((long long)row.pos <= lo_f && (long long)row.rend >= hi_f && !touch) ? 2 : 0;
}

// One workgroup per kept event.  The region's participating rows are sorted by pos: those from the first with pos >= hi_f on are not looked
// at and are cut off by a binary search.  One pass classes every looked-at row (a thread's counts in registers, a wave's sum, three LDS
// atomics per wave) and adds 1 to row_indels of a PRESENT row; then the four-cell sweep of k6_walk.h over the PRESENT and ABSENT rows with
// assignment 1 / 2.
__global__ void __launch_bounds__(LCR_BLOCK) k18_tables(BatchView b, const int32_t* __restrict__ part_off, const K18Row* __restrict__ rows,
                                                         const K18Gap* __restrict__ gaps, int32_t flank, int32_t n_kept, lcr_indel* __restrict__ indel,
                                                         lcr_indel* __restrict__ host_indel, int32_t* __restrict__ row_indels,
                                                         unsigned long long* __restrict__ n_total) {
  __shared__ int sh_end;
  __shared__ uint32_t sh_n[3];
  const int j = blockIdx.x, tid = threadIdx.x;
  if (j >= n_kept) return;
  const lcr_indel rec = indel[j];
  const int g = rec.region;
  const long long sl = rec.start0;
  const long long lo_f = sl - flank, hi_f = sl + rec.shift + (rec.type ? 0 : rec.len) + flank;
  const unsigned long long key = ((unsigned long long)(uint32_t)sl << 32) | ((unsigned long long)rec.type << 31) |
                                 (rec.type ? ((uint32_t)rec.len << 24) | rec.seq : (uint32_t)rec.len);
  const int p0 = part_off[b.read_begin[g]], p1 = part_off[b.read_begin[g + 1]];
  if (tid == 0) {
    int lo = p0, hi = p1;   // first row in [p0, p1) with pos >= hi_f
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if ((long long)rows[mid].pos >= hi_f) hi = mid; else lo = mid + 1; }
    sh_end = lo;
    sh_n[0] = sh_n[1] = sh_n[2] = 0;
  }
  __syncthreads();
  const int p_end = sh_end;
  uint32_t n0 = 0, n1 = 0, n2 = 0;   // other, present, absent
  for (int p = p0 + tid; p < p_end; p += LCR_BLOCK) {
    const K18Row row = rows[p];
    if (!((long long)row.pos < hi_f && (long long)row.rend > lo_f)) continue;
    const int cls = k18_class(row, gaps, key, lo_f, hi_f);
    n0 += cls == 0; n1 += cls == 1; n2 += cls == 2;
    if (cls == 1) atomicAdd(&row_indels[row.frow], 1);
  }
  n0 = wave_sum_u32(n0); n1 = wave_sum_u32(n1); n2 = wave_sum_u32(n2);
  if ((tid & 63) == 0) {
    if (n0) atomicAdd(&sh_n[0], n0);
    if (n1) atomicAdd(&sh_n[1], n1);
    if (n2) atomicAdd(&sh_n[2], n2);
  }
  __syncthreads();
  const uint32_t n_other = sh_n[0], n_present = sh_n[1], n_absent = sh_n[2];
  const K6Cells best = sweep_phase_set_cells(
      rows, p0, p_end,
      [&](const K18Row& row) {
        return (row.hap == 1 || row.hap == 2) && (long long)row.pos < hi_f && (long long)row.rend > lo_f && k18_class(row, gaps, key, lo_f, hi_f) != 0;
      },
      [&](const K18Row& row) { return (row.hap - 1) * 2 + (k18_class(row, gaps, key, lo_f, hi_f) == 2 ? 1 : 0); });
  if (tid == 0) {
    lcr_indel o = rec;
    o.n_present = n_present; o.n_absent = n_absent; o.n_other = n_other;   // (n_present equals the table's count: both count the rows that hold the key)
    o.phase_set = best.ps; o.n_phase_sets = best.n_sets;
    o.h1_present = best.n[0]; o.h1_absent = best.n[1]; o.h2_present = best.n[2]; o.h2_absent = best.n[3];
    indel[j] = o; host_indel[j] = o;
    if (n_present) atomicAdd(n_total, (unsigned long long)n_present);
  }
}

__global__ void k18_export(int32_t n_rows, const int32_t* __restrict__ row_indels, int32_t* __restrict__ host_row_indels,
                           const unsigned long long* __restrict__ n_total, unsigned long long* __restrict__ host_n_total) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0) *host_n_total = *n_total;
  if (r < n_rows) host_row_indels[r] = row_indels[r];
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_k18_count(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, uint32_t max_ins, uint32_t max_del,
                      int32_t* part_flag, int32_t* ngap, int32_t* nev, hipStream_t s) {
  if (b.n_reads <= 0) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k18_walk<false>, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, row_region_off, rec, max_ins, max_del,
                     part_flag, ngap, nev, (const int32_t*)nullptr, (const int32_t*)nullptr, (K18Row*)nullptr, (K18Gap*)nullptr, (int32_t*)nullptr,
                     (int32_t*)nullptr);
}
void launch_k18_sizes(const BatchView& b, const int32_t* part_off, const int32_t* gap_off, const int32_t* ev_off, int32_t* tsz, int32_t* host_ctl,
                      hipStream_t s) {
  hipLaunchKernelGGL(k18_sizes, dim3((std::max(b.n_regions, 1) + 255) / 256), dim3(256), 0, s, b.read_begin, b.n_regions, b.n_reads, part_off, gap_off,
                     ev_off, tsz, host_ctl);
}
size_t launch_k18_row_bytes() { return sizeof(K18Row); }
size_t launch_k18_gap_bytes() { return sizeof(K18Gap); }
void launch_k18_emit(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, uint32_t max_ins, uint32_t max_del,
                     const int32_t* part_flag, const int32_t* part_off, const int32_t* gap_off, void* rows, void* gaps, int32_t* gap_read, int32_t* diff,
                     hipStream_t s) {
  if (b.n_reads <= 0) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k18_walk<true>, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, row_region_off, rec, max_ins, max_del,
                     const_cast<int32_t*>(part_flag), (int32_t*)nullptr, (int32_t*)nullptr, part_off, gap_off, (K18Row*)rows, (K18Gap*)gaps, gap_read, diff);
}
void launch_k18_insert(const BatchView& b, const void* gaps, const int32_t* gap_read, const int32_t* gap_off, int32_t n_gaps, const int32_t* tbl_off,
                       uint32_t hash_mask, uint64_t* tbl_key, uint32_t* tbl_cnt, hipStream_t s) {
  if (n_gaps > 0) hipLaunchKernelGGL(k18_insert, dim3((n_gaps + 255) / 256), dim3(256), 0, s, b, (const K18Gap*)gaps, gap_read, gap_off, n_gaps, tbl_off,
                                     hash_mask, (unsigned long long*)tbl_key, tbl_cnt);
}
void launch_k18_flag(const BatchView& b, const uint64_t* tbl_key, const uint32_t* tbl_cnt, int32_t n_slots, const int32_t* tbl_off, const int32_t* dscan,
                     uint32_t min_count, uint32_t min_permille, int32_t* flag, hipStream_t s) {
  if (n_slots > 0) hipLaunchKernelGGL(k18_flag, dim3((n_slots + 255) / 256), dim3(256), 0, s, b, (const unsigned long long*)tbl_key, tbl_cnt, n_slots, tbl_off,
                                      dscan, min_count, min_permille, flag);
}
void launch_k18_offsets(const int32_t* tbl_off, const int32_t* koff, int32_t ng, int32_t n_slots, int32_t* off, int32_t* host_off, int32_t* host_ctl,
                        hipStream_t s) {
  hipLaunchKernelGGL(k18_offsets, dim3((ng + 1 + 255) / 256), dim3(256), 0, s, tbl_off, koff, ng, n_slots, off, host_off, host_ctl);
}
void launch_k18_place(const BatchView& b, const uint64_t* tbl_key, const uint32_t* tbl_cnt, const int32_t* flag, const int32_t* koff,
                      const int32_t* tbl_off, int32_t n_slots, const int32_t* off, const int32_t* dscan, int32_t n_kept, uint64_t* ck, uint32_t* cc,
                      int32_t* cgr, lcr_indel* indel, hipStream_t s) {
  if (n_slots <= 0 || n_kept <= 0) return;
  hipLaunchKernelGGL(k18_compact, dim3((n_slots + 255) / 256), dim3(256), 0, s, (const unsigned long long*)tbl_key, tbl_cnt, flag, koff, tbl_off, b.n_regions,
                     n_slots, (unsigned long long*)ck, cc, cgr);
  hipLaunchKernelGGL(k18_rank, dim3((n_kept + 255) / 256), dim3(256), 0, s, b, (const unsigned long long*)ck, cc, cgr, off, dscan, n_kept, indel);
}
void launch_k18_tables(const BatchView& b, const int32_t* part_off, const void* rows, const void* gaps, uint32_t flank, int32_t n_kept, lcr_indel* indel,
                       lcr_indel* host_indel, int32_t* row_indels, uint64_t* n_total, hipStream_t s) {
  if (n_kept <= 0) return;
  hipLaunchKernelGGL(k18_tables, dim3(n_kept), dim3(LCR_BLOCK), 0, s, b, part_off, (const K18Row*)rows, (const K18Gap*)gaps, (int32_t)flank, n_kept, indel,
                     host_indel, row_indels, (unsigned long long*)n_total);
}
void launch_k18_export(int32_t n_rows, const int32_t* row_indels, int32_t* host_row_indels, const uint64_t* n_total, uint64_t* host_n_total,
                       hipStream_t s) {
  hipLaunchKernelGGL(k18_export, dim3((std::max(n_rows, 1) + 255) / 256), dim3(256), 0, s, n_rows, row_indels, host_row_indels,
                     (const unsigned long long*)n_total, (unsigned long long*)host_n_total);
}

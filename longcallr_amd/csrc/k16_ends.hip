// k16_ends.hip — K16: haplotype x transcript-end sites over the phased rows (lcr_transcript_ends; DESIGN.md "Allele-specific transcript ends").
//
// The contract (include/lcr.h) per region g, over the PARTICIPATING rows -- fragment rows with assignment 1 / 2 whose read has a
// transcript strand.  The peak rule and the nearest-peak rule are local (each looks at 2 W neighbours at most), so nothing is sorted: a
// hash table of the distinct end coordinates per region, as K6 has for junctions, answers both by lookups.
//   k16_count     one thread per read: is it a participating row (assignment, strand by strand_mode)                     (one scan follows)
//   k16_sizes     per region the slots of its segment of the end table: 2 x (2 x its participating rows), a power of two (one scan follows)
//   k16_walk      sixteen lanes per read walk its CIGAR for rend (k6_walk.h, a sink that does nothing): the row's record, and its two keys
//                 strand << 33 | side << 32 | (uint32_t)x into the region's segment (64-bit atomicCAS, atomicAdd of c_h1 / c_h2)
//   k16_peaks     one thread per slot: an occupied slot looks its 2 W neighbours of the same class up and sets its peak flag
//   k16_assign    a launch of its own behind the flags: per occupied slot the nearest peak (d = 0, -1, +1, -2, +2, ...: ties go down), and
//                 its counts into the peak's n_h1 / n_h2 / n_peak, min0 / max0
//   k16_flag      slot kept = peak && n_h1 + n_h2 >= min_count                                                            (one scan follows)
//   k16_offsets   sites in front of every region, to HBM and to pinned host memory
//   k16_compact   the kept slots, region after region (in slot order)
//   k16_rank      every kept site to its rank among the region's kept sites (p, then strand, then side), its record without the table
//   k16_rows      row -> its two slots -> their peaks -> the records: row_site, the same into the row's record, and n_assigned
//   k16_export    row_site, all of it, and n_assigned to pinned host memory
//   k16_tables    one workgroup per kept site: present, absent, the phase set with the most rows, the four cells
// Coordinates are the contig's (the batch's int32 positions); all arithmetic is integer, and nothing in the output depends on the order in
// which atomics land: a slot's position inside its segment does, the sorted records, the counts and row_site do not.
#include <algorithm>

#include "k6_walk.h"
#include "lcr_dev.h"

namespace {

constexpr unsigned long long K16_EMPTY = ~0ull;   // no key: strand <= 2 keeps bit 34 of every key clear

struct K16Row {           // a participating row, in read order (= by pos inside a region)
  int32_t pos, rend;      // [pos, rend) on the contig
  uint32_t ps;            // phase set, 0 = none
  int32_t hap, strand;    // 1 / 2 each
  int32_t frow;           // its row of the fragment matrix
  int32_t slot[2];        // the slots of its left and right end
  int32_t site[2];        // k16_rows: the kept records they are assigned to, or -1
};
static_assert(sizeof(K16Row) == 40, "K16Row is ten words");

struct K16Slot {                 // what becomes of a slot behind the insertion (k16_peaks writes all of it, k16_assign adds to the peaks')
  uint32_t n_h1, n_h2, n_peak;   // of a peak: the rows assigned to it per haplotype; those that end exactly at it
  int32_t min0, max0;            // of a peak: the smallest and largest assigned coordinate
  int32_t to;                    // the slot of the peak this coordinate is assigned to, or -1
  int32_t peak, region;          // 1 = a peak; the region of its segment (-1: an empty slot)
};
static_assert(sizeof(K16Slot) == 32, "K16Slot is eight words");

__device__ __forceinline__ uint32_t k16_hash(unsigned long long key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32); }
__device__ __forceinline__ unsigned long long k16_key(uint32_t cls /* strand << 1 | side */, int32_t x) { return ((unsigned long long)cls << 32) | (uint32_t)x; }

// transcript strand of a read from its flags (include/lcr.h): 1 = '+', 2 = '-', 0 = none
__device__ __forceinline__ int k16_strand(uint32_t flags, uint32_t strand_mode) {
  const int rev = flags & 1u, ts = (flags >> 1) & 3u;
  if (ts == 1) return rev ? 2 : 1;
  if (ts == 2) return rev ? 1 : 2;
  return strand_mode == LCR_ENDS_STRAND_READ ? (rev ? 2 : 1) : 0;
}

// the slot of `key` in the segment [t0, t0 + mask], or -1: the segment is at most half full, so a probe of an absent key ends at an empty slot
__device__ __forceinline__ int k16_find(const unsigned long long* __restrict__ tbl_key, int t0, uint32_t mask, uint32_t hmask, unsigned long long key) {
  uint32_t h = k16_hash(key) & hmask & mask;
  for (uint32_t i = 0; i <= mask; i++, h = (h + 1) & mask) {
    const unsigned long long k = tbl_key[t0 + h];
    if (k == key) return t0 + (int)h;
    if (k == K16_EMPTY) return -1;
  }
  return -1;
}

// row k of region g is the region's k-th read (fragment.rs:293-307: the reads up to the last candidate); a read behind them is no row
__global__ void k16_count(BatchView b, const int32_t* __restrict__ row_region_off, const lcr_read_record* __restrict__ rec, uint32_t strand_mode,
                          int32_t* __restrict__ part_flag) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= b.n_reads) return;
  const int g = region_of_read(b, r);
  const int k = r - b.read_begin[g], row0 = row_region_off[g];
  bool part = k < row_region_off[g + 1] - row0 && k16_strand(b.flags[r], strand_mode) != 0;
  if (part) { const int a = rec[row0 + k].assignment; part = a == 1 || a == 2; }
  part_flag[r] = part ? 1 : 0;
}

// per region: slots of its table segment = 2 x its keys (two per participating row) rounded up to a power of two (0 without rows)
__global__ void k16_sizes(const int32_t* __restrict__ read_begin, int32_t ng, int32_t nr, const int32_t* __restrict__ part_off,
                          int32_t* __restrict__ tsz, int32_t* __restrict__ host_ctl) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) host_ctl[0] = part_off[nr];
  if (g >= ng) return;
  const long long p = part_off[read_begin[g + 1]] - part_off[read_begin[g]];
  long long s = 0;
  if (p > 0) { s = 2; while (s < 4 * p) s <<= 1; }
  tsz[g] = (int32_t)s;   // (the host refuses a batch whose segments do not fit 2^30 slots)
}

__global__ void __launch_bounds__(LCR_BLOCK) k16_walk(BatchView b, const int32_t* __restrict__ row_region_off, const lcr_read_record* __restrict__ rec,
                                                       uint32_t strand_mode, uint32_t hmask, const int32_t* __restrict__ part_flag,
                                                       const int32_t* __restrict__ part_off, const int32_t* __restrict__ tbl_off,
                                                       K16Row* __restrict__ rows, unsigned long long* __restrict__ tbl_key, uint32_t* __restrict__ tbl_cnt) {
  const int lane = threadIdx.x & 63, l16 = lane & 15, rbase = lane & 48;
  const long long rl = ((long long)blockIdx.x * LCR_BLOCK + threadIdx.x) >> 4;
  if (rl >= b.n_reads) return;   // (a whole row leaves)
  const int r = (int)rl;
  if (!part_flag[r]) return;
  const int g = region_of_read(b, r);
  const int frow = row_region_off[g] + (r - b.read_begin[g]);
  const lcr_read_record rr = rec[frow];
  const int hap = rr.assignment, strand = k16_strand(b.flags[r], strand_mode);
  const int pos = b.pos[r];
  int n_n, rend;
  row16_walk_junctions(b, r, [](int, int, int) {}, &n_n, &rend);
  // lane 0 inserts the left end, lane 1 the right one.  The segment has at least twice the region's keys in slots: an empty one is met
  // before the probe comes round.
  int slot = -1;
  if (l16 < 2) {
    const int t0 = tbl_off[g];
    const uint32_t mask = (uint32_t)(tbl_off[g + 1] - t0) - 1u;   // (a participating row has two keys: the segment is not empty)
    const unsigned long long key = k16_key((uint32_t)strand << 1 | (uint32_t)l16, l16 ? rend - 1 : pos);
    uint32_t h = k16_hash(key) & hmask & mask;
    for (uint32_t i = 0; i <= mask; i++, h = (h + 1) & mask) {
      const unsigned long long prev = atomicCAS(&tbl_key[t0 + h], K16_EMPTY, key);
      if (prev == K16_EMPTY || prev == key) {
        slot = t0 + (int)h;
        atomicAdd(&tbl_cnt[2 * (size_t)slot + (hap - 1)], 1u);
        break;
      }
    }
  }
  const int slot1 = __shfl(slot, rbase + 1, 64);   // (the partner is a lane of the same row)
  if (l16 != 0) return;
  rows[part_off[r]] = K16Row{pos, rend, rr.phase_set, hap, strand, frow, {slot, slot1}, {-1, -1}};
}

// the region whose segment holds slot t: the last g with tbl_off[g] <= t (empty segments share an offset)
__device__ __forceinline__ int k16_slot_region(const int32_t* __restrict__ tbl_off, int ng, int t) {
  int lo = 0, hi = ng;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tbl_off[mid] <= t) lo = mid; else hi = mid; }
  return lo;
}

// One thread per slot.  x is a peak iff no other coordinate y of its class within W stands in front of it in the strict order
// "more rows first, then the smaller coordinate".
__global__ void k16_peaks(const unsigned long long* __restrict__ tbl_key, const uint32_t* __restrict__ tbl_cnt, const int32_t* __restrict__ tbl_off,
                          int32_t ng, int32_t n_slots, int32_t window, uint32_t hmask, K16Slot* __restrict__ slots) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots) return;
  const unsigned long long key = tbl_key[t];
  if (key == K16_EMPTY) { slots[t] = K16Slot{0, 0, 0, 0, 0, -1, 0, -1}; return; }
  const int g = k16_slot_region(tbl_off, ng, t);
  const int t0 = tbl_off[g];
  const uint32_t mask = (uint32_t)(tbl_off[g + 1] - t0) - 1u;
  const uint32_t cls = (uint32_t)(key >> 32);
  const int32_t x = (int32_t)(uint32_t)key;
  const uint32_t c = tbl_cnt[2 * (size_t)t] + tbl_cnt[2 * (size_t)t + 1];
  bool peak = true;
  for (int d = 1; peak && d <= window; d++) {
    for (int sgn = -1; sgn <= 1; sgn += 2) {
      const long long y = (long long)x + sgn * d;
      if (y < INT_MIN || y > INT_MAX) continue;
      const int u = k16_find(tbl_key, t0, mask, hmask, k16_key(cls, (int32_t)y));
      if (u < 0) continue;
      const uint32_t cy = tbl_cnt[2 * (size_t)u] + tbl_cnt[2 * (size_t)u + 1];
      if (cy > c || (cy == c && sgn < 0)) peak = false;
    }
  }
  slots[t] = K16Slot{0, 0, 0, x, x, -1, peak ? 1 : 0, g};
}

// One thread per slot, behind k16_peaks' flags (the kernel boundary orders them).  The nearest peak within W, the smaller coordinate first at
// equal distance; a peak finds itself at d == 0.
__global__ void k16_assign(const unsigned long long* __restrict__ tbl_key, const uint32_t* __restrict__ tbl_cnt, const int32_t* __restrict__ tbl_off,
                           int32_t n_slots, int32_t window, uint32_t hmask, K16Slot* __restrict__ slots) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots) return;
  const unsigned long long key = tbl_key[t];
  if (key == K16_EMPTY) return;
  const int g = slots[t].region;
  const int t0 = tbl_off[g];
  const uint32_t mask = (uint32_t)(tbl_off[g + 1] - t0) - 1u;
  const uint32_t cls = (uint32_t)(key >> 32);
  const int32_t x = (int32_t)(uint32_t)key;
  int to = slots[t].peak ? t : -1;
  for (int d = 1; to < 0 && d <= window; d++) {
    for (int sgn = -1; to < 0 && sgn <= 1; sgn += 2) {
      const long long y = (long long)x + sgn * d;
      if (y < INT_MIN || y > INT_MAX) continue;
      const int u = k16_find(tbl_key, t0, mask, hmask, k16_key(cls, (int32_t)y));
      if (u >= 0 && slots[u].peak) to = u;
    }
  }
  slots[t].to = to;
  if (to < 0) return;
  const uint32_t c1 = tbl_cnt[2 * (size_t)t], c2 = tbl_cnt[2 * (size_t)t + 1];
  if (c1) atomicAdd(&slots[to].n_h1, c1);
  if (c2) atomicAdd(&slots[to].n_h2, c2);
  if (to == t) { slots[to].n_peak = c1 + c2; return; }   // (min0 / max0 start at the peak's own coordinate)
  atomicMin(&slots[to].min0, x);
  atomicMax(&slots[to].max0, x);
}

__global__ void k16_flag(const K16Slot* __restrict__ slots, int32_t n_slots, uint32_t min_count, int32_t* __restrict__ flag) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots) return;
  const K16Slot s = slots[t];
  flag[t] = (s.peak && s.n_h1 + s.n_h2 >= min_count) ? 1 : 0;
}

// koff: kept slots in front of every slot ([n_slots] = all of them; slots behind the last segment are never filled)
__global__ void k16_offsets(const int32_t* __restrict__ tbl_off, const int32_t* __restrict__ koff, int32_t ng, int32_t n_slots,
                            int32_t* __restrict__ off, int32_t* __restrict__ host_off, int32_t* __restrict__ host_ctl) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) host_ctl[1] = koff[n_slots];
  if (g > ng) return;
  const int v = koff[tbl_off[g]];
  off[g] = v; host_off[g] = v;
}

__global__ void k16_compact(const int32_t* __restrict__ flag, const int32_t* __restrict__ koff, int32_t n_slots, int32_t* __restrict__ cslot) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_slots && flag[t]) cslot[koff[t]] = t;
}

// the record order inside a region: p, then strand ('+' first), then side (left first)
__device__ __forceinline__ long long k16_order(unsigned long long key) { return (long long)(int32_t)(uint32_t)key * 8 + (long long)(key >> 32); }

// A kept site's place is its rank among the region's kept sites, found by counting the smaller ones (as k6_rank): kept sites are bounded by
// rows / min_count and lie more than W apart per class, so they are few.  A region with many is still ordered correctly, only more slowly.
__global__ void k16_rank(const unsigned long long* __restrict__ tbl_key, const K16Slot* __restrict__ slots, const int32_t* __restrict__ cslot,
                         const int32_t* __restrict__ off, int32_t n_kept, lcr_end_site* __restrict__ site, int32_t* __restrict__ crank) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_kept) return;
  const int t = cslot[j];
  const K16Slot s = slots[t];
  const unsigned long long key = tbl_key[t];
  const long long mine = k16_order(key);
  const int g = s.region, lo = off[g], hi = off[g + 1];
  int rank = 0;
  for (int k = lo; k < hi; k++) rank += k16_order(tbl_key[cslot[k]]) < mine ? 1 : 0;
  const uint32_t cls = (uint32_t)(key >> 32);
  lcr_end_site o{};
  o.region = g; o.strand = (uint8_t)(cls >> 1); o.side = (uint8_t)(cls & 1u);
  o.kind = (uint8_t)((o.strand == 1) == (o.side == 0) ? 0 : 1);   // 5' ends: the left of '+', the right of '-'
  o.peak0 = (int64_t)(int32_t)(uint32_t)key;
  o.min0 = s.min0; o.max0 = s.max0;
  o.n_h1 = s.n_h1; o.n_h2 = s.n_h2; o.n_reads = s.n_h1 + s.n_h2; o.n_peak = s.n_peak;
  site[lo + rank] = o;
  crank[j] = lo + rank;
}

// One thread per participating row; every thread of a wave takes part in the sum.
__global__ void k16_rows(int32_t n_part, K16Row* __restrict__ rows, const K16Slot* __restrict__ slots, const int32_t* __restrict__ flag,
                         const int32_t* __restrict__ koff, const int32_t* __restrict__ crank, int32_t* __restrict__ row_site,
                         unsigned long long* __restrict__ n_assigned) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t n = 0;
  if (p < n_part) {
    const K16Row row = rows[p];
#pragma unroll
    for (int d = 0; d < 2; d++) {
      const int sl = row.slot[d];
      const int to = sl >= 0 ? slots[sl].to : -1;   // (an end always finds a slot: the guard keeps a broken table from indexing)
      const int j = (to >= 0 && flag[to]) ? crank[koff[to]] : -1;
      rows[p].site[d] = j;
      if (j >= 0) { row_site[2 * (size_t)row.frow + d] = j; n++; }
    }
  }
  n = wave_sum_u32(n);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(n_assigned, (unsigned long long)n);
}

__global__ void k16_export(int32_t n_words, const int32_t* __restrict__ row_site, int32_t* __restrict__ host_row_site,
                           const unsigned long long* __restrict__ n_assigned, unsigned long long* __restrict__ host_n_assigned) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0) *host_n_assigned = *n_assigned;
  if (r < n_words) host_row_site[r] = row_site[r];
}

// One workgroup per kept site (g, t, d, p).  The region's participating rows are sorted by pos: a row with pos > p + W + 1 is neither present
// (both its ends lie right of the window; "+ 1" because the right end of a read without a reference-consuming op is pos - 1) nor absent, and
// those are cut off by a binary search.  The others go through the four-cell sweep of k6_walk.h; presence is asked first.
__global__ void __launch_bounds__(LCR_BLOCK) k16_tables(BatchView b, const int32_t* __restrict__ part_off, const K16Row* __restrict__ rows,
                                                         int32_t window, int32_t n_kept, lcr_end_site* __restrict__ site,
                                                         lcr_end_site* __restrict__ host_site) {
  __shared__ int sh_end;
  const int j = blockIdx.x, tid = threadIdx.x;
  if (j >= n_kept) return;
  const lcr_end_site rec = site[j];
  const int g = rec.region, strand = rec.strand, d = rec.side;
  const long long lo_w = rec.peak0 - window, hi_w = rec.peak0 + window;   // the site's window [p - W, p + W]
  const int p0 = part_off[b.read_begin[g]], p1 = part_off[b.read_begin[g + 1]];
  if (tid == 0) {
    int lo = p0, hi = p1;   // first row in [p0, p1) with pos > p + W + 1
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if ((long long)rows[mid].pos > hi_w + 1) hi = mid; else lo = mid + 1; }
    sh_end = lo;
  }
  __syncthreads();
  const K6Cells best = sweep_phase_set_cells(
      rows, p0, sh_end,
      [&](const K16Row& row) {
        return row.strand == strand && ((d ? row.site[1] : row.site[0]) == j || (lo_w >= 0 && (long long)row.pos <= lo_w && (long long)row.rend >= hi_w + 1));
      },
      [&](const K16Row& row) { return (row.hap - 1) * 2 + ((d ? row.site[1] : row.site[0]) == j ? 1 : 0); });
  if (tid == 0) {
    lcr_end_site o = rec;
    o.phase_set = best.ps; o.n_phase_sets = best.n_sets;
    o.h1_absent = best.n[0]; o.h1_present = best.n[1]; o.h2_absent = best.n[2]; o.h2_present = best.n[3];
    site[j] = o; host_site[j] = o;
  }
}

}  // namespace

// ---- launchers (every one guards against a zero size) ------------------------------------------------------------------------
void launch_k16_count(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, uint32_t strand_mode, int32_t* part_flag, hipStream_t s) {
  if (b.n_reads > 0) hipLaunchKernelGGL(k16_count, dim3((b.n_reads + 255) / 256), dim3(256), 0, s, b, row_region_off, rec, strand_mode, part_flag);
}
void launch_k16_sizes(const BatchView& b, const int32_t* part_off, int32_t* tsz, int32_t* host_ctl, hipStream_t s) {
  hipLaunchKernelGGL(k16_sizes, dim3((std::max(b.n_regions, 1) + 255) / 256), dim3(256), 0, s, b.read_begin, b.n_regions, b.n_reads, part_off, tsz, host_ctl);
}
size_t launch_k16_row_bytes() { return sizeof(K16Row); }
size_t launch_k16_slot_bytes() { return sizeof(K16Slot); }
void launch_k16_walk(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, uint32_t strand_mode, uint32_t hash_mask,
                     const int32_t* part_flag, const int32_t* part_off, const int32_t* tbl_off, void* rows, uint64_t* tbl_key, uint32_t* tbl_cnt, hipStream_t s) {
  if (b.n_reads <= 0) return;
  const long long threads = (long long)b.n_reads * 16;
  hipLaunchKernelGGL(k16_walk, dim3((unsigned)((threads + LCR_BLOCK - 1) / LCR_BLOCK)), dim3(LCR_BLOCK), 0, s, b, row_region_off, rec, strand_mode, hash_mask,
                     part_flag, part_off, tbl_off, (K16Row*)rows, (unsigned long long*)tbl_key, tbl_cnt);
}
void launch_k16_peaks(const uint64_t* tbl_key, const uint32_t* tbl_cnt, const int32_t* tbl_off, int32_t ng, int32_t n_slots, uint32_t window,
                      uint32_t hash_mask, void* slots, hipStream_t s) {
  if (n_slots <= 0) return;
  hipLaunchKernelGGL(k16_peaks, dim3((n_slots + 255) / 256), dim3(256), 0, s, (const unsigned long long*)tbl_key, tbl_cnt, tbl_off, ng, n_slots,
                     (int32_t)window, hash_mask, (K16Slot*)slots);
  hipLaunchKernelGGL(k16_assign, dim3((n_slots + 255) / 256), dim3(256), 0, s, (const unsigned long long*)tbl_key, tbl_cnt, tbl_off, n_slots,
                     (int32_t)window, hash_mask, (K16Slot*)slots);
}
void launch_k16_flag(const void* slots, int32_t n_slots, uint32_t min_count, int32_t* flag, hipStream_t s) {
  if (n_slots > 0) hipLaunchKernelGGL(k16_flag, dim3((n_slots + 255) / 256), dim3(256), 0, s, (const K16Slot*)slots, n_slots, min_count, flag);
}
void launch_k16_offsets(const int32_t* tbl_off, const int32_t* koff, int32_t ng, int32_t n_slots, int32_t* off, int32_t* host_off, int32_t* host_ctl,
                        hipStream_t s) {
  hipLaunchKernelGGL(k16_offsets, dim3((ng + 1 + 255) / 256), dim3(256), 0, s, tbl_off, koff, ng, n_slots, off, host_off, host_ctl);
}
void launch_k16_place(const uint64_t* tbl_key, const void* slots, const int32_t* flag, const int32_t* koff, int32_t n_slots, const int32_t* off,
                      int32_t n_kept, int32_t* cslot, int32_t* crank, lcr_end_site* site, hipStream_t s) {
  if (n_slots <= 0 || n_kept <= 0) return;
  hipLaunchKernelGGL(k16_compact, dim3((n_slots + 255) / 256), dim3(256), 0, s, flag, koff, n_slots, cslot);
  hipLaunchKernelGGL(k16_rank, dim3((n_kept + 255) / 256), dim3(256), 0, s, (const unsigned long long*)tbl_key, (const K16Slot*)slots, cslot, off, n_kept,
                     site, crank);
}
void launch_k16_rows(int32_t n_part, void* rows, const void* slots, const int32_t* flag, const int32_t* koff, const int32_t* crank, int32_t* row_site,
                     uint64_t* n_assigned, hipStream_t s) {
  if (n_part <= 0) return;
  hipLaunchKernelGGL(k16_rows, dim3((n_part + 255) / 256), dim3(256), 0, s, n_part, (K16Row*)rows, (const K16Slot*)slots, flag, koff, crank, row_site,
                     (unsigned long long*)n_assigned);
}
void launch_k16_export(int32_t n_rows, const int32_t* row_site, int32_t* host_row_site, const uint64_t* n_assigned, uint64_t* host_n_assigned, hipStream_t s) {
  const int32_t n_words = 2 * n_rows;
  hipLaunchKernelGGL(k16_export, dim3((std::max(n_words, 1) + 255) / 256), dim3(256), 0, s, n_words, row_site, host_row_site,
                     (const unsigned long long*)n_assigned, (unsigned long long*)host_n_assigned);
}
void launch_k16_tables(const BatchView& b, const int32_t* part_off, const void* rows, uint32_t window, int32_t n_kept, lcr_end_site* site,
                       lcr_end_site* host_site, hipStream_t s) {
  if (n_kept <= 0) return;
  hipLaunchKernelGGL(k16_tables, dim3(n_kept), dim3(LCR_BLOCK), 0, s, b, part_off, (const K16Row*)rows, (int32_t)window, n_kept, site, host_site);
}

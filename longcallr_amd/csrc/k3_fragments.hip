// k3_fragments.hip — K3: read x SNP fragment matrix in CSR (gfx950).
//
// Replaces SNPFrag::get_fragments (reference src/fragment.rs:10-309): per read one CIGAR walk against
// the region's candidates (sorted by position), sixteen lanes per read.  Two passes (count -> scan -> fill)
// give a canonical CSR: row = k-th read of the region that starts at or before the last candidate
// (fragment.rs:51-54, empty rows included), columns ascending.  Entry = (candidate index, u8 value
// q5 | p-bit | base code).  Entries with p = 0 or at dense candidates are dropped (fragment.rs:148).
#include "lcr_dev.h"

// rows per region and the first row of every region in one launch: a thread per region finds its rows (the reads with pos <= the last
// candidate's; reads are sorted by pos), then the exclusive prefix sums -- one workgroup that takes the regions 1 024 at a time, so that
// lcr_fragments starts without an upload
__global__ void __launch_bounds__(1024) k3_rows_offsets(BatchView b, const lcr_candidate* __restrict__ cand, const int32_t* __restrict__ cand_region_off,
                                                        int32_t* __restrict__ region_rows, int32_t* __restrict__ row_region_off, int32_t* __restrict__ host_rows) {
  __shared__ int wsum[16];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ng = b.n_regions;
  if (tid == 0) { base_s = 0; row_region_off[0] = 0; }
  __syncthreads();
  for (int g0 = 0; g0 < ng; g0 += 1024) {
    const int g = g0 + tid;
    int rows = 0;
    if (g < ng) {
      const int c0 = cand_region_off[g], c1 = cand_region_off[g + 1];
      if (c1 > c0) {   // fragment.rs:24-26, 51-54: reads with pos <= the last candidate's (reads are sorted by pos)
        const int64_t last = cand[c1 - 1].pos;
        int lo = b.read_begin[g], hi = b.read_begin[g + 1];
        const int rb = lo;
        // (a search with fifteen pivots a step, loaded together -- three dependent loads for a thousand reads where this one has ten --
        // took 26.5 us on C3 against 12.1: profiles/cand_frag_ab.txt)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int64_t)b.pos[mid] > last) hi = mid; else lo = mid + 1; }
        rows = lo - rb;
      }
      region_rows[g] = rows;
      if (host_rows) host_rows[g] = rows;
    }
    const int incl = wave_incl_scan(rows);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = base_s;
    for (int w = 0; w < wave; w++) before += wsum[w];
    if (g < ng) row_region_off[g + 1] = before + incl;
    __syncthreads();
    if (tid == 1023) base_s = before + incl;
    __syncthreads();
  }
}
void launch_k3_rows_offsets(const BatchView& b, const lcr_candidate* cand, const int32_t* cand_region_off, int32_t* region_rows, int32_t* row_region_off,
                            hipStream_t s, int32_t* host_rows) {
  hipLaunchKernelGGL(k3_rows_offsets, dim3(1), dim3(1024), 0, s, b, cand, cand_region_off, region_rows, row_region_off, host_rows);
}

// first entry of every region: row_ptr at the regions' first rows ([ng] = all entries)
__global__ void k3_region_entries(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ row_region_off, int32_t ng,
                                  int64_t* __restrict__ region_e_off, int64_t* __restrict__ host_out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g <= ng) { const int64_t v = row_ptr[row_region_off[g]]; region_e_off[g] = v; if (host_out) host_out[g] = v; }
}
void launch_k3_region_entries(const int64_t* row_ptr, const int32_t* row_region_off, int32_t ng, int64_t* region_e_off, hipStream_t s, int64_t* host_out) {
  hipLaunchKernelGGL(k3_region_entries, dim3((ng + 256) / 256), dim3(256), 0, s, row_ptr, row_region_off, ng, region_e_off, host_out);
}

// Sixteen lanes per row (row16_walk_sites, lcr_dev.h): the region's candidates inside the read's reference
// span are located against the CIGAR spread over the lanes; a row without such candidates never loads
// its CIGAR.  No trimming here: the reference's fragment walk takes every aligned base.
// The count pass keeps the first K3_INLINE entries of every row in a provisional per-row slot (most rows have
// fewer: a read crosses a handful of candidates), so the second pass is a copy for those rows (k3_place) and
// only longer rows are walked again (FILL: rows with more than K3_INLINE entries).
#define K3_INLINE 16
static_assert(K3_INLINE == LCR_HITS, "a row's provisional slot holds what k2_hist's hit list holds");
// one read (sixteen lanes) of the walk; `live` rows only do work
template <bool FILL>
__device__ __forceinline__ void k3_walk_read(const BatchView& b, const ReadBin* __restrict__ rbin, const lcr_candidate* __restrict__ cand,
        const int32_t* __restrict__ cand_region_off, const int32_t* __restrict__ row_region_off, int r_, bool live_in,
        int32_t* __restrict__ row_cnt, uint32_t* __restrict__ row_links, const int64_t* __restrict__ row_ptr,
        int32_t* __restrict__ col, uint8_t* __restrict__ val) {
  // rows are the first region_rows[g] reads of each region: index by read (one load for the region)
  const int r = (live_in && r_ < b.n_reads) ? r_ : 0;
  const int g = region_of_read(b, r);
  const int k = r - b.read_begin[g];
  const int row0 = row_region_off[g];
  bool live = live_in && r_ < b.n_reads && k < row_region_off[g + 1] - row0;
  const int row = live ? row0 + k : 0;
  if (FILL) {   // shorter rows were placed from their provisional slots: most waves have nothing left to do
    live = live && row_cnt[row] > K3_INLINE;
    if (!__any(live)) return;
  }
  const int l16 = threadIdx.x & 15;
  const int c_lo = cand_region_off[g], c_hi = cand_region_off[g + 1];
  const ReadBin h = rbin[r];
  const int64_t start0 = b.start0[g];
  const uint8_t* __restrict__ seq = b.bases + h.seq_off;
  const uint8_t* __restrict__ qual = b.quals + h.seq_off;
  int cnt = 0;
  uint32_t links = 0;
  // FILL: final position of the row's entries; count pass: the row's provisional slot
  int64_t w = FILL ? row_ptr[row] : (int64_t)row * K3_INLINE;
  const int rbase = threadIdx.x & 48;
  row16_walk_sites(b, live, h, b.read_rend[r], c_lo, c_hi,
    [&](int i) { return (int)(cand[i].pos - start0); },
    [&](int idx, int qq, bool hit) {   // lane <-> candidate; entries keep the candidates' order
      int p = 0; uint8_t base = 0; bool fphase = false;
      if (hit) {
        const lcr_candidate& c = cand[idx];
        base = seq[qq];
        if (base == c.ref_base) p = 1;                                                // fragment.rs:134-135
        else if (base == c.allele1 || base == c.allele2) p = -1;                      // fragment.rs:136-140
        if (c.flags & LCR_F_DENSE) p = 0;                                             // fragment.rs:148-152
        fphase = (c.flags & LCR_F_FOR_PHASING) != 0;                                  // fragment.rs:144-146,242-250
      }
      const unsigned int em = (unsigned int)(__ballot(p != 0) >> rbase) & 0xffffu;
      const unsigned int ph = (unsigned int)(__ballot(p != 0 && fphase) >> rbase) & 0xffffu;
      if (p != 0) {
        const int at = cnt + __popc(em & ((1u << l16) - 1u));
        if (FILL || at < K3_INLINE) {
          const uint8_t bq = qual[qq] < 30 ? qual[qq] : 30;                            // fragment.rs:127-131
          col[w + at] = idx;
          val[w + at] = (uint8_t)(bq | (p == 1 ? 32 : 0) | (base_code(base) << 6));
        }
      }
      cnt += __popc(em); links += __popc(ph);
    });
  if (!FILL && live && l16 == 0) { row_cnt[row] = cnt; row_links[row] = links; }
}
// every read of the batch (batches without hit lists: the dense-survivor path of lcr_candidates)
template <bool FILL>
__global__ void __launch_bounds__(LCR_BLOCK)
k3_walk(BatchView b, const ReadBin* __restrict__ rbin, const lcr_candidate* __restrict__ cand,
        const int32_t* __restrict__ cand_region_off, const int32_t* __restrict__ row_region_off, int32_t n_rows,
        int32_t* __restrict__ row_cnt, uint32_t* __restrict__ row_links, const int64_t* __restrict__ row_ptr,
        int32_t* __restrict__ col, uint8_t* __restrict__ val) {
  k3_walk_read<FILL>(b, rbin, cand, cand_region_off, row_region_off, (int)((blockIdx.x * LCR_BLOCK + threadIdx.x) >> 4), true, row_cnt, row_links, row_ptr, col, val);
}
// the reads of a list (those with more hits than k2_hist's list holds): the list role of a pass kernel (k3_count / k3_fill below), `nblk`
// workgroups of which this is workgroup `blk`, walk it with a stride
template <bool FILL>
__device__ __forceinline__ void k3_walk_list(const BatchView& b, const ReadBin* __restrict__ rbin, const lcr_candidate* __restrict__ cand,
             const int32_t* __restrict__ cand_region_off, const int32_t* __restrict__ row_region_off, const int32_t* __restrict__ n_list,
             const int32_t* __restrict__ list, int blk, int nblk, int32_t* __restrict__ row_cnt, uint32_t* __restrict__ row_links, const int64_t* __restrict__ row_ptr,
             int32_t* __restrict__ col, uint8_t* __restrict__ val) {
  const int n = *n_list, per = LCR_BLOCK / 16;
  for (int i0 = blk * per; i0 < n; i0 += nblk * per) {   // (uniform over the workgroup; the waves' rows differ)
    const int i = i0 + (int)(threadIdx.x >> 4);
    const int w0 = i0 + (int)((threadIdx.x >> 6) << 2);   // first list index of this wave
    if (w0 >= n) continue;                                 // (wave-uniform)
    k3_walk_read<FILL>(b, rbin, cand, cand_region_off, row_region_off, i < n ? list[i] : 0, i < n, row_cnt, row_links, row_ptr, col, val);
  }
}

// Count pass from k2_hist's hit lists: a row's entries are its hits at survivors that became candidates, in the same order --
// no CIGAR is read.  Sixteen lanes per read, lane <-> hit; reads with more hits than the list holds are left to the list role.
// The kernel is a handful of loads per row in three dependent levels (hit count, hits, region | keep, candidate slot, region's reads and
// rows | candidate record): a sixteen-lane group takes K3_R consecutive reads and asks for every load of a level, for all of them,
// before it uses the first value of that level.  (Worth 3 us of 47 on C3: the rest is not the chain's latency.)
#define K3_R 2   // (C3, the count pass with its list role: one read per group 47.0 us, two 43.9, four 42.4 with three times the spread)
__device__ __forceinline__ void k3_hits(const BatchView& b, const lcr_candidate* __restrict__ cand, const int32_t* __restrict__ row_region_off, const int32_t* __restrict__ hit_cnt,
        const uint2* __restrict__ hit_list, const int32_t* __restrict__ keep, const int32_t* __restrict__ pos, int blk,
        int32_t* __restrict__ row_cnt, uint32_t* __restrict__ row_links, int32_t* __restrict__ col, uint8_t* __restrict__ val) {
  const int r0 = (int)(((unsigned)blk * LCR_BLOCK + threadIdx.x) >> 4) * K3_R;
  const int l16 = threadIdx.x & 15, rbase = threadIdx.x & 48;
  bool in[K3_R]; int r[K3_R], nh[K3_R], g[K3_R]; uint2 hv[K3_R];
#pragma unroll
  for (int j = 0; j < K3_R; j++) {   // level 1
    in[j] = r0 + j < b.n_reads;
    r[j] = in[j] ? r0 + j : 0;
    nh[j] = hit_cnt[r[j]];
    hv[j] = hit_list[(size_t)r[j] * LCR_HITS + l16];   // (slots beyond nh hold stale values: used only below nh)
    g[j] = region_of_read(b, r[j]);
  }
  bool has[K3_R]; int kp[K3_R], idx[K3_R], rb[K3_R], row0[K3_R], row1[K3_R];
#pragma unroll
  for (int j = 0; j < K3_R; j++) {   // level 2
    has[j] = in[j] && nh[j] <= LCR_HITS && l16 < nh[j];
    // (lanes without a hit read survivor 0 and, below, candidate slot 0 -- hit lists mean at least one survivor, and the records' buffer
    // holds a slot per survivor: a load under a branch would be waited for inside it, one row after the other)
    const uint32_t sx = has[j] ? hv[j].x : 0u;
    const int kv = keep[sx], pv = pos[sx];
    kp[j] = has[j] ? kv : 0;
    idx[j] = has[j] ? pv : 0;
    rb[j] = b.read_begin[g[j]];
    row0[j] = row_region_off[g[j]];
    row1[j] = row_region_off[g[j] + 1];
  }
  uint32_t ca[K3_R], cf[K3_R];   // ref_base | allele1 << 8 | allele2 << 16 | n_alt << 24 (one word of the record), flags
#pragma unroll
  for (int j = 0; j < K3_R; j++) {   // level 3
    static_assert(offsetof(lcr_candidate, allele1) == offsetof(lcr_candidate, ref_base) + 1 && offsetof(lcr_candidate, allele2) == offsetof(lcr_candidate, ref_base) + 2 &&
                  offsetof(lcr_candidate, ref_base) % 4 == 0, "ref_base, allele1 and allele2 share an aligned word");
    const lcr_candidate& c = cand[kp[j] ? idx[j] : 0];
    ca[j] = *reinterpret_cast<const uint32_t*>(&c.ref_base);
    cf[j] = c.flags;
  }
#pragma unroll
  for (int j = 0; j < K3_R; j++) {
    const int k = r[j] - rb[j];
    const bool live = in[j] & (k < row1[j] - row0[j]) & (nh[j] <= LCR_HITS);   // (no short circuit: nothing to load behind a branch)
    const int row = live ? row0[j] + k : 0;
    int p = 0; uint8_t base = 0, rq = 0; bool fphase = false;
    if (has[j] && kp[j]) {
      base = (uint8_t)(hv[j].y & 0xffu); rq = (uint8_t)((hv[j].y >> 8) & 0xffu);
      if (base == (uint8_t)(ca[j] & 0xffu)) p = 1;                                                          // fragment.rs:134-135
      else if (base == (uint8_t)((ca[j] >> 8) & 0xffu) || base == (uint8_t)((ca[j] >> 16) & 0xffu)) p = -1;  // fragment.rs:136-140
      if (cf[j] & LCR_F_DENSE) p = 0;                                                                       // fragment.rs:148-152
      fphase = (cf[j] & LCR_F_FOR_PHASING) != 0;                                                            // fragment.rs:144-146,242-250
    }
    if (!live) p = 0;   // (a read behind the region's last candidate has no row: fragment.rs:51-54)
    const unsigned int em = (unsigned int)(__ballot(p != 0) >> rbase) & 0xffffu;
    const unsigned int ph = (unsigned int)(__ballot(p != 0 && fphase) >> rbase) & 0xffffu;
    if (p != 0) {
      const int64_t at = (int64_t)row * K3_INLINE + __popc(em & ((1u << l16) - 1u));
      const uint8_t bq = rq < 30 ? rq : 30;                                            // fragment.rs:127-131
      col[at] = idx[j];
      val[at] = (uint8_t)(bq | (p == 1 ? 32 : 0) | (base_code(base) << 6));
    }
    if (live && l16 == 0) { row_cnt[row] = __popc(em); row_links[row] = __popc(ph); }
  }
}

// rows with at most K3_INLINE entries: provisional slot -> final CSR position (one thread per row)
__device__ __forceinline__ void k3_place(int32_t n_rows, const int32_t* __restrict__ row_cnt, const int64_t* __restrict__ row_ptr,
         const int32_t* __restrict__ tmp_col, const uint8_t* __restrict__ tmp_val, int blk, int32_t* __restrict__ col, uint8_t* __restrict__ val) {
  const int row = blk * LCR_BLOCK + threadIdx.x;
  if (row >= n_rows) return;
  const int n = row_cnt[row];
  if (n > K3_INLINE) return;
  const int64_t at = row_ptr[row], from = (int64_t)row * K3_INLINE;
  for (int e = 0; e < n; e++) { col[at + e] = tmp_col[from + e]; val[at + e] = tmp_val[from + e]; }
}

// A pass of a batch with hit lists is ONE launch: its first `list_blocks` workgroups walk the reads of the overflow list, the others take
// k3_hits (count pass) / k3_place (fill pass).  The two roles write different rows -- a read is on the list exactly if it has more than
// LCR_HITS hits -- so nothing orders them, and the latency-bound walk runs beside the other role instead of behind it in the queue.
__global__ void __launch_bounds__(LCR_BLOCK)
k3_count(BatchView b, const ReadBin* __restrict__ rbin, const lcr_candidate* __restrict__ cand, const int32_t* __restrict__ cand_region_off,
         const int32_t* __restrict__ row_region_off, K3Hits hits, int list_blocks, int32_t* __restrict__ row_cnt, uint32_t* __restrict__ row_links,
         int32_t* __restrict__ col, uint8_t* __restrict__ val) {
  if ((int)blockIdx.x < list_blocks)
    k3_walk_list<false>(b, rbin, cand, cand_region_off, row_region_off, hits.ovf_cnt, hits.ovf_list, (int)blockIdx.x, list_blocks, row_cnt, row_links, nullptr, col, val);
  else
    k3_hits(b, cand, row_region_off, hits.hit_cnt, (const uint2*)hits.hit_list, hits.keep, hits.pos, (int)blockIdx.x - list_blocks, row_cnt, row_links, col, val);
}
__global__ void __launch_bounds__(LCR_BLOCK)
k3_fill(BatchView b, const ReadBin* __restrict__ rbin, const lcr_candidate* __restrict__ cand, const int32_t* __restrict__ cand_region_off,
        const int32_t* __restrict__ row_region_off, K3Hits hits, int list_blocks, int32_t n_rows, int32_t* __restrict__ row_cnt, const int64_t* __restrict__ row_ptr,
        const int32_t* __restrict__ tmp_col, const uint8_t* __restrict__ tmp_val, int32_t* __restrict__ col, uint8_t* __restrict__ val) {
  if ((int)blockIdx.x < list_blocks)
    k3_walk_list<true>(b, rbin, cand, cand_region_off, row_region_off, hits.ovf_cnt, hits.ovf_list, (int)blockIdx.x, list_blocks, row_cnt, nullptr, row_ptr, col, val);
  else
    k3_place(n_rows, row_cnt, row_ptr, tmp_col, tmp_val, (int)blockIdx.x - list_blocks, col, val);
}
// a batch without hit lists: rows of at most K3_INLINE entries from their slots, then k3_walk<true> for the others
__global__ void __launch_bounds__(LCR_BLOCK)
k3_place_rows(int32_t n_rows, const int32_t* __restrict__ row_cnt, const int64_t* __restrict__ row_ptr,
              const int32_t* __restrict__ tmp_col, const uint8_t* __restrict__ tmp_val, int32_t* __restrict__ col, uint8_t* __restrict__ val) {
  k3_place(n_rows, row_cnt, row_ptr, tmp_col, tmp_val, (int)blockIdx.x, col, val);
}

// Workgroups of the list role.  The list holds the reads with more than LCR_HITS survivor hits (C3: 1.7e4 of 4.4e5); nobody on the host
// knows its length when the pass is queued, so the role is sized for a list of one read in K3_LIST_SHARE and strides over a longer one
// (C3: 433 workgroups, two or three turns each; the count pass took 78 us with 128, 54 with 256, 44 with 433 and with 1 024).
#define K3_LIST_SHARE 64
#define K3_LIST_BLOCKS_MAX 512
static int k3_list_blocks(int32_t n_reads, int forced) {
  if (forced > 0) return forced;
  const int per = LCR_BLOCK / 16;
  return std::max(1, std::min(K3_LIST_BLOCKS_MAX, (n_reads / K3_LIST_SHARE + per - 1) / per));
}

void launch_k3_count(const BatchView& b, const ReadBin* rbin, const lcr_candidate* cand, const int32_t* cand_region_off,
                     const int32_t* row_region_off, int32_t n_rows, int32_t* row_cnt, uint32_t* row_links, int32_t* tmp_col,
                     uint8_t* tmp_val, const K3Hits& hits, int list_blocks, hipStream_t s) {
  if (n_rows == 0) return;
  const int per = LCR_BLOCK / 16;
  if (hits.hit_cnt) {
    const int lb = k3_list_blocks(b.n_reads, list_blocks), groups = (b.n_reads + K3_R - 1) / K3_R;
    hipLaunchKernelGGL(k3_count, dim3(lb + (groups + per - 1) / per), dim3(LCR_BLOCK), 0, s, b, rbin, cand, cand_region_off, row_region_off, hits, lb,
                       row_cnt, row_links, tmp_col, tmp_val);
    return;
  }
  hipLaunchKernelGGL(k3_walk<false>, dim3((b.n_reads + per - 1) / per), dim3(LCR_BLOCK), 0, s, b, rbin, cand,
                     cand_region_off, row_region_off, n_rows, row_cnt, row_links, (const int64_t*)nullptr, tmp_col, tmp_val);
}
void launch_k3_fill(const BatchView& b, const ReadBin* rbin, const lcr_candidate* cand, const int32_t* cand_region_off,
                    const int32_t* row_region_off, int32_t n_rows, int32_t* row_cnt, const int64_t* row_ptr, const int32_t* tmp_col,
                    const uint8_t* tmp_val, int32_t* col, uint8_t* val, const K3Hits& hits, int list_blocks, hipStream_t s) {
  if (n_rows == 0) return;
  const int per = LCR_BLOCK / 16, place_blocks = (n_rows + LCR_BLOCK - 1) / LCR_BLOCK;
  if (hits.hit_cnt) {   // (a row of more than K3_INLINE entries has more than LCR_HITS hits: it is on the list)
    const int lb = k3_list_blocks(b.n_reads, list_blocks);
    hipLaunchKernelGGL(k3_fill, dim3(lb + place_blocks), dim3(LCR_BLOCK), 0, s, b, rbin, cand, cand_region_off, row_region_off, hits, lb, n_rows,
                       row_cnt, row_ptr, tmp_col, tmp_val, col, val);
    return;
  }
  hipLaunchKernelGGL(k3_place_rows, dim3(place_blocks), dim3(LCR_BLOCK), 0, s, n_rows, row_cnt, row_ptr, tmp_col, tmp_val, col, val);
  hipLaunchKernelGGL(k3_walk<true>, dim3((b.n_reads + per - 1) / per), dim3(LCR_BLOCK), 0, s, b, rbin, cand,
                     cand_region_off, row_region_off, n_rows, row_cnt, (uint32_t*)nullptr, row_ptr, col, val);
}
int launch_k3_inline() { return K3_INLINE; }

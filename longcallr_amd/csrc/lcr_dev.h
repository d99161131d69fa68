// lcr_dev.h — shared host/device declarations of liblcr (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cstddef>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/lcr.h"

#ifndef LCR_TILE
#define LCR_TILE 256       // pileup columns per workgroup tile (512: K1 0.385 instead of 0.334 ms on C3, K0 0.23 = 0.24)
#endif
#define LCR_BLOCK 256      // threads per workgroup (4 wave64)
#define LCR_WAVE 64

// Device view of a bound batch (all pointers in HBM).
struct BatchView {
  int32_t n_reads, n_regions;
  int64_t n_bases;           // bytes in bases / quals
  const int32_t* pos;
  const int32_t* seq_len;
  const int32_t* lead;
  const int32_t* trail;
  const uint8_t* flags;
  const uint64_t* seq_off;
  const uint64_t* cig_off;
  const uint32_t* n_cig;
  const uint8_t* bases;
  const uint8_t* quals;
  const uint32_t* cigar;
  const int64_t* start0;
  const int32_t* len;
  const int64_t* col_off;
  const int32_t* read_begin;
  const uint8_t* ref;
  // derived by K0 (lcr_load_batch)
  const int32_t* region_first_tile;  // n_regions+1: first pileup tile of each region
  const int32_t* read_region;        // n_reads: region index of each read
  int32_t* error_flag;               // != 0 -> unknown CIGAR op seen
  int32_t* read_rend;                // n_reads: region-relative column one past the read's last reference base (K0 pass 0)
  // lcr_set_exon_mask: one bit per global column (k2_eval.h: exon_bit), or nullptr = no mask; read by pass 1 of the candidate filters only
  const uint32_t* exon_mask;
};

// Per-read header packed once per batch (k0_pack) so that K0 needs a single 64-byte load per read.
struct ReadBin {
  int32_t rel_pos;     // pos - start0[region]
  int32_t vec;         // region length in columns
  int32_t ftile;       // first tile of the region
  int32_t n_cig;
  int64_t gbase;       // col_off[region] + region (slot base in the intron difference array)
  uint64_t seq_off, cig_off;
  int32_t lead, reb;   // leading soft clip, seq_len - trailing soft clip
  int32_t flags, pad_;
  int64_t pad2_;
};
static_assert(sizeof(ReadBin) == 64, "ReadBin must be 64 bytes");

struct DevParams {
  int32_t ont;
  int32_t dist_to_end, polya_len;
  uint32_t min_baseq, min_depth, max_depth, min_qual, low_cnt_cut, min_linkers;
  int32_t use_strand_bias;
  float min_af, min_af_intron, low_frac_cut;
  float sor_threshold;
  int32_t dbg;  // (unused; the K1 ablation switches are compile-time, see k1_pileup.hip)
};

// K0's per-tile records (k0_ops.hip writes them, k1_pileup.hip and k2_hist_tiles read them), 64 bit:
// [0,40) byte offset of the first read base | [40,48) tile column | [48,56) length-1 | [56] REC_F_INS | [57] REC_F_DEL | [58,60) spare |
// [60] reverse strand | [61,63) transcript-strand class (0 none, 1 -> [0], 2 -> [1]); D / I / N records carry a marker in the offset field.
// The two flags are set on M records only (k0_ops.hip, "fold"): a 1-base indel that directly follows an M op of its read is not a record of
// its own but a flag of that op's record in its last tile --
//   REC_F_INS  one insertion point counted on the record's last column            (the I record it replaces: column col + len - 1)
//   REC_F_DEL  a deletion of length 1 on the column behind the record's last one  (the D record it replaces: column col + len, length 1;
//              K0 folds only where that column lies in the same tile)
// Every reader goes through the accessors below.
static_assert(LCR_TILE <= 256, "a record keeps its tile column and its length - 1 in 8 bits each");
#define REC_OFF_MASK 0xFFFFFFFFFFull
#define REC_KIND_D 0xFFFFFFFFFFull  // offset field of a D-run record
#define REC_KIND_I 0xFFFFFFFFFEull  // offset field of an I-point record
#define REC_KIND_N 0xFFFFFFFFFDull  // offset field of an N-run record (the part of an intron inside its first / last tile)
// the fields above bit 32 as K0 assembles them in a record's high word
#define REC_HI_COL_SHIFT 8
#define REC_HI_LEN_SHIFT 16
#define REC_HI_F_INS (1u << 24)
#define REC_HI_F_DEL (1u << 25)
#define REC_HI_STRAND_SHIFT 28
#define REC_HI_TS_SHIFT 29
#define REC_F_INS ((unsigned long long)REC_HI_F_INS << 32)
#define REC_F_DEL ((unsigned long long)REC_HI_F_DEL << 32)
#ifdef __HIPCC__
__device__ __forceinline__ unsigned long long rec_off(unsigned long long rec) { return rec & REC_OFF_MASK; }
__device__ __forceinline__ int rec_col(unsigned long long rec) { return (int)((uint32_t)(rec >> 40) & 255u); }
__device__ __forceinline__ int rec_len(unsigned long long rec) { return (int)((uint32_t)(rec >> 48) & 255u) + 1; }
__device__ __forceinline__ int rec_strand(unsigned long long rec) { return (int)((uint32_t)(rec >> 60) & 1u); }
__device__ __forceinline__ int rec_tscls(unsigned long long rec) { return (int)((uint32_t)(rec >> 61) & 3u); }
__device__ __forceinline__ bool rec_f_ins(unsigned long long rec) { return (rec & REC_F_INS) != 0; }
__device__ __forceinline__ bool rec_f_del(unsigned long long rec) { return (rec & REC_F_DEL) != 0; }
// kind of a record: 1 M-segment, 2 D-run, 3 I-point, 4 N-run (K0's numbering); an M-segment is whatever carries no marker
__device__ __forceinline__ bool rec_is_m(unsigned long long rec) { return rec_off(rec) < REC_KIND_N; }
__device__ __forceinline__ int rec_kind(unsigned long long rec) {
  const unsigned long long off = rec_off(rec);
  return off == REC_KIND_D ? 2 : off == REC_KIND_I ? 3 : off == REC_KIND_N ? 4 : 1;
}
#endif

// pass-1 survivor of the candidate filters (one per column that reaches the likelihood block)
struct Survivor {
  int64_t gcol;      // global column index (col_off[region] + column)
  int32_t region;
  int32_t col;       // column inside region
  uint8_t ref_base, allele1, allele2, n_alt;
  uint32_t cnt1, cnt2, depth;
  uint32_t ts_fwd, ts_rev;
  float af1, af2;
};

#define HIPCHK(ctx, expr)                                                              \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) {                                                            \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                  \
      return LCR_E_DEVICE;                                                             \
    }                                                                                  \
  } while (0)

// Process-wide cache of the blocks contexts give back (lcr_api.hip).  A context that is destroyed hands its device and page-locked
// buffers to the cache, the next context on that device takes them from there: a worker that recreates its context per task does not
// churn hipMalloc / hipFree (GBs per context), and -- profiles/r06_stall.txt -- a context created right behind a large upload no longer
// loses 65-85 ms in its first steps.  Bounded (LCR_CACHE_DEV_BYTES / LCR_CACHE_HOST_BYTES per device, beyond that blocks are freed);
// lcr_release_cached_memory() returns everything to the runtime.
void* lcr_cache_take(int host, size_t want, size_t* cap);   // a cached block with want <= cap <= 2 * want + 1 MiB of the current device, or nullptr
bool lcr_cache_put(int host, void* p, size_t cap);          // false: the cache is full, the caller frees the block

// Measurement aid (lcr_debug_set("host_trace", 1)): wall-clock marks of the calling thread inside the stage calls, printed to stderr by
// lcr_host_trace_flush (end of lcr_phase) as microseconds since the first mark -- where does the host wait, when does it queue what.
extern int g_lcr_host_trace;
void lcr_host_trace_mark(const char* tag);
void lcr_host_trace_flush();
#define HT(tag) do { if (g_lcr_host_trace) lcr_host_trace_mark(tag); } while (0)

// Byte fill on a stream by a kernel of the library's own (the same contract as hipMemsetAsync for device memory).  The runtime's fill is a blit
// kernel too, but behind an event record it starts 35 - 57 us late on this platform (profiles/r06_timeline.txt); lcr_debug_set("own_fill", 0)
// goes back to hipMemsetAsync.
extern int g_lcr_own_fill;
hipError_t lcr_fill_async(void* p, int byte, size_t bytes, hipStream_t s);
hipError_t lcr_fill_multi_async(int n /* <= 4 */, void* const* ptrs, const int* bytes_val, const size_t* sizes, hipStream_t s);

// Growable buffers that own their block: the destructor gives it back (the owner has drained its queues by then: lcr_ctx_destroy)
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p && !lcr_cache_put(0, p, cap)) (void)hipFree(p); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    // (hipFree waits for the device before it releases a block: so does handing one to the cache -- a kernel in flight may still read it)
    if (p) { (void)hipDeviceSynchronize(); if (!lcr_cache_put(0, p, cap)) (void)hipFree(p); }
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    if ((p = lcr_cache_take(0, want, &cap)) != nullptr) return hipSuccess;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want; else p = nullptr;
    return e;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
struct HostBuf {  // pinned
  void* p = nullptr;
  size_t cap = 0;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete; HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { if (p && !lcr_cache_put(1, p, cap)) (void)hipHostFree(p); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) { (void)hipDeviceSynchronize(); if (!lcr_cache_put(1, p, cap)) (void)hipHostFree(p); }
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    if ((p = lcr_cache_take(1, want, &cap)) != nullptr) return hipSuccess;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want; else p = nullptr;
    return e;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
  // the block as the device sees it: kernels write small results straight into it, no copy in the queue
  template <class T> hipError_t dev(T** out) const { return hipHostGetDevicePointer((void**)out, p, 0); }
};

// ---- phasing LUT (fixed point, scale 2^40; DESIGN.md "Decision arithmetic") ----
struct PhaseLutDev {
  int64_t fe[31], f1e[31];           // log10(eps), log10(1-eps), eps = 10^(-q/10) (q=0 -> q=1)
  int64_t f_homref, f_homvar, f_het0, f_log2;
};

// K0's control block: in HBM inside lcr_pileup's cleared scratch (PileScratch), and once more in pinned host memory, where k1_tiles_a
// leaves the host its copy.  k0_ops raises `error` (1 unknown CIGAR op, 2 CIGAR inconsistent with l_seq / soft clips, 3 pool overflow) and
// every kernel behind it leaves early while it is set; k1_tiles_a fills the other words from K0's accounting slots.
struct K0Ctl {
  unsigned int pool_top, n_items, n_recs;   // slots the fullest pool shard asked for; M / D / I / N items; records
  int32_t error;
  unsigned int desc_top;                    // descriptors the fullest shard asked for
  unsigned int empty_cols;                  // columns of the record-free tiles
  unsigned int pad_[2];
};
static_assert(sizeof(K0Ctl) == 32, "K0Ctl is eight words: the host fetches it with one 32-byte copy");
static_assert(offsetof(K0Ctl, error) == 12, "BatchView::error_flag is word 3 of K0Ctl");

// ---- kernel launchers (defined in the .hip files) ----
void launch_k0_region_setup(const int64_t* start0, const int32_t* len, const int64_t* col_off, const int32_t* read_begin, int32_t ng,
                            int32_t* first_tile, int64_t* h_start0, int32_t* h_len, int64_t* h_col_off, int32_t* h_read_begin,
                            hipStream_t s);
void launch_k0_tiles(const int32_t* first_tile, int32_t n_regions, int32_t* tile_region, int32_t* tile_col0, hipStream_t s);
void launch_k0_read_region(const BatchView& b, int32_t* read_region, hipStream_t s);
void launch_k0_tiles_read_region(const BatchView& b, const int32_t* first_tile, int32_t* tile_region, int32_t* tile_col0, int32_t* read_region, hipStream_t s);   // launch_k0_tiles + launch_k0_read_region in one kernel
void launch_k0_pack(const BatchView& b, ReadBin* out, int32_t* order_flag /* pinned host memory, device address */, hipStream_t s);
void launch_k0_bind_a(const int64_t* start0, const int32_t* len, const int64_t* col_off, const int32_t* read_begin, int32_t ng,
                      int32_t* first_tile, int64_t* h_start0, int32_t* h_len, int64_t* h_col_off, int32_t* h_read_begin,
                      const uint64_t* cig_off, const uint32_t* n_cig, int32_t nr, int64_t n_cigar, int32_t* out, hipStream_t s);
void launch_k0_bind_b(const BatchView& b, ReadBin* rbin, int32_t* order_flag, int32_t* read_region, int32_t n_tiles, int32_t* tile_region,
                      int32_t* tile_col0, uint64_t cig0, int32_t opb, int32_t n_blocks, int32_t* blk_first_read, hipStream_t s);
// k0_unpack.hip: BAM 4-bit bases -> ASCII, one wave per read; no launch for nr == 0.  bad: raised for a read whose ranges leave the arrays (skipped)
void launch_k0_unpack(int32_t nr, const int32_t* seq_len, const uint64_t* seq_off, const uint64_t* pack_off, const uint8_t* seq4, int64_t n_pack,
                      uint8_t* out, int64_t n_bases, int32_t* bad /* pinned host memory, device address */, hipStream_t s);
// K0 (k0_ops.hip): op-parallel CIGAR decode + per-tile record binning; load-time helpers
void launch_k0_cig_check(const uint64_t* cig_off, const uint32_t* n_cig, int32_t nr, int64_t n_cigar, int32_t* out, hipStream_t s);
void launch_k0_cig_compact(const uint32_t* cigar, const uint64_t* cig_off, const uint32_t* n_cig, const int32_t* new_off, int32_t nr,
                           uint32_t* out, uint64_t* out_off, hipStream_t s);
int launch_k0_opb();   // ops per K0 workgroup
void launch_k0_block_reads(const ReadBin* rbin, int32_t nr, uint64_t cig0, int32_t opb, int32_t n_blocks, int32_t* blk_first_read, hipStream_t s);
void launch_k0_ops(const BatchView& b, const ReadBin* rb, const int32_t* blk_first_read, uint64_t cig0, uint32_t n_ops, int ont, int D,
                   int fold /* 1-base indels behind an M op travel as flags of its record (REC_F_INS / REC_F_DEL); 0: every op its own record */,
                   int32_t n_tiles, int32_t* tile_fill, int32_t* tile_nchunks, int32_t* tile_ndiff, K0Ctl* ctl, unsigned int* acct /* launch_k0_acct_words() zeroed words */,
                   unsigned int pool_sub /* slots per shard */, unsigned long long* recs, unsigned int desc_sub, uint32_t* desc_tile, void* desc_val /* uint2 */,
                   void* read_scan /* n_reads x int2 scratch */, hipStream_t s);
int launch_k0_acct_words();
int launch_k0_acct_slots();
void launch_k0_desc_bin(const K0Ctl* ctl, const unsigned int* acct, unsigned int desc_sub, const uint32_t* desc_tile, const void* desc_val,
                        const int32_t* chunk_off, int32_t* cursor /* n_tiles zeroed ints */, void* sorted /* uint2, all shards */, int32_t n_blocks_hint,
                        hipStream_t s);
size_t launch_k1_tiles_tmp_words(int32_t n_tiles);
// lcr_pileup's one cleared buffer (lcr_ctx::k0_tile_fill), in 32-bit words from its start: what K0 and the tile passes count into.  The fill
// counters stay at the start: k2_filter and k2_import_emit take the buffer as their tile_fill.
struct PileScratch {
  size_t ctl;     // K0Ctl (behind the n_tiles fill counters and one spare word)
  size_t ndiff;   // tile-level intron difference array
  size_t nch;     // chunks per tile
  size_t cur;     // bin cursors of k0_desc_bin
  size_t acct;    // K0's accounting slots (launch_k0_acct_words())
  size_t tmp;     // scratch of the tile passes (TileScanTmp: class counts, cursors, n_full; block sums)
  size_t words;   // all of it, a multiple of 256 bytes: one fill kernel, not a body and a tail
};
inline PileScratch pile_scratch(int32_t n_tiles) {
  const size_t nt = (size_t)n_tiles;
  PileScratch L{};
  L.ctl = nt + 1; L.ndiff = nt + 16; L.nch = L.ndiff + nt + 8; L.cur = L.nch + nt + 8; L.acct = L.cur + nt + 8;
  L.tmp = L.acct + launch_k0_acct_words();
  L.words = (L.tmp + launch_k1_tiles_tmp_words(n_tiles) + 63) & ~(size_t)63;
  return L;
}
void launch_k1_tiles_a(int32_t n_tiles, const int32_t* tile_fill, const int32_t* tile_ndiff, const int32_t* tile_nent, int32_t* tmp /* zeroed */,
                       const unsigned int* acct, int32_t n_acct, K0Ctl* ctl, K0Ctl* host_ctl /* pinned host block as the device sees it, or nullptr */,
                       const int32_t* tile_region, const int32_t* tile_col0, const int32_t* region_len /* -> empty_cols of both blocks: columns of the record-free tiles */, hipStream_t s);
void launch_k1_tiles_b(int32_t n_tiles, const int32_t* tile_fill, const int32_t* tile_ndiff, const int32_t* tile_nent, int32_t* tmp,
                       int32_t* tile_nbase, int32_t* ent_off, int32_t* order, int32_t* flt_count /* != nullptr: 0 for every record-free tile */, hipStream_t s);
void launch_k1_pileup(const BatchView& b, const DevParams& p, const int32_t* tile_region, const int32_t* tile_col0,
                      int32_t n_tiles, int64_t n_cols, const int32_t* tile_fill, const int32_t* chunk_off, const void* chunks,
                      const unsigned long long* recs, const int32_t* tile_nbase, uint32_t* planes, const int32_t* order,
                      const int32_t* tiles_tmp /* scratch of launch_k1_tiles_a / _b */, hipStream_t s,
                      uint8_t* flt_flags /* n_cols: != nullptr = pass 1 of the candidate filters in the tally's epilogue (k2_filter's flags) */, int32_t* flt_count /* n_tiles: survivors per tile */);
#define K1_TMP_NFULL 80    // words of the tile passes' scratch (TileScanTmp, k1_pileup.hip): tiles with records ...
#define K1_TMP_STAGED 83   // ... and the survivors the lean tally has staged (exact beyond the staging capacity)
// the tally's lean form (fused-filter presets): no plane and no flag is stored; flt_count as above, and every pass-1 survivor's record in `stage`
// with its (tile, rank in tile) in `stage_key` (int2), in the order the tiles drew their slots -- launch_k2_place orders them
void launch_k1_pileup_lean(const BatchView& b, const DevParams& p, const int32_t* tile_region, const int32_t* tile_col0,
                           int32_t n_tiles, int64_t n_cols, const int32_t* tile_fill, const int32_t* chunk_off, const void* chunks,
                           const unsigned long long* recs, const int32_t* tile_nbase, const int32_t* order, int32_t* tiles_tmp /* zeroed before K0 */, hipStream_t s,
                           int32_t* flt_count, Survivor* stage, void* stage_key, int32_t stage_cap);
// staged record i < min(*n_staged, stage_cap) -> out[tile_off[tile] + rank] (dropped at out_cap and beyond): (tile, column) order whatever the staging order was
void launch_k2_place(const Survivor* stage, const void* stage_key, const int32_t* n_staged, int32_t stage_cap, const int32_t* tile_off,
                     Survivor* out, int32_t out_cap, hipStream_t s);
void launch_k1_empty_tiles(const BatchView& b, const int32_t* tile_region, const int32_t* tile_col0, int32_t n_tiles, int64_t n_cols,
                           const int32_t* tile_nbase, uint32_t* planes, const int32_t* order, const int32_t* tiles_tmp, hipStream_t s);
void launch_k1_zonefix(const BatchView& b, const ReadBin* rbin, int D, int L, int64_t n_cols, uint32_t* planes, hipStream_t s);
void launch_k2_filter(const BatchView& b, const DevParams& p, const int32_t* tile_region, const int32_t* tile_col0,
                      int32_t n_tiles, int64_t n_cols, const uint32_t* planes, const int32_t* tile_fill, uint8_t* flags,
                      int32_t* tile_count, hipStream_t s);   // tile_fill: K0's record counters of the last lcr_pileup
void launch_gather_i32(const int32_t* src, const int32_t* idx, int32_t n, int32_t n_src, const int32_t* total, int32_t* out, hipStream_t s,
                       int32_t* host_out = nullptr /* pinned host memory as the device sees it: the same values, no copy needed */);
void launch_scan_i32(DevBuf& tmp, const int32_t* in, int32_t* out_excl, int32_t n, int32_t* total, hipStream_t s);
void launch_k2_compact(const BatchView& b, const DevParams& p, const int32_t* tile_region, const int32_t* tile_col0,
                       int32_t n_tiles, int64_t n_cols, const uint32_t* planes, const uint8_t* flags,
                       const int32_t* tile_count, const int32_t* tile_off, Survivor* out, int32_t out_cap, hipStream_t s);
float lcr_device_sor_threshold(hipStream_t s);
#define LCR_HITS 16   // (read, survivor) hits k2_hist keeps per read for K3 (= K3's inline entries per row)
void launch_k2_hist(const BatchView& b, const DevParams& p, const ReadBin* rbin, const Survivor* sv, const int32_t* tile_off /* survivors in front of every tile (k2_compact's offsets) */, int32_t n_tiles, int32_t n_sv,
                    uint32_t* hist /* n_sv * 4 * 31 */, int32_t* hit_cnt /* n_reads, or nullptr: no hit lists */, void* hit_list /* n_reads x LCR_HITS x uint2 */,
                    int32_t* ovf_cnt /* zeroed */, int32_t* ovf_list /* n_reads */, hipStream_t s);
// the same histograms from K0's per-tile records instead of a walk over the reads (ONT presets, batches whose survivors are dense)
void launch_k2_hist_tiles(const BatchView& b, const int32_t* tile_col0, int32_t n_tiles, const int32_t* tile_count,
                          const int32_t* tile_off, const Survivor* sv, const int32_t* ent_off, const void* ents, const unsigned long long* recs,
                          uint32_t* hist, hipStream_t s);
void launch_k2_gt(const DevParams& p, const Survivor* sv, int32_t n_sv, const uint32_t* hist, const int64_t* start0,
                  lcr_candidate* out, int32_t* keep, hipStream_t s);
void launch_k2_finish(DevBuf& scan_tmp, const lcr_candidate* tmp, const int32_t* keep, int32_t n_sv, const int32_t* sv_region_off,
                      int32_t n_regions, int32_t* pos, int32_t* idx, lcr_candidate* out, int32_t* cand_off, uint32_t dense_win,
                      uint32_t min_dense_cnt, hipStream_t s, lcr_candidate* h_cand = nullptr, int32_t* h_off = nullptr);
// k2_import.hip: the candidate stage of caller-provided sites (lcr_import_candidates, candidate.rs:530-613)
void launch_k2_import_count(const BatchView& b, const int64_t* pos0, const uint8_t* gt, const float* qual, int32_t n_sites, int32_t* count /* n_regions */, hipStream_t s);
void launch_k2_import_emit(const BatchView& b, int64_t n_cols, const uint32_t* planes, const int32_t* tile_fill /* K0's record counters of the last lcr_pileup */, const int64_t* pos0, const uint8_t* gt, const float* qual,
                           int32_t n_sites, const int32_t* cand_off /* n_regions + 1 */, lcr_candidate* out, hipStream_t s,
                           lcr_candidate* h_cand /* pinned (device pointer): the records and ... */, int32_t* h_off /* ... their offsets, or nullptr */);
void launch_k2_import_check(const int64_t* pos0, const uint8_t* gt, int32_t n_sites, int32_t* bad /* zeroed */, hipStream_t s);
// k2_exon.hip: the exon-only mask (lcr_set_exon_mask).  The check of device-resident interval lists -> verdict[0] = 1 on a violation (zeroed by the
// caller), verdict[1] = iv_off[n_regions]; the builder: the bits of every interval, clipped to its region, set in the cleared plane
void launch_k2_exon_check(const int32_t* iv_off, const int64_t* iv_start0, const int64_t* iv_end0, int32_t n_regions, int32_t* verdict, hipStream_t s);
void launch_k2_exon_build(const BatchView& b, const int32_t* iv_off, const int64_t* iv_start0, const int64_t* iv_end0, int32_t n_iv, uint32_t* plane /* (n_cols + 31) / 32 words, zeroed */, hipStream_t s);
void launch_k3_region_entries(const int64_t* row_ptr, const int32_t* row_region_off, int32_t ng, int64_t* region_e_off, hipStream_t s, int64_t* host_out = nullptr);
struct K3Hits {   // what k2_hist left for K3 (hit_cnt == nullptr: nothing -- K3 walks every read's CIGAR itself)
  const int32_t* hit_cnt; const void* hit_list; const int32_t* ovf_cnt; const int32_t* ovf_list;
  const int32_t* keep; const int32_t* pos;   // survivor s is candidate pos[s] if keep[s]
};
void launch_k3_count(const BatchView& b, const ReadBin* rbin, const lcr_candidate* cand, const int32_t* cand_region_off,
                     const int32_t* row_region_off, int32_t n_rows, int32_t* row_cnt, uint32_t* row_links, int32_t* tmp_col,
                     uint8_t* tmp_val, const K3Hits& hits, int list_blocks /* of the overflow-list role; 0: sized from the reads */, hipStream_t s);   // tmp_*: launch_k3_inline() provisional entries per row
void launch_k3_fill(const BatchView& b, const ReadBin* rbin, const lcr_candidate* cand, const int32_t* cand_region_off,
                    const int32_t* row_region_off, int32_t n_rows, int32_t* row_cnt, const int64_t* row_ptr, const int32_t* tmp_col,
                    const uint8_t* tmp_val, int32_t* col, uint8_t* val, const K3Hits& hits, int list_blocks, hipStream_t s);
int launch_k3_inline();
void launch_k3_rows_offsets(const BatchView& b, const lcr_candidate* cand, const int32_t* cand_region_off, int32_t* region_rows, int32_t* row_region_off,
                            hipStream_t s, int32_t* host_rows = nullptr /* pinned host memory as the device sees it */);   // region_rows and their exclusive prefix sums
void launch_scan_i32_to_i64(DevBuf& tmp, const int32_t* in, int64_t* out_excl, int32_t n, hipStream_t s);

void launch_k5_span_window(const int32_t* ref_start, const int32_t* ref_end, int32_t n, int64_t contig_len, int32_t* out /* {INT_MAX, 0} */, hipStream_t s);
void launch_k5_span_diff(const int32_t* ref_start, const int32_t* ref_end, int32_t n, int64_t contig_len, int64_t lo /* first position of diff */, uint32_t* diff, hipStream_t s);
// cap: columns deeper than it break a region like uncovered ones (UINT32_MAX: none).  Count pass (write = false): blk_cnt, and *n_trunc (zeroed, or
// nullptr) += columns above the cap.  Write pass: starts / ends and imax (n_keys = 2 n_islands + 1, zeroed): [2 j + 1] island j and its closing column,
// [2 j] the breaks in front of island j from behind the previous closing column on.
void launch_k5_bounds(bool write, const int32_t* ex, int64_t contig_len, uint32_t cap, int32_t n_blocks, int32_t* blk_cnt, const int32_t* blk_off,
                      int32_t* starts, int32_t* ends, uint32_t* imax, int32_t n_keys, uint32_t* n_trunc, hipStream_t s);

// k6_junctions.hip: haplotype x junction counts over the phased rows (lcr_junctions)
void launch_k6_count(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, uint32_t min_junctions,
                     int32_t* part_flag, int32_t* npair, hipStream_t s);
void launch_k6_sizes(const BatchView& b, const int32_t* part_off /* n_reads + 1 */, const int32_t* pair_off /* n_reads + 1 */, int32_t* tsz /* n_regions */,
                     int32_t* host_ctl /* pinned (device pointer): [0] participating rows, [1] pairs */, hipStream_t s);
size_t launch_k6_row_bytes();   // bytes of a participating row's record
void launch_k6_emit(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, const int32_t* part_flag,
                    const int32_t* part_off, const int32_t* pair_off, const int32_t* tbl_off /* n_regions + 1 */, void* rows, uint64_t* keys,
                    uint64_t* tbl_key /* 0xff-filled */, uint32_t* tbl_cnt /* zeroed */, hipStream_t s);
void launch_k6_flag(const uint64_t* tbl_key, const uint32_t* tbl_cnt, int32_t n_slots, uint32_t min_count, int32_t* flag, hipStream_t s);
void launch_k6_offsets(const int32_t* tbl_off, const int32_t* koff /* n_slots + 1 */, int32_t ng, int32_t n_slots, int32_t* joff, int32_t* host_joff,
                       int32_t* host_ctl /* [2] kept junctions */, hipStream_t s);
void launch_k6_place(const BatchView& b, const uint64_t* tbl_key, const uint32_t* tbl_cnt, const int32_t* flag, const int32_t* koff,
                     const int32_t* tbl_off, int32_t n_slots, const int32_t* joff, int32_t n_kept, uint64_t* ck, uint32_t* cc, int32_t* cgr,
                     lcr_junction* junc, hipStream_t s);
void launch_k6_tables(const BatchView& b, const int32_t* part_off, const void* rows, const uint64_t* keys, int32_t n_kept, lcr_junction* junc,
                      lcr_junction* host_junc /* pinned (device pointer) */, hipStream_t s);

// k7_ase.hip: haplotype and parent-of-origin counts per region over the phased rows (lcr_ase)
void launch_k7_check(const int64_t* pos0, const uint8_t* pat, const uint8_t* mat, int32_t n_sites, int32_t* bad /* zeroed */, hipStream_t s);
void launch_k7_pick(const int32_t* row_region_off, const lcr_read_record* rec, int32_t ng, lcr_ase_region* out,
                    lcr_ase_region* host_out /* pinned (device pointer), or nullptr */, int32_t* row_tag /* n_rows, or nullptr: no votes follow */, hipStream_t s);
void launch_k7_sites(const lcr_candidate* cand, int32_t n_cand, double min_phase_score, const int64_t* pos0, const uint8_t* pat,
                     const uint8_t* mat, int32_t n_sites, lcr_ase_region* ase, uint8_t* site /* n_cand */, hipStream_t s);
void launch_k7_votes(const int32_t* row_tag, int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, const uint8_t* site,
                     uint32_t min_baseq, lcr_ase_region* ase, hipStream_t s);
void launch_k7_export(const lcr_ase_region* ase, int32_t ng, lcr_ase_region* host_out /* pinned (device pointer) */, hipStream_t s);

// k11_haplotag.hip: rows of the fragment matrix against the caller's phased sites (lcr_haplotag, in place of the phase stage)
struct K11Sites { const int64_t* pos0; const uint8_t* h1; const uint8_t* h2; const uint32_t* ps; int32_t n; };
struct K11Rows {   // what k11_rows writes per row: the phase stage's per-row results (PostIn's haplotag / assignment / phase_set / d_rec)
  int8_t* haplotag; uint8_t* assignment; uint32_t* phase_set;   // pinned host memory (device pointers)
  uint32_t* d_rec;                                              // lcr_read_record in HBM, three words per row
};
void launch_k11_check(const K11Sites& st, int32_t* bad /* zeroed, pinned (device pointer) */, hipStream_t s);
void launch_k11_sites(lcr_candidate* cand, int32_t n_cand, const K11Sites& st, uint8_t* site /* n_cand */, uint32_t* site_ps /* n_cand */,
                      lcr_haplotag_site* acc /* n_cand, cleared here */, hipStream_t s);
void launch_k11_rows(int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, const uint8_t* site, const uint32_t* site_ps,
                     const PhaseLutDev& lut /* the phase stage's table */, uint32_t min_linkers, double cutoff, const K11Rows& out, lcr_haplotag_site* acc, hipStream_t s);
void launch_k11_finish(lcr_candidate* cand, int32_t n_cand, const uint8_t* site, const lcr_haplotag_site* acc, lcr_candidate* host_cand /* pinned */,
                       lcr_haplotag_site* host_acc /* pinned */, hipStream_t s);

// k12_site_counts.hip: allele x haplotype counts per candidate over the fragment matrix (lcr_site_counts).  The per-candidate segments
// (col_segments.h) are shared with k14_somatic.hip: launch_colseg_count and launch_scan_i32_to_i64 size them, each unit's fill orders them
void launch_colseg_count(int32_t n_rows, const int64_t* row_ptr, const int32_t* col, int32_t n_cand, uint32_t* cnt /* n_cand, zeroed */, hipStream_t s);
void launch_k12_fill(int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, const lcr_read_record* rec, uint32_t min_baseq,
                     int32_t n_cand, uint32_t* cnt /* launch_colseg_count's: counted back down to 0 */, const int64_t* off /* n_cand + 1 */, uint64_t* seg /* nnz */, hipStream_t s);
void launch_k12_sites(const lcr_candidate* cand, int32_t n_cand, const int64_t* off, const uint64_t* seg, lcr_site_count* out,
                      lcr_site_count* host_out /* pinned (device pointer) */, hipStream_t s);

// k14_somatic.hip: reference / heterozygous / somatic per haplotype at every candidate (lcr_somatic), over the same segments
struct K14Tables {
  int64_t tab[4 * 31];   // fe, f1e, fs_ref, fs_alt by q: llround(log10(x) * 2^40) (include/lcr.h); 992 bytes, a kernel argument
  int64_t prior[3];      // ref, het, som
};
void launch_k14_fill(int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, const lcr_read_record* rec, const lcr_candidate* cand,
                     int32_t n_cand, uint32_t* cnt /* launch_colseg_count's: counted back down to 0 */, const int64_t* off /* n_cand + 1 */, uint64_t* seg /* nnz */, hipStream_t s);
void launch_k14_sites(const lcr_candidate* cand, int32_t n_cand, const int64_t* off, const uint64_t* seg, const K14Tables& t, uint32_t min_baseq,
                      lcr_somatic_site* out, lcr_somatic_site* host_out /* pinned (device pointer) */, hipStream_t s);

// k13_hap_coverage.hip: covered depth per haplotype class at every window column, run-length encoded (lcr_hap_coverage)
void launch_k13_blocks(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, int64_t n_cols,
                       uint32_t* planes /* 3 x n_cols, zeroed: difference planes by class */, hipStream_t s);
void launch_k13_scan(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, int64_t n_cols, uint32_t* planes /* -> depths */,
                     lcr_hap_cov_region* reg, int32_t* nseg /* n_regions: run starts */, hipStream_t s);
void launch_k13_offsets(int32_t ng, const int32_t* off /* ng + 1 */, const lcr_hap_cov_region* reg, int32_t* host_off, lcr_hap_cov_region* host_reg /* pinned (device pointers) */, hipStream_t s);
void launch_k13_emit(const BatchView& b, int64_t n_cols, const uint32_t* planes, const int32_t* off, lcr_hap_cov_segment* seg, int32_t* send /* per segment: its end column */, hipStream_t s);
void launch_k13_finish(int32_t n_seg, int32_t ng, const int64_t* start0, const int32_t* send, lcr_hap_cov_segment* seg, lcr_hap_cov_segment* host_seg /* pinned (device pointer) */, hipStream_t s);

// k15_isoforms.hip: haplotype x intron-chain counts over the phased rows (lcr_isoforms); participating rows and junctions per read are
// launch_k6_count's with min_junctions - 1
void launch_k15_sizes(const BatchView& b, const int32_t* part_off /* n_reads + 1 */, const int32_t* pair_off /* n_reads + 1 */, int32_t* tsz /* n_regions */,
                      int32_t* host_ctl /* pinned (device pointer): [0] participating rows, [1] pairs */, hipStream_t s);
size_t launch_k15_row_bytes();   // bytes of a participating row's record
void launch_k15_walk(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, const int32_t* part_flag, const int32_t* part_off,
                     const int32_t* pair_off, void* rows, uint64_t* keys, uint64_t* hash /* per participating row */, hipStream_t s);
void launch_k15_insert(int32_t n_part, const void* rows, const uint64_t* keys, const uint64_t* hash, uint64_t hash_mask /* the routing bits */,
                       const int32_t* tbl_off /* n_regions + 1 */, int32_t* tbl_rep /* 0xff-filled */, uint32_t* tbl_cnt /* two per slot, zeroed */,
                       int32_t* row_slot /* per participating row */, hipStream_t s);
void launch_k15_flag(const int32_t* tbl_rep, const uint32_t* tbl_cnt, const void* rows, int32_t n_slots, uint32_t min_count, int32_t* flag,
                     int32_t* plen /* keys of a kept slot's chain, else 0 */, hipStream_t s);
void launch_k15_offsets(const int32_t* tbl_off, const int32_t* koff /* n_slots + 1 */, const int32_t* poff /* n_slots + 1 */, int32_t ng, int32_t n_slots,
                        int32_t* off, int32_t* host_off, int32_t* pbase /* n_regions + 1: pool entries in front of every region */,
                        int32_t* host_ctl /* [2] kept chains, [3] pool entries */, hipStream_t s);
void launch_k15_place(const void* rows, const uint64_t* keys, const int32_t* tbl_rep, const uint32_t* tbl_cnt, const int32_t* flag, const int32_t* koff,
                      int32_t n_slots, const int32_t* off, const int32_t* pbase, int32_t n_kept, int32_t* cslot /* n_kept */, int32_t* crank /* n_kept */,
                      lcr_isoform* iso, uint64_t* chain, uint64_t* host_chain /* pinned (device pointer) */, hipStream_t s);
void launch_k15_rows(int32_t n_part, const void* rows, const int32_t* row_slot, const int32_t* flag, const int32_t* koff, const int32_t* crank,
                     int32_t* row_iso /* n_rows, 0xff-filled */, hipStream_t s);
void launch_k15_export(int32_t n_rows, const int32_t* row_iso, int32_t* host_row_iso /* pinned (device pointer) */, hipStream_t s);
void launch_k15_tables(const BatchView& b, const int32_t* part_off, const void* rows, const uint64_t* keys, const uint64_t* chain, int32_t n_kept,
                       lcr_isoform* iso, lcr_isoform* host_iso /* pinned (device pointer) */, hipStream_t s);

// k16_ends.hip: haplotype x transcript-end sites over the phased rows (lcr_transcript_ends).  hash_mask: the bits of a key's hash that route it
void launch_k16_count(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, uint32_t strand_mode, int32_t* part_flag /* n_reads */,
                      hipStream_t s);
void launch_k16_sizes(const BatchView& b, const int32_t* part_off /* n_reads + 1 */, int32_t* tsz /* n_regions */,
                      int32_t* host_ctl /* pinned (device pointer): [0] participating rows */, hipStream_t s);
size_t launch_k16_row_bytes();    // bytes of a participating row's record
size_t launch_k16_slot_bytes();   // bytes of a slot's record behind the insertion
void launch_k16_walk(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, uint32_t strand_mode, uint32_t hash_mask,
                     const int32_t* part_flag, const int32_t* part_off, const int32_t* tbl_off /* n_regions + 1 */, void* rows,
                     uint64_t* tbl_key /* 0xff-filled */, uint32_t* tbl_cnt /* two per slot, zeroed */, hipStream_t s);
void launch_k16_peaks(const uint64_t* tbl_key, const uint32_t* tbl_cnt, const int32_t* tbl_off, int32_t ng, int32_t n_slots, uint32_t window,
                      uint32_t hash_mask, void* slots /* n_slots records: k16_peaks writes all of them, k16_assign (the second launch) the peaks' sums */,
                      hipStream_t s);
void launch_k16_flag(const void* slots, int32_t n_slots, uint32_t min_count, int32_t* flag, hipStream_t s);
void launch_k16_offsets(const int32_t* tbl_off, const int32_t* koff /* n_slots + 1 */, int32_t ng, int32_t n_slots, int32_t* off, int32_t* host_off,
                        int32_t* host_ctl /* [1] kept sites */, hipStream_t s);
void launch_k16_place(const uint64_t* tbl_key, const void* slots, const int32_t* flag, const int32_t* koff, int32_t n_slots, const int32_t* off,
                      int32_t n_kept, int32_t* cslot /* n_kept */, int32_t* crank /* n_kept */, lcr_end_site* site, hipStream_t s);
void launch_k16_rows(int32_t n_part, void* rows, const void* slots, const int32_t* flag, const int32_t* koff, const int32_t* crank,
                     int32_t* row_site /* 2 x n_rows, 0xff-filled */, uint64_t* n_assigned /* zeroed */, hipStream_t s);
void launch_k16_export(int32_t n_rows, const int32_t* row_site, int32_t* host_row_site, const uint64_t* n_assigned,
                       uint64_t* host_n_assigned /* pinned (device pointers) */, hipStream_t s);
void launch_k16_tables(const BatchView& b, const int32_t* part_off, const void* rows, uint32_t window, int32_t n_kept, lcr_end_site* site,
                       lcr_end_site* host_site /* pinned (device pointer) */, hipStream_t s);

// k17_retention.hip: haplotype x intron retention over the phased rows (lcr_intron_retention).  hash_mask: the bits of a key's hash that route it
void launch_k17_count(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, int32_t* part_flag /* n_reads */,
                      int32_t* npair /* n_reads: junctions of a participating row */, hipStream_t s);
void launch_k17_sizes(const BatchView& b, const int32_t* part_off /* n_reads + 1 */, const int32_t* pair_off /* n_reads + 1 */, int32_t* tsz /* n_regions */,
                      int32_t* host_ctl /* pinned (device pointer): [0] participating rows, [1] pairs */, hipStream_t s);
size_t launch_k17_row_bytes();   // bytes of a participating row's record
void launch_k17_emit(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, uint32_t hash_mask, const int32_t* part_flag,
                     const int32_t* part_off, const int32_t* pair_off, const int32_t* tbl_off /* n_regions + 1; a segment may be empty */, void* rows,
                     uint64_t* keys, uint64_t* tbl_key /* 0xff-filled */, uint32_t* tbl_cnt /* zeroed */, hipStream_t s);
void launch_k17_flag(const uint64_t* tbl_key, const uint32_t* tbl_cnt, int32_t n_slots, uint32_t min_count, int32_t* flag, hipStream_t s);
void launch_k17_offsets(const int32_t* tbl_off, const int32_t* koff /* n_slots + 1 */, int32_t ng, int32_t n_slots, int32_t* off, int32_t* host_off,
                        int32_t* host_ctl /* [2] kept introns */, hipStream_t s);
void launch_k17_place(const BatchView& b, const uint64_t* tbl_key, const uint32_t* tbl_cnt, const int32_t* flag, const int32_t* koff,
                      const int32_t* tbl_off, int32_t n_slots, const int32_t* off, int32_t n_kept, uint64_t* ck, uint32_t* cc, int32_t* cgr /* n_kept each */,
                      lcr_retained_intron* intron, hipStream_t s);
void launch_k17_tables(const BatchView& b, const int32_t* part_off, const void* rows, const uint64_t* keys, uint32_t anchor, int32_t n_kept,
                       lcr_retained_intron* intron, lcr_retained_intron* host_intron /* pinned (device pointer) */, int32_t* row_retained /* n_rows, zeroed */,
                       uint64_t* n_total /* zeroed */, hipStream_t s);
void launch_k17_export(int32_t n_rows, const int32_t* row_retained, int32_t* host_row_retained, const uint64_t* n_total,
                       uint64_t* host_n_total /* pinned (device pointers) */, hipStream_t s);

// k18_indels.hip: phased small indels over the fragment rows (lcr_indels).  hash_mask: the bits of a key's hash that route it.  diff / dscan:
// the per-column difference array and its exclusive scan, a segment of len[g] + 1 words per region at col_off[g] + g (dscan: one word more)
void launch_k18_count(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, uint32_t max_ins, uint32_t max_del,
                      int32_t* part_flag, int32_t* ngap, int32_t* nev /* n_reads each */, hipStream_t s);
void launch_k18_sizes(const BatchView& b, const int32_t* part_off, const int32_t* gap_off, const int32_t* ev_off /* n_reads + 1 each */, int32_t* tsz /* n_regions */,
                      int32_t* host_ctl /* pinned (device pointer): [0] participating rows, [1] gaps, [3] event occurrences */, hipStream_t s);
size_t launch_k18_row_bytes();   // bytes of a participating row's record
size_t launch_k18_gap_bytes();   // bytes of a gap's record
void launch_k18_emit(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, uint32_t max_ins, uint32_t max_del,
                     const int32_t* part_flag, const int32_t* part_off, const int32_t* gap_off, void* rows, void* gaps, int32_t* gap_read /* n_gaps */,
                     int32_t* diff /* zeroed */, hipStream_t s);
void launch_k18_insert(const BatchView& b, const void* gaps, const int32_t* gap_read, const int32_t* gap_off, int32_t n_gaps,
                       const int32_t* tbl_off /* n_regions + 1; a segment may be empty */, uint32_t hash_mask, uint64_t* tbl_key /* 0xff-filled */,
                       uint32_t* tbl_cnt /* zeroed */, hipStream_t s);
void launch_k18_flag(const BatchView& b, const uint64_t* tbl_key, const uint32_t* tbl_cnt, int32_t n_slots, const int32_t* tbl_off, const int32_t* dscan,
                     uint32_t min_count, uint32_t min_permille, int32_t* flag, hipStream_t s);
void launch_k18_offsets(const int32_t* tbl_off, const int32_t* koff /* n_slots + 1 */, int32_t ng, int32_t n_slots, int32_t* off, int32_t* host_off,
                        int32_t* host_ctl /* [2] kept events */, hipStream_t s);
void launch_k18_place(const BatchView& b, const uint64_t* tbl_key, const uint32_t* tbl_cnt, const int32_t* flag, const int32_t* koff,
                      const int32_t* tbl_off, int32_t n_slots, const int32_t* off, const int32_t* dscan, int32_t n_kept, uint64_t* ck, uint32_t* cc,
                      int32_t* cgr /* n_kept each */, lcr_indel* indel, hipStream_t s);
void launch_k18_tables(const BatchView& b, const int32_t* part_off, const void* rows, const void* gaps, uint32_t flank, int32_t n_kept, lcr_indel* indel,
                       lcr_indel* host_indel /* pinned (device pointer) */, int32_t* row_indels /* n_rows, zeroed */, uint64_t* n_total /* zeroed */,
                       hipStream_t s);
void launch_k18_export(int32_t n_rows, const int32_t* row_indels, int32_t* host_row_indels, const uint64_t* n_total,
                       uint64_t* host_n_total /* pinned (device pointers) */, hipStream_t s);

// k19_site_pairs.hip: base x base counts of nearby site pairs over the fragment matrix (lcr_site_pairs), in the order of their launches; the
// two scans between them are launch_scan_i32.  elig / rank / list / erank / m: n_cand words each; off: n_cand + 1; pair: n_cand x max_partners
void launch_k19_elig(const lcr_candidate* cand, int32_t n_cand, uint32_t mode, int32_t* elig, hipStream_t s);
void launch_k19_list(const int32_t* elig, const int32_t* rank, int32_t n_cand, int32_t* list, int32_t* erank, hipStream_t s);
void launch_k19_count(const lcr_candidate* cand, int32_t n_cand, const int32_t* erank, const int32_t* list, const int32_t* n_elig, uint32_t max_partners,
                      uint32_t max_dist, int32_t* m, hipStream_t s);
void launch_k19_init(int32_t n_cand, uint32_t max_partners, const int32_t* erank, const int32_t* list, const int32_t* off, lcr_site_pair* pair, hipStream_t s);
void launch_k19_rows(int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, int32_t n_cand, const int32_t* erank,
                     const int32_t* off, uint32_t min_baseq, lcr_site_pair* pair, hipStream_t s);
void launch_k19_export(int32_t n_cand, uint32_t max_partners, const int32_t* n_elig /* the first scan's total */, const int32_t* off, lcr_site_pair* pair,
                       lcr_site_pair* host_pair, int32_t* host_off, int32_t* host_ctl /* pinned (device pointers): records, n_cand + 1 offsets, {n_eligible, n_pairs} */,
                       hipStream_t s);

// k8_genes.hip: read -> gene over the bound batch (lcr_assign_genes) and the per-gene counts on top of it (lcr_ase_genes)
void launch_k8_check(const lcr_gene_annotation& a /* device arrays */, int32_t* bad /* zeroed */, hipStream_t s);
void launch_k8_prefix_max(const lcr_gene_annotation& a, int64_t* pmax /* n_genes: running maximum of span_end0 */, hipStream_t s);
void launch_k8_assign(const BatchView& b, const lcr_gene_annotation& a, const int64_t* pmax, int32_t* gene, uint32_t* overlap /* n_reads each */, hipStream_t s);
void launch_k8_pair_count(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, const int32_t* gene, int32_t* n_pairs /* n_regions */,
                          hipStream_t s);
void launch_k8_pair_offsets(const int32_t* pair_off /* n_regions + 1 */, int32_t ng, int32_t* host_off, int32_t* host_ctl /* pinned (device pointers): the offsets, [0] pairs */,
                            hipStream_t s);
void launch_k8_pair_emit(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, const int32_t* gene, const int32_t* pair_off,
                         lcr_ase_gene* out, lcr_ase_gene* host_out /* pinned (device pointer), or nullptr */, int32_t* row_tag /* n_rows, or nullptr: no votes follow */,
                         hipStream_t s);
void launch_k8_sites(const lcr_candidate* cand, int32_t n_cand, double min_phase_score, const int64_t* pos0, const uint8_t* pat, const uint8_t* mat,
                     int32_t n_sites, const int32_t* pair_off, lcr_ase_gene* pairs, uint8_t* site /* n_cand */, uint32_t* site_ps /* n_cand */, hipStream_t s);
void launch_k8_votes(const int32_t* row_tag, int32_t n_rows, const int64_t* row_ptr, const int32_t* col, const uint8_t* val, const uint8_t* site,
                     const uint32_t* site_ps, uint32_t min_baseq, lcr_ase_gene* pairs, hipStream_t s);
void launch_k8_export(const lcr_ase_gene* pairs, int32_t n, lcr_ase_gene* host_out /* pinned (device pointer) */, hipStream_t s);

// k9_gene_junctions.hip: haplotype x junction counts per (region, gene) pair over the phased rows (lcr_junctions_genes)
struct K9Pairs {   // what k9_pairs<true> writes: per read its pair and row slot (n_reads each); per pair its region, gene, first row, rows and
  int32_t *read_pair, *row_slot, *region, *gene, *row0, *rows, *occ;   // junction occurrences (sized by n_reads, an upper bound of the pairs)
};
struct K9Row {            // a participating row; a pair's rows are contiguous, in read order (= by pos).  K10's DNA filter clears bit 2 of hap
  int32_t pos, rend;      // [pos, rend) on the contig
  uint32_t ps;            // phase set, 0 = none
  int32_t first, n;       // its junction keys are keys[first .. first + n), ascending
  int32_t hap;            // 1 / 2, + 4 when the row is counted (it shares a base with a merged exon of the pair's gene)
};
static_assert(sizeof(K9Row) == 24, "K9Row is six words");
void launch_k9_count(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, const int32_t* gene, uint32_t min_junctions,
                     int32_t* part_flag, int32_t* nocc, hipStream_t s);
void launch_k9_pair_count(const BatchView& b, const int32_t* gene, const int32_t* part_flag, int32_t* n_pairs /* n_regions */, hipStream_t s);
void launch_k9_pair_emit(const BatchView& b, const int32_t* gene, const int32_t* part_flag, const int32_t* nocc, const int32_t* pair_off /* n_regions + 1 */,
                         const int32_t* part_off /* n_reads + 1 */, const K9Pairs& pr, hipStream_t s);
void launch_k9_sizes(const BatchView& b, const int32_t* pair_off, const int32_t* part_off, const int32_t* occ_off /* n_reads + 1 */, const int32_t* pair_occ,
                     int32_t* tsz /* n_reads */, int32_t* host_ctl /* pinned (device pointer): [0] participating rows, [1] occurrences, [3] pairs */,
                     hipStream_t s);
size_t launch_k9_row_bytes();   // bytes of a participating row's record
void launch_k9_emit(const BatchView& b, const int32_t* row_region_off, const lcr_read_record* rec, const int32_t* gene, const int32_t* part_flag,
                    const int32_t* occ_off, const K9Pairs& pr, const int32_t* tbl_off /* n_reads + 1 */, const lcr_gene_annotation& a /* device arrays */,
                    void* rows, uint64_t* keys, uint64_t* tbl_key /* 0xff-filled */, uint32_t* tbl_cnt /* zeroed */, hipStream_t s);
void launch_k9_offsets(const int32_t* pair_off, const int32_t* tbl_off, const int32_t* koff /* n_slots + 1 */, int32_t ng, int32_t n_slots, int32_t* joff,
                       int32_t* host_joff, int32_t* host_ctl /* [2] kept junctions */, hipStream_t s);
void launch_k9_place(const BatchView& b, const uint64_t* tbl_key, const uint32_t* tbl_cnt, const int32_t* flag, const int32_t* koff,
                     const int32_t* tbl_off, const int32_t* pair_off, const K9Pairs& pr, int32_t n_slots, int32_t n_kept, uint64_t* ck, uint32_t* cc,
                     int32_t* cp, lcr_junction_gene* junc, int32_t* junc_pair /* n_kept: the pair of every record */, hipStream_t s);
void launch_k9_tables(const int32_t* junc_pair, const K9Pairs& pr, const void* rows, const uint64_t* keys, int32_t n_kept, lcr_junction_gene* junc,
                      lcr_junction_gene* host_junc /* pinned (device pointer) */, hipStream_t s);

// k10_asj_modes.hip: interior exon blocks, DNA support and gene coverage beside K9's table (lcr_asj_genes)
void launch_k10_dna_check(const int64_t* dna_pos0, int32_t n_dna, int32_t* bad /* zeroed */, hipStream_t s);
void launch_k10_count(const BatchView& b, const int32_t* gene, const int32_t* part_flag, uint32_t min_junctions, int32_t* nblk /* n_reads, or nullptr */,
                      int32_t* gene_reads /* n_genes, zeroed, or nullptr */, hipStream_t s);
void launch_k10_pair_blocks(const BatchView& b, const int32_t* part_flag, const int32_t* nblk, const int32_t* read_pair, int32_t* pair_blk /* zeroed */,
                            hipStream_t s);
void launch_k10_emit(const BatchView& b, const int32_t* part_flag, const int32_t* nblk, const int32_t* read_pair, const int32_t* xtbl_off,
                     uint64_t* xtbl_key /* 0xff-filled */, uint32_t* xtbl_cnt /* zeroed */, hipStream_t s);
void launch_k10_place(const uint64_t* xtbl_key, const uint32_t* xtbl_cnt, const int32_t* flag, const int32_t* koff, const int32_t* xtbl_off,
                      const int32_t* pair_off, const K9Pairs& pr, int32_t ng, int32_t n_slots, int32_t n_kept, uint64_t* ck, uint32_t* cc, int32_t* cp,
                      lcr_exon_gene* exon, lcr_exon_gene* host_exon /* pinned (device pointer) */, hipStream_t s);
void launch_k10_support(const lcr_candidate* cand, int32_t n_cand, const int32_t* cand_off, int32_t ng, double min_phase_score, const int64_t* dna_pos0,
                        int32_t n_dna, uint32_t* sup /* n_cand */, uint32_t* sup_uniq /* n_cand */, int32_t* sup_n /* n_regions */, hipStream_t s);
void launch_k10_filter(const BatchView& b, const int32_t* part_flag, const int32_t* row_slot, const int32_t* cand_off, const uint32_t* sup_uniq,
                       const int32_t* sup_n, void* rows, hipStream_t s);

// device helpers shared by kernels -------------------------------------------------------------
#ifdef __HIPCC__
__device__ __forceinline__ int base_code(uint8_t b) {
  // A,C,G,T (either case, as util.rs:822-889 matches 'A'|'a' ...) -> 0..3, else -1
  switch (b) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return -1;
  }
}
__device__ __forceinline__ int iabs_(int x) { return x < 0 ? -x : x; }

// util.rs:745-751: |curr_pos - leading_softclips| < D or |curr_pos - (seq_len - trailing)| < D
__device__ __forceinline__ bool in_end_zone(int c, int lead, int reb, int D) {
  return iabs_(c - lead) < D || iabs_(c - reb) < D;
}

// util.rs:754-789 restated as a single scan: the base at read position c facing reference byte R is
// masked iff a window of L identical bases X in {A,C,G,T}, X != R, starts at some t in [c-L, c+1]
// and lies inside the read.  Window [t, t+L-1] is all-X iff the L-1 adjacent equalities hold.
__device__ __forceinline__ bool polya_masked(const uint8_t* __restrict__ seq, int seq_len, int c, int L, uint8_t R) {
  int lo = c - L;            // first byte that can belong to a window
  int hi = c + L;            // last byte that can belong to a window (window t=c+1 ends at c+L)
  if (lo < 0) lo = 0;
  if (hi > seq_len - 1) hi = seq_len - 1;
  if (hi - lo + 1 < L) return false;
  int run = 1;               // length of the run of equal bytes ending at i
  uint8_t prev = seq[lo];
  bool masked = false;
  for (int i = lo + 1; i <= hi; i++) {
    uint8_t cur = seq[i];
    run = (cur == prev) ? run + 1 : 1;
    prev = cur;
    if (run >= L) {
      // window [i-L+1, i] is homopolymer of `cur`; its start t = i-L+1 must be in [c-L, c+1]
      int t = i - L + 1;
      if (t >= c - L && t <= c + 1 && cur != R && (cur == 'A' || cur == 'C' || cur == 'G' || cur == 'T')) masked = true;
    }
  }
  return masked;
}


// wave64 inclusive add-scan with DPP row shifts / row broadcasts (6 VALU ops, no LDS round trips).
// update_dpp(old = 0, ..., bound_ctrl = false): lanes without a source keep 0, the identity.
__device__ __forceinline__ int wave_incl_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1,3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2,3
  return v;
}

// wave64 reductions by xor shuffles: every lane gets the result.  (A 64-bit shuffle is two 32-bit ones; the adds wrap as unsigned.)
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (unsigned long long)__shfl_xor(v, d, 64);
  return v;
}

// inclusive add-scan inside each 16-lane DPP row (four reads share a wave in the site walkers)
__device__ __forceinline__ int row16_incl_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
  return v;
}

// Sixteen lanes (one DPP row) locate, for one read, the bases that face a sorted list of sites
// (region-relative columns site_col(i), i in [s_lo, s_hi), ascending).  This is the cursor walk of
// util.rs:700-944 / fragment.rs:60-240 turned inside out so that no load depends on a previous site:
//   1. the sites inside the read's reference span [max(rel_pos,0), rend) are found with one probe of
//      sixteen site columns per step (lanes <-> sites);
//   2. the CIGAR is read 64 ops at a time (four words per lane, one round trip), reference / read start
//      offsets of the ops come from two row scans per 16 ops (lanes <-> ops), and every covered site
//      records the read offset of its base in "its" lane (site j of the batch -> lane j);
//   3. sink(i, c, hit) is then called ONCE per batch of <= 16 sites with all sixteen lanes active:
//      lane j gets site i = first + j and c = read offset of the base an M/=/X op puts on that site
//      (hit = false: no such base).  The sink does its loads / atomics for up to 16 sites in parallel
//      and may use row ballots to keep the sites' order.
// A read that covers no site returns before touching its CIGAR.  Four reads share a wave64.
// `live` = this row has a read; rows without one pass live = false (their lanes still call).
// step 1 of the walk: first site with column >= key = max(rel_pos, 0) (cur) and first site with column >= rend (s_end) among the
// ascending sites [s_lo, s_hi); live = false or no site inside the span: cur >= s_end
template <class ColFn>
__device__ __forceinline__ void row16_find_sites(bool live, const ReadBin& h, int rend, int s_lo, int s_hi, ColFn site_col, int* cur_out, int* s_end_out) {
  const int lane = threadIdx.x & 63, l16 = lane & 15, rbase = lane & 48;
  int cur = s_hi, s_end = s_hi;
  if (live) {
    const int key = h.rel_pos > 0 ? h.rel_pos : 0;
    bool found_cur = false;
    for (int base = s_lo; base < s_hi; base += 16) {
      const int i = base + l16;
      const int colv = i < s_hi ? site_col(i) : INT_MAX;
      const unsigned int ge_key = (unsigned int)(__ballot(colv >= key) >> rbase) & 0xffffu;
      const unsigned int ge_end = (unsigned int)(__ballot(colv >= rend) >> rbase) & 0xffffu;
      if (!found_cur && ge_key) { cur = base + __ffs((int)ge_key) - 1; found_cur = true; }
      if (ge_end) { s_end = base + __ffs((int)ge_end) - 1; break; }
    }
    if (!found_cur) cur = s_end;
  }
  *cur_out = cur; *s_end_out = s_end;
}

// steps 2 + 3: the sites [cur, s_end) of the read against its CIGAR.  pre != nullptr: the read's first 64 ops (four words per lane, op
// 16 k + l16 in pre[k], 0 beyond the CIGAR) were requested by the caller beside its own loads (k2_hist: one round trip less in the chain)
template <class ColFn, class Sink>
__device__ __forceinline__ void row16_walk_range(const BatchView& b, const ReadBin& h, int cur, int s_end, const uint32_t* pre, ColFn site_col, Sink sink) {
  const int lane = threadIdx.x & 63, l16 = lane & 15, rbase = lane & 48;
  if (cur >= s_end) return;   // (row-uniform)
  const uint32_t ncig = (uint32_t)h.n_cig;
  const uint32_t* __restrict__ cg = b.cigar + h.cig_off;
  for (int first = cur; first < s_end; first += 16) {   // batches of 16 covered sites (one batch almost always)
    const int n = min(16, s_end - first);
    const int my_cc = l16 < n ? site_col(first + l16) : INT_MAX;
    const int last_cc = __shfl(my_cc, rbase + n - 1, 64);
    int myc = -1;
    int ref_cur = h.rel_pos;
    int q_cur = h.lead > 0 ? h.lead : 0;
    int j = 0;                                           // next site of the batch (row-uniform)
    int cc = __shfl(my_cc, rbase, 64);
    for (uint32_t c0 = 0; c0 < ncig && j < n; c0 += 64) {
      uint32_t w4[4];
      if (pre && c0 == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) w4[k] = pre[k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++) w4[k] = c0 + 16 * k + l16 < ncig ? cg[c0 + 16 * k + l16] : 0u;
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t w = w4[k];
        const int op = w & 15, len = (int)(w >> 4);
        const bool is_m = op == 0 || op == 7 || op == 8;     // (a padding word is a 0-length M: covers nothing)
        const int dr = (is_m || op == 2 || op == 3) ? len : 0;
        const int dq = (is_m || op == 1) ? len : 0;
        const int ir = row16_incl_scan(dr), iq = row16_incl_scan(dq);
        const int rs = ref_cur + ir - dr, qs = q_cur + iq - dq;
        const int chunk_end = ref_cur + __shfl(ir, rbase + 15, 64);
        while (j < n && cc < chunk_end) {
          const unsigned int m = (unsigned int)(__ballot(is_m && cc >= rs && cc < rs + len) >> rbase) & 0xffffu;
          if (m) {
            const int L = rbase + __ffs((int)m) - 1;
            const int c = __shfl(qs, L, 64) + (cc - __shfl(rs, L, 64));
            if (l16 == j) myc = c;
          }
          j++;
          cc = __shfl(my_cc, rbase + (j < n ? j : 0), 64);
        }
        ref_cur = chunk_end;
        q_cur += __shfl(iq, rbase + 15, 64);
      }
      if (ref_cur > last_cc) break;
    }
    sink(first + l16, myc, myc >= 0);
  }
}

template <class ColFn, class Sink>
__device__ __forceinline__ void row16_walk_sites(const BatchView& b, bool live, const ReadBin& h, int rend, int s_lo, int s_hi,
                                                 ColFn site_col, Sink sink) {
  int cur, s_end;
  row16_find_sites(live, h, rend, s_lo, s_hi, site_col, &cur, &s_end);
  row16_walk_range(b, h, cur, s_end, nullptr, site_col, sink);
}

// region index of read r: precomputed by k0_read_region (a binary search over read_begin would cost
// ~log2(n_regions) dependent global loads per read in every read-parallel kernel)
#define region_of_read(b_, r_) ((b_).read_region[(r_)])
#endif

// lcr_pileup.hip — the pileup stage's host driver (K0: CIGAR decode into per-tile records, the tile passes, K1: the tally) and
// lcr_get_columns, with the two functions that bring c->planes up to date for a reader (planes_tally, planes_materialise).  lcr_pileup is a
// short sequence of steps; each step's name says what it queues or waits for.
#include "lcr_ctx.h"

namespace {

// K0's record pool and descriptor array: the capacities asked for (grown after an overflow) and their cut into shards
struct PilePools {
  int32_t n_blocks = 0;                        // K0 workgroups
  size_t pool_cap64 = 0, desc_cap64 = 0;       // slots, descriptors
  size_t n_shards = 0;
  unsigned int pool_sub = 0, desc_sub = 0;     // per shard
};

// ---- K0: decode every CIGAR once into per-tile records (one op-parallel pass; a block's records lie back to back in the
// pool, grouped by tile, each group announced by a chunk descriptor)
// records <= M / D / I ops + their tile crossings (M: <= bases / tile) + at most two per intron.  Long D runs can exceed
// the estimate: K0 then flags an overflow (writes are bounds-checked) and the stage is repeated with larger pools.
PilePools pile_size_pools(const lcr_ctx* c) {
  PilePools P;
  const int opb = launch_k0_opb();
  P.n_blocks = (int32_t)(((uint64_t)c->n_ops + opb - 1) / opb);
  // (a block's records of one tile take whole 16-slot units: + 15 slots per (block, tile) group at most)
  P.desc_cap64 = (size_t)P.n_blocks * 128 + (size_t)c->bv.n_reads / 4 + 1024;
  P.pool_cap64 = (size_t)c->n_ops + (size_t)c->n_ops / 2 + (size_t)c->bv.n_reads + (size_t)c->n_bases / LCR_TILE + 8 * P.desc_cap64 + 1024;
  return P;
}

// the pool and the descriptor array are cut into launch_k0_acct_slots() shards (a block allocates from shard blockIdx % shards)
int pile_reserve_pools(lcr_ctx* c, PilePools& P) {
  const size_t nsh = P.n_shards = (size_t)launch_k0_acct_slots();
  const size_t pool_sub64 = (P.pool_cap64 + nsh - 1) / nsh + 256, desc_sub64 = (P.desc_cap64 + nsh - 1) / nsh + 64;
  if (pool_sub64 * nsh > 0xFFFFFFF0ull || desc_sub64 * nsh > 0x7FFFFFF0ull) { c->err = "batch too large for the 32-bit record pool: split it"; return LCR_E_ARG; }
  P.pool_sub = (unsigned int)pool_sub64; P.desc_sub = (unsigned int)desc_sub64;
  HIPCHK(c, c->k0_items.reserve(pool_sub64 * nsh * 8));
  HIPCHK(c, c->desc_tile.reserve(desc_sub64 * nsh * 4));
  HIPCHK(c, c->desc_val.reserve(desc_sub64 * nsh * 8));
  // entries of 16 slots: a group of c records inside a block's tile window takes ceil(c / 16) entries AND ceil(c / 16) * 16
  // pool slots, a record outside the window one pool slot, one descriptor and one entry of its own -- so the entry list is
  // bounded by pool / 16 + descriptors, not by pool / 16 (thousands of reads across an intron of > 65 536 columns)
  HIPCHK(c, c->chunks.reserve((pool_sub64 * nsh / 16 + desc_sub64 * nsh + 16) * 8));
  return LCR_OK;
}

// the cleared scratch (PileScratch, lcr_dev.h) and the tile tables the tile passes write
int pile_reserve_scratch(lcr_ctx* c, const PileScratch& L) {
  const int nt = c->n_tiles;
  HIPCHK(c, c->k0_tile_fill.reserve(L.words * 4));
  c->bv.error_flag = &reinterpret_cast<K0Ctl*>(c->k0_tile_fill.as<int32_t>() + L.ctl)->error;
  HIPCHK(c, c->tile_order.reserve(std::max(nt, 1) * 4));
  HIPCHK(c, c->tile_nbase.reserve(std::max(nt, 1) * 4));
  HIPCHK(c, c->chunk_off.reserve(((size_t)nt + 2) * 4));
  HIPCHK(c, c->read_scan.reserve(std::max<size_t>(c->bv.n_reads, 1) * 8));
  HIPCHK(c, c->h_stage[0].reserve(64));   // (the host's K0Ctl)
  return LCR_OK;
}

int pile_queue_k0(lcr_ctx* c, const PileScratch& L, const PilePools& P, bool& gated) {
  int32_t* const fill = c->k0_tile_fill.as<int32_t>();
  HIPCHK(c, lcr_fill_async(fill, 0, L.words * 4, c->stream));
  // (async_phase: K0 waits for the restarts of a phase stage still in flight, beside its tails -- a matter of speed, not of order: the fill
  // in front of it runs early)
  if (!gated) { HIPCHK(c, c->phase.gate_stream(c->stream)); gated = true; }
  Timer t(c, LCR_K_SPANS);
  launch_k0_ops(c->bv, c->read_bin.as<ReadBin>(), c->blk_first_read.as<int32_t>(), c->cig0, c->n_ops, c->dp.ont, c->dp.dist_to_end, c->dbg_fold_indels, c->n_tiles,
                fill, fill + L.nch, fill + L.ndiff, reinterpret_cast<K0Ctl*>(fill + L.ctl), (unsigned int*)(fill + L.acct), P.pool_sub, c->k0_items.as<unsigned long long>(),
                P.desc_sub, c->desc_tile.as<uint32_t>(), c->desc_val.p, c->read_scan.p, c->stream);
  return LCR_OK;
}

// tile order for K1, introns per whole tile, chunk offsets, K0's accounting (one workgroup); K0's verdict (CIGAR
// validation, pool overflow) and counts then leave for the host before the rest is queued: the host waits for them while
// K1 runs and returns without waiting for K1 -- later calls queue behind it
int pile_queue_tally(lcr_ctx* c, const PileScratch& L, const PilePools& P, bool fuse, bool lean) {
  BatchView& b = c->bv;
  const int nt = c->n_tiles;
  int32_t* const fill = c->k0_tile_fill.as<int32_t>();
  K0Ctl* const d_ctl = reinterpret_cast<K0Ctl*>(fill + L.ctl);
  { Timer t(c, LCR_K_PILEUP);   // (the tally kernel with its ordering and chunk-binning passes)
    if (nt > 0) {   // (k1_tiles_a writes K0's verdict and counts straight into the pinned block: no copy in the queue in front of k1_tiles_b)
      K0Ctl* h_ctl_dev = nullptr;
      HIPCHK(c, c->h_stage[0].dev(&h_ctl_dev));
      launch_k1_tiles_a(nt, fill, fill + L.ndiff, fill + L.nch, fill + L.tmp, (unsigned int*)(fill + L.acct), launch_k0_acct_slots(),
                        d_ctl, h_ctl_dev, c->tile_region.as<int32_t>(), c->tile_col0.as<int32_t>(), b.len, c->stream);
    } else HIPCHK(c, hipMemcpyAsync(c->h_stage[0].p, d_ctl, sizeof(K0Ctl), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_ctl, c->stream));
    if (nt > 0) launch_k1_tiles_b(nt, fill, fill + L.ndiff, fill + L.nch, fill + L.tmp, c->tile_nbase.as<int32_t>(), c->chunk_off.as<int32_t>(),
                                  c->tile_order.as<int32_t>(), fuse ? c->tile_count.as<int32_t>() : nullptr, c->stream);
    if (nt > 0 && c->n_ops > 0)
      launch_k0_desc_bin(d_ctl, (const unsigned int*)(fill + L.acct), P.desc_sub, c->desc_tile.as<uint32_t>(), c->desc_val.p, c->chunk_off.as<int32_t>(), fill + L.cur,
                         c->chunks.p, P.n_blocks / 8 + 1, c->stream);
    // ---- K1: per-tile tally from the records (leaves at once if K0 flagged an error) -- the record-free tiles' planes stay
    // unwritten (planes_dense), and in the lean form those of the tiles with records as well (planes_tallied): the survivors of pass 1 are staged
    // for lcr_candidates instead --; K1z: poly-A / homopolymer mask of the HiFi presets
    if (lean)
      launch_k1_pileup_lean(b, c->dp, c->tile_region.as<int32_t>(), c->tile_col0.as<int32_t>(), nt, c->n_cols, fill, c->chunk_off.as<int32_t>(),
                            c->chunks.p, c->k0_items.as<unsigned long long>(), c->tile_nbase.as<int32_t>(), c->tile_order.as<int32_t>(), fill + L.tmp,
                            c->stream, c->tile_count.as<int32_t>(), c->sv_stage.as<Survivor>(), c->sv_stage_key.p, c->sv_stage_cap);
    else
      launch_k1_pileup(b, c->dp, c->tile_region.as<int32_t>(), c->tile_col0.as<int32_t>(), nt, c->n_cols, fill, c->chunk_off.as<int32_t>(),
                       c->chunks.p, c->k0_items.as<unsigned long long>(), c->tile_nbase.as<int32_t>(), c->planes.as<uint32_t>(),
                       c->tile_order.as<int32_t>(), fill + L.tmp, c->stream, fuse ? c->flags.as<uint8_t>() : nullptr, fuse ? c->tile_count.as<int32_t>() : nullptr);
    if (!c->dp.ont && c->dp.dist_to_end > 0)
      launch_k1_zonefix(b, c->read_bin.as<ReadBin>(), c->dp.dist_to_end, c->dp.polya_len, c->n_cols, c->planes.as<uint32_t>(), c->stream); }
  HIPCHK(c, hipGetLastError());
  return LCR_OK;
}

// waits for K0's control block (K1 is running); *retry: the pools overflowed -- K0 kept counting, so the block says what to ask for
int pile_read_verdict(lcr_ctx* c, K0Ctl* out, bool* retry) {
  HIPCHK(c, hipEventSynchronize(c->ev_ctl));
  HT("pile:ctl");
  *out = *c->h_stage[0].as<K0Ctl>();
  if (c->n_tiles == 0) out->empty_cols = 0;   // (k1_tiles_a counts them: with the words this wait is for anyway)
  if (*c->h_order.as<int32_t>() != 0) { c->err = "the reads of a region must be sorted by position (lcr_reads.pos)"; return LCR_E_ARG; }
  if (out->error == 1) { c->err = "unknown CIGAR operation (reference panics: util.rs:944)"; return LCR_E_CIGAR; }
  if (out->error == 2) { c->err = "CIGAR inconsistent with l_seq / soft clips"; return LCR_E_CIGAR; }
  *retry = out->error != 0;
  return LCR_OK;
}

}  // namespace

// the planes of the tiles with records, when the current pileup's tally ran in its lean form: the same kernel in its full form over the tile order,
// n_full, chunk tables and record pool that pileup left (lcr_ctx.h: nothing else rewrites them) -- once, when a reader of the planes turns up.
// with_filter: pass 1's flags and per-tile counts too, for the pileup's own parameters (lcr_candidates' fallback on k2_compact).
int planes_tally(lcr_ctx* c, bool with_filter) {
  if (c->planes_tallied && !with_filter) return LCR_OK;   // (with_filter is asked for behind a lean tally only: the flags were never stored)
  if (with_filter) HIPCHK(c, c->flags.reserve(std::max<size_t>(c->n_cols, 1)));
  launch_k1_pileup(c->bv, c->flt_dp, c->tile_region.as<int32_t>(), c->tile_col0.as<int32_t>(), c->n_tiles, c->n_cols, c->k0_tile_fill.as<int32_t>(),
                   c->chunk_off.as<int32_t>(), c->chunks.p, c->k0_items.as<unsigned long long>(), c->tile_nbase.as<int32_t>(), c->planes.as<uint32_t>(),
                   c->tile_order.as<int32_t>(), c->k0_tile_fill.as<int32_t>() + pile_scratch(c->n_tiles).tmp, c->stream,
                   with_filter ? c->flags.as<uint8_t>() : nullptr, with_filter ? c->tile_count.as<int32_t>() : nullptr);
  HIPCHK(c, hipGetLastError());
  c->planes_tallied = true;
  return LCR_OK;
}

// ... and the record-free tiles' constant planes of the current pileup behind them, stored once when somebody asks for every column (lcr_ctx::planes_dense)
int planes_materialise(lcr_ctx* c) {
  { int rc = planes_tally(c, false); if (rc) return rc; }
  if (c->planes_dense) return LCR_OK;
  launch_k1_empty_tiles(c->bv, c->tile_region.as<int32_t>(), c->tile_col0.as<int32_t>(), c->n_tiles, c->n_cols, c->tile_nbase.as<int32_t>(),
                        c->planes.as<uint32_t>(), c->tile_order.as<int32_t>(), c->k0_tile_fill.as<int32_t>() + pile_scratch(c->n_tiles).tmp, c->stream);
  HIPCHK(c, hipGetLastError());
  c->planes_dense = true;
  return LCR_OK;
}

// what the byte getters add behind a lean tally: 48 bytes per survivor it stored (S').  The host reads the tally's counter once, unless
// lcr_candidates has had the number already.
int pile_staged_bytes(lcr_ctx* c, int64_t* bytes) {
  *bytes = 0;
  if (!c->pile_lean || c->stage < ST_PILED) return LCR_OK;
  if (c->sv_stage_n < 0) {
    int32_t n = 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(&n, c->k0_tile_fill.as<int32_t>() + pile_scratch(c->n_tiles).tmp + K1_TMP_STAGED, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->sv_stage_n = std::min(n, c->sv_stage_cap);
  }
  *bytes = (int64_t)sizeof(Survivor) * c->sv_stage_n;
  return LCR_OK;
}

extern "C" {

int lcr_pileup(lcr_ctx* c, const lcr_params* p) {
  HT("pileup");
  if (!c || !p) return LCR_E_ARG;
  if (c->stage < ST_LOADED) { c->err = "lcr_pileup before lcr_load_batch"; return LCR_E_STATE; }
  if (p->polya_len == 0) { c->err = "polya_len must be >= 1"; return LCR_E_ARG; }
  // (the ends kernel of the poly-A mask takes dist_to_end <= 63 and polya_len in 2..16 -- every preset --, the per-offset kernel the rest;
  // the thread index of the latter runs over n_reads x 2 x dist_to_end)
  if ((uint64_t)c->bv.n_reads * 2ull * p->dist_to_end > 0x7FFFFF00ull * (uint64_t)LCR_BLOCK) { c->err = "dist_to_end x reads too large for one launch; split the batch"; return LCR_E_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  if (c->sor_thr < 0.f) c->sor_thr = lcr_device_sor_threshold(c->stream);  // candidate.rs:49-51, evaluated by the device's logf
  c->dp = to_dev(p, c->sor_thr);
  c->dp.dbg = 0;
  HIPCHK(c, c->planes.reserve(std::max<size_t>((size_t)c->n_cols * LCR_NPLANES, 1) * 4));
  rewind_to(c, ST_LOADED);   // (from here on the planes, the tile tables and the record pool are rewritten)
  if (c->dbg_poison_planes) HIPCHK(c, lcr_fill_async(c->planes.p, 0xA5, (size_t)c->n_cols * LCR_NPLANES * 4, c->stream));
  const int nt = c->n_tiles;
  PilePools P = pile_size_pools(c);
  const PileScratch L = pile_scratch(nt);
  int rc;
  if ((rc = pile_reserve_scratch(c, L))) return rc;
  // pass 1 of the candidate filters inside the tally's epilogue (k2_eval.h): presets whose planes are final when K1 stores them (ONT: the
  // HiFi presets subtract the poly-A mask afterwards, k1_zonefix); lcr_candidates uses the flags if it is called with the same filters
  const bool fuse = c->dbg_fuse_filter != 0 && c->dp.ont && nt > 0;
  // the tally's lean form (k1_pileup.hip): no planes and no flags for the tiles with records either, the survivors of pass 1 handed to lcr_candidates
  // as staged records -- from a context's second batch on, when the last candidate stage left a guess of their number to size the staging by
  const bool lean = fuse && c->sv_cap_guess > 0 && c->dbg_lean_planes != 0;
  if (fuse) HIPCHK(c, c->tile_count.reserve(std::max(nt, 1) * 4));
  if (fuse && !lean) HIPCHK(c, c->flags.reserve(std::max<size_t>(c->n_cols, 1)));
  if (lean) {
    c->sv_stage_cap = c->sv_cap_guess;
    HIPCHK(c, c->sv_stage.reserve((size_t)c->sv_stage_cap * sizeof(Survivor)));
    HIPCHK(c, c->sv_stage_key.reserve((size_t)c->sv_stage_cap * 8));
  }
  K0Ctl ctl{};
  bool gated = false;   // (the gate on a phase stage in flight is queued once: pile_queue_k0)
  for (bool retry = true; retry;) {
    if ((rc = pile_reserve_pools(c, P))) return rc;
    if ((rc = pile_queue_k0(c, L, P, gated))) return rc;
    if ((rc = pile_queue_tally(c, L, P, fuse, lean))) return rc;
    if ((rc = pile_read_verdict(c, &ctl, &retry))) return rc;
    if (retry) {   // grow to what the fullest shard asked for
      P.pool_cap64 = std::max<size_t>(P.pool_cap64 * 2, ((size_t)ctl.pool_top + 1024) * P.n_shards);
      P.desc_cap64 = std::max<size_t>(P.desc_cap64 * 2, ((size_t)ctl.desc_top + 1024) * P.n_shards);
    }
  }
  c->pile_items = (int64_t)ctl.n_items; c->pile_recs = (int64_t)ctl.n_recs;
  // bytes K1 itself has to move: read bases once + 8-byte records + reference byte per column, 13 u32
  // planes written per column of a tile with records (the record-free tiles' planes are not written by this stage)
  // (8 bytes per M / D / I / N item: the extra records of items that cross a tile boundary are overhead, not algorithm)
  // A lean tally stores no plane: 48 bytes per staged survivor instead, added by the getters (lcr_api.hip) once their number is known -- the tally
  // is still running here.  A later replay of the planes for a getter is not the stage's traffic, as k1_empty_tiles is not.
  const int64_t plane_cols = lean ? 0 : c->n_cols - (int64_t)ctl.empty_cols;
  c->pileup_bytes = c->n_bases + 8 * (int64_t)(int32_t)ctl.n_items + c->n_cols + 4 * LCR_NPLANES * plane_cols;
  c->stage_bytes = c->n_bases + 4 * c->n_cigar + 37 * (int64_t)c->bv.n_reads + c->n_cols + 4 * LCR_NPLANES * plane_cols;
  c->stage = ST_PILED;
  c->planes_tallied = !lean; c->sv_staged = c->pile_lean = lean; c->sv_stage_n = -1;
  c->flt_fused = fuse; c->flt_dp = c->dp; c->flt_mask_gen = c->mask_gen;
  c->pile_platform = p->platform; c->pile_dist_to_end = p->dist_to_end;
  return LCR_OK;
}

int lcr_get_columns(lcr_ctx* c, lcr_columns* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PILED) { c->err = "lcr_get_columns before lcr_pileup"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = planes_materialise(c); if (rc) return rc; }
  const size_t bytes = (size_t)c->n_cols * LCR_NPLANES * 4;
  HIPCHK(c, c->h_planes.reserve(std::max<size_t>(bytes, 1)));
  if (bytes) HIPCHK(c, hipMemcpyAsync(c->h_planes.p, c->planes.p, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  out->n_cols = c->n_cols;
  out->planes = c->h_planes.as<uint32_t>();
  return LCR_OK;
}

}  // extern "C"

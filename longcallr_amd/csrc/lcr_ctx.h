// lcr_ctx.h — the context behind the C ABI (include/lcr.h) and what its host units share: the stage state, timers, uploads, the settle
// functions.  Private to lcr_api.hip (lifecycle, cache, fills, debug switches, phase entry, region discovery), lcr_batch.hip (binding and
// upload), lcr_pileup.hip (lcr_pileup, lcr_get_columns), lcr_calls.hip (candidate, import and fragment stages with their getters) and
// lcr_junctions.hip (lcr_junctions, lcr_get_junctions), lcr_ase.hip (lcr_ase, lcr_get_ase) and lcr_genes.hip (lcr_assign_genes, lcr_get_read_genes,
// lcr_ase_genes, lcr_get_ase_genes), lcr_junctions_genes.hip (lcr_junctions_genes, lcr_get_junctions_genes) and lcr_asj_genes.hip
// (lcr_asj_genes, lcr_get_asj_genes).  The last two fill one struct each, GeneJunctions, by the same steps (declared at the end), and the
// three calls that take a gene annotation share its upload and verdict (annotation_queue, annotation_verdict).  lcr_haplotag.hip
// (lcr_haplotag, lcr_get_haplotag_sites, lcr_haplotag_ms) stands where the phase entry stands and fills the phase stage's result blocks;
// lcr_site_counts.hip (lcr_site_counts, lcr_get_site_counts, lcr_site_counts_ms) and lcr_hap_coverage.hip (lcr_hap_coverage,
// lcr_get_hap_coverage, lcr_hap_coverage_ms) are two more calls behind either of them, lcr_somatic.hip (lcr_somatic, lcr_get_somatic,
// lcr_somatic_ms) a third, lcr_isoforms.hip (lcr_isoforms, lcr_get_isoforms, lcr_isoforms_ms) a fourth, lcr_ends.hip (lcr_transcript_ends,
// lcr_get_transcript_ends, lcr_transcript_ends_ms) a fifth, lcr_retention.hip (lcr_intron_retention, lcr_get_intron_retention,
// lcr_intron_retention_ms) a sixth, lcr_indels.hip (lcr_indels, lcr_get_indels, lcr_indels_ms) a seventh, lcr_site_pairs.hip (lcr_site_pairs, lcr_get_site_pairs, lcr_site_pairs_ms) an eighth.  Every call behind the phase stage keeps its bookkeeping in one CallState
// (below): lcr_ctx::post_calls() lists them for lcr_ctx_create / lcr_ctx_destroy / rewind_to.
#pragma once
#include <algorithm>
#include <array>
#include <cstring>

#include "lcr_dev.h"
#include "lcr_phase_host.h"

// How far the bound batch has come.  Every driver asks for the stage it reads (stage >= X) and moves the value with rewind_to() /
// by assignment at its successful end: nothing else says which buffers hold what.
enum Stage { ST_NONE, ST_LOADED, ST_PILED, ST_CALLED, ST_FRAGGED, ST_PHASED };

// What every call behind the phase stage keeps beside its buffers: whether its last results belong to the phase results of the bound batch
// (rewind_to), the event behind its last kernel, and HIP events around its kernels when timing is on (not a slot of lcr_kernel_ms,
// include/lcr.h).  All three events live from lcr_ctx_create to lcr_ctx_destroy.  The helpers follow lcr_ctx.
struct CallState {
  bool valid = false;        // the getter may hand the last call's results out
  bool timed = false;        // ev_t brackets the last call's kernels
  hipEvent_t ev = nullptr;   // behind the call's host waits, then behind its last kernel: the getter waits for it (no timing)
  hipEvent_t ev_t[2] = {};   // first kernel to last of the last call
};

// The per-candidate segments of the fragment matrix (col_segments.h), shared by lcr_site_counts and lcr_somatic: both run on the context's
// stream, and nothing reads them behind a call's last kernel
struct ColSegs { DevBuf cnt, off, seg; };   // entries per candidate (counted up, then back down); their 64-bit offsets; a word per entry, by candidate

// A gene annotation's five arrays in HBM: where a call copies a host annotation (annotation_queue)
struct AnnotationCopy { DevBuf span_s, span_e, exon_off, exon_s, exon_e; };

// A hash table over the (region, gene) pairs' segments and what becomes of its slots: flagged, counted per region, placed in order.  Three
// of them: K9's junctions, K10's junctions, K10's interior exon blocks.
struct SlotTable {
  int32_t n_slots = 0;                    // of the last fill (slot_table_clear)
  DevBuf tbl_key, tbl_cnt, flag, koff;    // key and count per slot (0xff / 0: empty); kept && n_reads >= min_count; the flags' running sum
  DevBuf ck, cc, cp;                      // the kept slots of a region as the place kernel orders them: key, count, pair
  DevBuf off;                             // kept slots in front of every region (n_regions + 1)
};

// The per-gene junction table of one call (lcr_junctions_genes.hip: the gj_* steps).  The context holds two, lcr_junctions_genes' and
// lcr_asj_genes', so each call keeps its table across the other's.
struct GeneJunctions {
  CallState st;          // valid: the last call's table belongs to the phase results and the gene assignment of the bound batch (rewind_to);
                         // ev: behind the verdict's kernels, the two size waits, then the call's last kernel; ev_t: the list's kernel_ms
  int32_t n = 0, ng = 0;
  AnnotationCopy ann;
  DevBuf part, nocc, part_off, occ_off, cnt, pair_off, read_pair, row_slot, pregion, pgene, prow0, prows, pocc, tsz, tbl_off, rows, keys, jpair;
  SlotTable t;
  DevBuf d_junc;
  HostBuf h_junc, h_off;   // pinned: the records; their offsets per region
  HostBuf h_ctl;           // pinned sizes: [0] participating rows, [1] occurrences, [2] kept junctions, [3] pairs; K10: [4..7] the same for blocks / exons
  HostBuf h_bad;           // pinned verdicts: [0] the annotation's; K10: [1] the DNA sites'
  int32_t *d_off = nullptr, *d_ctl = nullptr;   // h_off and h_ctl as the device sees them (gj_begin)
  K9Pairs pairs() const {
    return {read_pair.as<int32_t>(), row_slot.as<int32_t>(), pregion.as<int32_t>(), pgene.as<int32_t>(), prow0.as<int32_t>(), prows.as<int32_t>(), pocc.as<int32_t>()};
  }
};

// What lcr_asj_genes has beside its GeneJunctions: the exon table, the DNA support, the gene coverage
struct AsjModes {
  int32_t nx = 0, n_genes = 0;   // exon records; genes of the annotation (gene_reads' length)
  bool cov = false;              // the last call counted gene_reads
  DevBuf dna;                    // host DNA sites copied to HBM
  DevBuf nblk, blk_off, pblk, xtsz, xtbl_off, d_exon;   // interior blocks per read, their running sum, per pair; the exon table's segments; the records
  SlotTable x;
  DevBuf sup, sup_uniq, sup_n, cov_n;   // per candidate its supported phase set; per region the distinct ones and their number; reads per gene
  HostBuf h_exon, h_xoff, h_cov;        // pinned: the exon records; their offsets per region; reads per gene
};

struct lcr_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  Stage stage = ST_NONE;

  // bound batch
  BatchView bv{};
  int64_t n_cols = 0, n_bases = 0, n_cigar = 0;
  int32_t n_tiles = 0;
  std::vector<int64_t> h_start0, h_col_off;
  std::vector<int32_t> h_len, h_read_begin, h_region_first_tile;
  DevBuf in_[16];  // device copies of host inputs (LCR_MEM_HOST)
  // asynchronous input path (lcr_load_batch_async / lcr_bind_batch): two staging slots, filled on an upload stream
  struct UploadSlot { DevBuf buf[16]; DevBuf seq4, pack_off;   // (a packed batch: its nibbles and their offsets; buf[] of the bases is the unpack kernel's output)
                      hipEvent_t ev = nullptr; bool filled = false; lcr_reads rd{}; lcr_regions rg{}; } up[2];
  hipStream_t up_stream = nullptr;
  int bound_slot = -1;
  bool bound_host = false;   // the bound batch was copied into in_[] (LCR_MEM_HOST)
  // packed batches (lcr_load_batch_packed, k0_unpack.hip): a host batch's nibbles and offsets in HBM (its bases are unpacked into in_[]);
  // a device batch's unpacked bases; the kernel's verdict word; HIP events around the last unpack kernel when timing is on
  DevBuf in_seq4, in_pack_off, unpacked;
  HostBuf h_unpack_bad;
  hipEvent_t ev_unpack_t[2] = {};
  bool unpack_timed = false;
  DevBuf scan_tmp, read_region, read_bin, read_rend, tile_region, tile_col0, first_tile, k0_tile_fill, k0_items, tile_nbase, tile_order;
  DevBuf desc_tile, desc_val, chunks, chunk_off;   // K0's chunk descriptors, the same sorted by tile, their per-tile offsets
  DevBuf blk_first_read, read_scan, cig_compact, cig_off_new, cig_new_off32;   // K0 op blocks (k0_ops.hip)
  uint64_t cig0 = 0;      // index of the batch's first op in bv.cigar
  uint32_t n_ops = 0;     // ops of the batch (one flat op space)
  int64_t pile_items = 0, pile_recs = 0;   // the last lcr_pileup: M / D / I / N items with a count, records K0 emitted for them (lcr_pileup_records)
  int dbg_fold_indels = 1;   // lcr_debug_set("fold_indels"): 0 = K0 emits a record of its own for every item (no REC_F_INS / REC_F_DEL)

  // K1
  // Which planes exist after lcr_pileup ("Which planes exist when"):
  //   record-free tiles (K0's fill counter == 0)   never written by the stage: their planes are constants -- 0, the intron plane tile_nbase[tile] --
  //                     and what lies at their columns is whatever an earlier batch left there.  planes_dense: the constants have been stored for the
  //                     current pileup (planes_materialise: k1_empty_tiles over the tile order, tile_nbase and n_full of that pileup);
  //   tiles with records   written by the tally in its full form.  In its lean form (sv_staged: ONT presets, fused filter, a survivor guess, "lean_planes")
  //                     the tally keeps its counts in LDS, hands the pass-1 survivors to lcr_candidates as staged records and stores no plane and no
  //                     flag: planes_tallied says whether these tiles' planes are in c->planes.  planes_tally replays k1_pileup in the full form over
  //                     the tables the pileup left -- tile_order / tile_nbase / chunk_off / chunks / k0_items / k0_tile_fill are rewritten by lcr_pileup
  //                     only, tile_region / tile_col0 by lcr_load_batch only, no other stage uses them as scratch, and both calls clear the three flags:
  //                     rewind_to.  All counts are u32 sums, so the replay's planes are the tally's bit for bit.
  // Who reads c->planes, what each calls first, and why a record-free tile that was never written is safe with it:
  //   k1_pileup's fused filter epilogue   nothing: runs in the workgroups of tiles with records, on their LDS counters;
  //   k1_zonefix / _ends / _slots         nothing (HiFi presets: always the full form): atomicSub at the column of an aligned base inside the region: that base's
  //                                       M record is in the tile;
  //   k2_filter (eval_column)             planes_tally (reached only when the fused verdicts cannot be used); leaves at tile_fill == 0 with tile_count = 0;
  //   k2_compact (eval_column, ts planes) planes_tally with the filter outputs when it runs behind a lean pileup (more survivors than the staging buffer holds);
  //                                       leaves at tile_count == 0 -- k2_filter's 0, or k1_tiles_b's on the fused path;
  //   k2_place / k2_hist / k2_hist_tiles / k2_gt, K3, K4   never touch the planes (k2_hist_tiles walks K0's records of tiles with tile_count > 0);
  //   k2_import_emit                      planes_tally; takes the four counts of a site in a tile with tile_fill == 0 as 0 without loading them;
  //   lcr_get_columns                     planes_materialise (planes_tally + the constants): the one reader of every column.
  // planes_tally / planes_materialise read, beside those tables, bv.error_flag (K0Ctl::error in k0_tile_fill, 0 after a pileup that returned LCR_OK), the
  // batch's bases and reference, and the region arrays bv.len / bv.col_off: the context's copies of a host batch, the caller's arrays of a LCR_MEM_DEVICE
  // batch, which therefore have to stay alive for lcr_get_columns as for every stage call (include/lcr.h).
  // lcr_debug_set("poison_planes", 1) fills the whole buffer with 0xA5 in front of every pileup: a reader that looks at an unwritten tile
  // then differs from a run without it, whatever the previous batch was (tests/test_sparse_planes.py, tests/test_lean_planes_gpu.py).
  bool planes_dense = false;
  bool planes_tallied = false;
  int dbg_poison_planes = 0;
  int dbg_lean_planes = 1;    // lcr_debug_set("lean_planes"): 0 = the tally always stores its planes (and, fused, the flags)
  DevBuf planes;
  // the lean tally's hand-over: survivor records in the order the tiles drew their slots, beside each its (tile, rank in tile); their number is
  // TileScanTmp::n_staged in the cleared pileup scratch (exact even beyond the capacity)
  bool sv_staged = false;     // the last lcr_pileup left them, with flt_count, for the parameters flt_dp
  int32_t sv_stage_cap = 0;   // records the two buffers hold (the survivor guess of that pileup)
  int64_t sv_stage_n = -1;    // records stored: min(n_staged, capacity) once the host has read n_staged (lcr_candidates, or the byte getters), -1 before
  DevBuf sv_stage, sv_stage_key;
  DevParams dp{};
  int32_t pile_platform = -1; uint32_t pile_dist_to_end = 0;   // lcr_pileup's platform / dist_to_end: lcr_candidates must be called with the same
  float sor_thr = -1.f;
  HostBuf h_planes;
  HostBuf h_nnz;              // pinned: first entry of every region of the fragment matrix, [ng] = entry count (lcr_fragments -> frag_settle)
  DevBuf region_e_off, frag_tmp_col, frag_tmp_val;
  // one of each per context (lcr_ctx_create): K0's verdict, the survivors' number, the candidate stage's host copies, the entry counts,
  // the verdict on device-resident import sites
  hipEvent_t ev_ctl = nullptr, ev_sv = nullptr, ev_cand = nullptr, ev_nnz = nullptr, ev_imp = nullptr;
  int32_t sv_cap_guess = 0;   // lcr_candidates: survivors the buffers are sized for before their number is known (the last call's + a quarter; 0: wait first)
  bool nnz_pending = false, cand_pending = false;
  HostBuf h_order;      // pinned: k0_pack raises it when a region's reads are not sorted by position
  static constexpr int UP_LANES = 4;   // staging lanes of pageable host uploads (upload_bytes): two page-locked 8 MB buffers + events each
  HostBuf h_up[2 * UP_LANES]; hipEvent_t ev_up[2 * UP_LANES] = {}; bool up_busy[2 * UP_LANES] = {};
  HostBuf h_stage[4];   // pinned staging of lcr_candidates / lcr_fragments: survivor offsets, candidate records, keep flags, region rows

  // K2
  bool cand_used = false;   // lcr_phase has rewritten the records' FOR_PHASING bit, variant type and genotype (k4_post.h), which K3 and k4_stage read:
                            // lcr_fragments / lcr_phase need a fresh candidate stage
  DevBuf flags, tile_count, tile_off, total, survivors, sv_region_off, hist, cand_tmp, keep;
  DevBuf hit_cnt, hit_list, ovf_list;   // k2_hist's (read, survivor) hits for K3; the overflow counter sits behind the histograms
  bool hits_valid = false; int32_t hits_n_sv = 0;
  int dbg_hist_tiles = 0;   // lcr_debug_set("hist_tiles"): 0 = by survivor density, 1 = the tile form whenever it applies, -1 = never
  int dbg_spec_compact = 1; // lcr_debug_set("spec_compact"): 0 = lcr_candidates waits for the survivors' number before it queues their compaction
  int dbg_fuse_filter = 1;  // lcr_debug_set("fuse_filter"): 0 = pass 1 of the candidate filters always by k2_filter (its own pass over the planes)
  bool flt_fused = false;   // the last lcr_pileup left k2_filter's flags and per-tile counts (ONT presets: no poly-A pass behind the tally)
  DevParams flt_dp{};       // ... computed with these parameters
  // the exon-only mask (lcr_set_exon_mask): bv.exon_mask names the plane while a mask is set (nullptr: none; rewind_to clears it with the binding).
  // Every set or clear draws a new mask_gen; lcr_pileup notes the one its epilogue filtered under (flt_mask_gen), cand_queue_pass1 compares.
  uint64_t mask_gen = 0, flt_mask_gen = 0;
  DevBuf exon_plane, ex_off, ex_s, ex_e;   // the bit plane; host interval lists copied to HBM
  hipEvent_t ev_mask_t[2] = {};            // timing enabled: around the last build (clear + k2_exon_build), created on first use
  bool mask_timed = false;
  int dbg_k3_hits = 1;      // lcr_debug_set("k3_hits"): 0 = K3's count pass walks every read's CIGAR itself (the path of batches without hit lists)
  int dbg_k3_list_blocks = 0;   // lcr_debug_set("k3_list_blocks"): workgroups that walk the overflow list in K3's two passes; 0 = sized from the batch's reads
  std::vector<lcr_candidate> h_cand;
  std::vector<int32_t> h_cand_off;
  DevBuf d_cand, d_cand_off;
  DevBuf imp_pos, imp_gt, imp_q, imp_cnt;   // lcr_import_candidates: host sites copied to HBM, sites kept per region
  HostBuf h_imp_bad;                         // ... verdict of the check of device-resident sites

  // K3
  uint32_t min_linkers = 1;
  int32_t n_rows = 0;
  int64_t nnz = 0;
  std::vector<int32_t> h_row_region_off;
  DevBuf region_rows, row_region_off, row_cnt, row_links, row_ptr, col, val;
  HostBuf h_row_ptr, h_row_read, h_col, h_val, h_row_fp, h_row_links;

  // K4 + post-phase
  bool res_valid = false;   // lcr_collect_phase: the last lcr_phase's results (host + HBM) are intact -- they outlive lcr_load_batch / lcr_pileup of the next batch
  int32_t res_ng = 0;
  int phase_slot = -1;      // staging slot of the batch whose (asynchronous) phase stage may be in flight: -1 = the caller's own device arrays, -2 = in_[] (a host batch)
  PhaseHost phase;
  std::vector<int32_t> ld_off, ld_snps;   // lcr_get_ld_blocks
  // down-sampling: the sticky setting (lcr_set_downsample; 0 = off) and the caller's own sample for the next lcr_phase (lcr_set_downsample_rows)
  uint32_t ds_depth = 0; uint64_t ds_seed = 0;
  std::vector<uint8_t> ds_rows; bool ds_rows_set = false;

  // K11 (lcr_haplotag, in place of lcr_phase): it fills what the phase stage fills -- the candidate records, PhaseHost's pinned result blocks
  // and read records -- and owns the site arrays, the per-candidate site byte / phase set, and the site records
  CallState hap;             // lcr_get_haplotag_sites; ev: behind the sites' check, then behind the call's last kernel
  bool hap_pending = false;  // its kernels may be in flight: haplotag_settle waits for hap.ev and copies the candidate mirror into h_cand
  int32_t hap_ncand = 0;
  DevBuf ht_pos, ht_h1, ht_h2, ht_ps, ht_site, ht_site_ps, d_hsite;   // host sites copied to HBM; a byte and a word per candidate; the records
  HostBuf h_hsite, h_hap_bad;            // pinned: the site records; the verdict on the sites

  // K6 (lcr_junctions): scratch and results of its own -- no other stage or getter reads them
  CallState junc;            // lcr_get_junctions (timed by LCR_K_JUNCTIONS: ev_t is not used)
  int32_t junc_n = 0, junc_ng = 0;
  DevBuf j_part, j_npair, j_part_off, j_pair_off, j_tsz, j_tbl_off, j_rows, j_keys, j_tbl_key, j_tbl_cnt, j_flag, j_koff, j_ck, j_cc, j_cg, j_off, d_junc;
  HostBuf h_junc_ctl, h_junc, h_junc_off;   // pinned: {participating rows, pairs, kept junctions}; the records; their offsets per region

  // K7 (lcr_ase): scratch and results of its own -- no other stage or getter reads them
  CallState ase;             // lcr_get_ase; ev: behind the sites' check, then behind the call's last kernel (timed by LCR_K_ASE: ev_t is not used)
  int32_t ase_ng = 0;
  DevBuf a_pos, a_pat, a_mat, a_tag, a_site, d_ase;   // host sites copied to HBM; a word per row, a byte per candidate; the records
  HostBuf h_ase, h_ase_bad;                            // pinned: the records; the verdict on the parental sites

  // K12 (lcr_site_counts) and K14 (lcr_somatic): the segments they share; results of their own -- no other stage or getter reads them
  ColSegs colsegs;
  CallState sc;              // lcr_get_site_counts
  int32_t sc_ncand = 0;
  DevBuf d_sc;               // the records
  HostBuf h_sc;              // pinned: the records
  CallState som;             // lcr_get_somatic
  int32_t som_ncand = 0;
  DevBuf d_som;              // the records
  HostBuf h_som;             // pinned: the records

  // K13 (lcr_hap_coverage): scratch and results of its own -- no other stage or getter reads them
  CallState hc;              // lcr_get_hap_coverage; ev: behind the count pass, then behind the call's last kernel
  int32_t hc_ng = 0, hc_n = 0;
  DevBuf hc_planes, hc_nseg, hc_off, hc_send, d_hc_seg, d_hc_reg;   // three u32 planes (differences, then depths); run starts per region; their offsets; a segment's end column; the records
  HostBuf h_hc_seg, h_hc_off, h_hc_reg;   // pinned: the segments; their offsets per region; the region records

  // K15 (lcr_isoforms): scratch and results of its own -- no other stage or getter reads them
  CallState iso;             // lcr_get_isoforms; ev: behind the two size waits, then behind the call's last kernel
  int32_t iso_ng = 0, iso_n = 0, iso_nchain = 0, iso_nrows = 0;
  int dbg_iso_hash_bits = 64;   // lcr_debug_set("iso_hash_bits"): the low bits of a chain's hash that route it; identity never depends on them
  DevBuf iso_part, iso_npair, iso_part_off, iso_pair_off, iso_tsz, iso_tbl_off;   // per read: participates, junctions, their running sums; per region: its table segment
  DevBuf iso_rows, iso_keys, iso_hash, iso_row_slot;                              // per participating row: record, keys, chain hash, the slot it joined
  DevBuf iso_tbl_rep, iso_tbl_cnt, iso_flag, iso_koff, iso_plen, iso_poff;        // per slot: representative row, n_h1 / n_h2, kept, kept in front, chain length, keys in front
  DevBuf iso_off, iso_pbase, iso_cslot, iso_crank;                                // per region: kept chains / pool entries in front; per kept slot: its slot, its record
  DevBuf d_iso, d_iso_chain, d_iso_row;                                           // the records, the pool, row_isoform
  HostBuf h_iso_ctl, h_iso, h_iso_off, h_iso_chain, h_iso_row;   // pinned: {participating rows, pairs, kept chains, pool entries}; the four outputs

  // K16 (lcr_transcript_ends): scratch and results of its own -- no other stage or getter reads them
  CallState ends;            // lcr_get_transcript_ends; ev: behind the two size waits, then behind the call's last kernel
  int32_t ends_ng = 0, ends_n = 0, ends_nrows = 0, ends_npart = 0;
  int dbg_ends_hash_bits = 32;   // lcr_debug_set("ends_hash_bits"): the low bits of a key's hash that route it; the results never depend on them
  DevBuf e_part, e_part_off, e_tsz, e_tbl_off;        // per read: participates, the running sum; per region: its table segment
  DevBuf e_rows;                                      // per participating row: its record (ends' slots, then their records)
  DevBuf e_tbl_key, e_tbl_cnt, e_slot, e_flag, e_koff;   // per slot: key, c_h1 / c_h2, peak / target / the peak's sums, kept, kept in front
  DevBuf e_off, e_cslot, e_crank, e_nasg;             // per region: kept sites in front; per kept slot: its slot, its record; n_assigned
  DevBuf d_end, d_end_row;                            // the records, row_site
  HostBuf h_end_ctl, h_end, h_end_off, h_end_row;     // pinned: {participating rows, kept sites, n_assigned (64 bit)}; the three outputs

  // K17 (lcr_intron_retention): scratch and results of its own -- no other stage or getter reads them
  CallState ret;             // lcr_get_intron_retention; ev: behind the two size waits, then behind the call's last kernel
  int32_t ret_ng = 0, ret_n = 0, ret_nrows = 0, ret_npart = 0;
  int dbg_ir_hash_bits = 32;     // lcr_debug_set("ir_hash_bits"): the low bits of a key's hash that route it; the results never depend on them
  DevBuf r_part, r_npair, r_part_off, r_pair_off, r_tsz, r_tbl_off;   // per read: participates, junctions, their running sums; per region: its table segment
  DevBuf r_rows, r_keys;                                              // per participating row: its record; its junction keys
  DevBuf r_tbl_key, r_tbl_cnt, r_flag, r_koff;                        // per slot: key, rows that hold it, kept, kept in front
  DevBuf r_off, r_ck, r_cc, r_cg, r_ntot;                             // per region: kept introns in front; per kept slot: key, count, region; n_retained_total
  DevBuf d_ret, d_ret_row;                                            // the records, row_retained
  HostBuf h_ret_ctl, h_ret, h_ret_off, h_ret_row;     // pinned: {participating rows, pairs, kept introns, -, n_retained_total (64 bit)}; the three outputs

  // K18 (lcr_indels): scratch and results of its own -- no other stage or getter reads them
  CallState indel;           // lcr_get_indels; ev: behind the two size waits, then behind the call's last kernel
  int32_t ind_ng = 0, ind_n = 0, ind_nrows = 0, ind_npart = 0;
  int64_t ind_nev = 0;
  int dbg_indel_hash_bits = 32;  // lcr_debug_set("indel_hash_bits"): the low bits of a key's hash that route it; the results never depend on them
  DevBuf i_part, i_ngap, i_nev, i_part_off, i_gap_off, i_ev_off, i_tsz, i_tbl_off;   // per read: participates, gaps, events, their running sums; per region: its table segment
  DevBuf i_rows, i_gaps, i_gap_read;                                  // per participating row: its record; per gap: its record, its read
  DevBuf i_diff, i_dscan;                                             // per window column (+ 1 per region): block-end differences, their exclusive scan
  DevBuf i_tbl_key, i_tbl_cnt, i_flag, i_koff;                        // per slot: key, rows that hold it, kept, kept in front
  DevBuf i_off, i_ck, i_cc, i_cg, i_ntot;                             // per region: kept events in front; per kept slot: key, count, region; n_present_total
  DevBuf d_ind, d_ind_row;                                            // the records, row_indels
  HostBuf h_ind_ctl, h_ind, h_ind_off, h_ind_row;     // pinned: {participating rows, gaps, kept events, event occurrences, n_present_total (64 bit)}; the three outputs

  // K19 (lcr_site_pairs): scratch and results of its own -- no other stage or getter reads them
  CallState pairs;           // lcr_get_site_pairs; ev: behind the call's last kernel (the call has no host wait)
  int32_t sp_ncand = 0;
  DevBuf sp_elig, sp_rank, sp_list, sp_erank, sp_m, sp_ctl;   // per candidate: eligible, its rank, rank -> candidate, rank or -1, pairs it starts; n_eligible
  DevBuf sp_off, d_sp;                                        // pair_off (n_cand + 1); the records
  HostBuf h_sp, h_sp_off, h_sp_ctl;                           // pinned: the records; pair_off; {n_eligible, n_pairs}

  // K8 (lcr_assign_genes): read -> gene of the bound batch; (lcr_ase_genes): the per-gene counts -- scratch and results of their own
  bool genes_valid = false;  // lcr_get_read_genes / lcr_ase_genes: the last lcr_assign_genes' result belongs to the bound batch (rewind_to)
  int32_t genes_nr = 0, genes_n_genes = 0;   // reads of that batch; genes of that annotation (lcr_junctions_genes takes the annotation again)
  AnnotationCopy g_ann;
  DevBuf g_pmax, d_gene, d_gene_ov;        // running maximum of the spans' ends; the result
  HostBuf h_gene, h_gene_ov, h_gene_bad;   // pinned: the result; the verdict on the annotation
  hipEvent_t ev_genes = nullptr;           // behind the annotation's check, then behind the copies of the result
  CallState agene;           // lcr_get_ase_genes: the records belong to the phase results and the gene assignment of the bound batch (timed by LCR_K_ASE_GENES)
  int32_t agene_ng = 0, agene_n = 0;
  DevBuf ag_pos, ag_pat, ag_mat, ag_cnt, ag_off, ag_tag, ag_site, ag_site_ps, d_agene;
  HostBuf h_agene, h_agene_off, h_agene_ctl, h_agene_bad;   // pinned: the records; their offsets per region; the number of pairs; the verdict on the parental sites

  // K9 (lcr_junctions_genes) and K10 (lcr_asj_genes): one per-gene junction table each (GeneJunctions: the same steps fill both), and beside
  // K10's what its other modes add (AsjModes) -- scratch and results of their own, no other stage or getter reads them, each other's included
  GeneJunctions jgene, ajgene;
  AsjModes asj;

  // every call behind the phase stage: their events are created and destroyed, and their results invalidated, through this list
  std::array<CallState*, 14> post_calls() { return {&hap, &junc, &ase, &agene, &sc, &hc, &som, &iso, &ends, &ret, &indel, &pairs, &jgene.st, &ajgene.st}; }

  // region discovery (N3)
  DevBuf rd_start, rd_end, rd_diff, rd_ex, rd_cnt, rd_off, rd_s, rd_e, rd_max;
  std::vector<int64_t> rl_start0;
  std::vector<int32_t> rl_len;
  std::vector<uint32_t> rl_max;

  // timing
  bool timing = false;
  uint32_t timing_mask = 0;   // lcr_debug_set("timing_mask"): bit k = LCR_K_* k is timed; 0 = all of them (every timer is two event records on the stream)
  hipEvent_t ev[LCR_NTIMERS][2] = {};
  bool ev_valid[LCR_NTIMERS] = {};
  int64_t pileup_bytes = 0, stage_bytes = 0;   // of the last lcr_pileup; behind a lean tally (pile_lean) without the 48 bytes per staged survivor (sv_stage_n)
  bool pile_lean = false;
};

// Back to stage `to` (no-op above it): a driver calls this at the point where it begins to overwrite what the stages behind `to` read --
// not at its successful end, so a call that fails part of the way leaves nothing downstream looking valid -- and sets its own stage
// when it has queued everything.  What belongs to the stages that are dropped goes with them, each rule once:
inline void rewind_to(lcr_ctx* c, Stage to) {
  if (c->stage > to) c->stage = to;
  if (to < ST_PILED) {
    c->planes_dense = false;   // tile order / tile_nbase / tile tables are rewritten: the stored constants are another pileup's (or batch's)
    c->planes_tallied = false; // ... and so are the planes of the tiles with records
    c->sv_staged = false;      // ... and the staged survivors
    c->flt_fused = false;      // the tally's epilogue has not left this pileup's pass-1 flags yet
  }
  if (to < ST_LOADED) c->bv.exon_mask = nullptr;   // the exon mask names the columns of ONE bound batch
  if (to < ST_CALLED) {
    c->hits_valid = false;     // k2_hist's hit lists name the survivors of the candidate stage that is going away
    c->cand_used = false;      // the records lcr_phase rewrote are replaced by the next candidate stage
  }
  if (to < ST_FRAGGED) c->ds_rows_set = false;   // a sample names the rows of ONE fragment stage
  if (to < ST_PHASED) for (CallState* st : c->post_calls()) st->valid = false;   // every table and record list behind the phase stage counts the rows of ONE phase stage
  if (to < ST_LOADED) c->genes_valid = false;    // read -> gene names the reads of ONE bound batch (what was built on it -- agene, jgene, ajgene -- went above)
  // Deliberately not here: res_valid / res_ng (the last phase's results outlive load and pileup of the next batch and die at the next
  // candidate stage: cand_begin), sv_cap_guess (a size guess, good across batches), phase_slot (names the batch of a stage in flight),
  // cand_pending / nnz_pending (hand-overs of copies in flight: their settle functions are only reached through a valid stage), and
  // flt_fused across a candidate stage that does not overwrite the flags (lcr_import_candidates: to == ST_PILED).
}

struct Timer {  // records HIP events on the ctx stream around one kernel
  lcr_ctx* c; int k;
  bool on() const { return c->timing && (c->timing_mask == 0 || ((c->timing_mask >> k) & 1u)); }
  Timer(lcr_ctx* c_, int k_) : c(c_), k(k_) { if (on()) { (void)hipEventRecord(c->ev[k][0], c->stream); } }
  ~Timer() { if (on()) { (void)hipEventRecord(c->ev[k][1], c->stream); c->ev_valid[k] = true; } }
};

inline DevParams to_dev(const lcr_params* p, float sor_thr) {
  DevParams d{};
  d.ont = p->platform == LCR_PLATFORM_ONT;
  d.dist_to_end = (int32_t)p->dist_to_end;
  d.polya_len = (int32_t)p->polya_len;
  d.min_baseq = p->min_baseq; d.min_depth = p->min_depth; d.max_depth = p->max_depth; d.min_qual = p->min_qual;
  d.low_cnt_cut = p->low_cnt_cut; d.min_linkers = p->min_linkers; d.use_strand_bias = p->use_strand_bias;
  d.min_af = p->min_af; d.min_af_intron = p->min_af_intron; d.low_frac_cut = p->low_frac_cut;
  d.sor_threshold = sor_thr;
  return d;
}

// Host -> device copy of a caller's array on a queue of the context (nullptr: its stream); lcr_batch.hip
int upload_bytes(lcr_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t q = nullptr);

template <class T>
int upload(lcr_ctx* c, DevBuf& buf, const T* src, size_t n, const T** dst, int mem) {
  if (mem == LCR_MEM_DEVICE) { *dst = src; return LCR_OK; }
  HIPCHK(c, buf.reserve(std::max<size_t>(n, 1) * sizeof(T)));
  if (n) { const int rc = upload_bytes(c, buf.p, src, n * sizeof(T)); if (rc) return rc; }
  *dst = buf.as<T>();
  return LCR_OK;
}

// lcr_phase leaves its kernels in flight on the phase stage's own queues (lcr_phase_host.h): whoever needs its results, or is about
// to overwrite what it reads / writes, collects them first
int haplotag_settle(lcr_ctx* c);   // lcr_haplotag stands in place of lcr_phase and leaves its kernels in flight on the context's stream (lcr_haplotag.hip)
inline int phase_settle(lcr_ctx* c) {
  const int rc = c->phase.settle(&c->err);
  if (rc || !c->hap_pending) return rc;
  return haplotag_settle(c);
}
int cand_settle(lcr_ctx* c);   // the candidate stage's host copies (lcr_calls.hip)
// lcr_pileup.hip.  planes_tally: the planes of the tiles with records are in c->planes -- behind a lean pileup it queues k1_pileup's full form once
// (with_filter: with pass 1's flags and per-tile counts for the pileup's parameters, as a full fused pileup leaves them).  planes_materialise: that and
// the record-free tiles' constants.  pile_staged_bytes: what the byte getters add behind a lean tally, 48 sv_stage_n (waits for the tally if nobody has
// read the count yet); 0 otherwise.
int planes_tally(lcr_ctx* c, bool with_filter);
int planes_materialise(lcr_ctx* c);
int pile_staged_bytes(lcr_ctx* c, int64_t* bytes);
int frag_settle(lcr_ctx* c);   // lcr_fragments' entry count (lcr_calls.hip)

// A host wait on the context's stream: what the kernels queued so far left in pinned memory is the host's to read
inline int stream_wait(lcr_ctx* c, hipEvent_t ev) {
  HIPCHK(c, hipEventRecord(ev, c->stream));
  HIPCHK(c, hipEventSynchronize(ev));
  HIPCHK(c, hipGetLastError());
  return LCR_OK;
}

// The bookkeeping of a call behind the phase stage (CallState).  A driver clears valid where it begins to overwrite the last call's results.
// Bracket: the timing events around the call's kernels, closed before call_end.  call_end: the event the getter waits for; valid.  call_wait: the
// getter's wait.  call_ms: the body of lcr_<call>_ms.
struct Bracket {
  lcr_ctx* c; CallState& st;
  Bracket(lcr_ctx* c_, CallState& st_) : c(c_), st(st_) { if (c->timing) (void)hipEventRecord(st.ev_t[0], c->stream); }
  ~Bracket() { if (c->timing) { (void)hipEventRecord(st.ev_t[1], c->stream); st.timed = true; } }
};
inline int call_end(lcr_ctx* c, CallState& st) {
  HIPCHK(c, hipEventRecord(st.ev, c->stream));
  HIPCHK(c, hipGetLastError());
  st.valid = true;
  return LCR_OK;
}
inline int call_wait(lcr_ctx* c, CallState& st) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(st.ev));
  HIPCHK(c, hipGetLastError());
  return LCR_OK;
}
inline int call_ms(lcr_ctx* c, CallState& st, const char* fn_ms, const char* fn, float* ms) {
  if (!c->timing || !st.timed) { c->err = std::string(fn_ms) + ": no " + fn + " with timing enabled"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(st.ev_t[1]));
  HIPCHK(c, hipEventElapsedTime(ms, st.ev_t[0], st.ev_t[1]));
  return LCR_OK;
}

// The per-candidate segments of the bound batch's fragment matrix, queued for n_cand > 0 candidates (lcr_site_counts.hip): reserve, clear,
// count, scan -> the counters (to be counted back down by the caller's fill), the 64-bit offsets, the words' buffer
int colseg_queue(lcr_ctx* c, int32_t n_cand, uint32_t** cnt, int64_t** off, uint64_t** seg);

// A gene annotation on its way to the kernels (lcr_genes.hip; lcr_assign_genes, lcr_junctions_genes, lcr_asj_genes).  annotation_queue:
// copied (host) or read in place (device) -> *d, and k8_check queued on it into word 0 of the pinned verdict block, whose two words are
// zeroed here (-> *d_bad, the block as the device sees it; no kernel for an annotation without genes).  The caller queues what else
// belongs in front of the wait, then annotation_verdict: the wait on `ev`, and LCR_E_ARG with `fn`'s name in the text when word 0 is set.
int annotation_queue(lcr_ctx* c, AnnotationCopy& to, const lcr_gene_annotation* a, int32_t mem, HostBuf& h_bad, lcr_gene_annotation* d, int32_t** d_bad);
int annotation_verdict(lcr_ctx* c, const HostBuf& h_bad, hipEvent_t ev, const char* fn);

// The steps that fill a GeneJunctions, in the order of their launches (lcr_junctions_genes.hip).  lcr_junctions_genes is these and nothing
// else; lcr_asj_genes queues K10's kernels between them.  The host waits twice in between: gj_wait_counts and a stream_wait.  Their
// kernels stand inside a Bracket on g.st.
int gj_begin(lcr_ctx* c, GeneJunctions& g);   // from here on the last table is overwritten: valid = false, the pinned blocks reserved and quiet, h_ctl zeroed
int gj_counts(lcr_ctx* c, GeneJunctions& g, uint32_t min_junctions);   // junctions per read, participating reads, the pairs, their table segments -> h_ctl[0], [1], [3]
int gj_wait_counts(lcr_ctx* c, GeneJunctions& g, const char* fn, bool* empty);   // the first wait -> no participating row or no occurrence; LCR_E_ARG beyond 2^28 of them
int slot_table_clear(lcr_ctx* c, SlotTable& t, int32_t n_slots);       // reserved for n_slots and emptied
int gj_rows(lcr_ctx* c, GeneJunctions& g, const lcr_gene_annotation& d);   // row records, keys, the table: 4 x all occurrences bound its slots without a third wait
int gj_keep(lcr_ctx* c, SlotTable& t, const int32_t* pair_off, const int32_t* tbl_off, uint32_t min_count, int32_t* d_hoff, int32_t* d_ctl);   // -> pinned offsets, d_ctl[2]
int gj_tables(lcr_ctx* c, GeneJunctions& g, int32_t n_kept);           // order, motif, tables: the records go to HBM and to pinned host memory
void no_records(const HostBuf& h_off, int32_t ng, int32_t* n);         // a table without a record: every region's offset and *n are 0
int gj_finish(lcr_ctx* c, GeneJunctions& g);                           // the event the getter waits for; valid
template <class List>   // lcr_junction_gene_list, lcr_asj_gene_list: the getter's wait, the fields both lists have, kernel_ms
int gj_get(lcr_ctx* c, GeneJunctions& g, List* out) {
  { int rc = call_wait(c, g.st); if (rc) return rc; }
  out->n_regions = g.ng; out->n_junctions = g.n;
  out->junc = g.n ? g.h_junc.as<lcr_junction_gene>() : nullptr;
  out->junc_region_off = g.h_off.as<int32_t>();
  out->dev_junc = g.n ? g.d_junc.as<lcr_junction_gene>() : nullptr;
  out->kernel_ms = -1.f;
  if (c->timing && g.st.timed) {
    HIPCHK(c, hipEventSynchronize(g.st.ev_t[1]));
    HIPCHK(c, hipEventElapsedTime(&out->kernel_ms, g.st.ev_t[0], g.st.ev_t[1]));
  }
  return LCR_OK;
}

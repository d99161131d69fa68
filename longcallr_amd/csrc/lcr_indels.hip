// lcr_indels.hip — the host driver of K18 (k18_indels.hip): the phased small-indel records over the fragment rows, their getter and their
// timer.  A call of its own behind lcr_phase / lcr_haplotag, shaped like lcr_intron_retention: it reads the bound batch (CIGARs, bases,
// positions, the window reference, region tables), the fragment stage's row offsets and the phase stage's read records, and writes buffers
// no other stage or getter reads (lcr_ctx: i_*, d_ind*, h_ind*).  Two host waits: participating rows, gaps and events, then kept events.
#include "lcr_ctx.h"

namespace {

// the kernels of one call; *n_part / *n_ev / *n_kept stay 0 when a wait finds nothing to go on with
int indels_queue(lcr_ctx* c, const lcr_indel_params* p, uint32_t min_count, int32_t* d_ctl, int32_t* d_hoff, int32_t* n_part_out, int64_t* n_ev_out,
                 int32_t* n_kept_out) {
  const BatchView& b = c->bv;
  const int nr = b.n_reads, ng = b.n_regions;
  hipStream_t s = c->stream;
  const int32_t* const h_ctl = c->h_ind_ctl.as<int32_t>();
  if (nr == 0 || ng == 0 || c->n_rows == 0) return LCR_OK;
  const lcr_read_record* rec = c->phase.d_read_rec.as<lcr_read_record>();
  const int32_t* rro = c->row_region_off.as<int32_t>();
  const int bits = c->dbg_indel_hash_bits;
  const uint32_t hash_mask = bits >= 32 ? ~0u : bits <= 0 ? 0u : ((1u << bits) - 1u);
  // 1. gaps and events per read, participating rows; their offsets; the table segments
  HIPCHK(c, c->i_part.reserve((size_t)nr * 4)); HIPCHK(c, c->i_ngap.reserve((size_t)nr * 4)); HIPCHK(c, c->i_nev.reserve((size_t)nr * 4));
  HIPCHK(c, c->i_part_off.reserve(((size_t)nr + 1) * 4)); HIPCHK(c, c->i_gap_off.reserve(((size_t)nr + 1) * 4));
  HIPCHK(c, c->i_ev_off.reserve(((size_t)nr + 1) * 4));
  HIPCHK(c, c->i_tsz.reserve((size_t)ng * 4)); HIPCHK(c, c->i_tbl_off.reserve(((size_t)ng + 1) * 4)); HIPCHK(c, c->i_off.reserve(((size_t)ng + 1) * 4));
  int32_t* part_off = c->i_part_off.as<int32_t>();
  int32_t* gap_off = c->i_gap_off.as<int32_t>();
  int32_t* ev_off = c->i_ev_off.as<int32_t>();
  int32_t* tbl_off = c->i_tbl_off.as<int32_t>();
  launch_k18_count(b, rro, rec, p->max_ins, p->max_del, c->i_part.as<int32_t>(), c->i_ngap.as<int32_t>(), c->i_nev.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->i_part.as<int32_t>(), part_off, nr, part_off + nr, s);
  launch_scan_i32(c->scan_tmp, c->i_ngap.as<int32_t>(), gap_off, nr, gap_off + nr, s);
  launch_scan_i32(c->scan_tmp, c->i_nev.as<int32_t>(), ev_off, nr, ev_off + nr, s);
  launch_k18_sizes(b, part_off, gap_off, ev_off, c->i_tsz.as<int32_t>(), d_ctl, s);
  launch_scan_i32(c->scan_tmp, c->i_tsz.as<int32_t>(), tbl_off, ng, tbl_off + ng, s);
  { int rc = stream_wait(c, c->indel.ev); if (rc) return rc; }   // the host sizes the row and gap records and the table from the three totals
  const int32_t n_part = h_ctl[0], n_gaps = h_ctl[1], n_ev = h_ctl[3];
  if (n_part <= 0) return LCR_OK;
  *n_part_out = n_part;
  if (n_ev < 0 || n_ev > (1 << 28) || n_gaps < 0 || n_gaps > (1 << 28)) {
    c->err = "lcr_indels: more than 2^28 gaps or event occurrences in one batch; split it"; return LCR_E_ARG;
  }
  *n_ev_out = n_ev;
  if (n_ev == 0) return LCR_OK;   // no row holds an event
  // 2. row and gap records, the block-end differences and their scan, the regions' table segments.  A segment has fewer than 4 x its events
  // in slots, so 4 x all events bounds the table without a third wait; the slots behind the last segment stay empty.
  const int32_t n_slots = 4 * n_ev;
  const int32_t n_diff = (int32_t)(c->n_cols + ng);   // (lcr_indels has checked that it fits)
  HIPCHK(c, c->i_rows.reserve((size_t)n_part * launch_k18_row_bytes()));
  HIPCHK(c, c->i_gaps.reserve((size_t)n_gaps * launch_k18_gap_bytes())); HIPCHK(c, c->i_gap_read.reserve((size_t)n_gaps * 4));
  HIPCHK(c, c->i_diff.reserve((size_t)n_diff * 4)); HIPCHK(c, c->i_dscan.reserve(((size_t)n_diff + 1) * 4));
  HIPCHK(c, c->i_tbl_key.reserve((size_t)n_slots * 8)); HIPCHK(c, c->i_tbl_cnt.reserve((size_t)n_slots * 4));
  HIPCHK(c, c->i_flag.reserve((size_t)n_slots * 4)); HIPCHK(c, c->i_koff.reserve(((size_t)n_slots + 1) * 4));
  HIPCHK(c, lcr_fill_async(c->i_diff.p, 0, (size_t)n_diff * 4, s));
  HIPCHK(c, lcr_fill_async(c->i_tbl_key.p, 0xff, (size_t)n_slots * 8, s));
  HIPCHK(c, lcr_fill_async(c->i_tbl_cnt.p, 0, (size_t)n_slots * 4, s));
  int32_t* dscan = c->i_dscan.as<int32_t>();
  launch_k18_emit(b, rro, rec, p->max_ins, p->max_del, c->i_part.as<int32_t>(), part_off, gap_off, c->i_rows.p, c->i_gaps.p, c->i_gap_read.as<int32_t>(),
                  c->i_diff.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->i_diff.as<int32_t>(), dscan, n_diff, dscan + n_diff, s);
  launch_k18_insert(b, c->i_gaps.p, c->i_gap_read.as<int32_t>(), gap_off, n_gaps, tbl_off, hash_mask, c->i_tbl_key.as<uint64_t>(),
                    c->i_tbl_cnt.as<uint32_t>(), s);
  // 3. kept events and their number per region
  int32_t* koff = c->i_koff.as<int32_t>();
  launch_k18_flag(b, c->i_tbl_key.as<uint64_t>(), c->i_tbl_cnt.as<uint32_t>(), n_slots, tbl_off, dscan, min_count, p->min_permille, c->i_flag.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->i_flag.as<int32_t>(), koff, n_slots, koff + n_slots, s);
  launch_k18_offsets(tbl_off, koff, ng, n_slots, c->i_off.as<int32_t>(), d_hoff, d_ctl, s);
  { int rc = stream_wait(c, c->indel.ev); if (rc) return rc; }   // the number of kept events sizes the records and the last kernels' grids
  const int32_t n_kept = h_ctl[2];
  if (n_kept <= 0) return LCR_OK;
  // 4. order, extent, tables: the records go to HBM and, by the same kernel, to pinned host memory
  HIPCHK(c, c->i_ck.reserve((size_t)n_kept * 8)); HIPCHK(c, c->i_cc.reserve((size_t)n_kept * 4)); HIPCHK(c, c->i_cg.reserve((size_t)n_kept * 4));
  HIPCHK(c, c->d_ind.reserve((size_t)n_kept * sizeof(lcr_indel)));
  HIPCHK(c, c->h_ind.reserve((size_t)n_kept * sizeof(lcr_indel)));
  lcr_indel* d_hind = nullptr;
  HIPCHK(c, c->h_ind.dev(&d_hind));
  launch_k18_place(b, c->i_tbl_key.as<uint64_t>(), c->i_tbl_cnt.as<uint32_t>(), c->i_flag.as<int32_t>(), koff, tbl_off, n_slots, c->i_off.as<int32_t>(),
                   dscan, n_kept, c->i_ck.as<uint64_t>(), c->i_cc.as<uint32_t>(), c->i_cg.as<int32_t>(), c->d_ind.as<lcr_indel>(), s);
  launch_k18_tables(b, part_off, c->i_rows.p, c->i_gaps.p, p->flank, n_kept, c->d_ind.as<lcr_indel>(), d_hind, c->d_ind_row.as<int32_t>(),
                    c->i_ntot.as<uint64_t>(), s);
  *n_kept_out = n_kept;
  return LCR_OK;
}

}  // namespace

extern "C" {

int lcr_indels(lcr_ctx* c, const lcr_indel_params* p) {
  if (!c || !p) return LCR_E_ARG;
  if (c->stage < ST_PHASED) { c->err = "lcr_indels before lcr_phase / lcr_haplotag"; return LCR_E_STATE; }
  if (p->flank > 4096) { c->err = "lcr_indels: flank above 4096"; return LCR_E_ARG; }
  if (p->max_ins > 12) { c->err = "lcr_indels: max_ins above 12"; return LCR_E_ARG; }
  if (p->max_del > 65535) { c->err = "lcr_indels: max_del above 65535"; return LCR_E_ARG; }
  if (c->n_cols + c->bv.n_regions > (int64_t)INT32_MAX - 1) { c->err = "lcr_indels: more than 2^31 - 2 window columns in one batch; split it"; return LCR_E_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }       // an asynchronous phase stage in flight writes the read records
  static_assert(sizeof(lcr_indel) == 64, "lcr_indel is 64 bytes");
  const int ng = c->bv.n_regions;
  const int32_t n_rows = c->n_rows;
  hipStream_t s = c->stream;
  c->indel.valid = false;   // (from here on the last call's records are overwritten)
  HIPCHK(c, c->h_ind_ctl.reserve(64));
  HIPCHK(c, c->h_ind_off.reserve(((size_t)std::max(ng, 0) + 1) * 4));
  HIPCHK(c, c->h_ind_row.reserve((size_t)std::max(n_rows, 1) * 4));
  HIPCHK(c, c->d_ind_row.reserve((size_t)std::max(n_rows, 1) * 4));
  HIPCHK(c, c->i_ntot.reserve(8));
  int32_t* const h_ctl = c->h_ind_ctl.as<int32_t>();   // [0] participating rows, [1] gaps, [2] kept events, [3] event occurrences, [4..5] n_present_total as one 64-bit word
  int32_t* const h_off = c->h_ind_off.as<int32_t>();
  int32_t *d_ctl = nullptr, *d_hoff = nullptr, *d_hrow = nullptr;
  HIPCHK(c, c->h_ind_ctl.dev(&d_ctl));
  HIPCHK(c, c->h_ind_off.dev(&d_hoff));
  HIPCHK(c, c->h_ind_row.dev(&d_hrow));
  HIPCHK(c, hipStreamSynchronize(s));   // (an earlier call's last kernels write the pinned blocks that are reused from here on)
  for (int k = 0; k < 6; k++) h_ctl[k] = 0;
  for (int g = 0; g <= ng; g++) h_off[g] = 0;                    // (k18_offsets overwrites them when the call gets that far)
  int32_t n_part = 0, n_kept = 0;
  int64_t n_ev = 0;
  {
    Bracket t(c, c->indel);
    if (n_rows > 0) HIPCHK(c, lcr_fill_async(c->d_ind_row.p, 0, (size_t)n_rows * 4, s));   // k18_tables adds 1 per event a row is PRESENT at
    HIPCHK(c, lcr_fill_async(c->i_ntot.p, 0, 8, s));
    const uint32_t min_count = p->min_count ? p->min_count : 1u;
    { int rc = indels_queue(c, p, min_count, d_ctl, d_hoff, &n_part, &n_ev, &n_kept); if (rc) return rc; }
    launch_k18_export(n_rows, c->d_ind_row.as<int32_t>(), d_hrow, c->i_ntot.as<uint64_t>(), (uint64_t*)(d_ctl + 4), s);   // (also when nothing is kept: every row's 0)
  }
  c->ind_ng = ng; c->ind_n = n_kept; c->ind_nrows = n_rows; c->ind_npart = n_part; c->ind_nev = n_ev;
  return call_end(c, c->indel);     // lcr_get_indels waits for its event
}

int lcr_get_indels(lcr_ctx* c, lcr_indel_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->indel.valid) {
    c->err = "lcr_get_indels before lcr_indels (its records die with the phase results)"; return LCR_E_STATE;
  }
  { int rc = call_wait(c, c->indel); if (rc) return rc; }
  out->n_regions = c->ind_ng; out->n_indels = c->ind_n; out->n_rows = c->ind_nrows; out->n_part = c->ind_npart;
  out->n_events = c->ind_nev;
  std::memcpy(&out->n_present_total, c->h_ind_ctl.as<int32_t>() + 4, 8);
  out->indel = c->ind_n ? c->h_ind.as<lcr_indel>() : nullptr;
  out->indel_region_off = c->h_ind_off.as<int32_t>();
  out->row_indels = c->ind_nrows ? c->h_ind_row.as<int32_t>() : nullptr;
  out->dev_indel = c->ind_n ? c->d_ind.as<lcr_indel>() : nullptr;
  out->dev_row_indels = c->ind_nrows ? c->d_ind_row.as<int32_t>() : nullptr;
  return LCR_OK;
}

int lcr_indels_ms(lcr_ctx* c, float* ms) {
  if (!c || !ms) return LCR_E_ARG;
  return call_ms(c, c->indel, "lcr_indels_ms", "lcr_indels", ms);
}

}  // extern "C"

// lcr_ends.hip — the host driver of K16 (k16_ends.hip): the haplotype x transcript-end site table over the phased rows, its getter and its
// timer.  A call of its own behind lcr_phase / lcr_haplotag, shaped like lcr_isoforms: it reads the bound batch (CIGARs, positions, flags,
// region tables), the fragment stage's row offsets and the phase stage's read records, and writes buffers no other stage or getter reads
// (lcr_ctx: e_*, d_end*, h_end*).  Two host waits: participating rows, then kept sites.
#include "lcr_ctx.h"

namespace {

// the kernels of one call; *n_part / *n_kept stay 0 when a wait finds nothing to go on with
int ends_queue(lcr_ctx* c, const lcr_end_params* p, uint32_t min_count, int32_t* d_ctl, int32_t* d_hoff, int32_t* n_part_out, int32_t* n_kept_out) {
  const BatchView& b = c->bv;
  const int nr = b.n_reads, ng = b.n_regions;
  hipStream_t s = c->stream;
  const int32_t* const h_ctl = c->h_end_ctl.as<int32_t>();
  if (nr == 0 || ng == 0 || c->n_rows == 0) return LCR_OK;
  const lcr_read_record* rec = c->phase.d_read_rec.as<lcr_read_record>();
  const int32_t* rro = c->row_region_off.as<int32_t>();
  const int bits = c->dbg_ends_hash_bits;
  const uint32_t hash_mask = bits >= 32 ? ~0u : bits <= 0 ? 0u : ((1u << bits) - 1u);
  // 1. participating rows; their offsets; the table segments
  HIPCHK(c, c->e_part.reserve((size_t)nr * 4)); HIPCHK(c, c->e_part_off.reserve(((size_t)nr + 1) * 4));
  HIPCHK(c, c->e_tsz.reserve((size_t)ng * 4)); HIPCHK(c, c->e_tbl_off.reserve(((size_t)ng + 1) * 4));
  HIPCHK(c, c->e_off.reserve(((size_t)ng + 1) * 4));
  int32_t* part_off = c->e_part_off.as<int32_t>();
  int32_t* tbl_off = c->e_tbl_off.as<int32_t>();
  launch_k16_count(b, rro, rec, p->strand_mode, c->e_part.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->e_part.as<int32_t>(), part_off, nr, part_off + nr, s);
  launch_k16_sizes(b, part_off, c->e_tsz.as<int32_t>(), d_ctl, s);
  launch_scan_i32(c->scan_tmp, c->e_tsz.as<int32_t>(), tbl_off, ng, tbl_off + ng, s);
  { int rc = stream_wait(c, c->ends.ev); if (rc) return rc; }   // the host sizes the row records and the table from the participating rows
  const int32_t n_part = h_ctl[0];
  if (n_part <= 0) return LCR_OK;
  if (n_part > (1 << 27)) { c->err = "lcr_transcript_ends: more than 2^27 participating rows in one batch; split it"; return LCR_E_ARG; }
  *n_part_out = n_part;
  // 2. row records and the table's keys and counts; peaks, then, in a launch of its own, the assignment.  A segment has fewer than 8 x its
  // rows in slots, so 8 x all participating rows bounds the table without another wait; the slots behind the last segment stay empty.
  const int32_t n_slots = 8 * n_part;
  HIPCHK(c, c->e_rows.reserve((size_t)n_part * launch_k16_row_bytes()));
  HIPCHK(c, c->e_tbl_key.reserve((size_t)n_slots * 8)); HIPCHK(c, c->e_tbl_cnt.reserve((size_t)n_slots * 8));
  HIPCHK(c, c->e_slot.reserve((size_t)n_slots * launch_k16_slot_bytes()));
  HIPCHK(c, c->e_flag.reserve((size_t)n_slots * 4)); HIPCHK(c, c->e_koff.reserve(((size_t)n_slots + 1) * 4));
  HIPCHK(c, lcr_fill_async(c->e_tbl_key.p, 0xff, (size_t)n_slots * 8, s));
  HIPCHK(c, lcr_fill_async(c->e_tbl_cnt.p, 0, (size_t)n_slots * 8, s));
  launch_k16_walk(b, rro, rec, p->strand_mode, hash_mask, c->e_part.as<int32_t>(), part_off, tbl_off, c->e_rows.p, c->e_tbl_key.as<uint64_t>(),
                  c->e_tbl_cnt.as<uint32_t>(), s);
  launch_k16_peaks(c->e_tbl_key.as<uint64_t>(), c->e_tbl_cnt.as<uint32_t>(), tbl_off, ng, n_slots, p->window, hash_mask, c->e_slot.p, s);
  // 3. kept sites and their number per region
  int32_t* koff = c->e_koff.as<int32_t>();
  launch_k16_flag(c->e_slot.p, n_slots, min_count, c->e_flag.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->e_flag.as<int32_t>(), koff, n_slots, koff + n_slots, s);
  launch_k16_offsets(tbl_off, koff, ng, n_slots, c->e_off.as<int32_t>(), d_hoff, d_ctl, s);
  { int rc = stream_wait(c, c->ends.ev); if (rc) return rc; }   // kept sites size the records and the last kernels' grids
  const int32_t n_kept = h_ctl[1];
  if (n_kept <= 0) return LCR_OK;
  // 4. order, row_site, tables: the results go to HBM and, by the same kernels, to pinned host memory
  HIPCHK(c, c->e_cslot.reserve((size_t)n_kept * 4)); HIPCHK(c, c->e_crank.reserve((size_t)n_kept * 4));
  HIPCHK(c, c->d_end.reserve((size_t)n_kept * sizeof(lcr_end_site))); HIPCHK(c, c->h_end.reserve((size_t)n_kept * sizeof(lcr_end_site)));
  lcr_end_site* d_hsite = nullptr;
  HIPCHK(c, c->h_end.dev(&d_hsite));
  launch_k16_place(c->e_tbl_key.as<uint64_t>(), c->e_slot.p, c->e_flag.as<int32_t>(), koff, n_slots, c->e_off.as<int32_t>(), n_kept,
                   c->e_cslot.as<int32_t>(), c->e_crank.as<int32_t>(), c->d_end.as<lcr_end_site>(), s);
  launch_k16_rows(n_part, c->e_rows.p, c->e_slot.p, c->e_flag.as<int32_t>(), koff, c->e_crank.as<int32_t>(), c->d_end_row.as<int32_t>(),
                  c->e_nasg.as<uint64_t>(), s);
  launch_k16_tables(b, part_off, c->e_rows.p, p->window, n_kept, c->d_end.as<lcr_end_site>(), d_hsite, s);
  *n_kept_out = n_kept;
  return LCR_OK;
}

}  // namespace

extern "C" {

int lcr_transcript_ends(lcr_ctx* c, const lcr_end_params* p) {
  if (!c || !p) return LCR_E_ARG;
  if (c->stage < ST_PHASED) { c->err = "lcr_transcript_ends before lcr_phase / lcr_haplotag"; return LCR_E_STATE; }
  if (p->window > 4096) { c->err = "lcr_transcript_ends: window above 4096"; return LCR_E_ARG; }
  if (p->strand_mode > LCR_ENDS_STRAND_READ) { c->err = "lcr_transcript_ends: strand_mode is LCR_ENDS_STRAND_TS or LCR_ENDS_STRAND_READ"; return LCR_E_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }       // an asynchronous phase stage in flight writes the read records
  static_assert(sizeof(lcr_end_site) == 64, "lcr_end_site is 64 bytes");
  const int ng = c->bv.n_regions;
  const int32_t n_rows = c->n_rows;
  if (n_rows > (1 << 29)) { c->err = "lcr_transcript_ends: more than 2^29 fragment rows in one batch; split it"; return LCR_E_ARG; }
  hipStream_t s = c->stream;
  c->ends.valid = false;   // (from here on the last call's records are overwritten)
  HIPCHK(c, c->h_end_ctl.reserve(64));
  HIPCHK(c, c->h_end_off.reserve(((size_t)std::max(ng, 0) + 1) * 4));
  HIPCHK(c, c->h_end_row.reserve((size_t)std::max(n_rows, 1) * 8));
  HIPCHK(c, c->d_end_row.reserve((size_t)std::max(n_rows, 1) * 8));
  HIPCHK(c, c->e_nasg.reserve(8));
  int32_t* const h_ctl = c->h_end_ctl.as<int32_t>();   // [0] participating rows, [1] kept sites, [2..3] n_assigned as one 64-bit word
  int32_t* const h_off = c->h_end_off.as<int32_t>();
  int32_t *d_ctl = nullptr, *d_hoff = nullptr, *d_hrow = nullptr;
  HIPCHK(c, c->h_end_ctl.dev(&d_ctl));
  HIPCHK(c, c->h_end_off.dev(&d_hoff));
  HIPCHK(c, c->h_end_row.dev(&d_hrow));
  HIPCHK(c, hipStreamSynchronize(s));   // (an earlier call's last kernels write the pinned blocks that are reused from here on)
  h_ctl[0] = h_ctl[1] = h_ctl[2] = h_ctl[3] = 0;
  for (int g = 0; g <= ng; g++) h_off[g] = 0;                    // (k16_offsets overwrites them when the call gets that far)
  int32_t n_part = 0, n_kept = 0;
  {
    Bracket t(c, c->ends);
    if (n_rows > 0) HIPCHK(c, lcr_fill_async(c->d_end_row.p, 0xff, (size_t)n_rows * 8, s));   // -1: k16_rows overwrites the ends that have a kept site
    HIPCHK(c, lcr_fill_async(c->e_nasg.p, 0, 8, s));
    const uint32_t min_count = p->min_count ? p->min_count : 1u;
    { int rc = ends_queue(c, p, min_count, d_ctl, d_hoff, &n_part, &n_kept); if (rc) return rc; }
    launch_k16_export(n_rows, c->d_end_row.as<int32_t>(), d_hrow, c->e_nasg.as<uint64_t>(), (uint64_t*)(d_ctl + 2), s);   // (also when nothing is kept: every end's -1)
  }
  c->ends_ng = ng; c->ends_n = n_kept; c->ends_nrows = n_rows; c->ends_npart = n_part;
  return call_end(c, c->ends);     // lcr_get_transcript_ends waits for its event
}

int lcr_get_transcript_ends(lcr_ctx* c, lcr_end_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->ends.valid) {
    c->err = "lcr_get_transcript_ends before lcr_transcript_ends (its records die with the phase results)"; return LCR_E_STATE;
  }
  { int rc = call_wait(c, c->ends); if (rc) return rc; }
  out->n_regions = c->ends_ng; out->n_sites = c->ends_n; out->n_rows = c->ends_nrows; out->n_part = c->ends_npart;
  std::memcpy(&out->n_assigned, c->h_end_ctl.as<int32_t>() + 2, 8);
  out->site = c->ends_n ? c->h_end.as<lcr_end_site>() : nullptr;
  out->site_region_off = c->h_end_off.as<int32_t>();
  out->row_site = c->ends_nrows ? c->h_end_row.as<int32_t>() : nullptr;
  out->dev_site = c->ends_n ? c->d_end.as<lcr_end_site>() : nullptr;
  out->dev_row_site = c->ends_nrows ? c->d_end_row.as<int32_t>() : nullptr;
  return LCR_OK;
}

int lcr_transcript_ends_ms(lcr_ctx* c, float* ms) {
  if (!c || !ms) return LCR_E_ARG;
  return call_ms(c, c->ends, "lcr_transcript_ends_ms", "lcr_transcript_ends", ms);
}

}  // extern "C"

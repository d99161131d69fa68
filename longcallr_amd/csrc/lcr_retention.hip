// lcr_retention.hip — the host driver of K17 (k17_retention.hip): the haplotype x intron-retention table over the phased rows, its getter and
// its timer.  A call of its own behind lcr_phase / lcr_haplotag, shaped like lcr_transcript_ends: it reads the bound batch (CIGARs,
// positions, region tables), the fragment stage's row offsets and the phase stage's read records, and writes buffers no other stage or
// getter reads (lcr_ctx: r_*, d_ret*, h_ret*).  Two host waits: participating rows and pairs, then kept introns.
#include "lcr_ctx.h"

namespace {

// the kernels of one call; *n_part / *n_kept stay 0 when a wait finds nothing to go on with
int retention_queue(lcr_ctx* c, const lcr_retention_params* p, uint32_t min_count, int32_t* d_ctl, int32_t* d_hoff, int32_t* n_part_out, int32_t* n_kept_out) {
  const BatchView& b = c->bv;
  const int nr = b.n_reads, ng = b.n_regions;
  hipStream_t s = c->stream;
  const int32_t* const h_ctl = c->h_ret_ctl.as<int32_t>();
  if (nr == 0 || ng == 0 || c->n_rows == 0) return LCR_OK;
  const lcr_read_record* rec = c->phase.d_read_rec.as<lcr_read_record>();
  const int32_t* rro = c->row_region_off.as<int32_t>();
  const int bits = c->dbg_ir_hash_bits;
  const uint32_t hash_mask = bits >= 32 ? ~0u : bits <= 0 ? 0u : ((1u << bits) - 1u);
  // 1. junctions per read, participating rows; their offsets; the table segments
  HIPCHK(c, c->r_part.reserve((size_t)nr * 4)); HIPCHK(c, c->r_npair.reserve((size_t)nr * 4));
  HIPCHK(c, c->r_part_off.reserve(((size_t)nr + 1) * 4)); HIPCHK(c, c->r_pair_off.reserve(((size_t)nr + 1) * 4));
  HIPCHK(c, c->r_tsz.reserve((size_t)ng * 4)); HIPCHK(c, c->r_tbl_off.reserve(((size_t)ng + 1) * 4)); HIPCHK(c, c->r_off.reserve(((size_t)ng + 1) * 4));
  int32_t* part_off = c->r_part_off.as<int32_t>();
  int32_t* pair_off = c->r_pair_off.as<int32_t>();
  int32_t* tbl_off = c->r_tbl_off.as<int32_t>();
  launch_k17_count(b, rro, rec, c->r_part.as<int32_t>(), c->r_npair.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->r_part.as<int32_t>(), part_off, nr, part_off + nr, s);
  launch_scan_i32(c->scan_tmp, c->r_npair.as<int32_t>(), pair_off, nr, pair_off + nr, s);
  launch_k17_sizes(b, part_off, pair_off, c->r_tsz.as<int32_t>(), d_ctl, s);
  launch_scan_i32(c->scan_tmp, c->r_tsz.as<int32_t>(), tbl_off, ng, tbl_off + ng, s);
  { int rc = stream_wait(c, c->ret.ev); if (rc) return rc; }   // the host sizes the row records, the keys and the table from the two totals
  const int32_t n_part = h_ctl[0], n_pairs = h_ctl[1];
  if (n_part <= 0) return LCR_OK;
  *n_part_out = n_part;
  if (n_pairs <= 0) return LCR_OK;   // every tagged read is unspliced: no intron is an event here
  if (n_pairs > (1 << 28)) { c->err = "lcr_intron_retention: more than 2^28 junction occurrences in one batch; split it"; return LCR_E_ARG; }
  // 2. row records, keys, the regions' table segments.  A segment has fewer than 4 x its pairs in slots, so 4 x all pairs bounds the table
  // without a third wait; the slots behind the last segment stay empty.
  const int32_t n_slots = 4 * n_pairs;
  HIPCHK(c, c->r_rows.reserve((size_t)n_part * launch_k17_row_bytes()));
  HIPCHK(c, c->r_keys.reserve((size_t)n_pairs * 8));
  HIPCHK(c, c->r_tbl_key.reserve((size_t)n_slots * 8)); HIPCHK(c, c->r_tbl_cnt.reserve((size_t)n_slots * 4));
  HIPCHK(c, c->r_flag.reserve((size_t)n_slots * 4)); HIPCHK(c, c->r_koff.reserve(((size_t)n_slots + 1) * 4));
  HIPCHK(c, lcr_fill_async(c->r_tbl_key.p, 0xff, (size_t)n_slots * 8, s));
  HIPCHK(c, lcr_fill_async(c->r_tbl_cnt.p, 0, (size_t)n_slots * 4, s));
  launch_k17_emit(b, rro, rec, hash_mask, c->r_part.as<int32_t>(), part_off, pair_off, tbl_off, c->r_rows.p, c->r_keys.as<uint64_t>(),
                  c->r_tbl_key.as<uint64_t>(), c->r_tbl_cnt.as<uint32_t>(), s);
  // 3. kept introns and their number per region
  int32_t* koff = c->r_koff.as<int32_t>();
  launch_k17_flag(c->r_tbl_key.as<uint64_t>(), c->r_tbl_cnt.as<uint32_t>(), n_slots, min_count, c->r_flag.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->r_flag.as<int32_t>(), koff, n_slots, koff + n_slots, s);
  launch_k17_offsets(tbl_off, koff, ng, n_slots, c->r_off.as<int32_t>(), d_hoff, d_ctl, s);
  { int rc = stream_wait(c, c->ret.ev); if (rc) return rc; }   // the number of kept introns sizes the records and the last kernels' grids
  const int32_t n_kept = h_ctl[2];
  if (n_kept <= 0) return LCR_OK;
  // 4. order, motif, tables: the records go to HBM and, by the same kernel, to pinned host memory
  HIPCHK(c, c->r_ck.reserve((size_t)n_kept * 8)); HIPCHK(c, c->r_cc.reserve((size_t)n_kept * 4)); HIPCHK(c, c->r_cg.reserve((size_t)n_kept * 4));
  HIPCHK(c, c->d_ret.reserve((size_t)n_kept * sizeof(lcr_retained_intron)));
  HIPCHK(c, c->h_ret.reserve((size_t)n_kept * sizeof(lcr_retained_intron)));
  lcr_retained_intron* d_hret = nullptr;
  HIPCHK(c, c->h_ret.dev(&d_hret));
  launch_k17_place(b, c->r_tbl_key.as<uint64_t>(), c->r_tbl_cnt.as<uint32_t>(), c->r_flag.as<int32_t>(), koff, tbl_off, n_slots, c->r_off.as<int32_t>(),
                   n_kept, c->r_ck.as<uint64_t>(), c->r_cc.as<uint32_t>(), c->r_cg.as<int32_t>(), c->d_ret.as<lcr_retained_intron>(), s);
  launch_k17_tables(b, part_off, c->r_rows.p, c->r_keys.as<uint64_t>(), p->anchor, n_kept, c->d_ret.as<lcr_retained_intron>(), d_hret,
                    c->d_ret_row.as<int32_t>(), c->r_ntot.as<uint64_t>(), s);
  *n_kept_out = n_kept;
  return LCR_OK;
}

}  // namespace

extern "C" {

int lcr_intron_retention(lcr_ctx* c, const lcr_retention_params* p) {
  if (!c || !p) return LCR_E_ARG;
  if (c->stage < ST_PHASED) { c->err = "lcr_intron_retention before lcr_phase / lcr_haplotag"; return LCR_E_STATE; }
  if (p->anchor > 4096) { c->err = "lcr_intron_retention: anchor above 4096"; return LCR_E_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }       // an asynchronous phase stage in flight writes the read records
  static_assert(sizeof(lcr_retained_intron) == 56, "lcr_retained_intron is 56 bytes");
  const int ng = c->bv.n_regions;
  const int32_t n_rows = c->n_rows;
  hipStream_t s = c->stream;
  c->ret.valid = false;   // (from here on the last call's records are overwritten)
  HIPCHK(c, c->h_ret_ctl.reserve(64));
  HIPCHK(c, c->h_ret_off.reserve(((size_t)std::max(ng, 0) + 1) * 4));
  HIPCHK(c, c->h_ret_row.reserve((size_t)std::max(n_rows, 1) * 4));
  HIPCHK(c, c->d_ret_row.reserve((size_t)std::max(n_rows, 1) * 4));
  HIPCHK(c, c->r_ntot.reserve(8));
  int32_t* const h_ctl = c->h_ret_ctl.as<int32_t>();   // [0] participating rows, [1] pairs, [2] kept introns, [4..5] n_retained_total as one 64-bit word
  int32_t* const h_off = c->h_ret_off.as<int32_t>();
  int32_t *d_ctl = nullptr, *d_hoff = nullptr, *d_hrow = nullptr;
  HIPCHK(c, c->h_ret_ctl.dev(&d_ctl));
  HIPCHK(c, c->h_ret_off.dev(&d_hoff));
  HIPCHK(c, c->h_ret_row.dev(&d_hrow));
  HIPCHK(c, hipStreamSynchronize(s));   // (an earlier call's last kernels write the pinned blocks that are reused from here on)
  for (int k = 0; k < 6; k++) h_ctl[k] = 0;
  for (int g = 0; g <= ng; g++) h_off[g] = 0;                    // (k17_offsets overwrites them when the call gets that far)
  int32_t n_part = 0, n_kept = 0;
  {
    Bracket t(c, c->ret);
    if (n_rows > 0) HIPCHK(c, lcr_fill_async(c->d_ret_row.p, 0, (size_t)n_rows * 4, s));   // k17_tables adds 1 per intron a row is RETAINED at
    HIPCHK(c, lcr_fill_async(c->r_ntot.p, 0, 8, s));
    const uint32_t min_count = p->min_count ? p->min_count : 1u;
    { int rc = retention_queue(c, p, min_count, d_ctl, d_hoff, &n_part, &n_kept); if (rc) return rc; }
    launch_k17_export(n_rows, c->d_ret_row.as<int32_t>(), d_hrow, c->r_ntot.as<uint64_t>(), (uint64_t*)(d_ctl + 4), s);   // (also when nothing is kept: every row's 0)
  }
  c->ret_ng = ng; c->ret_n = n_kept; c->ret_nrows = n_rows; c->ret_npart = n_part;
  return call_end(c, c->ret);     // lcr_get_intron_retention waits for its event
}

int lcr_get_intron_retention(lcr_ctx* c, lcr_retention_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->ret.valid) {
    c->err = "lcr_get_intron_retention before lcr_intron_retention (its records die with the phase results)"; return LCR_E_STATE;
  }
  { int rc = call_wait(c, c->ret); if (rc) return rc; }
  out->n_regions = c->ret_ng; out->n_introns = c->ret_n; out->n_rows = c->ret_nrows; out->n_part = c->ret_npart;
  std::memcpy(&out->n_retained_total, c->h_ret_ctl.as<int32_t>() + 4, 8);
  out->intron = c->ret_n ? c->h_ret.as<lcr_retained_intron>() : nullptr;
  out->intron_region_off = c->h_ret_off.as<int32_t>();
  out->row_retained = c->ret_nrows ? c->h_ret_row.as<int32_t>() : nullptr;
  out->dev_intron = c->ret_n ? c->d_ret.as<lcr_retained_intron>() : nullptr;
  out->dev_row_retained = c->ret_nrows ? c->d_ret_row.as<int32_t>() : nullptr;
  return LCR_OK;
}

int lcr_intron_retention_ms(lcr_ctx* c, float* ms) {
  if (!c || !ms) return LCR_E_ARG;
  return call_ms(c, c->ret, "lcr_intron_retention_ms", "lcr_intron_retention", ms);
}

}  // extern "C"

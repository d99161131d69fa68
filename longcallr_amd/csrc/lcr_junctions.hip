// lcr_junctions.hip — the host driver of K6 (k6_junctions.hip): the haplotype x junction table over the phased rows, and its getter.
// A call of its own behind lcr_phase: it reads the bound batch (CIGARs, positions, region tables), the fragment stage's row offsets and
// the phase stage's read records, and writes buffers no other stage or getter reads (lcr_ctx: j_*, d_junc, h_junc*).
#include "lcr_ctx.h"

extern "C" {

int lcr_junctions(lcr_ctx* c, const lcr_junction_params* p) {
  if (!c || !p) return LCR_E_ARG;
  if (c->stage < ST_PHASED) { c->err = "lcr_junctions before lcr_phase"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }       // an asynchronous phase stage in flight writes the read records
  static_assert(sizeof(lcr_junction) == 48, "lcr_junction is 48 bytes");
  c->junc.valid = false;   // (from here on the last call's table is overwritten)
  const BatchView& b = c->bv;
  const int nr = b.n_reads, ng = b.n_regions;
  hipStream_t s = c->stream;
  HIPCHK(c, c->h_junc_ctl.reserve(64));
  HIPCHK(c, c->h_junc_off.reserve((size_t)(ng + 1) * 4));
  HIPCHK(c, c->h_junc.reserve(sizeof(lcr_junction)));
  int32_t* const h_ctl = c->h_junc_ctl.as<int32_t>();
  int32_t* const h_off = c->h_junc_off.as<int32_t>();
  int32_t *d_ctl = nullptr, *d_hoff = nullptr;
  HIPCHK(c, c->h_junc_ctl.dev(&d_ctl));
  HIPCHK(c, c->h_junc_off.dev(&d_hoff));
  HIPCHK(c, hipStreamSynchronize(s));   // (an earlier call's last kernels write the pinned blocks that are reused from here on)
  h_ctl[0] = h_ctl[1] = h_ctl[2] = 0;
  const auto finish_empty = [&]() {   // no participating row, no pair or no kept junction
    for (int g = 0; g <= ng; g++) h_off[g] = 0;
    c->junc_n = 0; c->junc_ng = ng; c->junc.valid = true;
    return LCR_OK;
  };
  if (nr == 0 || ng == 0 || c->n_rows == 0) return finish_empty();
  Timer t(c, LCR_K_JUNCTIONS);
  const lcr_read_record* rec = c->phase.d_read_rec.as<lcr_read_record>();
  const int32_t* rro = c->row_region_off.as<int32_t>();
  // 1. junctions per read, participating rows; their offsets
  HIPCHK(c, c->j_part.reserve((size_t)nr * 4)); HIPCHK(c, c->j_npair.reserve((size_t)nr * 4));
  HIPCHK(c, c->j_part_off.reserve(((size_t)nr + 1) * 4)); HIPCHK(c, c->j_pair_off.reserve(((size_t)nr + 1) * 4));
  HIPCHK(c, c->j_tsz.reserve((size_t)ng * 4)); HIPCHK(c, c->j_tbl_off.reserve(((size_t)ng + 1) * 4)); HIPCHK(c, c->j_off.reserve(((size_t)ng + 1) * 4));
  int32_t* part_off = c->j_part_off.as<int32_t>();
  int32_t* pair_off = c->j_pair_off.as<int32_t>();
  int32_t* tbl_off = c->j_tbl_off.as<int32_t>();
  launch_k6_count(b, rro, rec, p->min_junctions, c->j_part.as<int32_t>(), c->j_npair.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->j_part.as<int32_t>(), part_off, nr, part_off + nr, s);
  launch_scan_i32(c->scan_tmp, c->j_npair.as<int32_t>(), pair_off, nr, pair_off + nr, s);
  launch_k6_sizes(b, part_off, pair_off, c->j_tsz.as<int32_t>(), d_ctl, s);
  launch_scan_i32(c->scan_tmp, c->j_tsz.as<int32_t>(), tbl_off, ng, tbl_off + ng, s);
  { int rc = stream_wait(c, c->junc.ev); if (rc) return rc; }   // the host sizes the row records, the keys and the table from the two totals
  const int32_t n_part = h_ctl[0], n_pairs = h_ctl[1];
  if (n_part <= 0 || n_pairs <= 0) return finish_empty();
  if (n_pairs > (1 << 28)) { c->err = "lcr_junctions: more than 2^28 junction occurrences in one batch; split it"; return LCR_E_ARG; }
  // 2. row records, keys, the regions' table segments.  A segment has fewer than 4 x its pairs in slots, so 4 x all pairs bounds the table
  // without a third wait; the slots behind the last segment stay empty.
  const int32_t n_slots = 4 * n_pairs;
  HIPCHK(c, c->j_rows.reserve((size_t)n_part * launch_k6_row_bytes()));
  HIPCHK(c, c->j_keys.reserve((size_t)n_pairs * 8));
  HIPCHK(c, c->j_tbl_key.reserve((size_t)n_slots * 8)); HIPCHK(c, c->j_tbl_cnt.reserve((size_t)n_slots * 4));
  HIPCHK(c, c->j_flag.reserve((size_t)n_slots * 4)); HIPCHK(c, c->j_koff.reserve(((size_t)n_slots + 1) * 4));
  HIPCHK(c, lcr_fill_async(c->j_tbl_key.p, 0xff, (size_t)n_slots * 8, s));
  HIPCHK(c, lcr_fill_async(c->j_tbl_cnt.p, 0, (size_t)n_slots * 4, s));
  launch_k6_emit(b, rro, rec, c->j_part.as<int32_t>(), part_off, pair_off, tbl_off, c->j_rows.p, c->j_keys.as<uint64_t>(),
                 c->j_tbl_key.as<uint64_t>(), c->j_tbl_cnt.as<uint32_t>(), s);
  // 3. kept junctions and their number per region
  int32_t* koff = c->j_koff.as<int32_t>();
  launch_k6_flag(c->j_tbl_key.as<uint64_t>(), c->j_tbl_cnt.as<uint32_t>(), n_slots, p->min_count, c->j_flag.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->j_flag.as<int32_t>(), koff, n_slots, koff + n_slots, s);
  launch_k6_offsets(tbl_off, koff, ng, n_slots, c->j_off.as<int32_t>(), d_hoff, d_ctl, s);
  { int rc = stream_wait(c, c->junc.ev); if (rc) return rc; }   // the number of kept junctions sizes the records and the last kernels' grids
  const int32_t n_kept = h_ctl[2];
  if (n_kept <= 0) return finish_empty();
  // 4. order, motif, tables: the records go to HBM and, by the last kernel, to pinned host memory
  HIPCHK(c, c->j_ck.reserve((size_t)n_kept * 8)); HIPCHK(c, c->j_cc.reserve((size_t)n_kept * 4)); HIPCHK(c, c->j_cg.reserve((size_t)n_kept * 4));
  HIPCHK(c, c->d_junc.reserve((size_t)n_kept * sizeof(lcr_junction)));
  HIPCHK(c, c->h_junc.reserve((size_t)n_kept * sizeof(lcr_junction)));
  lcr_junction* d_hjunc = nullptr;
  HIPCHK(c, c->h_junc.dev(&d_hjunc));
  launch_k6_place(b, c->j_tbl_key.as<uint64_t>(), c->j_tbl_cnt.as<uint32_t>(), c->j_flag.as<int32_t>(), koff, tbl_off, n_slots, c->j_off.as<int32_t>(),
                  n_kept, c->j_ck.as<uint64_t>(), c->j_cc.as<uint32_t>(), c->j_cg.as<int32_t>(), c->d_junc.as<lcr_junction>(), s);
  launch_k6_tables(b, part_off, c->j_rows.p, c->j_keys.as<uint64_t>(), n_kept, c->d_junc.as<lcr_junction>(), d_hjunc, s);
  c->junc_n = n_kept; c->junc_ng = ng;
  return call_end(c, c->junc);     // lcr_get_junctions waits for its event
}

int lcr_get_junctions(lcr_ctx* c, lcr_junction_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->junc.valid) { c->err = "lcr_get_junctions before lcr_junctions (its table dies with the phase stage's results)"; return LCR_E_STATE; }
  { int rc = call_wait(c, c->junc); if (rc) return rc; }
  out->n_regions = c->junc_ng; out->n_junctions = c->junc_n;
  out->junc = c->junc_n ? c->h_junc.as<lcr_junction>() : nullptr;
  out->junc_region_off = c->h_junc_off.as<int32_t>();
  out->dev_junc = c->junc_n ? c->d_junc.as<lcr_junction>() : nullptr;
  return LCR_OK;
}

}  // extern "C"

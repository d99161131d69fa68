// lcr_isoforms.hip — the host driver of K15 (k15_isoforms.hip): the haplotype x intron-chain table over the phased rows, its getter and
// its timer.  A call of its own behind lcr_phase / lcr_haplotag, shaped like lcr_junctions: it reads the bound batch (CIGARs, positions,
// region tables), the fragment stage's row offsets and the phase stage's read records, and writes buffers no other stage or getter reads
// (lcr_ctx: iso_*, d_iso*, h_iso*).  Two host waits: participating rows and pairs, then kept chains and pool entries.
#include "lcr_ctx.h"

namespace {

// the kernels of one call; *n_kept / *n_pool stay 0 when a wait finds nothing to go on with
int iso_queue(lcr_ctx* c, const lcr_isoform_params* p, int32_t* d_ctl, int32_t* d_hoff, int32_t* n_kept_out, int32_t* n_pool_out) {
  const BatchView& b = c->bv;
  const int nr = b.n_reads, ng = b.n_regions;
  hipStream_t s = c->stream;
  const int32_t* const h_ctl = c->h_iso_ctl.as<int32_t>();
  if (nr == 0 || ng == 0 || c->n_rows == 0) return LCR_OK;
  const lcr_read_record* rec = c->phase.d_read_rec.as<lcr_read_record>();
  const int32_t* rro = c->row_region_off.as<int32_t>();
  // 1. junctions per read, participating rows (k >= min_junctions = more than min_junctions - 1); their offsets; the table segments
  HIPCHK(c, c->iso_part.reserve((size_t)nr * 4)); HIPCHK(c, c->iso_npair.reserve((size_t)nr * 4));
  HIPCHK(c, c->iso_part_off.reserve(((size_t)nr + 1) * 4)); HIPCHK(c, c->iso_pair_off.reserve(((size_t)nr + 1) * 4));
  HIPCHK(c, c->iso_tsz.reserve((size_t)ng * 4)); HIPCHK(c, c->iso_tbl_off.reserve(((size_t)ng + 1) * 4));
  HIPCHK(c, c->iso_off.reserve(((size_t)ng + 1) * 4)); HIPCHK(c, c->iso_pbase.reserve(((size_t)ng + 1) * 4));
  int32_t* part_off = c->iso_part_off.as<int32_t>();
  int32_t* pair_off = c->iso_pair_off.as<int32_t>();
  int32_t* tbl_off = c->iso_tbl_off.as<int32_t>();
  launch_k6_count(b, rro, rec, p->min_junctions - 1u, c->iso_part.as<int32_t>(), c->iso_npair.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->iso_part.as<int32_t>(), part_off, nr, part_off + nr, s);
  launch_scan_i32(c->scan_tmp, c->iso_npair.as<int32_t>(), pair_off, nr, pair_off + nr, s);
  launch_k15_sizes(b, part_off, pair_off, c->iso_tsz.as<int32_t>(), d_ctl, s);
  launch_scan_i32(c->scan_tmp, c->iso_tsz.as<int32_t>(), tbl_off, ng, tbl_off + ng, s);
  { int rc = stream_wait(c, c->iso.ev); if (rc) return rc; }   // the host sizes the row records, the keys and the table from the two totals
  const int32_t n_part = h_ctl[0], n_pairs = h_ctl[1];
  if (n_part <= 0 || n_pairs <= 0) return LCR_OK;
  if (n_pairs > (1 << 28)) { c->err = "lcr_isoforms: more than 2^28 junction occurrences in one batch; split it"; return LCR_E_ARG; }
  // 2. row records, keys, hashes; then, in a launch of its own, the insertion.  A segment has fewer than 4 x its rows in slots, so 4 x all
  // participating rows bounds the table without a third wait; the slots behind the last segment stay empty.
  const int32_t n_slots = 4 * n_part;   // (n_part <= n_pairs <= 2^28)
  HIPCHK(c, c->iso_rows.reserve((size_t)n_part * launch_k15_row_bytes()));
  HIPCHK(c, c->iso_keys.reserve((size_t)n_pairs * 8));
  HIPCHK(c, c->iso_hash.reserve((size_t)n_part * 8)); HIPCHK(c, c->iso_row_slot.reserve((size_t)n_part * 4));
  HIPCHK(c, c->iso_tbl_rep.reserve((size_t)n_slots * 4)); HIPCHK(c, c->iso_tbl_cnt.reserve((size_t)n_slots * 8));
  HIPCHK(c, c->iso_flag.reserve((size_t)n_slots * 4)); HIPCHK(c, c->iso_koff.reserve(((size_t)n_slots + 1) * 4));
  HIPCHK(c, c->iso_plen.reserve((size_t)n_slots * 4)); HIPCHK(c, c->iso_poff.reserve(((size_t)n_slots + 1) * 4));
  HIPCHK(c, lcr_fill_async(c->iso_tbl_rep.p, 0xff, (size_t)n_slots * 4, s));
  HIPCHK(c, lcr_fill_async(c->iso_tbl_cnt.p, 0, (size_t)n_slots * 8, s));
  launch_k15_walk(b, rro, rec, c->iso_part.as<int32_t>(), part_off, pair_off, c->iso_rows.p, c->iso_keys.as<uint64_t>(), c->iso_hash.as<uint64_t>(), s);
  const int bits = c->dbg_iso_hash_bits;
  const uint64_t hash_mask = bits >= 64 ? ~0ull : bits <= 0 ? 0ull : ((1ull << bits) - 1ull);
  launch_k15_insert(n_part, c->iso_rows.p, c->iso_keys.as<uint64_t>(), c->iso_hash.as<uint64_t>(), hash_mask, tbl_off, c->iso_tbl_rep.as<int32_t>(),
                    c->iso_tbl_cnt.as<uint32_t>(), c->iso_row_slot.as<int32_t>(), s);
  // 3. kept chains, their number and their keys per region
  int32_t* koff = c->iso_koff.as<int32_t>();
  int32_t* poff = c->iso_poff.as<int32_t>();
  launch_k15_flag(c->iso_tbl_rep.as<int32_t>(), c->iso_tbl_cnt.as<uint32_t>(), c->iso_rows.p, n_slots, p->min_count, c->iso_flag.as<int32_t>(),
                  c->iso_plen.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->iso_flag.as<int32_t>(), koff, n_slots, koff + n_slots, s);
  launch_scan_i32(c->scan_tmp, c->iso_plen.as<int32_t>(), poff, n_slots, poff + n_slots, s);
  launch_k15_offsets(tbl_off, koff, poff, ng, n_slots, c->iso_off.as<int32_t>(), d_hoff, c->iso_pbase.as<int32_t>(), d_ctl, s);
  { int rc = stream_wait(c, c->iso.ev); if (rc) return rc; }   // kept chains and pool entries size the records, the pool and the last kernels' grids
  const int32_t n_kept = h_ctl[2], n_pool = h_ctl[3];
  if (n_kept <= 0) return LCR_OK;
  // 4. order, pool, row_isoform, tables: the results go to HBM and, by the same kernels, to pinned host memory
  HIPCHK(c, c->iso_cslot.reserve((size_t)n_kept * 4)); HIPCHK(c, c->iso_crank.reserve((size_t)n_kept * 4));
  HIPCHK(c, c->d_iso.reserve((size_t)n_kept * sizeof(lcr_isoform))); HIPCHK(c, c->h_iso.reserve((size_t)n_kept * sizeof(lcr_isoform)));
  HIPCHK(c, c->d_iso_chain.reserve((size_t)n_pool * 8)); HIPCHK(c, c->h_iso_chain.reserve((size_t)n_pool * 8));
  lcr_isoform* d_hiso = nullptr;
  uint64_t* d_hchain = nullptr;
  HIPCHK(c, c->h_iso.dev(&d_hiso));
  HIPCHK(c, c->h_iso_chain.dev(&d_hchain));
  launch_k15_place(c->iso_rows.p, c->iso_keys.as<uint64_t>(), c->iso_tbl_rep.as<int32_t>(), c->iso_tbl_cnt.as<uint32_t>(), c->iso_flag.as<int32_t>(), koff,
                   n_slots, c->iso_off.as<int32_t>(), c->iso_pbase.as<int32_t>(), n_kept, c->iso_cslot.as<int32_t>(), c->iso_crank.as<int32_t>(),
                   c->d_iso.as<lcr_isoform>(), c->d_iso_chain.as<uint64_t>(), d_hchain, s);
  launch_k15_rows(n_part, c->iso_rows.p, c->iso_row_slot.as<int32_t>(), c->iso_flag.as<int32_t>(), koff, c->iso_crank.as<int32_t>(),
                  c->d_iso_row.as<int32_t>(), s);
  launch_k15_tables(b, part_off, c->iso_rows.p, c->iso_keys.as<uint64_t>(), c->d_iso_chain.as<uint64_t>(), n_kept, c->d_iso.as<lcr_isoform>(), d_hiso, s);
  *n_kept_out = n_kept; *n_pool_out = n_pool;
  return LCR_OK;
}

}  // namespace

extern "C" {

int lcr_isoforms(lcr_ctx* c, const lcr_isoform_params* p) {
  if (!c || !p) return LCR_E_ARG;
  if (c->stage < ST_PHASED) { c->err = "lcr_isoforms before lcr_phase / lcr_haplotag"; return LCR_E_STATE; }
  if (p->min_junctions == 0) { c->err = "lcr_isoforms: min_junctions must be at least 1 (an unspliced read has no chain)"; return LCR_E_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }       // an asynchronous phase stage in flight writes the read records
  static_assert(sizeof(lcr_isoform) == 64, "lcr_isoform is 64 bytes");
  const int ng = c->bv.n_regions;
  const int32_t n_rows = c->n_rows;
  hipStream_t s = c->stream;
  c->iso.valid = false;   // (from here on the last call's records are overwritten)
  HIPCHK(c, c->h_iso_ctl.reserve(64));
  HIPCHK(c, c->h_iso_off.reserve(((size_t)std::max(ng, 0) + 1) * 4));
  HIPCHK(c, c->h_iso_row.reserve((size_t)std::max(n_rows, 1) * 4));
  HIPCHK(c, c->d_iso_row.reserve((size_t)std::max(n_rows, 1) * 4));
  int32_t* const h_ctl = c->h_iso_ctl.as<int32_t>();
  int32_t* const h_off = c->h_iso_off.as<int32_t>();
  int32_t *d_ctl = nullptr, *d_hoff = nullptr, *d_hrow = nullptr;
  HIPCHK(c, c->h_iso_ctl.dev(&d_ctl));
  HIPCHK(c, c->h_iso_off.dev(&d_hoff));
  HIPCHK(c, c->h_iso_row.dev(&d_hrow));
  HIPCHK(c, hipStreamSynchronize(s));   // (an earlier call's last kernels write the pinned blocks that are reused from here on)
  h_ctl[0] = h_ctl[1] = h_ctl[2] = h_ctl[3] = 0;
  for (int g = 0; g <= ng; g++) h_off[g] = 0;                    // (k15_offsets overwrites them when the call gets that far)
  int32_t n_kept = 0, n_pool = 0;
  {
    Bracket t(c, c->iso);
    if (n_rows > 0) HIPCHK(c, lcr_fill_async(c->d_iso_row.p, 0xff, (size_t)n_rows * 4, s));   // -1: k15_rows overwrites the rows that hold a kept chain
    { int rc = iso_queue(c, p, d_ctl, d_hoff, &n_kept, &n_pool); if (rc) return rc; }
    launch_k15_export(n_rows, c->d_iso_row.as<int32_t>(), d_hrow, s);   // (also when nothing is kept: every row's -1)
  }
  c->iso_ng = ng; c->iso_n = n_kept; c->iso_nchain = n_pool; c->iso_nrows = n_rows;
  return call_end(c, c->iso);     // lcr_get_isoforms waits for its event
}

int lcr_get_isoforms(lcr_ctx* c, lcr_isoform_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->iso.valid) { c->err = "lcr_get_isoforms before lcr_isoforms (its records die with the phase results)"; return LCR_E_STATE; }
  { int rc = call_wait(c, c->iso); if (rc) return rc; }
  out->n_regions = c->iso_ng; out->n_isoforms = c->iso_n; out->n_chain = c->iso_nchain; out->n_rows = c->iso_nrows;
  out->iso = c->iso_n ? c->h_iso.as<lcr_isoform>() : nullptr;
  out->iso_region_off = c->h_iso_off.as<int32_t>();
  out->chain = c->iso_nchain ? c->h_iso_chain.as<uint64_t>() : nullptr;
  out->row_isoform = c->iso_nrows ? c->h_iso_row.as<int32_t>() : nullptr;
  out->dev_iso = c->iso_n ? c->d_iso.as<lcr_isoform>() : nullptr;
  out->dev_chain = c->iso_nchain ? c->d_iso_chain.as<uint64_t>() : nullptr;
  out->dev_row_isoform = c->iso_nrows ? c->d_iso_row.as<int32_t>() : nullptr;
  return LCR_OK;
}

int lcr_isoforms_ms(lcr_ctx* c, float* ms) {
  if (!c || !ms) return LCR_E_ARG;
  return call_ms(c, c->iso, "lcr_isoforms_ms", "lcr_isoforms", ms);
}

}  // extern "C"

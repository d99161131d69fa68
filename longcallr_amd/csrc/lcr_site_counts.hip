// lcr_site_counts.hip — the host driver of K12 (k12_site_counts.hip): allele x haplotype counts per candidate over the fragment matrix, its
// getter and its timer.  A call of its own behind lcr_phase / lcr_haplotag, shaped like lcr_ase: it reads the fragment stage's CSR, the
// candidate records and the phase stage's read records, and writes buffers no other stage or getter reads (lcr_ctx: d_sc, h_sc) beside the
// segments it shares with lcr_somatic (colsegs; colseg_queue, below, is both calls' first half).
// Five launches (clear, count, two of the scan, fill, sites -- six at most), no host wait of its own: the entry count is the fragment stage's.
#include "lcr_ctx.h"

int colseg_queue(lcr_ctx* c, int32_t n_cand, uint32_t** cnt, int64_t** off, uint64_t** seg) {
  ColSegs& g = c->colsegs;
  HIPCHK(c, g.cnt.reserve((size_t)n_cand * 4));
  HIPCHK(c, g.off.reserve(((size_t)n_cand + 1) * 8));
  HIPCHK(c, g.seg.reserve((size_t)std::max<int64_t>(c->nnz, 1) * 8));
  *cnt = g.cnt.as<uint32_t>(); *off = g.off.as<int64_t>(); *seg = g.seg.as<uint64_t>();
  HIPCHK(c, lcr_fill_async(*cnt, 0, (size_t)n_cand * 4, c->stream));
  launch_colseg_count(c->n_rows, c->row_ptr.as<int64_t>(), c->col.as<int32_t>(), n_cand, *cnt, c->stream);
  launch_scan_i32_to_i64(c->scan_tmp, (const int32_t*)*cnt, *off, n_cand, c->stream);   // (a column has fewer than 2^31 entries: one per row; the offsets are 64 bits)
  return LCR_OK;
}

extern "C" {

int lcr_site_counts(lcr_ctx* c, const lcr_site_count_params* p) {
  if (!c) return LCR_E_ARG;
  if (!p) { c->err = "lcr_site_counts: null params"; return LCR_E_ARG; }
  if (p->min_baseq > 30) { c->err = "lcr_site_counts: min_baseq above 30 (the fragment matrix clamps qualities to 30)"; return LCR_E_ARG; }
  if (c->stage < ST_PHASED) { c->err = "lcr_site_counts before lcr_phase / lcr_haplotag"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }       // an asynchronous phase stage in flight writes the read records and the candidates
  { int rc = cand_settle(c); if (rc) return rc; }
  { int rc = frag_settle(c); if (rc) return rc; }        // (the entry count: long since there behind a phase stage)
  static_assert(sizeof(lcr_site_count) == 64, "lcr_site_count is 64 bytes");
  const int n_rows = c->n_rows, n_cand = (int)c->h_cand.size();
  hipStream_t s = c->stream;
  c->sc.valid = false;   // (from here on the last call's records are overwritten)
  const size_t nc1 = (size_t)std::max(n_cand, 1);
  HIPCHK(c, c->d_sc.reserve(nc1 * sizeof(lcr_site_count)));
  HIPCHK(c, c->h_sc.reserve(nc1 * sizeof(lcr_site_count)));
  lcr_site_count* d_hsc = nullptr;
  HIPCHK(c, c->h_sc.dev(&d_hsc));
  if (Bracket t(c, c->sc); n_cand > 0) {
    uint32_t* cnt; int64_t* off; uint64_t* seg;
    { int rc = colseg_queue(c, n_cand, &cnt, &off, &seg); if (rc) return rc; }
    launch_k12_fill(n_rows, c->row_ptr.as<int64_t>(), c->col.as<int32_t>(), c->val.as<uint8_t>(), c->phase.d_read_rec.as<lcr_read_record>(), p->min_baseq,
                    n_cand, cnt, off, seg, s);
    launch_k12_sites(c->d_cand.as<lcr_candidate>(), n_cand, off, seg, c->d_sc.as<lcr_site_count>(), d_hsc, s);
  }
  c->sc_ncand = n_cand;
  return call_end(c, c->sc);     // lcr_get_site_counts waits for its event
}

int lcr_get_site_counts(lcr_ctx* c, int32_t* n_cand, const lcr_site_count** rec, const lcr_site_count** dev_rec) {
  if (!c || !n_cand || !rec || !dev_rec) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->sc.valid) { c->err = "lcr_get_site_counts before lcr_site_counts (its records die with the phase results)"; return LCR_E_STATE; }
  { int rc = call_wait(c, c->sc); if (rc) return rc; }
  *n_cand = c->sc_ncand;
  *rec = c->sc_ncand ? c->h_sc.as<lcr_site_count>() : nullptr;
  *dev_rec = c->sc_ncand ? c->d_sc.as<lcr_site_count>() : nullptr;
  return LCR_OK;
}

int lcr_site_counts_ms(lcr_ctx* c, float* ms) {
  if (!c || !ms) return LCR_E_ARG;
  return call_ms(c, c->sc, "lcr_site_counts_ms", "lcr_site_counts", ms);
}

}  // extern "C"

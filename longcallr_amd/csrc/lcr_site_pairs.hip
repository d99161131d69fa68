// lcr_site_pairs.hip — the host driver of K19 (k19_site_pairs.hip): base x base counts of nearby site pairs over the fragment matrix, its
// getter and its timer.  A call of its own behind lcr_phase / lcr_haplotag, shaped like lcr_site_counts: it reads the fragment stage's CSR
// and the candidate records, and writes buffers no other stage or getter reads (lcr_ctx: sp_*, d_sp, h_sp*).
// Eleven launches at most (elig, two or four of the first scan, list, count, the second scan's, init, rows, export), no host wait of its own:
// every buffer is sized from n_cand x max_partners, and the last kernel leaves n_eligible and n_pairs in pinned memory for the getter.
#include "lcr_ctx.h"

extern "C" {

int lcr_site_pairs(lcr_ctx* c, const lcr_site_pair_params* p) {
  if (!c) return LCR_E_ARG;
  if (!p) { c->err = "lcr_site_pairs: null params"; return LCR_E_ARG; }
  if (p->mode != LCR_PAIRS_ALL && p->mode != LCR_PAIRS_PHASED) { c->err = "lcr_site_pairs: unknown mode"; return LCR_E_ARG; }
  if (p->max_partners < 1 || p->max_partners > LCR_PAIRS_MAX_PARTNERS) { c->err = "lcr_site_pairs: max_partners outside 1..8"; return LCR_E_ARG; }
  if (p->min_baseq > 30) { c->err = "lcr_site_pairs: min_baseq above 30 (the fragment matrix clamps qualities to 30)"; return LCR_E_ARG; }
  if (c->stage < ST_PHASED) { c->err = "lcr_site_pairs before lcr_phase / lcr_haplotag"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }       // an asynchronous phase stage in flight writes the candidates
  { int rc = cand_settle(c); if (rc) return rc; }
  { int rc = frag_settle(c); if (rc) return rc; }
  static_assert(sizeof(lcr_site_pair) == 80, "lcr_site_pair is 80 bytes");
  const int n_rows = c->n_rows, n_cand = (int)c->h_cand.size();
  const uint32_t K = p->max_partners;
  if ((uint64_t)n_cand * K > 0x7fffffffull) { c->err = "lcr_site_pairs: n_cand x max_partners above 2^31 - 1"; return LCR_E_ARG; }
  hipStream_t s = c->stream;
  c->pairs.valid = false;   // (from here on the last call's records are overwritten)
  const size_t nc1 = (size_t)std::max(n_cand, 1), np1 = nc1 * K;
  for (DevBuf* b : {&c->sp_elig, &c->sp_rank, &c->sp_list, &c->sp_erank, &c->sp_m}) HIPCHK(c, b->reserve(nc1 * 4));
  HIPCHK(c, c->sp_ctl.reserve(4));
  HIPCHK(c, c->sp_off.reserve((nc1 + 1) * 4));
  HIPCHK(c, c->d_sp.reserve(np1 * sizeof(lcr_site_pair)));
  HIPCHK(c, c->h_sp.reserve(np1 * sizeof(lcr_site_pair)));
  HIPCHK(c, c->h_sp_off.reserve((nc1 + 1) * 4));
  HIPCHK(c, c->h_sp_ctl.reserve(8));
  lcr_site_pair* d_hsp = nullptr; int32_t *d_hoff = nullptr, *d_hctl = nullptr;
  HIPCHK(c, c->h_sp.dev(&d_hsp));
  HIPCHK(c, c->h_sp_off.dev(&d_hoff));
  HIPCHK(c, c->h_sp_ctl.dev(&d_hctl));
  {
    Bracket t(c, c->pairs);
    const lcr_candidate* cand = c->d_cand.as<lcr_candidate>();
    int32_t *elig = c->sp_elig.as<int32_t>(), *rank = c->sp_rank.as<int32_t>(), *list = c->sp_list.as<int32_t>(), *erank = c->sp_erank.as<int32_t>();
    int32_t *m = c->sp_m.as<int32_t>(), *n_elig = c->sp_ctl.as<int32_t>(), *off = c->sp_off.as<int32_t>();
    lcr_site_pair* pair = c->d_sp.as<lcr_site_pair>();
    launch_k19_elig(cand, n_cand, p->mode, elig, s);
    launch_scan_i32(c->scan_tmp, elig, rank, n_cand, n_elig, s);        // (n_cand == 0: clears the total)
    launch_k19_list(elig, rank, n_cand, list, erank, s);
    launch_k19_count(cand, n_cand, erank, list, n_elig, K, p->max_dist, m, s);
    launch_scan_i32(c->scan_tmp, m, off, n_cand, off + n_cand, s);      // (n_cand == 0: off[0] = 0)
    launch_k19_init(n_cand, K, erank, list, off, pair, s);
    launch_k19_rows(n_rows, c->row_ptr.as<int64_t>(), c->col.as<int32_t>(), c->val.as<uint8_t>(), n_cand, erank, off, p->min_baseq, pair, s);
    launch_k19_export(n_cand, K, n_elig, off, pair, d_hsp, d_hoff, d_hctl, s);
  }
  c->sp_ncand = n_cand;
  return call_end(c, c->pairs);     // lcr_get_site_pairs waits for its event
}

int lcr_get_site_pairs(lcr_ctx* c, lcr_site_pair_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->pairs.valid) { c->err = "lcr_get_site_pairs before lcr_site_pairs (its records die with the phase results)"; return LCR_E_STATE; }
  { int rc = call_wait(c, c->pairs); if (rc) return rc; }
  const int32_t* ctl = c->h_sp_ctl.as<int32_t>();
  out->n_cand = c->sp_ncand; out->n_eligible = ctl[0]; out->n_pairs = ctl[1]; out->pad_ = 0;
  out->pair = ctl[1] ? c->h_sp.as<lcr_site_pair>() : nullptr;
  out->pair_off = c->h_sp_off.as<int32_t>();
  out->dev_pair = ctl[1] ? c->d_sp.as<lcr_site_pair>() : nullptr;
  out->dev_pair_off = c->sp_off.as<int32_t>();
  return LCR_OK;
}

int lcr_site_pairs_ms(lcr_ctx* c, float* ms) {
  if (!c || !ms) return LCR_E_ARG;
  return call_ms(c, c->pairs, "lcr_site_pairs_ms", "lcr_site_pairs", ms);
}

}  // extern "C"

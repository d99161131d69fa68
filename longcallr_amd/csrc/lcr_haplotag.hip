// lcr_haplotag.hip — the host driver of K11 (k11_haplotag.hip): the rows of the fragment matrix tagged on the caller's haplotypes, in place of
// lcr_phase.  It reads the fragment stage's CSR and the candidate records, and fills what the phase stage fills -- the candidate records
// (HBM, and through PhaseHost's pinned mirror the host's), the per-row results in PhaseHost's pinned block, the read records in HBM -- so
// every getter and every call behind lcr_phase answers as it does there.  Its own: the site arrays, a byte and a word per candidate, the
// site records (lcr_ctx: ht_*, d_hsite, h_hsite).  Down-sampling is ignored: the stage is linear in the entries and sees every row.
#include "lcr_ctx.h"

// What the call left in flight on the context's stream: its last kernel wrote the candidates' mirror into pinned memory; the host's
// records follow here, for whoever asks first (phase_settle, lcr_ctx.h)
int haplotag_settle(lcr_ctx* c) {
  if (!c->hap_pending) return LCR_OK;
  c->hap_pending = false;
  HIPCHK(c, hipEventSynchronize(c->hap.ev));
  HIPCHK(c, hipGetLastError());
  if ((int32_t)c->h_cand.size() == c->hap_ncand && c->hap_ncand > 0)
    memcpy(c->h_cand.data(), c->phase.h_cand_obj.p, (size_t)c->hap_ncand * sizeof(lcr_candidate));
  return LCR_OK;
}

extern "C" {

int lcr_haplotag(lcr_ctx* c, const lcr_params* p, int32_t mem, int32_t n_sites, const int64_t* pos0, const uint8_t* h1, const uint8_t* h2,
                 const uint32_t* phase_set) {
  if (!c) return LCR_E_ARG;
  if (!p || n_sites < 0 || (mem != LCR_MEM_HOST && mem != LCR_MEM_DEVICE)) {
    c->err = "lcr_haplotag: null params, n_sites < 0 or mem not LCR_MEM_HOST / LCR_MEM_DEVICE";
    return LCR_E_ARG;
  }
  if (n_sites > 0 && (!pos0 || !h1 || !h2 || !phase_set)) { c->err = "lcr_haplotag: null site array"; return LCR_E_ARG; }
  if (c->stage < ST_FRAGGED) { c->err = "lcr_haplotag before lcr_fragments"; return LCR_E_STATE; }
  if (c->cand_used) { c->err = "lcr_haplotag after lcr_phase / lcr_haplotag: the candidate records have been rewritten; run the candidate stage again"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }   // (an asynchronous phase stage in flight owns the pinned result blocks)
  { int rc = cand_settle(c); if (rc) return rc; }
  { int rc = frag_settle(c); if (rc) return rc; }
  static_assert(sizeof(lcr_haplotag_site) == 32, "lcr_haplotag_site is 32 bytes");
  hipStream_t s = c->stream;
  // the sites: copied (host) or read in place (device), then checked by a kernel -- the call's one host wait.  Nothing the last stage
  // left is touched before the verdict: a refused call changes nothing.
  K11Sites st{nullptr, nullptr, nullptr, nullptr, n_sites};
  if (n_sites > 0) {
    { int rc = upload(c, c->ht_pos, pos0, (size_t)n_sites, &st.pos0, mem); if (rc) return rc; }
    { int rc = upload(c, c->ht_h1, h1, (size_t)n_sites, &st.h1, mem); if (rc) return rc; }
    { int rc = upload(c, c->ht_h2, h2, (size_t)n_sites, &st.h2, mem); if (rc) return rc; }
    { int rc = upload(c, c->ht_ps, phase_set, (size_t)n_sites, &st.ps, mem); if (rc) return rc; }
    HIPCHK(c, c->h_hap_bad.reserve(64));
    int32_t* bad = c->h_hap_bad.as<int32_t>();
    *bad = 0;
    int32_t* d_bad = nullptr;
    HIPCHK(c, c->h_hap_bad.dev(&d_bad));
    launch_k11_check(st, d_bad, s);
    { int rc = stream_wait(c, c->hap.ev); if (rc) return rc; }
    if (*(volatile int32_t*)bad) {
      c->err = "lcr_haplotag: sites must be sorted by position without duplicates, h1 and h2 one of ACGT each and different, phase_set non-zero";
      return LCR_E_ARG;
    }
  }
  const int ng = c->bv.n_regions, n_rows = c->n_rows, n_cand = (int)c->h_cand.size();
  const size_t nr1 = (size_t)std::max(n_rows, 1), nc1 = (size_t)std::max(n_cand, 1);
  PhaseHost& ph = c->phase;
  // the phase stage's result blocks, laid out as PhaseHost::size_buffers lays them out: phase set u32 | haplotag | assignment
  const size_t res_ps = 0, res_tag = nr1 * 4, res_asg = nr1 * 5;
  HIPCHK(c, ph.h_res.reserve(nr1 * 6));
  HIPCHK(c, ph.h_cand_obj.reserve(nc1 * sizeof(lcr_candidate)));
  HIPCHK(c, ph.d_read_rec.reserve(nr1 * 12));
  HIPCHK(c, c->ht_site.reserve(nc1)); HIPCHK(c, c->ht_site_ps.reserve(nc1 * 4));
  HIPCHK(c, c->d_hsite.reserve(nc1 * sizeof(lcr_haplotag_site))); HIPCHK(c, c->h_hsite.reserve(nc1 * sizeof(lcr_haplotag_site)));
  uint8_t* d_res = nullptr; lcr_candidate* d_hc = nullptr; lcr_haplotag_site* d_hs = nullptr;
  HIPCHK(c, ph.h_res.dev(&d_res)); HIPCHK(c, ph.h_cand_obj.dev(&d_hc)); HIPCHK(c, c->h_hsite.dev(&d_hs));
  // from here on the candidate records and the last result blocks are rewritten
  c->cand_used = true;
  c->hap.valid = false;
  c->ds_rows_set = false;   // (a sample given for "the next lcr_phase" is not kept for a later one)
  lcr_candidate* cand = c->d_cand.as<lcr_candidate>();
  const K11Rows rows{(int8_t*)(d_res + res_tag), d_res + res_asg, (uint32_t*)(d_res + res_ps), ph.d_read_rec.as<uint32_t>()};
  {
    Bracket t(c, c->hap);
    launch_k11_sites(cand, n_cand, st, c->ht_site.as<uint8_t>(), c->ht_site_ps.as<uint32_t>(), c->d_hsite.as<lcr_haplotag_site>(), s);
    launch_k11_rows(n_rows, c->row_ptr.as<int64_t>(), c->col.as<int32_t>(), c->val.as<uint8_t>(), c->ht_site.as<uint8_t>(), c->ht_site_ps.as<uint32_t>(),
                    phase_lut_dev(), p->min_linkers, p->read_assign_cutoff, rows, c->d_hsite.as<lcr_haplotag_site>(), s);
    launch_k11_finish(cand, n_cand, c->ht_site.as<uint8_t>(), c->d_hsite.as<lcr_haplotag_site>(), d_hc, d_hs, s);
  }
  { int rc = call_end(c, c->hap); if (rc) return rc; }   // haplotag_settle and lcr_get_haplotag_sites wait for its event
  // what the getters of the phase stage hand out: the per-row results are read in place, no optimiser ran
  ph.r_haplotag = (const int8_t*)(ph.h_res.as<uint8_t>() + res_tag); ph.r_assignment = ph.h_res.as<uint8_t>() + res_asg;
  ph.r_phase_set = (const uint32_t*)(ph.h_res.as<uint8_t>() + res_ps);
  ph.objective.assign((size_t)ng, 0.0);
  memset(ph.tie_census, 0, sizeof(ph.tie_census));
  ph.chain_desc.clear();   // (lcr_get_ld_blocks: no region built blocks)
  ph.ds_applied.assign((size_t)ng, 0); ph.ds_any = false; ph.ds_ng = ng; ph.ds_nrow = n_rows;   // (lcr_get_downsample: no region was down-sampled)
  c->hap_ncand = n_cand; c->hap_pending = true;
  c->stage = ST_PHASED;
  c->res_valid = true; c->res_ng = ng;
  c->phase_slot = c->bound_slot >= 0 ? c->bound_slot : (c->bound_host ? -2 : -1);
  return LCR_OK;
}

int lcr_get_haplotag_sites(lcr_ctx* c, int32_t* n_cand, const lcr_haplotag_site** rec, const lcr_haplotag_site** dev_rec) {
  if (!c || !n_cand || !rec || !dev_rec) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->hap.valid) { c->err = "lcr_get_haplotag_sites before lcr_haplotag (its records die with the phase results)"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }
  { int rc = call_wait(c, c->hap); if (rc) return rc; }
  *n_cand = c->hap_ncand;
  *rec = c->hap_ncand ? c->h_hsite.as<lcr_haplotag_site>() : nullptr;
  *dev_rec = c->hap_ncand ? c->d_hsite.as<lcr_haplotag_site>() : nullptr;
  return LCR_OK;
}

int lcr_haplotag_ms(lcr_ctx* c, float* ms) {
  if (!c || !ms) return LCR_E_ARG;
  return call_ms(c, c->hap, "lcr_haplotag_ms", "lcr_haplotag", ms);
}

}  // extern "C"

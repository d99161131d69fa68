// lcr_ase.hip — the host driver of K7 (k7_ase.hip): haplotype and parent-of-origin counts per region over the phased rows, and its getter.
// A call of its own behind lcr_phase, shaped like lcr_junctions: it reads the fragment stage's row offsets and CSR, the candidate records
// and the phase stage's read records, and writes buffers no other stage or getter reads (lcr_ctx: a_*, d_ase, h_ase*).
#include "lcr_ctx.h"

extern "C" {

int lcr_ase(lcr_ctx* c, const lcr_ase_params* p, int32_t mem, int32_t n_sites, const int64_t* pos0, const uint8_t* pat, const uint8_t* mat) {
  if (!c) return LCR_E_ARG;
  if (!p || n_sites < 0 || (mem != LCR_MEM_HOST && mem != LCR_MEM_DEVICE)) {
    c->err = "lcr_ase: null params, n_sites < 0 or mem not LCR_MEM_HOST / LCR_MEM_DEVICE";
    return LCR_E_ARG;
  }
  if (p->min_baseq > 30) { c->err = "lcr_ase: min_baseq above 30 (the fragment matrix clamps qualities to 30)"; return LCR_E_ARG; }
  if (n_sites > 0 && (!pos0 || !pat || !mat)) { c->err = "lcr_ase: null site array"; return LCR_E_ARG; }
  if (c->stage < ST_PHASED) { c->err = "lcr_ase before lcr_phase"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }       // an asynchronous phase stage in flight writes the read records and the candidates
  { int rc = cand_settle(c); if (rc) return rc; }
  static_assert(sizeof(lcr_ase_region) == 40, "lcr_ase_region is 40 bytes");
  const int ng = c->bv.n_regions, n_rows = c->n_rows, n_cand = (int)c->h_cand.size();
  hipStream_t s = c->stream;
  // the parental sites: copied (host) or read in place (device), then checked by a kernel -- the call's one host wait.  Nothing the last
  // call left is touched before the verdict: a refused call changes nothing.
  const int64_t* d_pos = nullptr; const uint8_t* d_pat = nullptr; const uint8_t* d_mat = nullptr;
  if (n_sites > 0) {
    { int rc = upload(c, c->a_pos, pos0, (size_t)n_sites, &d_pos, mem); if (rc) return rc; }
    { int rc = upload(c, c->a_pat, pat, (size_t)n_sites, &d_pat, mem); if (rc) return rc; }
    { int rc = upload(c, c->a_mat, mat, (size_t)n_sites, &d_mat, mem); if (rc) return rc; }
    HIPCHK(c, c->h_ase_bad.reserve(64));
    int32_t* bad = c->h_ase_bad.as<int32_t>();
    *bad = 0;
    int32_t* d_bad = nullptr;
    HIPCHK(c, c->h_ase_bad.dev(&d_bad));
    launch_k7_check(d_pos, d_pat, d_mat, n_sites, d_bad, s);
    { int rc = stream_wait(c, c->ase.ev); if (rc) return rc; }
    if (*(volatile int32_t*)bad) {
      c->err = "lcr_ase: parental sites must be sorted by position without duplicates, pat and mat one of ACGT each and different";
      return LCR_E_ARG;
    }
  }
  c->ase.valid = false;   // (from here on the last call's records are overwritten)
  HIPCHK(c, c->d_ase.reserve((size_t)std::max(ng, 1) * sizeof(lcr_ase_region)));
  HIPCHK(c, c->h_ase.reserve((size_t)std::max(ng, 1) * sizeof(lcr_ase_region)));
  lcr_ase_region* d_hase = nullptr;
  HIPCHK(c, c->h_ase.dev(&d_hase));
  lcr_ase_region* d_ase = c->d_ase.as<lcr_ase_region>();
  const lcr_read_record* rec = c->phase.d_read_rec.as<lcr_read_record>();
  const int32_t* rro = c->row_region_off.as<int32_t>();
  if (n_sites > 0) {
    HIPCHK(c, c->a_tag.reserve((size_t)std::max(n_rows, 1) * 4));
    HIPCHK(c, c->a_site.reserve((size_t)std::max(n_cand, 1)));
  }
  {
    Timer t(c, LCR_K_ASE);
    if (n_sites == 0) {
      launch_k7_pick(rro, rec, ng, d_ase, d_hase, nullptr, s);   // the records go to HBM and to pinned host memory by the one kernel
    } else {
      launch_k7_pick(rro, rec, ng, d_ase, nullptr, c->a_tag.as<int32_t>(), s);
      launch_k7_sites(c->d_cand.as<lcr_candidate>(), n_cand, (double)p->min_phase_score, d_pos, d_pat, d_mat, n_sites, d_ase, c->a_site.as<uint8_t>(), s);
      launch_k7_votes(c->a_tag.as<int32_t>(), n_rows, c->row_ptr.as<int64_t>(), c->col.as<int32_t>(), c->val.as<uint8_t>(), c->a_site.as<uint8_t>(),
                      p->min_baseq, d_ase, s);
      launch_k7_export(d_ase, ng, d_hase, s);
    }
  }
  c->ase_ng = ng;
  return call_end(c, c->ase);     // lcr_get_ase waits for its event
}

int lcr_get_ase(lcr_ctx* c, lcr_ase_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->ase.valid) { c->err = "lcr_get_ase before lcr_ase (its records die with the phase stage's results)"; return LCR_E_STATE; }
  { int rc = call_wait(c, c->ase); if (rc) return rc; }
  out->n_regions = c->ase_ng;
  out->rec = c->ase_ng ? c->h_ase.as<lcr_ase_region>() : nullptr;
  out->dev_rec = c->ase_ng ? c->d_ase.as<lcr_ase_region>() : nullptr;
  return LCR_OK;
}

}  // extern "C"

// lcr_somatic.hip — the host driver of K14 (k14_somatic.hip): the three-class model per haplotype at every candidate over the fragment
// matrix, its getter and its timer.  A call of its own behind lcr_phase / lcr_haplotag, shaped like lcr_site_counts: it reads the fragment
// stage's CSR, the candidate records and the phase stage's read records, and writes buffers no other stage or getter reads (lcr_ctx:
// d_som, h_som) beside the segments it shares with lcr_site_counts (colsegs, colseg_queue).  The tables are built here per call and travel as a kernel argument, so a repeated call with other params waits
// for nothing.  Six launches (clear, count, two of the scan, fill, sites), no host wait of its own: the entry count is the fragment stage's.
#include <cmath>

#include "lcr_ctx.h"

namespace {

constexpr double FX_SCALE = 1099511627776.0;   // 2^40, the phase stage's scale (k4_dev.h)

// include/lcr.h: llround(log10(x) * 2^40); eps_q = 10^(-q / 10), q = 0 as q = 1 (HostLut's rule, k4_phase.hip)
K14Tables somatic_tables(const lcr_somatic_params& p) {
  K14Tables t;
  auto fx = [](double x) { return (int64_t)std::llround(std::log10(x) * FX_SCALE); };
  for (int q = 0; q <= 30; q++) {
    const int qq = q == 0 ? 1 : q;
    const double eps = std::pow(10.0, -(double)qq / 10.0);
    t.tab[q] = fx(eps);
    t.tab[31 + q] = fx(1.0 - eps);
    t.tab[62 + q] = fx(p.purity * eps + (1.0 - p.purity) * (1.0 - eps));   // somatic.rs:22: a reference base on a somatic haplotype
    t.tab[93 + q] = fx(p.purity * (1.0 - eps) + (1.0 - p.purity) * eps);   // somatic.rs:28: an alternate base
  }
  t.prior[0] = fx(1.0 - p.het_rate - p.som_rate); t.prior[1] = fx(p.het_rate); t.prior[2] = fx(p.som_rate);
  return t;
}

}  // namespace

extern "C" {

int lcr_somatic(lcr_ctx* c, const lcr_somatic_params* p) {
  if (!c) return LCR_E_ARG;
  if (!p) { c->err = "lcr_somatic: null params"; return LCR_E_ARG; }
  if (!(p->purity > 0.0 && p->purity <= 1.0)) { c->err = "lcr_somatic: purity outside (0, 1]"; return LCR_E_ARG; }
  if (!(p->som_rate > 0.0) || !(p->het_rate > 0.0) || !(p->het_rate + p->som_rate < 1.0)) {
    c->err = "lcr_somatic: som_rate and het_rate must be positive and add up to less than 1"; return LCR_E_ARG;
  }
  if (p->min_baseq > 30) { c->err = "lcr_somatic: min_baseq above 30 (the fragment matrix clamps qualities to 30)"; return LCR_E_ARG; }
  if (c->stage < ST_PHASED) { c->err = "lcr_somatic before lcr_phase / lcr_haplotag"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }       // an asynchronous phase stage in flight writes the read records and the candidates
  { int rc = cand_settle(c); if (rc) return rc; }
  { int rc = frag_settle(c); if (rc) return rc; }        // (the entry count: long since there behind a phase stage)
  static_assert(sizeof(lcr_somatic_site) == 80, "lcr_somatic_site is 80 bytes");
  const K14Tables t = somatic_tables(*p);
  const int n_rows = c->n_rows, n_cand = (int)c->h_cand.size();
  hipStream_t s = c->stream;
  c->som.valid = false;   // (from here on the last call's records are overwritten)
  const size_t nc1 = (size_t)std::max(n_cand, 1);
  HIPCHK(c, c->d_som.reserve(nc1 * sizeof(lcr_somatic_site)));
  HIPCHK(c, c->h_som.reserve(nc1 * sizeof(lcr_somatic_site)));
  lcr_somatic_site* d_hsom = nullptr;
  HIPCHK(c, c->h_som.dev(&d_hsom));
  if (Bracket br(c, c->som); n_cand > 0) {
    uint32_t* cnt; int64_t* off; uint64_t* seg;
    { int rc = colseg_queue(c, n_cand, &cnt, &off, &seg); if (rc) return rc; }
    launch_k14_fill(n_rows, c->row_ptr.as<int64_t>(), c->col.as<int32_t>(), c->val.as<uint8_t>(), c->phase.d_read_rec.as<lcr_read_record>(),
                    c->d_cand.as<lcr_candidate>(), n_cand, cnt, off, seg, s);
    launch_k14_sites(c->d_cand.as<lcr_candidate>(), n_cand, off, seg, t, p->min_baseq, c->d_som.as<lcr_somatic_site>(), d_hsom, s);
  }
  c->som_ncand = n_cand;
  return call_end(c, c->som);     // lcr_get_somatic waits for its event
}

int lcr_get_somatic(lcr_ctx* c, int32_t* n_cand, const lcr_somatic_site** rec, const lcr_somatic_site** dev_rec) {
  if (!c || !n_cand || !rec || !dev_rec) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->som.valid) { c->err = "lcr_get_somatic before lcr_somatic (its records die with the phase results)"; return LCR_E_STATE; }
  { int rc = call_wait(c, c->som); if (rc) return rc; }
  *n_cand = c->som_ncand;
  *rec = c->som_ncand ? c->h_som.as<lcr_somatic_site>() : nullptr;
  *dev_rec = c->som_ncand ? c->d_som.as<lcr_somatic_site>() : nullptr;
  return LCR_OK;
}

int lcr_somatic_ms(lcr_ctx* c, float* ms) {
  if (!c || !ms) return LCR_E_ARG;
  return call_ms(c, c->som, "lcr_somatic_ms", "lcr_somatic", ms);
}

}  // extern "C"

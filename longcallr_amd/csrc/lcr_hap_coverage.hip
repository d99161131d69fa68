// lcr_hap_coverage.hip — the host driver of K13 (k13_hap_coverage.hip): covered depth per haplotype class at every window column as
// run-length segments, its getter and its timer.  A call of its own behind lcr_phase / lcr_haplotag, shaped like lcr_junctions: it reads
// the bound batch (CIGARs, positions, region tables), the candidate stage's rows per region and the phase stage's read records, and writes
// buffers no other stage or getter reads (lcr_ctx: hc_*, d_hc_*, h_hc_*).  Count-pass form: one host wait, on the number of segments.
#include "lcr_ctx.h"

extern "C" {

int lcr_hap_coverage(lcr_ctx* c) {
  if (!c) return LCR_E_ARG;
  if (c->stage < ST_PHASED) { c->err = "lcr_hap_coverage before lcr_phase / lcr_haplotag"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }       // an asynchronous phase stage in flight writes the read records
  static_assert(sizeof(lcr_hap_cov_segment) == 32, "lcr_hap_cov_segment is 32 bytes");
  static_assert(sizeof(lcr_hap_cov_region) == 56, "lcr_hap_cov_region is 56 bytes");
  const BatchView& b = c->bv;
  const int ng = b.n_regions;
  const int64_t n_cols = c->n_cols;
  hipStream_t s = c->stream;
  c->hc.valid = false;   // (from here on the last call's records are overwritten)
  const size_t ng1 = (size_t)std::max(ng, 1);
  HIPCHK(c, c->hc_planes.reserve((size_t)std::max<int64_t>(n_cols, 1) * 12));
  HIPCHK(c, c->hc_nseg.reserve(ng1 * 4));
  HIPCHK(c, c->hc_off.reserve((ng1 + 1) * 4));
  HIPCHK(c, c->d_hc_reg.reserve(ng1 * sizeof(lcr_hap_cov_region)));
  HIPCHK(c, c->h_hc_reg.reserve(ng1 * sizeof(lcr_hap_cov_region)));
  HIPCHK(c, c->h_hc_off.reserve((ng1 + 1) * 4));
  int32_t* const h_off = c->h_hc_off.as<int32_t>();
  int32_t* d_hoff = nullptr;
  lcr_hap_cov_region* d_hreg = nullptr;
  HIPCHK(c, c->h_hc_off.dev(&d_hoff));
  HIPCHK(c, c->h_hc_reg.dev(&d_hreg));
  int32_t n_seg = 0;
  if (Bracket t(c, c->hc); ng > 0) {
    uint32_t* planes = c->hc_planes.as<uint32_t>();
    int32_t* off = c->hc_off.as<int32_t>();
    const int32_t* rro = c->row_region_off.as<int32_t>();
    const lcr_read_record* rec = c->phase.d_read_rec.as<lcr_read_record>();
    // 1. difference planes, depths, region records, run starts per region and their offsets
    if (n_cols > 0) HIPCHK(c, lcr_fill_async(planes, 0, (size_t)n_cols * 12, s));
    launch_k13_blocks(b, rro, rec, n_cols, planes, s);
    launch_k13_scan(b, rro, rec, n_cols, planes, c->d_hc_reg.as<lcr_hap_cov_region>(), c->hc_nseg.as<int32_t>(), s);
    launch_scan_i32(c->scan_tmp, c->hc_nseg.as<int32_t>(), off, ng, off + ng, s);
    launch_k13_offsets(ng, off, c->d_hc_reg.as<lcr_hap_cov_region>(), d_hoff, d_hreg, s);
    { int rc = stream_wait(c, c->hc.ev); if (rc) return rc; }   // the number of segments sizes the records
    n_seg = h_off[ng];
    for (int g = 0; g < ng; g++)
      if (h_off[g + 1] < h_off[g]) { c->err = "lcr_hap_coverage: more than 2^31 - 1 segments in one batch; split it"; return LCR_E_ARG; }
    // 2. the segments, in order; the records go to HBM and, by the last kernel, to pinned host memory
    if (n_seg > 0) {
      HIPCHK(c, c->hc_send.reserve((size_t)n_seg * 4));
      HIPCHK(c, c->d_hc_seg.reserve((size_t)n_seg * sizeof(lcr_hap_cov_segment)));
      HIPCHK(c, c->h_hc_seg.reserve((size_t)n_seg * sizeof(lcr_hap_cov_segment)));
      lcr_hap_cov_segment* d_hseg = nullptr;
      HIPCHK(c, c->h_hc_seg.dev(&d_hseg));
      launch_k13_emit(b, n_cols, planes, off, c->d_hc_seg.as<lcr_hap_cov_segment>(), c->hc_send.as<int32_t>(), s);
      launch_k13_finish(n_seg, ng, b.start0, c->hc_send.as<int32_t>(), c->d_hc_seg.as<lcr_hap_cov_segment>(), d_hseg, s);
    }
  } else {
    h_off[0] = 0;
  }
  c->hc_ng = ng; c->hc_n = n_seg;
  return call_end(c, c->hc);     // lcr_get_hap_coverage waits for its event
}

int lcr_get_hap_coverage(lcr_ctx* c, lcr_hap_cov_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->hc.valid) { c->err = "lcr_get_hap_coverage before lcr_hap_coverage (its records die with the phase results)"; return LCR_E_STATE; }
  { int rc = call_wait(c, c->hc); if (rc) return rc; }
  out->n_regions = c->hc_ng; out->n_segments = c->hc_n;
  out->seg = c->hc_n ? c->h_hc_seg.as<lcr_hap_cov_segment>() : nullptr;
  out->seg_region_off = c->h_hc_off.as<int32_t>();
  out->reg = c->hc_ng ? c->h_hc_reg.as<lcr_hap_cov_region>() : nullptr;
  out->dev_seg = c->hc_n ? c->d_hc_seg.as<lcr_hap_cov_segment>() : nullptr;
  out->dev_reg = c->hc_ng ? c->d_hc_reg.as<lcr_hap_cov_region>() : nullptr;
  return LCR_OK;
}

int lcr_hap_coverage_ms(lcr_ctx* c, float* ms) {
  if (!c || !ms) return LCR_E_ARG;
  return call_ms(c, c->hc, "lcr_hap_coverage_ms", "lcr_hap_coverage", ms);
}

}  // extern "C"

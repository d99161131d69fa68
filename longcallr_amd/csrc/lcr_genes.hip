// lcr_genes.hip — the host driver of K8 (k8_genes.hip): read -> gene over the bound batch (lcr_assign_genes, lcr_get_read_genes) and the
// per-gene form of K7's counts on top of it (lcr_ase_genes, lcr_get_ase_genes).  lcr_assign_genes reads the bound batch's positions and
// CIGARs only, at any stage, and does not move the stage; lcr_ase_genes is shaped like lcr_ase and reads what it reads plus the gene of
// every read.  Both write buffers no other stage or getter reads (lcr_ctx: g_ann, g_pmax, d_gene*, h_gene*; ag_*, d_agene, h_agene*).
// annotation_queue / annotation_verdict (lcr_ctx.h): the upload and check of an annotation, for every call that takes one.
#include "lcr_ctx.h"
#include "lcr_asj_args.h"

int annotation_queue(lcr_ctx* c, AnnotationCopy& to, const lcr_gene_annotation* a, int32_t mem, HostBuf& h_bad, lcr_gene_annotation* d, int32_t** d_bad) {
  *d = lcr_gene_annotation{};
  d->n_genes = a->n_genes; d->n_exons = a->n_exons;
  HIPCHK(c, h_bad.reserve(64));
  h_bad.as<int32_t>()[0] = h_bad.as<int32_t>()[1] = 0;
  HIPCHK(c, h_bad.dev(d_bad));
  if (a->n_genes == 0) return LCR_OK;
  const size_t n = (size_t)a->n_genes, nx = (size_t)a->n_exons;
  { int rc = upload(c, to.span_s, a->span_start0, n, &d->span_start0, mem); if (rc) return rc; }
  { int rc = upload(c, to.span_e, a->span_end0, n, &d->span_end0, mem); if (rc) return rc; }
  { int rc = upload(c, to.exon_off, a->exon_off, n + 1, &d->exon_off, mem); if (rc) return rc; }
  { int rc = upload(c, to.exon_s, a->exon_start0, nx, &d->exon_start0, mem); if (rc) return rc; }
  { int rc = upload(c, to.exon_e, a->exon_end0, nx, &d->exon_end0, mem); if (rc) return rc; }
  launch_k8_check(*d, *d_bad, c->stream);
  return LCR_OK;
}

int annotation_verdict(lcr_ctx* c, const HostBuf& h_bad, hipEvent_t ev, const char* fn) {
  { int rc = stream_wait(c, ev); if (rc) return rc; }
  if (!*(volatile int32_t*)h_bad.p) return LCR_OK;
  c->err = std::string(fn) + ": genes must be sorted by (span_start0, span_end0), every gene needs exons that are ascending and disjoint, "
           "the first one starting at its span_start0 and the last one ending at its span_end0, and exon_off must run from 0 to n_exons";
  return LCR_E_ARG;
}

extern "C" {

int lcr_assign_genes(lcr_ctx* c, int32_t mem, const lcr_gene_annotation* a) {
  if (!c) return LCR_E_ARG;
  if (!lcr_annotation_sizes_ok(mem, a)) { c->err = "lcr_assign_genes: null annotation" LCR_ANNOTATION_SIZES_MSG; return LCR_E_ARG; }
  if (!lcr_annotation_arrays_ok(a)) { c->err = "lcr_assign_genes" LCR_ANNOTATION_ARRAYS_MSG; return LCR_E_ARG; }
  if (c->stage < ST_LOADED) { c->err = "lcr_assign_genes before lcr_load_batch / lcr_bind_batch"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  const BatchView& b = c->bv;
  const int nr = b.n_reads, n_genes = a->n_genes;
  hipStream_t s = c->stream;
  // the annotation: copied (host) or read in place (device), then checked by a kernel -- the call's one host wait.  Nothing of the last
  // call's result is touched before the verdict: a refused call changes nothing (the copies of the last annotation are overwritten in
  // front of it: nothing reads them once that call's k8_assign has run, and the stream orders the uploads behind it).
  lcr_gene_annotation d{};
  int32_t* d_bad = nullptr;
  if (n_genes > 0) HIPCHK(c, c->g_pmax.reserve((size_t)n_genes * 8));
  { int rc = annotation_queue(c, c->g_ann, a, mem, c->h_gene_bad, &d, &d_bad); if (rc) return rc; }
  if (n_genes > 0) {
    launch_k8_prefix_max(d, c->g_pmax.as<int64_t>(), s);   // (gene-scale, built beside the check: the upload's part of the work)
    { int rc = annotation_verdict(c, c->h_gene_bad, c->ev_genes, "lcr_assign_genes"); if (rc) return rc; }
  }
  c->genes_valid = false;   // (from here on the last call's result is overwritten)
  c->agene.valid = false;   // (... and the pair records of lcr_ase_genes counted the rows of that assignment)
  c->jgene.st.valid = c->ajgene.st.valid = false;   // (... and so did the junction tables of lcr_junctions_genes and lcr_asj_genes)
  const size_t n1 = (size_t)std::max(nr, 1);
  HIPCHK(c, c->d_gene.reserve(n1 * 4)); HIPCHK(c, c->d_gene_ov.reserve(n1 * 4));
  HIPCHK(c, c->h_gene.reserve(n1 * 4)); HIPCHK(c, c->h_gene_ov.reserve(n1 * 4));
  {
    Timer t(c, LCR_K_GENES);
    launch_k8_assign(b, d, c->g_pmax.as<int64_t>(), c->d_gene.as<int32_t>(), c->d_gene_ov.as<uint32_t>(), s);
    if (nr > 0) {
      HIPCHK(c, hipMemcpyAsync(c->h_gene.p, c->d_gene.p, (size_t)nr * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipMemcpyAsync(c->h_gene_ov.p, c->d_gene_ov.p, (size_t)nr * 4, hipMemcpyDeviceToHost, s));
    }
  }
  HIPCHK(c, hipEventRecord(c->ev_genes, s));   // lcr_get_read_genes waits for it
  HIPCHK(c, hipGetLastError());
  c->genes_nr = nr; c->genes_n_genes = n_genes; c->genes_valid = true;
  return LCR_OK;
}

int lcr_get_read_genes(lcr_ctx* c, int32_t* n_reads, const int32_t** gene, const uint32_t** overlap, const int32_t** dev_gene) {
  if (!c || !n_reads || !gene || !overlap) return LCR_E_ARG;
  if (c->stage < ST_LOADED || !c->genes_valid) { c->err = "lcr_get_read_genes before lcr_assign_genes (its result dies at lcr_load_batch / lcr_bind_batch)"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(c->ev_genes));
  HIPCHK(c, hipGetLastError());
  *n_reads = c->genes_nr;
  *gene = c->genes_nr ? c->h_gene.as<int32_t>() : nullptr;
  *overlap = c->genes_nr ? c->h_gene_ov.as<uint32_t>() : nullptr;
  if (dev_gene) *dev_gene = c->genes_nr ? c->d_gene.as<int32_t>() : nullptr;
  return LCR_OK;
}

int lcr_ase_genes(lcr_ctx* c, const lcr_ase_params* p, int32_t mem, int32_t n_sites, const int64_t* pos0, const uint8_t* pat, const uint8_t* mat) {
  if (!c) return LCR_E_ARG;
  if (!p || n_sites < 0 || (mem != LCR_MEM_HOST && mem != LCR_MEM_DEVICE)) {
    c->err = "lcr_ase_genes: null params, n_sites < 0 or mem not LCR_MEM_HOST / LCR_MEM_DEVICE";
    return LCR_E_ARG;
  }
  if (p->min_baseq > 30) { c->err = "lcr_ase_genes: min_baseq above 30 (the fragment matrix clamps qualities to 30)"; return LCR_E_ARG; }
  if (n_sites > 0 && (!pos0 || !pat || !mat)) { c->err = "lcr_ase_genes: null site array"; return LCR_E_ARG; }
  if (c->stage < ST_PHASED) { c->err = "lcr_ase_genes before lcr_phase"; return LCR_E_STATE; }
  if (!c->genes_valid) { c->err = "lcr_ase_genes before lcr_assign_genes on the bound batch"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }       // an asynchronous phase stage in flight writes the read records and the candidates
  { int rc = cand_settle(c); if (rc) return rc; }
  static_assert(sizeof(lcr_ase_gene) == 48, "lcr_ase_gene is 48 bytes");
  static_assert(offsetof(lcr_ase_gene, gene) == sizeof(lcr_ase_region), "lcr_ase_gene is lcr_ase_region's fields, then the gene");
  const BatchView& b = c->bv;
  const int ng = b.n_regions, n_rows = c->n_rows, n_cand = (int)c->h_cand.size();
  hipStream_t s = c->stream;
  // the parental sites: as in lcr_ase
  const int64_t* d_pos = nullptr; const uint8_t* d_pat = nullptr; const uint8_t* d_mat = nullptr;
  if (n_sites > 0) {
    { int rc = upload(c, c->ag_pos, pos0, (size_t)n_sites, &d_pos, mem); if (rc) return rc; }
    { int rc = upload(c, c->ag_pat, pat, (size_t)n_sites, &d_pat, mem); if (rc) return rc; }
    { int rc = upload(c, c->ag_mat, mat, (size_t)n_sites, &d_mat, mem); if (rc) return rc; }
    HIPCHK(c, c->h_agene_bad.reserve(64));
    int32_t* bad = c->h_agene_bad.as<int32_t>();
    *bad = 0;
    int32_t* d_bad = nullptr;
    HIPCHK(c, c->h_agene_bad.dev(&d_bad));
    launch_k7_check(d_pos, d_pat, d_mat, n_sites, d_bad, s);
    { int rc = stream_wait(c, c->agene.ev); if (rc) return rc; }
    if (*(volatile int32_t*)bad) {
      c->err = "lcr_ase_genes: parental sites must be sorted by position without duplicates, pat and mat one of ACGT each and different";
      return LCR_E_ARG;
    }
  }
  c->agene.valid = false;   // (from here on the last call's records are overwritten)
  const lcr_read_record* rec = c->phase.d_read_rec.as<lcr_read_record>();
  const int32_t* rro = c->row_region_off.as<int32_t>();
  const int32_t* gene = c->d_gene.as<int32_t>();
  HIPCHK(c, c->ag_cnt.reserve((size_t)std::max(ng, 1) * 4)); HIPCHK(c, c->ag_off.reserve(((size_t)ng + 1) * 4));
  HIPCHK(c, c->h_agene_off.reserve(((size_t)ng + 1) * 4)); HIPCHK(c, c->h_agene_ctl.reserve(64));
  int32_t* const h_ctl = c->h_agene_ctl.as<int32_t>();
  int32_t* const h_off = c->h_agene_off.as<int32_t>();
  int32_t *d_ctl = nullptr, *d_hoff = nullptr;
  HIPCHK(c, c->h_agene_ctl.dev(&d_ctl));
  HIPCHK(c, c->h_agene_off.dev(&d_hoff));
  h_ctl[0] = 0;
  if (ng == 0) { h_off[0] = 0; c->agene_n = 0; c->agene_ng = 0; c->agene.valid = true; HIPCHK(c, hipEventRecord(c->agene.ev, s)); return LCR_OK; }
  int32_t* pair_off = c->ag_off.as<int32_t>();
  Timer t(c, LCR_K_ASE_GENES);
  // 1. pairs per region, their offsets; the host sizes the records from their number (the call's one wait beside the sites' verdict)
  launch_k8_pair_count(b, rro, rec, gene, c->ag_cnt.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->ag_cnt.as<int32_t>(), pair_off, ng, pair_off + ng, s);
  launch_k8_pair_offsets(pair_off, ng, d_hoff, d_ctl, s);
  { int rc = stream_wait(c, c->agene.ev); if (rc) return rc; }
  const int32_t n_pairs = h_ctl[0];
  if (n_pairs > (1 << 28)) { c->err = "lcr_ase_genes: more than 2^28 (region, gene) pairs in one batch; split it"; return LCR_E_ARG; }
  // 2. the records: to HBM and, by the call's last kernel, to pinned host memory
  HIPCHK(c, c->d_agene.reserve((size_t)std::max(n_pairs, 1) * sizeof(lcr_ase_gene)));
  HIPCHK(c, c->h_agene.reserve((size_t)std::max(n_pairs, 1) * sizeof(lcr_ase_gene)));
  lcr_ase_gene* d_hrec = nullptr;
  HIPCHK(c, c->h_agene.dev(&d_hrec));
  lcr_ase_gene* d_rec = c->d_agene.as<lcr_ase_gene>();
  if (n_pairs > 0) {
    if (n_sites == 0) {
      launch_k8_pair_emit(b, rro, rec, gene, pair_off, d_rec, d_hrec, nullptr, s);
    } else {
      HIPCHK(c, c->ag_tag.reserve((size_t)std::max(n_rows, 1) * 4));
      HIPCHK(c, c->ag_site.reserve((size_t)std::max(n_cand, 1)));
      HIPCHK(c, c->ag_site_ps.reserve((size_t)std::max(n_cand, 1) * 4));
      launch_k8_pair_emit(b, rro, rec, gene, pair_off, d_rec, nullptr, c->ag_tag.as<int32_t>(), s);
      launch_k8_sites(c->d_cand.as<lcr_candidate>(), n_cand, (double)p->min_phase_score, d_pos, d_pat, d_mat, n_sites, pair_off, d_rec,
                      c->ag_site.as<uint8_t>(), c->ag_site_ps.as<uint32_t>(), s);
      launch_k8_votes(c->ag_tag.as<int32_t>(), n_rows, c->row_ptr.as<int64_t>(), c->col.as<int32_t>(), c->val.as<uint8_t>(), c->ag_site.as<uint8_t>(),
                      c->ag_site_ps.as<uint32_t>(), p->min_baseq, d_rec, s);
      launch_k8_export(d_rec, n_pairs, d_hrec, s);
    }
  }
  c->agene_n = n_pairs; c->agene_ng = ng;
  return call_end(c, c->agene);     // lcr_get_ase_genes waits for its event
}

int lcr_get_ase_genes(lcr_ctx* c, lcr_ase_gene_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->agene.valid) {
    c->err = "lcr_get_ase_genes before lcr_ase_genes (its records die with the phase stage's results and with the gene assignment)";
    return LCR_E_STATE;
  }
  { int rc = call_wait(c, c->agene); if (rc) return rc; }
  out->n_regions = c->agene_ng; out->n_pairs = c->agene_n;
  out->rec = c->agene_n ? c->h_agene.as<lcr_ase_gene>() : nullptr;
  out->pair_region_off = c->h_agene_off.as<int32_t>();
  out->dev_rec = c->agene_n ? c->d_agene.as<lcr_ase_gene>() : nullptr;
  return LCR_OK;
}

}  // extern "C"

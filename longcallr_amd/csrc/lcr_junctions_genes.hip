// lcr_junctions_genes.hip — the host driver of K9 (k9_gene_junctions.hip): the haplotype x junction table per (region, gene) pair over the
// phased rows, and its getter.  Shaped like lcr_junctions: a call of its own behind lcr_phase and lcr_assign_genes that reads the bound
// batch, the fragment stage's row offsets, the phase stage's read records and the gene of every read, and writes buffers no other stage or
// getter reads (lcr_ctx: jg_*, d_jgene, h_jgene*).  The launch count does not depend on the numbers of regions, genes, reads or junctions;
// the host waits for the annotation's verdict and for two sets of sizes in pinned memory.
#include "lcr_ctx.h"

extern "C" {

int lcr_junctions_genes(lcr_ctx* c, const lcr_junction_params* p, int32_t mem, const lcr_gene_annotation* a) {
  if (!c) return LCR_E_ARG;
  if (!p || !a || (mem != LCR_MEM_HOST && mem != LCR_MEM_DEVICE) || a->n_genes < 0 || a->n_exons < 0) {
    c->err = "lcr_junctions_genes: null params or annotation, a negative size or mem not LCR_MEM_HOST / LCR_MEM_DEVICE";
    return LCR_E_ARG;
  }
  if (a->n_genes > 0 && (!a->span_start0 || !a->span_end0 || !a->exon_off || !a->exon_start0 || !a->exon_end0 || a->n_exons < a->n_genes)) {
    c->err = "lcr_junctions_genes: null annotation array, or fewer exons than genes";
    return LCR_E_ARG;
  }
  if (c->stage < ST_PHASED) { c->err = "lcr_junctions_genes before lcr_phase"; return LCR_E_STATE; }
  if (!c->genes_valid) { c->err = "lcr_junctions_genes before lcr_assign_genes on the bound batch"; return LCR_E_STATE; }
  if (a->n_genes != c->genes_n_genes) {
    c->err = "lcr_junctions_genes: the annotation has another number of genes than the one lcr_assign_genes was called with";
    return LCR_E_ARG;
  }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }       // an asynchronous phase stage in flight writes the read records
  static_assert(sizeof(lcr_junction_gene) == 56, "lcr_junction_gene is 56 bytes");
  static_assert(offsetof(lcr_junction_gene, gene) == sizeof(lcr_junction), "lcr_junction_gene is lcr_junction's fields, then the gene");
  const BatchView& b = c->bv;
  const int nr = b.n_reads, ng = b.n_regions, n_genes = a->n_genes;
  hipStream_t s = c->stream;
  // the annotation: copied (host) or read in place (device), then checked by lcr_assign_genes' kernel.  Nothing of the last call's result
  // is touched before the verdict: a refused call changes nothing (the jg_* copies of the last annotation are overwritten in front of it:
  // nothing reads them once that call's kernels have run, and the stream orders the uploads behind them).
  lcr_gene_annotation d{};
  d.n_genes = n_genes; d.n_exons = a->n_exons;
  if (n_genes > 0) {
    { int rc = upload(c, c->jg_span_s, a->span_start0, (size_t)n_genes, &d.span_start0, mem); if (rc) return rc; }
    { int rc = upload(c, c->jg_span_e, a->span_end0, (size_t)n_genes, &d.span_end0, mem); if (rc) return rc; }
    { int rc = upload(c, c->jg_exon_off, a->exon_off, (size_t)n_genes + 1, &d.exon_off, mem); if (rc) return rc; }
    { int rc = upload(c, c->jg_exon_s, a->exon_start0, (size_t)a->n_exons, &d.exon_start0, mem); if (rc) return rc; }
    { int rc = upload(c, c->jg_exon_e, a->exon_end0, (size_t)a->n_exons, &d.exon_end0, mem); if (rc) return rc; }
    HIPCHK(c, c->h_jgene_bad.reserve(64));
    int32_t* bad = c->h_jgene_bad.as<int32_t>();
    *bad = 0;
    int32_t* d_bad = nullptr;
    HIPCHK(c, c->h_jgene_bad.dev(&d_bad));
    launch_k8_check(d, d_bad, s);
    HIPCHK(c, hipEventRecord(c->ev_jgene, s));
    HIPCHK(c, hipEventSynchronize(c->ev_jgene));
    HIPCHK(c, hipGetLastError());
    if (*(volatile int32_t*)bad) {
      c->err = "lcr_junctions_genes: genes must be sorted by (span_start0, span_end0), every gene needs exons that are ascending and disjoint, "
               "the first one starting at its span_start0 and the last one ending at its span_end0, and exon_off must run from 0 to n_exons";
      return LCR_E_ARG;
    }
  }
  c->jgene_valid = false;   // (from here on the last call's table is overwritten)
  c->jgene_timed = false;
  HIPCHK(c, c->h_jgene_ctl.reserve(64));
  HIPCHK(c, c->h_jgene_off.reserve((size_t)(ng + 1) * 4));
  HIPCHK(c, c->h_jgene.reserve(sizeof(lcr_junction_gene)));
  int32_t* const h_ctl = c->h_jgene_ctl.as<int32_t>();
  int32_t* const h_off = c->h_jgene_off.as<int32_t>();
  int32_t *d_ctl = nullptr, *d_hoff = nullptr;
  HIPCHK(c, c->h_jgene_ctl.dev(&d_ctl));
  HIPCHK(c, c->h_jgene_off.dev(&d_hoff));
  HIPCHK(c, hipStreamSynchronize(s));   // (an earlier call's last kernels write the pinned blocks that are reused from here on)
  h_ctl[0] = h_ctl[1] = h_ctl[2] = h_ctl[3] = 0;
  const auto finish_empty = [&]() {   // no participating row, no occurrence or no kept junction
    for (int g = 0; g <= ng; g++) h_off[g] = 0;
    c->jgene_n = 0; c->jgene_ng = ng; c->jgene_valid = true;
    return LCR_OK;
  };
  if (nr == 0 || ng == 0 || c->n_rows == 0 || n_genes == 0) return finish_empty();
  struct Bracket {   // HIP events around the call's kernels when timing is on: not a slot of lcr_kernel_ms (include/lcr.h)
    lcr_ctx* c;
    explicit Bracket(lcr_ctx* c_) : c(c_) { if (c->timing) (void)hipEventRecord(c->ev_jgene_t[0], c->stream); }
    ~Bracket() { if (c->timing) { (void)hipEventRecord(c->ev_jgene_t[1], c->stream); c->jgene_timed = true; } }
  } t(c);
  const lcr_read_record* rec = c->phase.d_read_rec.as<lcr_read_record>();
  const int32_t* rro = c->row_region_off.as<int32_t>();
  const int32_t* gene = c->d_gene.as<int32_t>();
  // 1. junctions per read, participating reads; the pairs of every region, every read's pair and row slot; the pairs' table segments
  const size_t n4 = (size_t)nr * 4, n14 = ((size_t)nr + 1) * 4;
  HIPCHK(c, c->jg_part.reserve(n4)); HIPCHK(c, c->jg_nocc.reserve(n4));
  HIPCHK(c, c->jg_part_off.reserve(n14)); HIPCHK(c, c->jg_occ_off.reserve(n14));
  HIPCHK(c, c->jg_cnt.reserve((size_t)ng * 4)); HIPCHK(c, c->jg_pair_off.reserve(((size_t)ng + 1) * 4)); HIPCHK(c, c->jg_off.reserve(((size_t)ng + 1) * 4));
  HIPCHK(c, c->jg_read_pair.reserve(n4)); HIPCHK(c, c->jg_row_slot.reserve(n4));
  HIPCHK(c, c->jg_pregion.reserve(n4)); HIPCHK(c, c->jg_pgene.reserve(n4)); HIPCHK(c, c->jg_prow0.reserve(n4)); HIPCHK(c, c->jg_prows.reserve(n4));
  HIPCHK(c, c->jg_pocc.reserve(n4)); HIPCHK(c, c->jg_tsz.reserve(n4)); HIPCHK(c, c->jg_tbl_off.reserve(n14));
  int32_t* part = c->jg_part.as<int32_t>();
  int32_t* nocc = c->jg_nocc.as<int32_t>();
  int32_t* part_off = c->jg_part_off.as<int32_t>();
  int32_t* occ_off = c->jg_occ_off.as<int32_t>();
  int32_t* pair_off = c->jg_pair_off.as<int32_t>();
  int32_t* tbl_off = c->jg_tbl_off.as<int32_t>();
  const K9Pairs pr{c->jg_read_pair.as<int32_t>(), c->jg_row_slot.as<int32_t>(), c->jg_pregion.as<int32_t>(), c->jg_pgene.as<int32_t>(),
                   c->jg_prow0.as<int32_t>(), c->jg_prows.as<int32_t>(), c->jg_pocc.as<int32_t>()};
  launch_k9_count(b, rro, rec, gene, p->min_junctions, part, nocc, s);
  launch_scan_i32(c->scan_tmp, part, part_off, nr, part_off + nr, s);
  launch_scan_i32(c->scan_tmp, nocc, occ_off, nr, occ_off + nr, s);
  launch_k9_pair_count(b, gene, part, c->jg_cnt.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->jg_cnt.as<int32_t>(), pair_off, ng, pair_off + ng, s);
  launch_k9_pair_emit(b, gene, part, nocc, pair_off, part_off, pr, s);
  launch_k9_sizes(b, pair_off, part_off, occ_off, pr.occ, c->jg_tsz.as<int32_t>(), d_ctl, s);
  launch_scan_i32(c->scan_tmp, c->jg_tsz.as<int32_t>(), tbl_off, nr, tbl_off + nr, s);
  HIPCHK(c, hipEventRecord(c->ev_jgene, s));
  HIPCHK(c, hipEventSynchronize(c->ev_jgene));   // the host sizes the row records, the keys and the table from the two totals
  HIPCHK(c, hipGetLastError());
  const int32_t n_part = h_ctl[0], n_occ = h_ctl[1];
  if (n_part <= 0 || n_occ <= 0) return finish_empty();
  if (n_occ > (1 << 28)) { c->err = "lcr_junctions_genes: more than 2^28 junction occurrences in one batch; split it"; return LCR_E_ARG; }
  // 2. row records, keys, the pairs' table segments.  A segment has fewer than 4 x its occurrences in slots, so 4 x all occurrences bounds
  // the table without a third wait; the slots behind the last segment stay empty.
  const int32_t n_slots = 4 * n_occ;
  HIPCHK(c, c->jg_rows.reserve((size_t)n_part * launch_k9_row_bytes()));
  HIPCHK(c, c->jg_keys.reserve((size_t)n_occ * 8));
  HIPCHK(c, c->jg_tbl_key.reserve((size_t)n_slots * 8)); HIPCHK(c, c->jg_tbl_cnt.reserve((size_t)n_slots * 4));
  HIPCHK(c, c->jg_flag.reserve((size_t)n_slots * 4)); HIPCHK(c, c->jg_koff.reserve(((size_t)n_slots + 1) * 4));
  HIPCHK(c, lcr_fill_async(c->jg_tbl_key.p, 0xff, (size_t)n_slots * 8, s));
  HIPCHK(c, lcr_fill_async(c->jg_tbl_cnt.p, 0, (size_t)n_slots * 4, s));
  launch_k9_emit(b, rro, rec, gene, part, occ_off, pr, tbl_off, d, c->jg_rows.p, c->jg_keys.as<uint64_t>(), c->jg_tbl_key.as<uint64_t>(),
                 c->jg_tbl_cnt.as<uint32_t>(), s);
  // 3. kept junctions and their number per region (the flag is K6's: occupied && n_reads >= min_count)
  int32_t* koff = c->jg_koff.as<int32_t>();
  launch_k6_flag(c->jg_tbl_key.as<uint64_t>(), c->jg_tbl_cnt.as<uint32_t>(), n_slots, p->min_count, c->jg_flag.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->jg_flag.as<int32_t>(), koff, n_slots, koff + n_slots, s);
  launch_k9_offsets(pair_off, tbl_off, koff, ng, n_slots, c->jg_off.as<int32_t>(), d_hoff, d_ctl, s);
  HIPCHK(c, hipEventRecord(c->ev_jgene, s));
  HIPCHK(c, hipEventSynchronize(c->ev_jgene));   // the number of kept junctions sizes the records and the last kernels' grids
  HIPCHK(c, hipGetLastError());
  const int32_t n_kept = h_ctl[2];
  if (n_kept <= 0) return finish_empty();
  // 4. order, motif, tables: the records go to HBM and, by the last kernel, to pinned host memory
  HIPCHK(c, c->jg_ck.reserve((size_t)n_kept * 8)); HIPCHK(c, c->jg_cc.reserve((size_t)n_kept * 4)); HIPCHK(c, c->jg_cp.reserve((size_t)n_kept * 4));
  HIPCHK(c, c->jg_jpair.reserve((size_t)n_kept * 4));
  HIPCHK(c, c->d_jgene.reserve((size_t)n_kept * sizeof(lcr_junction_gene)));
  HIPCHK(c, c->h_jgene.reserve((size_t)n_kept * sizeof(lcr_junction_gene)));
  lcr_junction_gene* d_hjunc = nullptr;
  HIPCHK(c, c->h_jgene.dev(&d_hjunc));
  launch_k9_place(b, c->jg_tbl_key.as<uint64_t>(), c->jg_tbl_cnt.as<uint32_t>(), c->jg_flag.as<int32_t>(), koff, tbl_off, pair_off, pr, n_slots, n_kept,
                  c->jg_ck.as<uint64_t>(), c->jg_cc.as<uint32_t>(), c->jg_cp.as<int32_t>(), c->d_jgene.as<lcr_junction_gene>(), c->jg_jpair.as<int32_t>(), s);
  launch_k9_tables(c->jg_jpair.as<int32_t>(), pr, c->jg_rows.p, c->jg_keys.as<uint64_t>(), n_kept, c->d_jgene.as<lcr_junction_gene>(), d_hjunc, s);
  HIPCHK(c, hipEventRecord(c->ev_jgene, s));     // lcr_get_junctions_genes waits for it
  HIPCHK(c, hipGetLastError());
  c->jgene_n = n_kept; c->jgene_ng = ng; c->jgene_valid = true;
  return LCR_OK;
}

int lcr_get_junctions_genes(lcr_ctx* c, lcr_junction_gene_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->jgene_valid) {
    c->err = "lcr_get_junctions_genes before lcr_junctions_genes (its table dies with the phase stage's results and with the gene assignment)";
    return LCR_E_STATE;
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(c->ev_jgene));
  HIPCHK(c, hipGetLastError());
  out->n_regions = c->jgene_ng; out->n_junctions = c->jgene_n;
  out->junc = c->jgene_n ? c->h_jgene.as<lcr_junction_gene>() : nullptr;
  out->junc_region_off = c->h_jgene_off.as<int32_t>();
  out->dev_junc = c->jgene_n ? c->d_jgene.as<lcr_junction_gene>() : nullptr;
  out->kernel_ms = -1.f;
  if (c->timing && c->jgene_timed) {
    HIPCHK(c, hipEventSynchronize(c->ev_jgene_t[1]));
    HIPCHK(c, hipEventElapsedTime(&out->kernel_ms, c->ev_jgene_t[0], c->ev_jgene_t[1]));
  }
  return LCR_OK;
}

}  // extern "C"

// lcr_asj_genes.hip — the host driver of K10 (k10_asj_modes.hip): lcr_junctions_genes' table with the script's other three modes -- interior
// exon blocks for clustering, the DNA-VCF filter, the per-gene read coverage -- and its getter.  The junction table is a GeneJunctions of
// the call's own (c->ajgene), filled by the gj_* steps of lcr_junctions_genes.hip, so lcr_junctions_genes' results on the same context
// are never touched; what the modes add lives in c->asj (AsjModes), and K10's kernels are queued between the steps.  The exon table is a
// SlotTable like the junctions' and goes through the same gj_keep.  The launch count does not depend on any size; the host waits are
// K9's: one verdict (annotation and DNA sites together) and two sets of sizes.
#include "lcr_ctx.h"
#include "lcr_asj_args.h"

extern "C" {

int lcr_asj_genes(lcr_ctx* c, const lcr_asj_params* p, int32_t mem, const lcr_gene_annotation* a) {
  if (!c) return LCR_E_ARG;
  if (const char* msg = lcr_asj_check_args(p, mem, a)) { c->err = msg; return LCR_E_ARG; }
  if (c->stage < ST_PHASED) { c->err = "lcr_asj_genes before lcr_phase"; return LCR_E_STATE; }
  if (!c->genes_valid) { c->err = "lcr_asj_genes before lcr_assign_genes on the bound batch"; return LCR_E_STATE; }
  if (a->n_genes != c->genes_n_genes) {
    c->err = "lcr_asj_genes: the annotation has another number of genes than the one lcr_assign_genes was called with";
    return LCR_E_ARG;
  }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }       // an asynchronous phase stage in flight writes the read records and the candidates
  { int rc = cand_settle(c); if (rc) return rc; }
  static_assert(sizeof(lcr_exon_gene) == 24, "lcr_exon_gene is 24 bytes");
  static_assert(sizeof(lcr_asj_params) == 32, "lcr_asj_params is 32 bytes");
  const bool want_exons = p->flags & LCR_ASJ_EXONS, want_dna = p->flags & LCR_ASJ_DNA_FILTER, want_cov = p->flags & LCR_ASJ_COVERAGE;
  GeneJunctions& g = c->ajgene;
  AsjModes& m = c->asj;
  const BatchView& b = c->bv;
  const int nr = b.n_reads, ng = b.n_regions, n_genes = a->n_genes, n_cand = (int)c->h_cand.size();
  const int32_t n_dna = want_dna ? p->n_dna : 0;
  hipStream_t s = c->stream;
  // the DNA sites and the annotation: copied (host) or read in place (device), then checked.  Nothing of the last call's result is touched
  // before the verdict: a refused call changes nothing (the copies are overwritten in front of it: nothing reads them once that call's
  // kernels have run, and the stream orders the uploads behind them).
  const int64_t* d_dna = nullptr;
  if (n_dna > 0) { int rc = upload(c, m.dna, p->dna_pos0, (size_t)n_dna, &d_dna, mem); if (rc) return rc; }
  lcr_gene_annotation d{};
  int32_t* d_bad = nullptr;
  { int rc = annotation_queue(c, g.ann, a, mem, g.h_bad, &d, &d_bad); if (rc) return rc; }
  if (n_genes > 0 || n_dna > 0) {
    launch_k10_dna_check(d_dna, n_dna, d_bad + 1, s);
    { int rc = annotation_verdict(c, g.h_bad, g.st.ev, "lcr_asj_genes"); if (rc) return rc; }
    if (g.h_bad.as<volatile int32_t>()[1]) { c->err = "lcr_asj_genes: dna_pos0 must be ascending without duplicates"; return LCR_E_ARG; }
  }
  { int rc = gj_begin(c, g); if (rc) return rc; }   // (from here on the last call's tables are overwritten)
  HIPCHK(c, m.h_xoff.reserve((size_t)(ng + 1) * 4)); HIPCHK(c, m.h_exon.reserve(sizeof(lcr_exon_gene)));
  HIPCHK(c, m.h_cov.reserve((size_t)std::max(n_genes, 1) * 4));
  for (int k = 0; k < n_genes; k++) m.h_cov.as<int32_t>()[k] = 0;
  m.cov = want_cov; m.n_genes = n_genes;
  int32_t* const h_ctl = g.h_ctl.as<int32_t>();   // [0..3] K9's sizes, [4..7] the same for blocks / exons
  int32_t *const d_ctl = g.d_ctl, *d_hxoff = nullptr;
  HIPCHK(c, m.h_xoff.dev(&d_hxoff));
  const auto finish_empty = [&]() { no_records(g.h_off, ng, &g.n); no_records(m.h_xoff, ng, &m.nx); return gj_finish(c, g); };
  if (nr == 0 || ng == 0 || n_genes == 0) return finish_empty();   // (not at n_rows == 0: the coverage counts reads)
  Bracket t(c, g.st);
  // 1. K9's counts; beside them the interior blocks per participating read, their sums per pair and the exon table's segments, and the
  // coverage, which is complete here
  { int rc = gj_counts(c, g, p->min_junctions); if (rc) return rc; }
  const int32_t* gene = c->d_gene.as<int32_t>();
  const int32_t *part = g.part.as<int32_t>(), *pair_off = g.pair_off.as<int32_t>(), *part_off = g.part_off.as<int32_t>();
  const K9Pairs pr = g.pairs();
  const size_t n4 = (size_t)nr * 4, n14 = ((size_t)nr + 1) * 4;
  int32_t *nblk = nullptr, *xtbl_off = nullptr;
  if (want_exons) {
    HIPCHK(c, m.nblk.reserve(n4)); HIPCHK(c, m.blk_off.reserve(n14)); HIPCHK(c, m.pblk.reserve(n4));
    HIPCHK(c, m.xtsz.reserve(n4)); HIPCHK(c, m.xtbl_off.reserve(n14)); HIPCHK(c, m.x.off.reserve(((size_t)ng + 1) * 4));
    nblk = m.nblk.as<int32_t>(); xtbl_off = m.xtbl_off.as<int32_t>();
    HIPCHK(c, lcr_fill_async(m.pblk.p, 0, n4, s));
  }
  int32_t* cov = nullptr;
  if (want_cov) {
    HIPCHK(c, m.cov_n.reserve((size_t)n_genes * 4));
    cov = m.cov_n.as<int32_t>();
    HIPCHK(c, lcr_fill_async(cov, 0, (size_t)n_genes * 4, s));
  }
  launch_k10_count(b, gene, part, p->min_junctions, nblk, cov, s);
  if (want_cov) HIPCHK(c, hipMemcpyAsync(m.h_cov.p, cov, (size_t)n_genes * 4, hipMemcpyDeviceToHost, s));
  if (want_exons) {
    int32_t* blk_off = m.blk_off.as<int32_t>();
    launch_scan_i32(c->scan_tmp, nblk, blk_off, nr, blk_off + nr, s);
    launch_k10_pair_blocks(b, part, nblk, pr.read_pair, m.pblk.as<int32_t>(), s);
    launch_k9_sizes(b, pair_off, part_off, blk_off, m.pblk.as<int32_t>(), m.xtsz.as<int32_t>(), d_ctl + 4, s);   // ([5] interior blocks)
    launch_scan_i32(c->scan_tmp, m.xtsz.as<int32_t>(), xtbl_off, nr, xtbl_off + nr, s);
  }
  bool empty = false;
  { int rc = gj_wait_counts(c, g, "lcr_asj_genes", &empty); if (rc) return rc; }   // ... and the exon table from the blocks and the pairs
  if (empty) return finish_empty();
  const int32_t n_pairs = h_ctl[3], n_blk = want_exons ? h_ctl[5] : 0;
  if (n_blk > (1 << 27)) { c->err = "lcr_asj_genes: more than 2^27 interior blocks in one batch; split it"; return LCR_E_ARG; }
  // 2. K9's rows; behind the walk that writes them the DNA filter clears the counted bit of unsupported rows; K9's kept slots
  { int rc = gj_rows(c, g, d); if (rc) return rc; }
  if (want_dna) {
    HIPCHK(c, m.sup.reserve((size_t)std::max(n_cand, 1) * 4)); HIPCHK(c, m.sup_uniq.reserve((size_t)std::max(n_cand, 1) * 4));
    HIPCHK(c, m.sup_n.reserve((size_t)ng * 4));
    launch_k10_support(c->d_cand.as<lcr_candidate>(), n_cand, c->d_cand_off.as<int32_t>(), ng, (double)p->min_phase_score, d_dna, n_dna,
                       m.sup.as<uint32_t>(), m.sup_uniq.as<uint32_t>(), m.sup_n.as<int32_t>(), s);
    launch_k10_filter(b, part, pr.row_slot, c->d_cand_off.as<int32_t>(), m.sup_uniq.as<uint32_t>(), m.sup_n.as<int32_t>(), g.rows.p, s);
  }
  { int rc = gj_keep(c, g.t, pair_off, g.tbl_off.as<int32_t>(), p->min_count, g.d_off, d_ctl); if (rc) return rc; }
  // The exon table beside it: a segment has fewer than 4 x its blocks in slots, two when it has none, so 4 x all blocks + 2 x all pairs
  // bounds the table without another wait.  Its kept slots by K9's step ([6] kept exons).
  const int32_t n_xslots = n_blk > 0 ? 4 * n_blk + 2 * n_pairs : 0;
  if (n_xslots > 0) {
    { int rc = slot_table_clear(c, m.x, n_xslots); if (rc) return rc; }
    launch_k10_emit(b, part, nblk, pr.read_pair, xtbl_off, m.x.tbl_key.as<uint64_t>(), m.x.tbl_cnt.as<uint32_t>(), s);
    { int rc = gj_keep(c, m.x, pair_off, xtbl_off, p->min_count, d_hxoff, d_ctl + 4); if (rc) return rc; }
  }
  { int rc = stream_wait(c, g.st.ev); if (rc) return rc; }   // the numbers of kept junctions and exons size the records and the last kernels' grids
  const int32_t n_kept = h_ctl[2], n_xkept = n_xslots > 0 ? h_ctl[6] : 0;
  // 3. K9's tables; the exon records
  if (n_kept <= 0) no_records(g.h_off, ng, &g.n);
  else { int rc = gj_tables(c, g, n_kept); if (rc) return rc; }
  if (n_xkept <= 0) no_records(m.h_xoff, ng, &m.nx);
  else {
    SlotTable& x = m.x;
    HIPCHK(c, x.ck.reserve((size_t)n_xkept * 8)); HIPCHK(c, x.cc.reserve((size_t)n_xkept * 4)); HIPCHK(c, x.cp.reserve((size_t)n_xkept * 4));
    HIPCHK(c, m.d_exon.reserve((size_t)n_xkept * sizeof(lcr_exon_gene)));
    HIPCHK(c, m.h_exon.reserve((size_t)n_xkept * sizeof(lcr_exon_gene)));
    lcr_exon_gene* d_hexon = nullptr;
    HIPCHK(c, m.h_exon.dev(&d_hexon));
    launch_k10_place(x.tbl_key.as<uint64_t>(), x.tbl_cnt.as<uint32_t>(), x.flag.as<int32_t>(), x.koff.as<int32_t>(), xtbl_off, pair_off, pr, ng, n_xslots,
                     n_xkept, x.ck.as<uint64_t>(), x.cc.as<uint32_t>(), x.cp.as<int32_t>(), m.d_exon.as<lcr_exon_gene>(), d_hexon, s);
    m.nx = n_xkept;
  }
  return gj_finish(c, g);
}

int lcr_get_asj_genes(lcr_ctx* c, lcr_asj_gene_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->ajgene.st.valid) {
    c->err = "lcr_get_asj_genes before lcr_asj_genes (its tables die with the phase stage's results and with the gene assignment)";
    return LCR_E_STATE;
  }
  const AsjModes& m = c->asj;
  out->n_exons = m.nx; out->n_genes = m.n_genes;
  out->exon = m.nx ? m.h_exon.as<lcr_exon_gene>() : nullptr;
  out->exon_region_off = m.h_xoff.as<int32_t>();
  out->dev_exon = m.nx ? m.d_exon.as<lcr_exon_gene>() : nullptr;
  out->gene_reads = m.cov ? m.h_cov.as<int32_t>() : nullptr;
  return gj_get(c, c->ajgene, out);
}

}  // extern "C"

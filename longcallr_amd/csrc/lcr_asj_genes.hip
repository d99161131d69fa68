// lcr_asj_genes.hip — the host driver of K10 (k10_asj_modes.hip): lcr_junctions_genes' table with the script's other three modes -- interior
// exon blocks for clustering, the DNA-VCF filter, the per-gene read coverage -- and its getter.  K9's launch sequence on buffers of K10's
// own (lcr_ctx: aj_*, d_ajgene, d_ajexon, h_aj*), with K10's kernels queued between its steps, so lcr_junctions_genes' results on the same
// context are never touched.  The launch count does not depend on any size; the host waits are K9's: one verdict (annotation and DNA
// sites together) and two sets of sizes.
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
  const BatchView& b = c->bv;
  const int nr = b.n_reads, ng = b.n_regions, n_genes = a->n_genes, n_cand = (int)c->h_cand.size();
  const int32_t n_dna = want_dna ? p->n_dna : 0;
  hipStream_t s = c->stream;
  // the annotation and the DNA sites: copied (host) or read in place (device), then checked.  Nothing of the last call's result is touched
  // before the verdict: a refused call changes nothing (the copies are overwritten in front of it: nothing reads them once that call's
  // kernels have run, and the stream orders the uploads behind them).
  lcr_gene_annotation d{};
  d.n_genes = n_genes; d.n_exons = a->n_exons;
  const int64_t* d_dna = nullptr;
  if (n_genes > 0) {
    { int rc = upload(c, c->aj_span_s, a->span_start0, (size_t)n_genes, &d.span_start0, mem); if (rc) return rc; }
    { int rc = upload(c, c->aj_span_e, a->span_end0, (size_t)n_genes, &d.span_end0, mem); if (rc) return rc; }
    { int rc = upload(c, c->aj_exon_off, a->exon_off, (size_t)n_genes + 1, &d.exon_off, mem); if (rc) return rc; }
    { int rc = upload(c, c->aj_exon_s, a->exon_start0, (size_t)a->n_exons, &d.exon_start0, mem); if (rc) return rc; }
    { int rc = upload(c, c->aj_exon_e, a->exon_end0, (size_t)a->n_exons, &d.exon_end0, mem); if (rc) return rc; }
  }
  if (n_dna > 0) { int rc = upload(c, c->aj_dna, p->dna_pos0, (size_t)n_dna, &d_dna, mem); if (rc) return rc; }
  if (n_genes > 0 || n_dna > 0) {
    HIPCHK(c, c->h_ajgene_bad.reserve(64));
    int32_t* bad = c->h_ajgene_bad.as<int32_t>();
    bad[0] = bad[1] = 0;
    int32_t* d_bad = nullptr;
    HIPCHK(c, c->h_ajgene_bad.dev(&d_bad));
    if (n_genes > 0) launch_k8_check(d, d_bad, s);
    launch_k10_dna_check(d_dna, n_dna, d_bad + 1, s);
    HIPCHK(c, hipEventRecord(c->ev_ajgene, s));
    HIPCHK(c, hipEventSynchronize(c->ev_ajgene));
    HIPCHK(c, hipGetLastError());
    if (((volatile int32_t*)bad)[0]) {
      c->err = "lcr_asj_genes: genes must be sorted by (span_start0, span_end0), every gene needs exons that are ascending and disjoint, "
               "the first one starting at its span_start0 and the last one ending at its span_end0, and exon_off must run from 0 to n_exons";
      return LCR_E_ARG;
    }
    if (((volatile int32_t*)bad)[1]) { c->err = "lcr_asj_genes: dna_pos0 must be ascending without duplicates"; return LCR_E_ARG; }
  }
  c->ajgene_valid = false;   // (from here on the last call's tables are overwritten)
  c->ajgene_timed = false;
  HIPCHK(c, c->h_ajgene_ctl.reserve(64));
  HIPCHK(c, c->h_ajgene_off.reserve((size_t)(ng + 1) * 4)); HIPCHK(c, c->h_ajexon_off.reserve((size_t)(ng + 1) * 4));
  HIPCHK(c, c->h_ajgene.reserve(sizeof(lcr_junction_gene))); HIPCHK(c, c->h_ajexon.reserve(sizeof(lcr_exon_gene)));
  HIPCHK(c, c->h_ajcov.reserve((size_t)std::max(n_genes, 1) * 4));
  int32_t* const h_ctl = c->h_ajgene_ctl.as<int32_t>();
  int32_t* const h_off = c->h_ajgene_off.as<int32_t>();
  int32_t* const h_xoff = c->h_ajexon_off.as<int32_t>();
  int32_t *d_ctl = nullptr, *d_hoff = nullptr, *d_hxoff = nullptr;
  HIPCHK(c, c->h_ajgene_ctl.dev(&d_ctl));
  HIPCHK(c, c->h_ajgene_off.dev(&d_hoff));
  HIPCHK(c, c->h_ajexon_off.dev(&d_hxoff));
  HIPCHK(c, hipStreamSynchronize(s));   // (an earlier call's last kernels write the pinned blocks that are reused from here on)
  for (int i = 0; i < 8; i++) h_ctl[i] = 0;
  for (int k = 0; k < n_genes; k++) c->h_ajcov.as<int32_t>()[k] = 0;
  c->ajgene_cov = want_cov; c->ajgene_n_genes = n_genes;
  const auto no_junctions = [&]() { for (int g = 0; g <= ng; g++) h_off[g] = 0; c->ajgene_n = 0; };
  const auto no_exons = [&]() { for (int g = 0; g <= ng; g++) h_xoff[g] = 0; c->ajgene_nx = 0; };
  const auto finish = [&]() -> int {
    HIPCHK(c, hipEventRecord(c->ev_ajgene, s));     // lcr_get_asj_genes waits for it
    HIPCHK(c, hipGetLastError());
    c->ajgene_ng = ng; c->ajgene_valid = true;
    return (int)LCR_OK;
  };
  if (nr == 0 || ng == 0 || n_genes == 0) { no_junctions(); no_exons(); return finish(); }
  struct Bracket {   // HIP events around the call's kernels when timing is on: not a slot of lcr_kernel_ms (include/lcr.h)
    lcr_ctx* c;
    explicit Bracket(lcr_ctx* c_) : c(c_) { if (c->timing) (void)hipEventRecord(c->ev_ajgene_t[0], c->stream); }
    ~Bracket() { if (c->timing) { (void)hipEventRecord(c->ev_ajgene_t[1], c->stream); c->ajgene_timed = true; } }
  } t(c);
  const lcr_read_record* rec = c->phase.d_read_rec.as<lcr_read_record>();
  const int32_t* rro = c->row_region_off.as<int32_t>();
  const int32_t* gene = c->d_gene.as<int32_t>();
  // 1. K9's first step; beside it the interior blocks per participating read, their sums per pair and the exon table's segments, and the
  // coverage, which is complete here
  const size_t n4 = (size_t)nr * 4, n14 = ((size_t)nr + 1) * 4;
  HIPCHK(c, c->aj_part.reserve(n4)); HIPCHK(c, c->aj_nocc.reserve(n4));
  HIPCHK(c, c->aj_part_off.reserve(n14)); HIPCHK(c, c->aj_occ_off.reserve(n14));
  HIPCHK(c, c->aj_cnt.reserve((size_t)ng * 4)); HIPCHK(c, c->aj_pair_off.reserve(((size_t)ng + 1) * 4)); HIPCHK(c, c->aj_off.reserve(((size_t)ng + 1) * 4));
  HIPCHK(c, c->aj_read_pair.reserve(n4)); HIPCHK(c, c->aj_row_slot.reserve(n4));
  HIPCHK(c, c->aj_pregion.reserve(n4)); HIPCHK(c, c->aj_pgene.reserve(n4)); HIPCHK(c, c->aj_prow0.reserve(n4)); HIPCHK(c, c->aj_prows.reserve(n4));
  HIPCHK(c, c->aj_pocc.reserve(n4)); HIPCHK(c, c->aj_tsz.reserve(n4)); HIPCHK(c, c->aj_tbl_off.reserve(n14));
  int32_t* part = c->aj_part.as<int32_t>();
  int32_t* nocc = c->aj_nocc.as<int32_t>();
  int32_t* part_off = c->aj_part_off.as<int32_t>();
  int32_t* occ_off = c->aj_occ_off.as<int32_t>();
  int32_t* pair_off = c->aj_pair_off.as<int32_t>();
  int32_t* tbl_off = c->aj_tbl_off.as<int32_t>();
  const K9Pairs pr{c->aj_read_pair.as<int32_t>(), c->aj_row_slot.as<int32_t>(), c->aj_pregion.as<int32_t>(), c->aj_pgene.as<int32_t>(),
                   c->aj_prow0.as<int32_t>(), c->aj_prows.as<int32_t>(), c->aj_pocc.as<int32_t>()};
  launch_k9_count(b, rro, rec, gene, p->min_junctions, part, nocc, s);
  launch_scan_i32(c->scan_tmp, part, part_off, nr, part_off + nr, s);
  launch_scan_i32(c->scan_tmp, nocc, occ_off, nr, occ_off + nr, s);
  launch_k9_pair_count(b, gene, part, c->aj_cnt.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->aj_cnt.as<int32_t>(), pair_off, ng, pair_off + ng, s);
  launch_k9_pair_emit(b, gene, part, nocc, pair_off, part_off, pr, s);
  launch_k9_sizes(b, pair_off, part_off, occ_off, pr.occ, c->aj_tsz.as<int32_t>(), d_ctl, s);
  launch_scan_i32(c->scan_tmp, c->aj_tsz.as<int32_t>(), tbl_off, nr, tbl_off + nr, s);
  int32_t *nblk = nullptr, *xtbl_off = nullptr;
  if (want_exons) {
    HIPCHK(c, c->aj_nblk.reserve(n4)); HIPCHK(c, c->aj_blk_off.reserve(n14)); HIPCHK(c, c->aj_pblk.reserve(n4));
    HIPCHK(c, c->aj_xtsz.reserve(n4)); HIPCHK(c, c->aj_xtbl_off.reserve(n14)); HIPCHK(c, c->aj_xoff.reserve(((size_t)ng + 1) * 4));
    nblk = c->aj_nblk.as<int32_t>(); xtbl_off = c->aj_xtbl_off.as<int32_t>();
    HIPCHK(c, lcr_fill_async(c->aj_pblk.p, 0, n4, s));
  }
  int32_t* cov = nullptr;
  if (want_cov) {
    HIPCHK(c, c->aj_cov.reserve((size_t)n_genes * 4));
    cov = c->aj_cov.as<int32_t>();
    HIPCHK(c, lcr_fill_async(c->aj_cov.p, 0, (size_t)n_genes * 4, s));
  }
  launch_k10_count(b, gene, part, p->min_junctions, nblk, cov, s);
  if (want_cov) HIPCHK(c, hipMemcpyAsync(c->h_ajcov.p, c->aj_cov.p, (size_t)n_genes * 4, hipMemcpyDeviceToHost, s));
  if (want_exons) {
    int32_t* blk_off = c->aj_blk_off.as<int32_t>();
    launch_scan_i32(c->scan_tmp, nblk, blk_off, nr, blk_off + nr, s);
    launch_k10_pair_blocks(b, part, nblk, pr.read_pair, c->aj_pblk.as<int32_t>(), s);
    launch_k9_sizes(b, pair_off, part_off, blk_off, c->aj_pblk.as<int32_t>(), c->aj_xtsz.as<int32_t>(), d_ctl + 4, s);   // ([5] interior blocks)
    launch_scan_i32(c->scan_tmp, c->aj_xtsz.as<int32_t>(), xtbl_off, nr, xtbl_off + nr, s);
  }
  HIPCHK(c, hipEventRecord(c->ev_ajgene, s));
  HIPCHK(c, hipEventSynchronize(c->ev_ajgene));   // the host sizes the row records, the keys and the two tables from the totals
  HIPCHK(c, hipGetLastError());
  const int32_t n_part = h_ctl[0], n_occ = h_ctl[1], n_pairs = h_ctl[3], n_blk = want_exons ? h_ctl[5] : 0;
  if (n_part <= 0 || n_occ <= 0) { no_junctions(); no_exons(); return finish(); }
  if (n_occ > (1 << 28)) { c->err = "lcr_asj_genes: more than 2^28 junction occurrences in one batch; split it"; return LCR_E_ARG; }
  if (n_blk > (1 << 27)) { c->err = "lcr_asj_genes: more than 2^27 interior blocks in one batch; split it"; return LCR_E_ARG; }
  // 2. K9's second and third steps: row records, keys, the junction table, its kept slots.  The DNA filter clears the counted bit of
  // unsupported rows behind the walk that writes the rows.  The exon table beside it: a segment has fewer than 4 x its blocks in slots,
  // two when it has none, so 4 x all blocks + 2 x all pairs bounds the table without another wait.
  const int32_t n_slots = 4 * n_occ;
  HIPCHK(c, c->aj_rows.reserve((size_t)n_part * launch_k9_row_bytes()));
  HIPCHK(c, c->aj_keys.reserve((size_t)n_occ * 8));
  HIPCHK(c, c->aj_tbl_key.reserve((size_t)n_slots * 8)); HIPCHK(c, c->aj_tbl_cnt.reserve((size_t)n_slots * 4));
  HIPCHK(c, c->aj_flag.reserve((size_t)n_slots * 4)); HIPCHK(c, c->aj_koff.reserve(((size_t)n_slots + 1) * 4));
  HIPCHK(c, lcr_fill_async(c->aj_tbl_key.p, 0xff, (size_t)n_slots * 8, s));
  HIPCHK(c, lcr_fill_async(c->aj_tbl_cnt.p, 0, (size_t)n_slots * 4, s));
  launch_k9_emit(b, rro, rec, gene, part, occ_off, pr, tbl_off, d, c->aj_rows.p, c->aj_keys.as<uint64_t>(), c->aj_tbl_key.as<uint64_t>(),
                 c->aj_tbl_cnt.as<uint32_t>(), s);
  if (want_dna) {
    HIPCHK(c, c->aj_sup.reserve((size_t)std::max(n_cand, 1) * 4)); HIPCHK(c, c->aj_sup_uniq.reserve((size_t)std::max(n_cand, 1) * 4));
    HIPCHK(c, c->aj_sup_n.reserve((size_t)ng * 4));
    launch_k10_support(c->d_cand.as<lcr_candidate>(), n_cand, c->d_cand_off.as<int32_t>(), ng, (double)p->min_phase_score, d_dna, n_dna,
                       c->aj_sup.as<uint32_t>(), c->aj_sup_uniq.as<uint32_t>(), c->aj_sup_n.as<int32_t>(), s);
    launch_k10_filter(b, part, pr.row_slot, c->d_cand_off.as<int32_t>(), c->aj_sup_uniq.as<uint32_t>(), c->aj_sup_n.as<int32_t>(), c->aj_rows.p, s);
  }
  int32_t* koff = c->aj_koff.as<int32_t>();
  launch_k6_flag(c->aj_tbl_key.as<uint64_t>(), c->aj_tbl_cnt.as<uint32_t>(), n_slots, p->min_count, c->aj_flag.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, c->aj_flag.as<int32_t>(), koff, n_slots, koff + n_slots, s);
  launch_k9_offsets(pair_off, tbl_off, koff, ng, n_slots, c->aj_off.as<int32_t>(), d_hoff, d_ctl, s);
  const int32_t n_xslots = n_blk > 0 ? 4 * n_blk + 2 * n_pairs : 0;
  int32_t* xkoff = nullptr;
  if (n_xslots > 0) {
    HIPCHK(c, c->aj_xtbl_key.reserve((size_t)n_xslots * 8)); HIPCHK(c, c->aj_xtbl_cnt.reserve((size_t)n_xslots * 4));
    HIPCHK(c, c->aj_xflag.reserve((size_t)n_xslots * 4)); HIPCHK(c, c->aj_xkoff.reserve(((size_t)n_xslots + 1) * 4));
    HIPCHK(c, lcr_fill_async(c->aj_xtbl_key.p, 0xff, (size_t)n_xslots * 8, s));
    HIPCHK(c, lcr_fill_async(c->aj_xtbl_cnt.p, 0, (size_t)n_xslots * 4, s));
    launch_k10_emit(b, part, nblk, pr.read_pair, xtbl_off, c->aj_xtbl_key.as<uint64_t>(), c->aj_xtbl_cnt.as<uint32_t>(), s);
    xkoff = c->aj_xkoff.as<int32_t>();
    launch_k6_flag(c->aj_xtbl_key.as<uint64_t>(), c->aj_xtbl_cnt.as<uint32_t>(), n_xslots, p->min_count, c->aj_xflag.as<int32_t>(), s);
    launch_scan_i32(c->scan_tmp, c->aj_xflag.as<int32_t>(), xkoff, n_xslots, xkoff + n_xslots, s);
    launch_k9_offsets(pair_off, xtbl_off, xkoff, ng, n_xslots, c->aj_xoff.as<int32_t>(), d_hxoff, d_ctl + 4, s);   // ([6] kept exons)
  }
  HIPCHK(c, hipEventRecord(c->ev_ajgene, s));
  HIPCHK(c, hipEventSynchronize(c->ev_ajgene));   // the numbers of kept junctions and exons size the records and the last kernels' grids
  HIPCHK(c, hipGetLastError());
  const int32_t n_kept = h_ctl[2], n_xkept = n_xslots > 0 ? h_ctl[6] : 0;
  // 3. order, motif, tables; the exon records
  if (n_kept <= 0) no_junctions();
  else {
    HIPCHK(c, c->aj_ck.reserve((size_t)n_kept * 8)); HIPCHK(c, c->aj_cc.reserve((size_t)n_kept * 4)); HIPCHK(c, c->aj_cp.reserve((size_t)n_kept * 4));
    HIPCHK(c, c->aj_jpair.reserve((size_t)n_kept * 4));
    HIPCHK(c, c->d_ajgene.reserve((size_t)n_kept * sizeof(lcr_junction_gene)));
    HIPCHK(c, c->h_ajgene.reserve((size_t)n_kept * sizeof(lcr_junction_gene)));
    lcr_junction_gene* d_hjunc = nullptr;
    HIPCHK(c, c->h_ajgene.dev(&d_hjunc));
    launch_k9_place(b, c->aj_tbl_key.as<uint64_t>(), c->aj_tbl_cnt.as<uint32_t>(), c->aj_flag.as<int32_t>(), koff, tbl_off, pair_off, pr, n_slots, n_kept,
                    c->aj_ck.as<uint64_t>(), c->aj_cc.as<uint32_t>(), c->aj_cp.as<int32_t>(), c->d_ajgene.as<lcr_junction_gene>(), c->aj_jpair.as<int32_t>(), s);
    launch_k9_tables(c->aj_jpair.as<int32_t>(), pr, c->aj_rows.p, c->aj_keys.as<uint64_t>(), n_kept, c->d_ajgene.as<lcr_junction_gene>(), d_hjunc, s);
    c->ajgene_n = n_kept;
  }
  if (n_xkept <= 0) no_exons();
  else {
    HIPCHK(c, c->aj_xck.reserve((size_t)n_xkept * 8)); HIPCHK(c, c->aj_xcc.reserve((size_t)n_xkept * 4)); HIPCHK(c, c->aj_xcp.reserve((size_t)n_xkept * 4));
    HIPCHK(c, c->d_ajexon.reserve((size_t)n_xkept * sizeof(lcr_exon_gene)));
    HIPCHK(c, c->h_ajexon.reserve((size_t)n_xkept * sizeof(lcr_exon_gene)));
    lcr_exon_gene* d_hexon = nullptr;
    HIPCHK(c, c->h_ajexon.dev(&d_hexon));
    launch_k10_place(c->aj_xtbl_key.as<uint64_t>(), c->aj_xtbl_cnt.as<uint32_t>(), c->aj_xflag.as<int32_t>(), xkoff, xtbl_off, pair_off, pr, ng, n_xslots,
                     n_xkept, c->aj_xck.as<uint64_t>(), c->aj_xcc.as<uint32_t>(), c->aj_xcp.as<int32_t>(), c->d_ajexon.as<lcr_exon_gene>(), d_hexon, s);
    c->ajgene_nx = n_xkept;
  }
  return finish();
}

int lcr_get_asj_genes(lcr_ctx* c, lcr_asj_gene_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->ajgene_valid) {
    c->err = "lcr_get_asj_genes before lcr_asj_genes (its tables die with the phase stage's results and with the gene assignment)";
    return LCR_E_STATE;
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(c->ev_ajgene));
  HIPCHK(c, hipGetLastError());
  out->n_regions = c->ajgene_ng; out->n_junctions = c->ajgene_n;
  out->junc = c->ajgene_n ? c->h_ajgene.as<lcr_junction_gene>() : nullptr;
  out->junc_region_off = c->h_ajgene_off.as<int32_t>();
  out->dev_junc = c->ajgene_n ? c->d_ajgene.as<lcr_junction_gene>() : nullptr;
  out->n_exons = c->ajgene_nx; out->n_genes = c->ajgene_n_genes;
  out->exon = c->ajgene_nx ? c->h_ajexon.as<lcr_exon_gene>() : nullptr;
  out->exon_region_off = c->h_ajexon_off.as<int32_t>();
  out->dev_exon = c->ajgene_nx ? c->d_ajexon.as<lcr_exon_gene>() : nullptr;
  out->gene_reads = c->ajgene_cov ? c->h_ajcov.as<int32_t>() : nullptr;
  out->kernel_ms = -1.f;
  if (c->timing && c->ajgene_timed) {
    HIPCHK(c, hipEventSynchronize(c->ev_ajgene_t[1]));
    HIPCHK(c, hipEventElapsedTime(&out->kernel_ms, c->ev_ajgene_t[0], c->ev_ajgene_t[1]));
  }
  return LCR_OK;
}

}  // extern "C"

// lcr_junctions_genes.hip — the host driver of K9 (k9_gene_junctions.hip): the haplotype x junction table per (region, gene) pair over the
// phased rows, and its getter.  Shaped like lcr_junctions: a call of its own behind lcr_phase and lcr_assign_genes that reads the bound
// batch, the fragment stage's row offsets, the phase stage's read records and the gene of every read, and writes a GeneJunctions
// (lcr_ctx.h) that no other stage or getter reads.  The sequence is written once, as the gj_* steps below, split at its two host waits:
// lcr_junctions_genes runs them on c->jgene, lcr_asj_genes (lcr_asj_genes.hip) on c->ajgene with K10's kernels between them.  The launch
// count does not depend on the numbers of regions, genes, reads or junctions; the host waits for the annotation's verdict and for two
// sets of sizes in pinned memory.
#include "lcr_ctx.h"
#include "lcr_asj_args.h"

int gj_begin(lcr_ctx* c, GeneJunctions& g) {
  g.st.valid = g.st.timed = false;
  HIPCHK(c, g.h_ctl.reserve(64));
  HIPCHK(c, g.h_off.reserve((size_t)(c->bv.n_regions + 1) * 4));
  HIPCHK(c, g.h_junc.reserve(sizeof(lcr_junction_gene)));
  HIPCHK(c, g.h_ctl.dev(&g.d_ctl));
  HIPCHK(c, g.h_off.dev(&g.d_off));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // (an earlier call's last kernels write the pinned blocks that are reused from here on)
  for (int i = 0; i < 8; i++) g.h_ctl.as<int32_t>()[i] = 0;
  return LCR_OK;
}

int gj_counts(lcr_ctx* c, GeneJunctions& g, uint32_t min_junctions) {
  const BatchView& b = c->bv;
  const int nr = b.n_reads, ng = b.n_regions;
  hipStream_t s = c->stream;
  const size_t n4 = (size_t)nr * 4, n14 = ((size_t)nr + 1) * 4;
  HIPCHK(c, g.part.reserve(n4)); HIPCHK(c, g.nocc.reserve(n4));
  HIPCHK(c, g.part_off.reserve(n14)); HIPCHK(c, g.occ_off.reserve(n14));
  HIPCHK(c, g.cnt.reserve((size_t)ng * 4)); HIPCHK(c, g.pair_off.reserve(((size_t)ng + 1) * 4)); HIPCHK(c, g.t.off.reserve(((size_t)ng + 1) * 4));
  HIPCHK(c, g.read_pair.reserve(n4)); HIPCHK(c, g.row_slot.reserve(n4));
  HIPCHK(c, g.pregion.reserve(n4)); HIPCHK(c, g.pgene.reserve(n4)); HIPCHK(c, g.prow0.reserve(n4)); HIPCHK(c, g.prows.reserve(n4));
  HIPCHK(c, g.pocc.reserve(n4)); HIPCHK(c, g.tsz.reserve(n4)); HIPCHK(c, g.tbl_off.reserve(n14));
  const int32_t* gene = c->d_gene.as<int32_t>();
  int32_t *part = g.part.as<int32_t>(), *nocc = g.nocc.as<int32_t>(), *part_off = g.part_off.as<int32_t>(), *occ_off = g.occ_off.as<int32_t>();
  int32_t *pair_off = g.pair_off.as<int32_t>(), *tbl_off = g.tbl_off.as<int32_t>();
  const K9Pairs pr = g.pairs();
  launch_k9_count(b, c->row_region_off.as<int32_t>(), c->phase.d_read_rec.as<lcr_read_record>(), gene, min_junctions, part, nocc, s);
  launch_scan_i32(c->scan_tmp, part, part_off, nr, part_off + nr, s);
  launch_scan_i32(c->scan_tmp, nocc, occ_off, nr, occ_off + nr, s);
  launch_k9_pair_count(b, gene, part, g.cnt.as<int32_t>(), s);
  launch_scan_i32(c->scan_tmp, g.cnt.as<int32_t>(), pair_off, ng, pair_off + ng, s);
  launch_k9_pair_emit(b, gene, part, nocc, pair_off, part_off, pr, s);
  launch_k9_sizes(b, pair_off, part_off, occ_off, pr.occ, g.tsz.as<int32_t>(), g.d_ctl, s);
  launch_scan_i32(c->scan_tmp, g.tsz.as<int32_t>(), tbl_off, nr, tbl_off + nr, s);
  return LCR_OK;
}

int gj_wait_counts(lcr_ctx* c, GeneJunctions& g, const char* fn, bool* empty) {
  { int rc = stream_wait(c, g.st.ev); if (rc) return rc; }   // the host sizes the row records, the keys and the table from the two totals
  const int32_t n_part = g.h_ctl.as<int32_t>()[0], n_occ = g.h_ctl.as<int32_t>()[1];
  *empty = n_part <= 0 || n_occ <= 0;
  if (!*empty && n_occ > (1 << 28)) { c->err = std::string(fn) + ": more than 2^28 junction occurrences in one batch; split it"; return LCR_E_ARG; }
  return LCR_OK;
}

int slot_table_clear(lcr_ctx* c, SlotTable& t, int32_t n_slots) {
  HIPCHK(c, t.tbl_key.reserve((size_t)n_slots * 8)); HIPCHK(c, t.tbl_cnt.reserve((size_t)n_slots * 4));
  HIPCHK(c, t.flag.reserve((size_t)n_slots * 4)); HIPCHK(c, t.koff.reserve(((size_t)n_slots + 1) * 4));
  HIPCHK(c, lcr_fill_async(t.tbl_key.p, 0xff, (size_t)n_slots * 8, c->stream));
  HIPCHK(c, lcr_fill_async(t.tbl_cnt.p, 0, (size_t)n_slots * 4, c->stream));
  t.n_slots = n_slots;
  return LCR_OK;
}

// A segment has fewer than 4 x its occurrences in slots; the slots behind the last segment stay empty.
int gj_rows(lcr_ctx* c, GeneJunctions& g, const lcr_gene_annotation& d) {
  const int32_t n_part = g.h_ctl.as<int32_t>()[0], n_occ = g.h_ctl.as<int32_t>()[1];
  HIPCHK(c, g.rows.reserve((size_t)n_part * launch_k9_row_bytes()));
  HIPCHK(c, g.keys.reserve((size_t)n_occ * 8));
  { int rc = slot_table_clear(c, g.t, 4 * n_occ); if (rc) return rc; }
  launch_k9_emit(c->bv, c->row_region_off.as<int32_t>(), c->phase.d_read_rec.as<lcr_read_record>(), c->d_gene.as<int32_t>(), g.part.as<int32_t>(),
                 g.occ_off.as<int32_t>(), g.pairs(), g.tbl_off.as<int32_t>(), d, g.rows.p, g.keys.as<uint64_t>(), g.t.tbl_key.as<uint64_t>(),
                 g.t.tbl_cnt.as<uint32_t>(), c->stream);
  return LCR_OK;
}

// kept slots and their number per region (the flag is K6's: occupied && n_reads >= min_count)
int gj_keep(lcr_ctx* c, SlotTable& t, const int32_t* pair_off, const int32_t* tbl_off, uint32_t min_count, int32_t* d_hoff, int32_t* d_ctl) {
  int32_t* koff = t.koff.as<int32_t>();
  launch_k6_flag(t.tbl_key.as<uint64_t>(), t.tbl_cnt.as<uint32_t>(), t.n_slots, min_count, t.flag.as<int32_t>(), c->stream);
  launch_scan_i32(c->scan_tmp, t.flag.as<int32_t>(), koff, t.n_slots, koff + t.n_slots, c->stream);
  launch_k9_offsets(pair_off, tbl_off, koff, c->bv.n_regions, t.n_slots, t.off.as<int32_t>(), d_hoff, d_ctl, c->stream);
  return LCR_OK;
}

int gj_tables(lcr_ctx* c, GeneJunctions& g, int32_t n_kept) {
  SlotTable& t = g.t;
  HIPCHK(c, t.ck.reserve((size_t)n_kept * 8)); HIPCHK(c, t.cc.reserve((size_t)n_kept * 4)); HIPCHK(c, t.cp.reserve((size_t)n_kept * 4));
  HIPCHK(c, g.jpair.reserve((size_t)n_kept * 4));
  HIPCHK(c, g.d_junc.reserve((size_t)n_kept * sizeof(lcr_junction_gene)));
  HIPCHK(c, g.h_junc.reserve((size_t)n_kept * sizeof(lcr_junction_gene)));
  lcr_junction_gene* d_hjunc = nullptr;
  HIPCHK(c, g.h_junc.dev(&d_hjunc));
  const K9Pairs pr = g.pairs();
  launch_k9_place(c->bv, t.tbl_key.as<uint64_t>(), t.tbl_cnt.as<uint32_t>(), t.flag.as<int32_t>(), t.koff.as<int32_t>(), g.tbl_off.as<int32_t>(),
                  g.pair_off.as<int32_t>(), pr, t.n_slots, n_kept, t.ck.as<uint64_t>(), t.cc.as<uint32_t>(), t.cp.as<int32_t>(),
                  g.d_junc.as<lcr_junction_gene>(), g.jpair.as<int32_t>(), c->stream);
  launch_k9_tables(g.jpair.as<int32_t>(), pr, g.rows.p, g.keys.as<uint64_t>(), n_kept, g.d_junc.as<lcr_junction_gene>(), d_hjunc, c->stream);
  g.n = n_kept;
  return LCR_OK;
}

void no_records(const HostBuf& h_off, int32_t ng, int32_t* n) {
  for (int r = 0; r <= ng; r++) h_off.as<int32_t>()[r] = 0;
  *n = 0;
}

int gj_finish(lcr_ctx* c, GeneJunctions& g) {
  g.ng = c->bv.n_regions;
  return call_end(c, g.st);
}

extern "C" {

int lcr_junctions_genes(lcr_ctx* c, const lcr_junction_params* p, int32_t mem, const lcr_gene_annotation* a) {
  if (!c) return LCR_E_ARG;
  if (!p || !lcr_annotation_sizes_ok(mem, a)) { c->err = "lcr_junctions_genes: null params or annotation" LCR_ANNOTATION_SIZES_MSG; return LCR_E_ARG; }
  if (!lcr_annotation_arrays_ok(a)) { c->err = "lcr_junctions_genes" LCR_ANNOTATION_ARRAYS_MSG; return LCR_E_ARG; }
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
  GeneJunctions& g = c->jgene;
  const int ng = c->bv.n_regions;
  // Nothing of the last call's result is touched before the annotation's verdict: a refused call changes nothing (the copies of the last
  // annotation are overwritten in front of it: nothing reads them once that call's kernels have run, and the stream orders the uploads
  // behind them).
  lcr_gene_annotation d{};
  int32_t* d_bad = nullptr;
  { int rc = annotation_queue(c, g.ann, a, mem, g.h_bad, &d, &d_bad); if (rc) return rc; }
  if (a->n_genes > 0) { int rc = annotation_verdict(c, g.h_bad, g.st.ev, "lcr_junctions_genes"); if (rc) return rc; }
  { int rc = gj_begin(c, g); if (rc) return rc; }
  const auto finish_empty = [&]() { no_records(g.h_off, ng, &g.n); return gj_finish(c, g); };   // no participating row, no occurrence or no kept junction
  if (c->bv.n_reads == 0 || ng == 0 || c->n_rows == 0 || a->n_genes == 0) return finish_empty();
  Bracket t(c, g.st);
  { int rc = gj_counts(c, g, p->min_junctions); if (rc) return rc; }
  bool empty = false;
  { int rc = gj_wait_counts(c, g, "lcr_junctions_genes", &empty); if (rc) return rc; }
  if (empty) return finish_empty();
  { int rc = gj_rows(c, g, d); if (rc) return rc; }
  { int rc = gj_keep(c, g.t, g.pair_off.as<int32_t>(), g.tbl_off.as<int32_t>(), p->min_count, g.d_off, g.d_ctl); if (rc) return rc; }
  { int rc = stream_wait(c, g.st.ev); if (rc) return rc; }   // the number of kept junctions sizes the records and the last kernels' grids
  const int32_t n_kept = g.h_ctl.as<int32_t>()[2];
  if (n_kept <= 0) return finish_empty();
  { int rc = gj_tables(c, g, n_kept); if (rc) return rc; }
  return gj_finish(c, g);
}

int lcr_get_junctions_genes(lcr_ctx* c, lcr_junction_gene_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED || !c->jgene.st.valid) {
    c->err = "lcr_get_junctions_genes before lcr_junctions_genes (its table dies with the phase stage's results and with the gene assignment)";
    return LCR_E_STATE;
  }
  return gj_get(c, c->jgene, out);
}

}  // extern "C"

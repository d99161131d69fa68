// lcr_calls.hip — the host drivers of the candidate stage (lcr_candidates: K2 on the pileup; lcr_import_candidates: the caller's sites;
// lcr_set_exon_mask: the column mask lcr_candidates' first filter pass reads) and of the fragment stage (lcr_fragments: K3), with their getters and
// the settle functions of the copies they leave in flight.
#include "lcr_ctx.h"

// lcr_candidates / lcr_import_candidates leave their last copies in flight: candidate records, per-region offsets, rows per region
int cand_settle(lcr_ctx* c) {
  if (!c->cand_pending) return LCR_OK;
  HIPCHK(c, hipEventSynchronize(c->ev_cand));
  const int ng = c->bv.n_regions;
  memcpy(c->h_cand_off.data(), c->h_stage[2].p, (size_t)(ng + 1) * 4);
  c->h_cand.assign(c->h_stage[1].as<lcr_candidate>(), c->h_stage[1].as<lcr_candidate>() + c->h_cand_off[ng]);
  c->cand_pending = false;
  return LCR_OK;
}

// lcr_fragments leaves the fill pass running; the entry count arrives on the host before that pass ends
int frag_settle(lcr_ctx* c) {
  if (!c->nnz_pending) return LCR_OK;
  HIPCHK(c, hipEventSynchronize(c->ev_nnz));
  c->nnz = c->h_nnz.as<int64_t>()[c->bv.n_regions];
  c->nnz_pending = false;
  return LCR_OK;
}

namespace {

// Both candidate stages, from the point where they begin to overwrite the candidate / fragment buffers: back to the pileup, and the
// last lcr_phase's results are gone (lcr_collect_phase had to come before this call).  The caller has settled the phase stage.
void cand_begin(lcr_ctx* c) {
  c->res_valid = false;
  rewind_to(c, ST_PILED);
}

// ... and their common end, behind the kernel that writes d_cand / d_cand_off and their pinned copies (h_stage[1], h_stage[2]): the
// rows of the fragment matrix per region (fragment.rs:51-54) depend on the candidates only, so they are computed here and
// lcr_fragments starts without a round trip.  No wait: the host copies are picked up by whoever needs them first (cand_settle) --
// lcr_fragments queues its count pass before it does, so the GPU does not idle across the call boundary.
int cand_tail(lcr_ctx* c) {
  const int ng = c->bv.n_regions;
  HIPCHK(c, c->region_rows.reserve(std::max(ng, 1) * 4));
  HIPCHK(c, c->h_stage[3].reserve(std::max(ng, 1) * 4));
  HIPCHK(c, c->row_region_off.reserve((ng + 1) * 4));
  { int32_t* d_rr = nullptr;   // (the rows per region also go straight into the pinned block: no copy in the queue)
    HIPCHK(c, c->h_stage[3].dev(&d_rr));
    launch_k3_rows_offsets(c->bv, c->d_cand.as<lcr_candidate>(), c->d_cand_off.as<int32_t>(), c->region_rows.as<int32_t>(), c->row_region_off.as<int32_t>(), c->stream, d_rr); }
  HIPCHK(c, hipEventRecord(c->ev_cand, c->stream));
  HIPCHK(c, hipGetLastError());
  c->cand_pending = true;
  c->stage = ST_CALLED;
  return LCR_OK;
}

// the pinned blocks the last kernel of a candidate stage writes the kept records and their offsets into (capacity: n_max records)
int cand_host_blocks(lcr_ctx* c, size_t n_max, lcr_candidate** hp, int32_t** ho) {
  const int ng = c->bv.n_regions;
  HIPCHK(c, c->h_stage[1].reserve(std::max<size_t>(n_max, 1) * sizeof(lcr_candidate)));
  HIPCHK(c, c->h_stage[2].reserve((size_t)(ng + 1) * 4));
  HIPCHK(c, c->h_stage[1].dev(hp));
  HIPCHK(c, c->h_stage[2].dev(ho));
  if (ng == 0) c->h_stage[2].as<int32_t>()[0] = 0;
  return LCR_OK;
}

// pass 1 of the candidate filters: flags per column, survivors per tile -- k2_filter, unless the tally's epilogue has taken the pass
// already (lcr_pileup ran with the same filter parameters and under the same exon mask: ONT presets, k2_eval.h)
int cand_queue_pass1(lcr_ctx* c) {
  const int nt = c->n_tiles;
  HIPCHK(c, c->flags.reserve(std::max<size_t>(c->n_cols, 1)));
  HIPCHK(c, c->tile_count.reserve(std::max(nt, 1) * 4));
  HIPCHK(c, c->tile_off.reserve((std::max(nt, 1) + 1) * 4));
  HIPCHK(c, c->total.reserve(16));
  const DevParams &fa = c->flt_dp, &fb = c->dp;
  const bool have_flt = c->flt_fused && c->dbg_fuse_filter != 0 && fa.ont == fb.ont && fa.min_depth == fb.min_depth && fa.max_depth == fb.max_depth && fa.low_cnt_cut == fb.low_cnt_cut &&
                        fa.use_strand_bias == fb.use_strand_bias && fa.min_af_intron == fb.min_af_intron && fa.low_frac_cut == fb.low_frac_cut && fa.sor_threshold == fb.sor_threshold &&
                        c->flt_mask_gen == c->mask_gen;
  if (!have_flt) { const int rc = planes_tally(c, false); if (rc) return rc; }   // (k2_filter reads the planes: a lean tally has not stored them)
  Timer t(c, LCR_K_CAND_FILTER);
  if (!have_flt) {
    c->flt_fused = false;   // (the pass below overwrites the flags and tile counts of lcr_pileup's epilogue)
    c->sv_staged = false;   // (... and the staged survivors are those of the pileup's parameters)
    launch_k2_filter(c->bv, c->dp, c->tile_region.as<int32_t>(), c->tile_col0.as<int32_t>(), nt, c->n_cols,
                     c->planes.as<uint32_t>(), c->k0_tile_fill.as<int32_t>(), c->flags.as<uint8_t>(), c->tile_count.as<int32_t>(), c->stream);
  }
  return LCR_OK;
}

void queue_compact(lcr_ctx* c, int32_t cap) {
  launch_k2_compact(c->bv, c->dp, c->tile_region.as<int32_t>(), c->tile_col0.as<int32_t>(), c->n_tiles, c->n_cols,
                    c->planes.as<uint32_t>(), c->flags.as<uint8_t>(), c->tile_count.as<int32_t>(), c->tile_off.as<int32_t>(),
                    c->survivors.as<Survivor>(), cap, c->stream);
}

// survivors per region = tile offsets at the regions' first tiles (gathered on the device, pinned D2H); waits for their number.
// The survivors' compaction (and the fill of their histograms) is queued BEFORE the host knows how many there are, into buffers sized
// by the last call's count + a quarter, and the host waits for an event in front of it: the round trip (28 us on C3) runs under that kernel
// instead of in front of it.  More survivors than the guess (or no guess yet): the kernel dropped the rest, and runs again in cand_queue_genotypes
// (behind a lean pileup: behind a second tally in the full fused form, which leaves it the planes and flags it reads).
// *compacted: survivors and a cleared hist are in place, or on their way.
int cand_count_survivors(lcr_ctx* c, int32_t* n_sv_out, bool* compacted) {
  const int ng = c->bv.n_regions, nt = c->n_tiles;
  HIPCHK(c, c->sv_region_off.reserve((ng + 1) * 4));
  HIPCHK(c, c->h_stage[0].reserve((ng + 2) * 4));
  int32_t* const sv_off = c->h_stage[0].as<int32_t>();
  { int32_t* d_sv = nullptr;   // (the gather writes the offsets into the pinned block as well: the wait needs no copy behind it)
    HIPCHK(c, c->h_stage[0].dev(&d_sv));
    launch_scan_i32(c->scan_tmp, c->tile_count.as<int32_t>(), c->tile_off.as<int32_t>(), nt, c->total.as<int32_t>(), c->stream);
    launch_gather_i32(c->tile_off.as<int32_t>(), c->first_tile.as<int32_t>(), ng + 1, nt, c->total.as<int32_t>(), c->sv_region_off.as<int32_t>(), c->stream, d_sv); }
  // Behind a lean pileup (sv_staged; its parameters are this call's: cand_queue_pass1) the survivors' records exist already, staged by the tally in
  // the order the tiles finished: k2_place copies them to their places -- (tile, column) order, the same from run to run -- in k2_compact's stead.
  // The capacity is the staging's: the guess lcr_pileup sized it by.
  const bool staged = c->sv_staged && nt > 0;
  const int32_t cap_guess = staged ? c->sv_stage_cap : (c->dbg_spec_compact && nt > 0) ? c->sv_cap_guess : 0;
  if (cap_guess > 0) {
    HIPCHK(c, hipEventRecord(c->ev_sv, c->stream));
    HIPCHK(c, c->survivors.reserve((size_t)cap_guess * sizeof(Survivor)));
    HIPCHK(c, c->hist.reserve((size_t)cap_guess * 124 * 4 + 64));
    HIPCHK(c, lcr_fill_async(c->hist.p, 0, (size_t)cap_guess * 124 * 4 + 64, c->stream));
    if (staged)
      launch_k2_place(c->sv_stage.as<Survivor>(), c->sv_stage_key.p, c->k0_tile_fill.as<int32_t>() + pile_scratch(nt).tmp + K1_TMP_STAGED, c->sv_stage_cap,
                      c->tile_off.as<int32_t>(), c->survivors.as<Survivor>(), cap_guess, c->stream);
    else queue_compact(c, cap_guess);
    HIPCHK(c, hipEventSynchronize(c->ev_sv));
  } else HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  const int32_t n_sv = sv_off[ng];
  *compacted = cap_guess > 0 && n_sv <= cap_guess;
  if (staged) {
    c->sv_stage_n = std::min(n_sv, c->sv_stage_cap);   // (the tile counts' sum is the tally's counter)
    if (!*compacted) {   // more survivors than the staging holds: the tally again in its full fused form -- planes, flags, counts --, then k2_compact (cand_queue_genotypes)
      const int rc = planes_tally(c, true);
      if (rc) return rc;
      c->sv_staged = false;
    }
  }
  c->sv_cap_guess = n_sv > 0 ? n_sv + n_sv / 4 + 64 : 0;
  *n_sv_out = n_sv;
  HT("cand:n_sv");
  if (c->phase.dbg.prof) fprintf(stderr, "[cand] %d survivors of the count filters in %lld columns, %d reads\n", n_sv, (long long)c->n_cols, c->bv.n_reads);
  return LCR_OK;
}

// quality histograms of the survivors and their genotype likelihoods (k2_gt: records in cand_tmp, keep flags)
int cand_queue_genotypes(lcr_ctx* c, const lcr_params* p, int32_t n_sv, bool compacted) {
  const int ng = c->bv.n_regions, nt = c->n_tiles;
  HIPCHK(c, c->survivors.reserve(std::max(n_sv, 1) * sizeof(Survivor)));
  HIPCHK(c, c->hist.reserve(std::max<size_t>(n_sv, 1) * 124 * 4 + 64));   // (+ the hit lists' overflow counter: cleared with the histograms)
  HIPCHK(c, c->cand_tmp.reserve(std::max<size_t>(n_sv, 1) * sizeof(lcr_candidate)));
  HIPCHK(c, c->keep.reserve(((size_t)std::max(n_sv, 1) * 3 + 2) * 4));   // keep | pos (+1) | het/hom index scratch
  HIPCHK(c, c->d_cand.reserve(std::max<size_t>(n_sv, 1) * sizeof(lcr_candidate)));   // (capacity: every survivor kept)
  HIPCHK(c, c->d_cand_off.reserve((ng + 1) * 4));
  c->h_cand.clear();
  c->h_cand_off.assign(ng + 1, 0);
  if (!n_sv) return LCR_OK;
  // from K0's per-tile records when the survivors are dense (>= 1 per 8 columns: a second
  // pileup -- C5), else by walking the reads that cover them.  The tile form needs the ONT presets (end trim already cut out of
  // the records) and u16 counters (a survivor's depth is <= max_depth).
  const bool tiles_ok = c->dp.ont && p->max_depth <= 65535u;
  const bool hist_tiles = tiles_ok && c->dbg_hist_tiles >= 0 && (c->dbg_hist_tiles > 0 || (int64_t)n_sv * 8 >= c->n_cols);
  if (!compacted) HIPCHK(c, lcr_fill_async(c->hist.p, 0, (size_t)n_sv * 124 * 4 + 64, c->stream));
  c->hits_valid = !hist_tiles && c->dbg_k3_hits != 0;   // (the walk below leaves K3 its hits; the tile form does not walk reads)
  c->hits_n_sv = n_sv;
  if (c->hits_valid) {
    HIPCHK(c, c->hit_cnt.reserve(std::max<size_t>(c->bv.n_reads, 1) * 4));
    HIPCHK(c, c->hit_list.reserve(std::max<size_t>(c->bv.n_reads, 1) * LCR_HITS * 8));
    HIPCHK(c, c->ovf_list.reserve(std::max<size_t>(c->bv.n_reads, 1) * 4));
  }
  { Timer t(c, LCR_K_CAND_HIST);
    if (!compacted) queue_compact(c, n_sv);
    if (hist_tiles)
      launch_k2_hist_tiles(c->bv, c->tile_col0.as<int32_t>(), nt, c->tile_count.as<int32_t>(), c->tile_off.as<int32_t>(), c->survivors.as<Survivor>(),
                           c->chunk_off.as<int32_t>(), c->chunks.p, c->k0_items.as<unsigned long long>(), c->hist.as<uint32_t>(), c->stream);
    else
      launch_k2_hist(c->bv, c->dp, c->read_bin.as<ReadBin>(), c->survivors.as<Survivor>(), c->tile_off.as<int32_t>(), nt, n_sv, c->hist.as<uint32_t>(),
                     c->hits_valid ? c->hit_cnt.as<int32_t>() : nullptr, c->hit_list.p, (int32_t*)(c->hist.as<uint32_t>() + (size_t)n_sv * 124), c->ovf_list.as<int32_t>(),
                     c->stream); }
  { Timer t(c, LCR_K_CAND_GT);
    launch_k2_gt(c->dp, c->survivors.as<Survivor>(), n_sv, c->hist.as<uint32_t>(), c->bv.start0,
                 c->cand_tmp.as<lcr_candidate>(), c->keep.as<int32_t>(), c->stream); }
  return LCR_OK;
}

// ordered compaction of the kept candidates + dense-cluster sweep (candidate.rs:465-526) on the device; the
// host copy (getters, chain-region host steps) arrives with the same round trip as the offsets
// (the kept records and their offsets leave for pinned host memory inside the last kernel, which knows the count: a copy of the records'
// capacity on a second queue -- 3 MB on C3 -- held up the fragment stage's first kernel for 30 us)
int cand_queue_finish(lcr_ctx* c, const lcr_params* p, int32_t n_sv) {
  int32_t* const d_keep = c->keep.as<int32_t>();
  int32_t* const d_pos = d_keep + std::max(n_sv, 1);
  int32_t* const d_idx = d_pos + std::max(n_sv, 1) + 1;
  lcr_candidate* hp = nullptr; int32_t* ho = nullptr;
  { int rc = cand_host_blocks(c, (size_t)n_sv, &hp, &ho); if (rc) return rc; }
  launch_k2_finish(c->scan_tmp, c->cand_tmp.as<lcr_candidate>(), d_keep, n_sv, c->sv_region_off.as<int32_t>(), c->bv.n_regions, d_pos, d_idx,
                   c->d_cand.as<lcr_candidate>(), c->d_cand_off.as<int32_t>(), p->dense_win, p->min_dense_cnt, c->stream, hp, ho);
  HT("cand:finish_q");
  return LCR_OK;
}

}  // namespace

extern "C" {

int lcr_candidates(lcr_ctx* c, const lcr_params* p) {
  HT("cand");
  if (!c || !p) return LCR_E_ARG;
  if (c->stage < ST_PILED) { c->err = "lcr_candidates before lcr_pileup"; return LCR_E_STATE; }
  // (k2_hist trims the read ends by dist_to_end on records K0 cut with the pileup's value, and the ONT / HiFi planes differ)
  if (p->platform != c->pile_platform || p->dist_to_end != c->pile_dist_to_end) {
    c->err = "lcr_candidates: platform and dist_to_end must be those of lcr_pileup";
    return LCR_E_ARG;
  }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }   // (the previous batch's phase stage reads the candidate / fragment buffers rewritten from here on)
  HT("cand:settled");
  cand_begin(c);
  c->dp = to_dev(p, c->dp.sor_threshold);
  int rc;
  int32_t n_sv = 0;
  bool compacted = false;
  if ((rc = cand_queue_pass1(c))) return rc;
  if ((rc = cand_count_survivors(c, &n_sv, &compacted))) return rc;
  if ((rc = cand_queue_genotypes(c, p, n_sv, compacted))) return rc;
  if ((rc = cand_queue_finish(c, p, n_sv))) return rc;
  rc = cand_tail(c);
  HT("cand:ret");
  return rc;
}

// replaces SNPFrag::import_external_candidates (candidate.rs:530-613) -- the candidate stage of thread.rs:107-116 -- for sites the
// caller brings (a VCF, lcr_vcf_*).  Leaves the context as lcr_candidates does for the stages behind it; the regular path's own state
// (pass-1 flags and tile counts of lcr_pileup, the survivors' size guess) is not touched, so lcr_candidates can follow on the same pileup.
int lcr_import_candidates(lcr_ctx* c, const lcr_params* p, int32_t mem, int32_t n_sites, const int64_t* pos0, const uint8_t* genotype,
                          const float* qual) {
  HT("import");
  if (!c) return LCR_E_ARG;
  if (!p || n_sites < 0 || (mem != LCR_MEM_HOST && mem != LCR_MEM_DEVICE)) {
    c->err = "lcr_import_candidates: null params, n_sites < 0 or mem not LCR_MEM_HOST / LCR_MEM_DEVICE";
    return LCR_E_ARG;
  }
  if (n_sites > 0 && (!pos0 || !genotype || !qual)) { c->err = "lcr_import_candidates: null site array"; return LCR_E_ARG; }
  if (c->stage < ST_PILED) { c->err = "lcr_import_candidates before lcr_pileup"; return LCR_E_STATE; }
  if (mem == LCR_MEM_HOST)
    for (int32_t i = 0; i < n_sites; i++)
      if (genotype[i] > 4 || (i > 0 && pos0[i - 1] >= pos0[i])) {
        c->err = "lcr_import_candidates: sites must be sorted by position without duplicates, genotype codes 0-4 (site " + std::to_string(i) + ")";
        return LCR_E_ARG;
      }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }   // (the previous batch's phase stage reads the candidate / fragment buffers rewritten from here on)
  const int ng = c->bv.n_regions;
  const int64_t* d_pos = nullptr; const uint8_t* d_gt = nullptr; const float* d_q = nullptr;
  { int rc = upload(c, c->imp_pos, pos0, (size_t)n_sites, &d_pos, mem); if (rc) return rc; }
  { int rc = upload(c, c->imp_gt, genotype, (size_t)n_sites, &d_gt, mem); if (rc) return rc; }
  { int rc = upload(c, c->imp_q, qual, (size_t)n_sites, &d_q, mem); if (rc) return rc; }
  if (mem == LCR_MEM_DEVICE && n_sites > 0) {   // (the one host wait of a device-resident list: its contract, as lcr_load_batch checks a device batch)
    HIPCHK(c, c->h_imp_bad.reserve(64));
    int32_t* bad = c->h_imp_bad.as<int32_t>();
    *bad = 0;
    int32_t* d_bad = nullptr;
    HIPCHK(c, c->h_imp_bad.dev(&d_bad));
    launch_k2_import_check(d_pos, d_gt, n_sites, d_bad, c->stream);
    HIPCHK(c, hipEventRecord(c->ev_imp, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev_imp));
    if (*(volatile int32_t*)bad) { c->err = "lcr_import_candidates: sites must be sorted by position without duplicates, genotype codes 0-4"; return LCR_E_ARG; }
  }
  cand_begin(c);   // (hits_valid goes with it: no hit lists, K3 walks the CIGARs)
  // records <= sites: every buffer is sized by n_sites, no count comes back to the host
  HIPCHK(c, c->imp_cnt.reserve(std::max(ng, 1) * 4));
  HIPCHK(c, c->d_cand.reserve(std::max<size_t>(n_sites, 1) * sizeof(lcr_candidate)));
  HIPCHK(c, c->d_cand_off.reserve((ng + 1) * 4));
  lcr_candidate* hp = nullptr; int32_t* ho = nullptr;
  { int rc = cand_host_blocks(c, (size_t)n_sites, &hp, &ho); if (rc) return rc; }
  c->h_cand.clear();
  c->h_cand_off.assign(ng + 1, 0);
  { const int rc = planes_tally(c, false); if (rc) return rc; }   // (k2_import_emit reads the sites' counts: a lean tally has not stored them)
  { Timer t(c, LCR_K_CAND_IMPORT);
    launch_k2_import_count(c->bv, d_pos, d_gt, d_q, n_sites, c->imp_cnt.as<int32_t>(), c->stream);
    launch_scan_i32(c->scan_tmp, c->imp_cnt.as<int32_t>(), c->d_cand_off.as<int32_t>(), ng, c->d_cand_off.as<int32_t>() + ng, c->stream);
    launch_k2_import_emit(c->bv, c->n_cols, c->planes.as<uint32_t>(), c->k0_tile_fill.as<int32_t>(), d_pos, d_gt, d_q, n_sites, c->d_cand_off.as<int32_t>(),
                          c->d_cand.as<lcr_candidate>(), c->stream, hp, ho); }
  const int rc = cand_tail(c);
  HT("import:ret");
  return rc;
}

// The exon-only mask of the bound batch (include/lcr.h).  Refused calls change nothing: the lists are checked -- on the host, or by k2_exon_check,
// whose verdict is the call's one wait -- before the plane is touched.  A set or clear behind lcr_pileup puts the context back at the pileup: the
// candidate records were made under another mask.  The pileup itself does not depend on the mask; its fused verdicts do (mask_gen).
int lcr_set_exon_mask(lcr_ctx* c, int32_t mem, const int32_t* iv_off, const int64_t* iv_start0, const int64_t* iv_end0) {
  if (!c) return LCR_E_ARG;
  if (mem != LCR_MEM_HOST && mem != LCR_MEM_DEVICE) { c->err = "lcr_set_exon_mask: mem not LCR_MEM_HOST / LCR_MEM_DEVICE"; return LCR_E_ARG; }
  if (c->stage < ST_LOADED) { c->err = "lcr_set_exon_mask before lcr_load_batch"; return LCR_E_STATE; }
  const char* const bad_lists = "lcr_set_exon_mask: iv_off must start at 0 and ascend, every interval needs end0 >= start0, and a non-zero count its two arrays";
  const int ng = c->bv.n_regions;
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t* plane = nullptr;
  if (iv_off) {
    int32_t n_iv = 0;
    const int32_t* d_off = nullptr; const int64_t *d_s = nullptr, *d_e = nullptr;
    if (mem == LCR_MEM_HOST) {
      bool ok = iv_off[0] == 0;
      for (int g = 0; g < ng && ok; g++) ok = iv_off[g] <= iv_off[g + 1];
      n_iv = ok ? iv_off[ng] : 0;
      ok = ok && (n_iv == 0 || (iv_start0 && iv_end0));
      for (int32_t i = 0; i < n_iv && ok; i++) ok = iv_end0[i] >= iv_start0[i];
      if (!ok) { c->err = bad_lists; return LCR_E_ARG; }
    } else {   // (the one host wait of device-resident lists: their contract, as lcr_import_candidates checks its sites)
      HIPCHK(c, c->h_imp_bad.reserve(64));
      int32_t* verdict = c->h_imp_bad.as<int32_t>();
      verdict[0] = verdict[1] = 0;
      int32_t* d_verdict = nullptr;
      HIPCHK(c, c->h_imp_bad.dev(&d_verdict));
      launch_k2_exon_check(iv_off, iv_start0, iv_end0, ng, d_verdict, c->stream);
      { const int rc = stream_wait(c, c->ev_imp); if (rc) return rc; }
      if (((volatile int32_t*)verdict)[0]) { c->err = bad_lists; return LCR_E_ARG; }
      n_iv = ((volatile int32_t*)verdict)[1];
    }
    { int rc = upload(c, c->ex_off, iv_off, (size_t)ng + 1, &d_off, mem); if (rc) return rc; }
    { int rc = upload(c, c->ex_s, iv_start0, (size_t)n_iv, &d_s, mem); if (rc) return rc; }
    { int rc = upload(c, c->ex_e, iv_end0, (size_t)n_iv, &d_e, mem); if (rc) return rc; }
    const size_t words = (size_t)((c->n_cols + 31) / 32);
    HIPCHK(c, c->exon_plane.reserve(std::max<size_t>(words, 1) * 4));
    if (c->timing && !c->ev_mask_t[0]) for (hipEvent_t& e : c->ev_mask_t) HIPCHK(c, hipEventCreate(&e));
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev_mask_t[0], c->stream));
    if (words) HIPCHK(c, lcr_fill_async(c->exon_plane.p, 0, words * 4, c->stream));
    launch_k2_exon_build(c->bv, d_off, d_s, d_e, n_iv, c->exon_plane.as<uint32_t>(), c->stream);
    if (c->timing) { HIPCHK(c, hipEventRecord(c->ev_mask_t[1], c->stream)); c->mask_timed = true; }
    HIPCHK(c, hipGetLastError());
    plane = c->exon_plane.as<uint32_t>();
  }
  c->bv.exon_mask = plane;
  c->mask_gen++;
  // behind the pileup: its planes stay, what the candidate stages made of them under the other mask goes (lcr_collect_phase keeps the last
  // lcr_phase's results until the next candidate stage, as it does across lcr_load_batch)
  rewind_to(c, ST_PILED);
  return LCR_OK;
}

int lcr_exon_mask_ms(lcr_ctx* c, float* ms) {
  if (!c || !ms) return LCR_E_ARG;
  if (!c->timing || !c->mask_timed) { c->err = "lcr_exon_mask_ms: no lcr_set_exon_mask with timing enabled"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(c->ev_mask_t[1]));
  HIPCHK(c, hipEventElapsedTime(ms, c->ev_mask_t[0], c->ev_mask_t[1]));
  return LCR_OK;
}

int lcr_get_candidates(lcr_ctx* c, lcr_candidate_list* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_CALLED) { c->err = "lcr_get_candidates before lcr_candidates"; return LCR_E_STATE; }
  { int rc = cand_settle(c); if (rc) return rc; }
  { int rc = phase_settle(c); if (rc) return rc; }   // (after lcr_phase the records carry its results)
  out->n_cand = (int32_t)c->h_cand.size();
  out->n_regions = c->bv.n_regions;
  out->cand = c->h_cand.data();
  out->region_off = c->h_cand_off.data();
  return LCR_OK;
}

int lcr_get_candidates_device(lcr_ctx* c, const lcr_candidate** dev_cand, int32_t* n_cand) {
  if (!c || !dev_cand || !n_cand) return LCR_E_ARG;
  if (c->stage < ST_CALLED) { c->err = "lcr_get_candidates_device before lcr_candidates"; return LCR_E_STATE; }
  { int rc = cand_settle(c); if (rc) return rc; }
  { int rc = phase_settle(c); if (rc) return rc; }
  *dev_cand = c->d_cand.as<lcr_candidate>();
  *n_cand = (int32_t)c->h_cand.size();
  return LCR_OK;
}

int lcr_fragments(lcr_ctx* c, const lcr_params* p) {
  HT("frag");
  if (!c || !p) return LCR_E_ARG;
  if (c->stage < ST_CALLED) { c->err = "lcr_fragments before lcr_candidates"; return LCR_E_STATE; }
  if (c->cand_used) { c->err = "lcr_fragments after lcr_phase: the phase stage has rewritten the candidate records; run the candidate stage again"; return LCR_E_STATE; }
  if (p->min_linkers == 0) { c->err = "min_linkers must be > 0 (fragment.rs:252)"; return LCR_E_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  rewind_to(c, ST_CALLED);   // (from here on the fragment matrix and its row tables are rewritten)
  const int ng = c->bv.n_regions;
  c->min_linkers = p->min_linkers;
  // The count pass is queued before the host knows the row count: buffers are sized for one row per read (rows are
  // a prefix of every region's reads), counts of the unused tail stay 0, so the scan puts the entry total at
  // row_ptr[n_rows] as well as at its end.
  const int nr_cap = c->bv.n_reads;
  HIPCHK(c, c->row_cnt.reserve(std::max(nr_cap, 1) * 4));   // (row_region_off is on the device since lcr_candidates)
  HIPCHK(c, c->frag_tmp_col.reserve((size_t)std::max(nr_cap, 1) * launch_k3_inline() * 4));   // provisional entries of the count pass
  HIPCHK(c, c->frag_tmp_val.reserve((size_t)std::max(nr_cap, 1) * launch_k3_inline()));
  HIPCHK(c, c->row_links.reserve(std::max(nr_cap, 1) * 4));
  HIPCHK(c, c->row_ptr.reserve((std::max(nr_cap, 1) + 1) * 8));
  if (nr_cap) HIPCHK(c, lcr_fill_async(c->row_cnt.p, 0, (size_t)nr_cap * 4, c->stream));
  HT("frag:memset_q");
  // the count pass takes the (read, survivor) hits lcr_candidates' walk left (candidates are a subset of the survivors): no second
  // CIGAR walk; without them (dense survivors: the tile histograms) it walks the reads itself
  K3Hits hits{};
  if (c->hits_valid) {
    const int32_t* d_keep = c->keep.as<int32_t>();
    hits = K3Hits{c->hit_cnt.as<int32_t>(), c->hit_list.p, (const int32_t*)(c->hist.as<uint32_t>() + (size_t)c->hits_n_sv * 124), c->ovf_list.as<int32_t>(),
                  d_keep, d_keep + std::max(c->hits_n_sv, 1)};
  }
  { Timer t(c, LCR_K_FRAG_COUNT);
    launch_k3_count(c->bv, c->read_bin.as<ReadBin>(), c->d_cand.as<lcr_candidate>(), c->d_cand_off.as<int32_t>(), c->row_region_off.as<int32_t>(), nr_cap,
                    c->row_cnt.as<int32_t>(), c->row_links.as<uint32_t>(), c->frag_tmp_col.as<int32_t>(), c->frag_tmp_val.as<uint8_t>(), hits, c->dbg_k3_list_blocks, c->stream);
    launch_scan_i32_to_i64(c->scan_tmp, c->row_cnt.as<int32_t>(), c->row_ptr.as<int64_t>(), nr_cap, c->stream); }
  // the regions' first entries ([ng] = all entries) follow the count pass to the host: the phase stage sizes its
  // work from them without a round trip of its own
  HIPCHK(c, c->h_nnz.reserve((size_t)(ng + 1) * 8));
  HIPCHK(c, c->region_e_off.reserve((size_t)(ng + 1) * 8));
  { int64_t* d_nnz = nullptr;   // (straight into the pinned block: no copy in the queue in front of the fill pass)
    HIPCHK(c, c->h_nnz.dev(&d_nnz));
    launch_k3_region_entries(c->row_ptr.as<int64_t>(), c->row_region_off.as<int32_t>(), ng, c->region_e_off.as<int64_t>(), c->stream, d_nnz); }
  HIPCHK(c, hipEventRecord(c->ev_nnz, c->stream));
  c->nnz_pending = true;
  HT("frag:count_q");
  // now the candidates' host copies (long since there): rows per region, candidates per region
  { int rc = cand_settle(c); if (rc) return rc; }
  if (c->phase.dbg.prof && c->hits_valid) {
  HT("frag:cand_settled");
    int32_t n_ovf = 0;
    HIPCHK(c, hipMemcpy(&n_ovf, c->hist.as<uint32_t>() + (size_t)c->hits_n_sv * 124, 4, hipMemcpyDeviceToHost));
    fprintf(stderr, "[frag] %d reads with more than %d survivor hits (walked again)\n", n_ovf, LCR_HITS);
  }
  const int32_t* rr = c->h_stage[3].as<int32_t>();   // rows per region, from lcr_candidates
  c->h_row_region_off.assign(ng + 1, 0);
  for (int g = 0; g < ng; g++) c->h_row_region_off[g + 1] = c->h_row_region_off[g] + rr[g];
  c->n_rows = c->h_row_region_off[ng];
  const int nrow = c->n_rows;
  // entries: at most rows x candidates per region.  When that bound is affordable the fill pass is queued right
  // behind the count pass and the true count is picked up later (frag_settle); otherwise wait for it first.
  int64_t bound = 0;
  for (int g = 0; g < ng; g++) bound += (int64_t)rr[g] * (c->h_cand_off[g + 1] - c->h_cand_off[g]);
  int64_t cap = bound;
  if (bound > ((int64_t)1 << 28)) {
    int rc = frag_settle(c);
    if (rc) return rc;
    cap = c->nnz;
  }
  HIPCHK(c, c->col.reserve(std::max<int64_t>(cap, 1) * 4));
  HIPCHK(c, c->val.reserve(std::max<int64_t>(cap, 1)));
  { Timer t(c, LCR_K_FRAG_FILL);
    launch_k3_fill(c->bv, c->read_bin.as<ReadBin>(), c->d_cand.as<lcr_candidate>(), c->d_cand_off.as<int32_t>(), c->row_region_off.as<int32_t>(), nrow,
                   c->row_cnt.as<int32_t>(), c->row_ptr.as<int64_t>(), c->frag_tmp_col.as<int32_t>(), c->frag_tmp_val.as<uint8_t>(),
                   c->col.as<int32_t>(), c->val.as<uint8_t>(), hits, c->dbg_k3_list_blocks, c->stream); }
  HIPCHK(c, hipGetLastError());
  c->stage = ST_FRAGGED;
  HT("frag:ret");
  return LCR_OK;
}

int lcr_get_fragmat(lcr_ctx* c, lcr_fragmat* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_FRAGGED) { c->err = "lcr_get_fragmat before lcr_fragments"; return LCR_E_STATE; }
  { int rc = frag_settle(c); if (rc) return rc; }
  const int nrow = c->n_rows, ng = c->bv.n_regions;
  const int64_t nnz = c->nnz;
  HIPCHK(c, c->h_row_ptr.reserve((nrow + 1) * 8));
  HIPCHK(c, c->h_row_read.reserve(std::max(nrow, 1) * 4));
  HIPCHK(c, c->h_col.reserve(std::max<int64_t>(nnz, 1) * 4));
  HIPCHK(c, c->h_val.reserve(std::max<int64_t>(nnz, 1)));
  HIPCHK(c, c->h_row_fp.reserve(std::max(nrow, 1)));
  HIPCHK(c, c->h_row_links.reserve(std::max(nrow, 1) * 4));
  HIPCHK(c, hipMemcpyAsync(c->h_row_ptr.p, c->row_ptr.p, (size_t)(nrow + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  if (nrow) HIPCHK(c, hipMemcpyAsync(c->h_row_links.p, c->row_links.p, (size_t)nrow * 4, hipMemcpyDeviceToHost, c->stream));
  if (nnz) {
    HIPCHK(c, hipMemcpyAsync(c->h_col.p, c->col.p, (size_t)nnz * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_val.p, c->val.p, (size_t)nnz, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int32_t* rread = c->h_row_read.as<int32_t>();
  uint8_t* fp = c->h_row_fp.as<uint8_t>();
  const uint32_t* links = c->h_row_links.as<uint32_t>();
  for (int g = 0; g < ng; g++)
    for (int r = c->h_row_region_off[g]; r < c->h_row_region_off[g + 1]; r++) rread[r] = c->h_read_begin[g] + (r - c->h_row_region_off[g]);
  for (int r = 0; r < nrow; r++) fp[r] = links[r] >= c->min_linkers ? 1 : 0;
  out->n_rows = nrow; out->nnz = nnz; out->n_regions = ng;
  out->row_region_off = c->h_row_region_off.data();
  out->row_ptr = c->h_row_ptr.as<int64_t>(); out->row_read = rread; out->col = c->h_col.as<int32_t>();
  out->val = c->h_val.as<uint8_t>(); out->row_for_phasing = fp; out->row_links = links;
  return LCR_OK;
}

}  // extern "C"

// lcr_phase_host.h — host driver of the phasing stage (K4 kernels + sequential control).
#pragma once
#include <string>

#include "lcr_dev.h"
#include "k4_types.h"

struct PhaseInputs {
  int32_t n_regions = 0, n_rows = 0;
  int64_t nnz = 0;
  const int32_t* row_region_off = nullptr;   // host, n_regions+1
  const int32_t* cand_region_off = nullptr;  // host, n_regions+1
  const int64_t* region_start0 = nullptr;    // host
  const int64_t* region_e_off = nullptr;     // host, n_regions+1: first entry of every region in the fragment matrix
  const int64_t* d_row_ptr = nullptr;        // device CSR
  const int32_t* d_col = nullptr;
  const uint8_t* d_val = nullptr;
  const uint32_t* d_row_links = nullptr;
  std::vector<lcr_candidate>* cand = nullptr;  // host candidates, updated in place
  const lcr_candidate* d_cand = nullptr;     // device copy of the same candidates (as K3 saw them)
  const int32_t* d_cand_off = nullptr;       // device, n_regions+1
  const int32_t* d_row_region_off = nullptr; // device, n_regions+1
  const int64_t* d_start0 = nullptr;         // device, region start columns
  // down-sampling (lcr_set_downsample / lcr_set_downsample_rows): regions with at least ds_depth > 0 fragment rows are phased on the ds_depth
  // rows k4_sample picks; ds_rows (host, n_rows bytes of 0 / 1; overrides the depth): the caller's own sample
  uint32_t ds_depth = 0; uint64_t ds_seed = 0; const uint8_t* ds_rows = nullptr;
  int snps(int g) const { return cand_region_off[g + 1] - cand_region_off[g]; }   // SNPs (candidates) of region g
};

// Debug / test switches of the phase stage (lcr_debug_set, include/lcr.h): none of them is read from the environment inside
// the library; the defaults are the product behaviour.
struct PhaseDebug {
  int prof = 0;                 // "phase_prof": per-step timers to stderr (2: also the per-workgroup histogram)
  long long grid_min = -1;      // "grid_min_entries": chain regions with at least this many phase entries get all CUs (-1: 2^17)
  int grid_generic = 0;         // "grid_generic": fenced grid barriers only
  int post_half = 0;            // "post_half": the eight-wave epilogue of the chain regions
  int enum_force_big = 0;       // "enum_force_big" / "enum_force_stream": the fallback enumeration kernels
  int enum_force_stream = 0;    // (every LDS-resident region by the streaming kernel, k4_enum_reg)
  int enum_elide = 1;           // "enum_elide": k4_enum_bits / k4_enum_reg skip the sigma / delta steps whose inputs have not changed since they last ran (0: every step is executed)
  int spec_batch = 1;           // "grid_spec_batch": eight speculative half-rounds per pass over the matrix (k4_grid_batch.h); 0: the side-by-side lanes below
  int spec_lanes = 8;           // "grid_spec_lanes": half-rounds of the perturbation loop run at once at grid scope (1: one after the other; C5 with packed entries: 454 / 370 / 348 / 366 ms with 2 / 4 / 8 / 16 -- eight lanes = one XCD each)
  int redo_lds = 64 * 1024;     // "redo_lds": bytes of dynamic LDS of the enumeration branch's repair pass (k4_enum_redo: state + matrix of a restart's region where they fit; 0: global memory)
  int chain_ties = 1;           // "chain_ties": chain regions of workgroup scope that meet a class-2 / class-4 tie run again under the complete tie contract (0: counted as unresolved)
  int tie_arith = 3;            // "tie_arith": which exact fixed-point ties the reference-order f64 arithmetic decides (PhaseDev::tie_arith; 3 = all that liblcr resolves)
  int async_phase = 0;          // "async_phase": lcr_phase returns when its kernels are queued (on a queue of its own); settle() collects the results
};

struct PhaseCall;   // k4_phase.hip
const PhaseLutDev& phase_lut_dev();   // the stage's fixed-point table (HostLut, k4_phase.hip); lcr_haplotag sums the same terms

struct PhaseHost {
  PhaseDebug dbg;
  std::string lock_dir;          // directory of the per-GPU lock file of persistent launches ("" = /tmp/liblcr-<uid>)
  std::vector<double> objective;
  const int8_t* r_haplotag = nullptr;      // results of the last run: per row, in the pinned block k4_post / k4_gpost wrote (h_res)
  const uint8_t* r_assignment = nullptr;
  const uint32_t* r_phase_set = nullptr;
  // ---- buffers, by the step that uses them (each grows to the largest batch seen; freed with the context)
  // staging matrices (k4_stage): region table, row / column-major phase matrices, per-SNP bytes and constants, cursors, source rows
  DevBuf d_reg, d_prow_ptr, d_pcol, d_pval, d_ccol_ptr, d_crow, d_cval, d_snp, d_snp_const, d_cur, d_prow_src;
  // down-sampling (k4_sample): byte per fragment row, draw ordinal per phasing row; pinned: the bytes again | the launch's regions
  DevBuf d_sampled, d_prow_ord; HostBuf h_sampled, h_smp_slots;
  std::vector<uint8_t> ds_applied;   // per region of the last run: down-sampled (lcr_get_downsample)
  bool ds_any = false;               // ... some region was: d_sampled / h_sampled hold the last run's bytes
  int32_t ds_ng = 0, ds_nrow = 0;    // ... its region and fragment-row counts (the fragment stage may have moved on since)
  DevBuf d_grid_ctl, d_grid_tot;   // grid-scope launches: barrier blocks, k4_stage's per-workgroup totals
  // result state: sigma | delta | eta | objective of the enumeration and of the chain regions, per-row records in HBM (k4_post),
  // f64 table of the tie paths (PostLut), tie census counters; k4_post's step clocks (phase_prof)
  DevBuf d_st_enum, d_st_chain, d_read_rec, d_lut64, d_tie, d_prof_clk;
  bool lut64_ready = false;
  // chain-region scratch: descriptors, post-phase slots, LD pair table, adjacency, partial counts, per-SNP ints / bytes / doubles,
  // block info, per-row / per-entry ints, working state, accumulators, sigma words
  DevBuf d_ch_desc, d_ch_slots, d_ch_tbl, d_ch_adj, d_ch_part, d_ch_snpi, d_ch_snpb, d_ch_q, d_ch_info, d_ch_rowi, d_ch_enti, d_ch_work, d_ch_macc, d_ch_sig;
  DevBuf d_spec_sig, d_spec_de, d_spec_res, d_pk, d_bt;   // working states / results of the speculative half-rounds (k4_grid.hip)
  DevBuf d_tie_flag, d_tie_q, d_tie_ch, d_tie_terms;      // k4_chain_wg: regions that met a class-2 / class-4 tie, scratch of their second run
  // enumeration jobs: upload table, objectives | winners, final states of the restarts, best objective seen per region (filled
  // before the staging kernel), state scratch, row scores and repair lists of the repair pass, f64 terms of the global-memory class
  DevBuf d_en_job, d_en_obj, d_en_st, d_en_rbest, d_en_scr, d_en_qrow, d_en_redo, d_en_terms;
  DevBuf d_gp_snp, d_gp_ent, d_gp_part;   // k4_gpost scratch: per SNP and row, per entry, partial counts
  // pinned: region sizes (k4_stage), k4_post's results and candidate mirror | objectives, tie census, the two upload tables
  HostBuf h_stat, h_res, h_cand_obj, h_census, h_en_up, h_ch_up;
  unsigned long long tie_census[TIE_NCTR] = {0, 0, 0, 0, 0, 0, 0, 0};   // of the last run (lcr_get_tie_census)
  hipStream_t side = nullptr;   // second queue: chain regions, every persistent launch
  hipEvent_t ev_in = nullptr, ev_csr = nullptr, ev_fork = nullptr, ev_join = nullptr;
  hipStream_t aux = nullptr;   // the bit-state and global-memory enumeration classes beside the streaming class
  // lcr_debug_set("async_phase", 1) (round 5, opt-in): the stage's FIRST queue is its own too, lcr_phase returns when everything is
  // queued, the caller's stream is free for the next batch's lcr_load_batch / lcr_pileup, and the results are collected by
  // settle(): every getter, lcr_ctx_sync, the next lcr_candidates / lcr_phase call it.  Persistent all-CU launches (device
  // lock) and phase_prof settle before run() returns.  Default: the caller's stream, settle() inside run().
  hipStream_t main_q = nullptr, q_first = nullptr;   // q_first: the queue the last run() used as its first
  // async_phase: the next batch's pileup is gated on these -- recorded behind the enumeration restarts on the stage's first queue and
  // on `aux`: the dense part of the stage.  What follows them (repair pass, resolve, post-phase: a few hundred workgroups) leaves
  // most CUs idle, and that is where the next pileup's kernels run -- beside the restarts they would only time-share the VALUs.
  hipEvent_t ev_gate[2] = {nullptr, nullptr};
  bool gate_set[2] = {false, false};
  // makes `s` wait for the dense part of a stage in flight (no-op otherwise)
  hipError_t gate_stream(hipStream_t s) {
    if (!pending) return hipSuccess;
    for (int k = 0; k < 2; k++) if (gate_set[k]) { hipError_t e = hipStreamWaitEvent(s, ev_gate[k], 0); if (e != hipSuccess) return e; }
    return hipSuccess;
  }
  hipEvent_t ev_user = nullptr;
  bool pending = false;
  struct Pending {
    int ng = 0;
    std::vector<int32_t> cand_off;
    size_t res_ps = 0, res_tag = 0, res_asg = 0, hc_obj = 0;
    std::vector<lcr_candidate>* cand = nullptr;
  } pend;
  int settle(std::string* err);
  ChainDev chain_dev{};                // chain-region buffers of the last run (LD blocks are read back from them)
  std::vector<ChainDesc> chain_desc;
  std::vector<std::string> chain_forms;            // phase_prof: the form launch_chain gave each chain region (report_prof prints them)
  std::vector<uint64_t> enum_keys;                   // scratch of the enumeration launch preparation, kept across calls
  std::vector<int64_t> enum_job_base, enum_st_base;
  // LD blocks of one region of the last run in the reference's order (candidate.rs:733-745): off[n_blocks + 1], SNP indices
  int ld_blocks(const PhaseInputs& in, int region, std::vector<int32_t>* off, std::vector<int32_t>* snps, hipStream_t s, std::string* err);
  int run(const PhaseInputs& in, const lcr_params& p, hipStream_t s, std::string* err);
  // the steps of run(), in order (k4_phase.hip); PhaseCall holds the values of one call
  int open_queues(PhaseCall& c), size_buffers(PhaseCall& c), sample(PhaseCall& c), stage(PhaseCall& c), classify(PhaseCall& c), wait_sizes(PhaseCall& c);
  int launch_enum(PhaseCall& c), launch_chain(PhaseCall& c), launch_gpost(PhaseCall& c), report_prof(PhaseCall& c);
  bool mark_pending(PhaseCall& c);
  // queues and events (the buffers free themselves; the owner has drained the queues: lcr_ctx_destroy)
  void release() {
    for (hipStream_t* q : {&side, &aux, &main_q}) { if (*q) (void)hipStreamDestroy(*q); *q = nullptr; }
    for (hipEvent_t* e : {&ev_in, &ev_csr, &ev_fork, &ev_join, &ev_user, &ev_gate[0], &ev_gate[1]}) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
    gate_set[0] = gate_set[1] = false;
    pending = false;
  }
};

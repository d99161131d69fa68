// k4_phase.hip — K4: haplotype phasing on gfx950, HOST CONTROL (buffer sizing, launches, collecting the results).
//
// Replaces SNPFrag::phase (reference src/phase.rs:1087-1296) with its kernel cross_optimize
// (phase.rs:810-976) and the probability functions phase.rs:32-49,77-96,128-176,257-276, plus the
// post-phase sequence of src/thread.rs:168-201 (snpfrags.rs:191-733).
//
// Kernel units (in launch order; one queue stages + enumerates + post-processes, a second queue carries the
// few chain regions, see PhaseHost::run); k4_kernels.h / k4_grid.h hold their launchers and LDS layouts:
//   k4_stage.hip  k4_stage / k4_stage_grid   phase matrices (CSR + CSC, per-SNP constants) of every region from K3's fragment CSR:
//                               one workgroup per region, or all CUs on one large region
//   k4_enum.hip   k4_enum_bits / k4_enum_reg   S <= max_enum_snps: all 2^S enumeration restarts (phase.rs:1097-1122), eight
//                               restarts per wave as bit states / one wave64 per restart with the entries streamed from LDS;
//                               every restart leaves its objective, final state and signature
//                 k4_enum_resolve  `prob > largest_prob` (phase.rs:1113-1119) per region: the maximal objective, and among
//                               the configurations that have it the reference's f64 sums (phase.rs:257-276) decide
//                 k4_enum_big + k4_enum_resolve_big  fallback on global memory (matrix beyond the LDS budget): the same
//                               decision, then the winner re-run to materialise its state
//   k4_grid.hip   k4_chain_wg / k4_chain_grid   S > max_enum_snps: the sequential chain (phase.rs:1123-1233) with one
//                               workgroup per region, or all CUs on one large region (LD-block flip pass, perturbation rounds)
//   k4_post.hip   k4_post / k4_gpost   post-phase assignment, rescue and phase sets (f64, reference observation order): one workgroup
//                               per region with its image in LDS, or all CUs on one large region
// cross_optimize alternates sigma / delta-eta Jacobi steps until neither improves (<= 21 iterations).
// Its decision arithmetic is exact: every emission term log10(eps_q) / log10(1-eps_q) comes from a
// 31-entry table in fixed point (scale 2^40, int64), so sums are order-free and every comparison
// the reference makes on f64 ratio scores (q < qn, argmax q1..q4, prob > largest_prob) becomes an
// integer comparison of the log sums (the ratios 1 - A/D share a negative denominator D).  Where such a comparison is an
// exact TIE the reference's outcome is the rounding noise of its reference-order f64 sums: those sums are formed there
// (sigma ties per row, `prob > largest_prob` per configuration; PhaseDebug::tie_arith, lcr_get_tie_census).  See
// DESIGN.md "Decision arithmetic".
// rand::thread_rng() is replaced by a counter-based generator evaluated at the draw index the
// reference's call order implies, so restarts can run in parallel.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <climits>
#include <map>
#include <mutex>
#include <fcntl.h>
#include <sys/file.h>
#include <unistd.h>
#include <sys/stat.h>
#include <cerrno>

#include "k4_dev.h"
#include "k4_grid.h"
#include "k4_post.h"
#include "k4_kernels.h"

namespace {

// ================================= host side ====================================================

struct HostLut {
  double le[31], l1e[31];  // log10(eps), log10(1-eps), eps = 10^(-q/10) (fragment.rs:132); q=0 treated as q=1
  double p_homref, p_homvar, log_theta, log2;
  PhaseLutDev dev;
  HostLut() {
    for (int q = 0; q <= 30; q++) {
      const int qq = q == 0 ? 1 : q;
      const double eps = std::pow(10.0, -(double)qq / 10.0);
      le[q] = std::log10(eps); l1e[q] = std::log10(1.0 - eps);
      dev.fe[q] = std::llround(le[q] * FX_SCALE); dev.f1e[q] = std::llround(l1e[q] * FX_SCALE);
    }
    p_homref = std::log10(1.0 - 1.5 * 0.001); p_homvar = std::log10(0.5 * 0.001);
    log_theta = std::log10(0.001); log2 = std::log10(2.0);
    dev.f_homref = std::llround(p_homref * FX_SCALE); dev.f_homvar = std::llround(p_homvar * FX_SCALE);
    dev.f_het0 = std::llround(log_theta * FX_SCALE); dev.f_log2 = std::llround(log2 * FX_SCALE);
  }
};
const HostLut& hlut() { static HostLut l; return l; }

}  // namespace

const PhaseLutDev& phase_lut_dev() { return hlut().dev; }

// Persistent all-CU launches of different processes (or contexts) on one GPU would wait for each other's workgroups forever:
// they are serialised per DEVICE -- a process-local mutex keyed by the PCI bus id, and across processes an flock on
// <lock_dir>/grid_<bus id>.lock (lock_dir: lcr_ctx_set_lock_dir, created 0700; default the machine-wide /tmp/liblcr-locks, refused unless it
// is a directory of this user; the file is opened O_NOFOLLOW | O_CLOEXEC).  A lock that cannot be taken is an error, never
// silently skipped.  The destructor drains the queues it was given before it lets go (error paths return early).
struct GridLock {
  int fd = -1;
  bool held = false;
  std::mutex* dev_mu = nullptr;
  hipStream_t q[3] = {nullptr, nullptr, nullptr};
  int n_q = 0;
  static std::mutex& device_mutex(const std::string& bus) {
    static std::mutex table_mu;
    static std::map<std::string, std::mutex*> table;
    std::lock_guard<std::mutex> g(table_mu);
    auto it = table.find(bus);
    if (it == table.end()) it = table.emplace(bus, new std::mutex()).first;
    return *it->second;
  }
  // returns an error text, or "" when the lock is held
  std::string acquire(const std::string& lock_dir, hipStream_t a, hipStream_t b, hipStream_t c) {
    if (held) return "";
    q[0] = a; q[1] = b; q[2] = c; n_q = 3;
    int dev = 0;
    char bus[64] = "gpu";
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetPCIBusId(bus, sizeof(bus), dev);
    for (char* ch = bus; *ch; ch++) if (*ch == ':' || *ch == '/') *ch = '_';
    std::string dir = lock_dir;
    bool shared = dir.empty();
    //  a directory is trusted if it is the caller's or root's, and -- when others can write into it -- sticky: the owner
    // of a directory can unlink and replace the lock file, which would let two processes' persistent launches meet on the GPU, and a
    // foreign owner could hold the lock for ever.  The machine-wide default /tmp/liblcr-locks is used when it passes that test (this
    // user created it, or an administrator did); otherwise the lock is per user: /tmp/liblcr-<uid>.
    auto trusted = [&](const std::string& d) {
      struct stat st;
      if (lstat(d.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) return false;
      if (st.st_uid != getuid() && st.st_uid != 0) return false;
      return !(st.st_mode & 0022) || (st.st_mode & S_ISVTX) || st.st_uid == getuid();
    };
    if (shared) {
      dir = "/tmp/liblcr-locks";
      if (mkdir(dir.c_str(), 01777) == 0) (void)chmod(dir.c_str(), 01777);   // (the umask)
      //  an untrusted machine-wide directory is an error, not a silent per-user lock: whoever created it would go on
      // trusting it while everybody else locked /tmp/liblcr-<uid>, and two users' persistent launches on one GPU would no longer be
      // serialised.  The per-user lock is there for whoever asks for it: lcr_ctx_set_lock_dir(ctx, "/tmp/liblcr-<uid>").
      if (!trusted(dir)) return "the machine-wide lock directory " + dir + " exists but is not root's or this user's (or is writable by others without the sticky bit): "
                                "remove it, have an administrator create it 1777, or name a directory all processes that share this GPU see with lcr_ctx_set_lock_dir";
    }
    if (!shared && mkdir(dir.c_str(), 0700) != 0 && errno != EEXIST) return "cannot create lock directory " + dir + ": " + strerror(errno);
    if (!trusted(dir)) return "lock directory " + dir + " is not a directory of this user or of root (sticky if others may write): lcr_ctx_set_lock_dir names another one";
    const std::string path = dir + "/grid_" + bus + ".lock";
    dev_mu = &device_mutex(bus);
    dev_mu->lock();
    auto fail = [&](const std::string& e) { if (fd >= 0) { close(fd); fd = -1; } dev_mu->unlock(); dev_mu = nullptr; return e; };
    const auto t_start = std::chrono::steady_clock::now();
    for (;;) {
      fd = open(path.c_str(), O_CREAT | O_RDWR | O_NOFOLLOW | O_CLOEXEC, shared ? 0666 : 0600);
      if (fd < 0) return fail("cannot open " + path + ": " + strerror(errno));
      if (shared) { struct stat fs; if (fstat(fd, &fs) == 0 && fs.st_uid == getuid()) (void)fchmod(fd, 0666); }   // (created under a umask)
      // bounded wait (a process that died holding the lock has released it; one that hangs must not hang everybody else for ever)
      int rc;
      while ((rc = flock(fd, LOCK_EX | LOCK_NB)) != 0 && (errno == EWOULDBLOCK || errno == EINTR)) {
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() > 600.0)
          return fail("the device lock " + path + " has been held by another process for 10 minutes");
        usleep(200);
      }
      if (rc != 0) return fail("flock(" + path + "): " + strerror(errno));
      // the file we hold must still be the one the path names (it may have been unlinked and recreated between open and flock)
      struct stat fa, fb;
      if (fstat(fd, &fa) == 0 && stat(path.c_str(), &fb) == 0 && fa.st_ino == fb.st_ino && fa.st_dev == fb.st_dev) break;
      (void)flock(fd, LOCK_UN); close(fd); fd = -1;
    }
    held = true;
    return "";
  }
  ~GridLock() {
    if (!held) return;
    for (int i = 0; i < n_q; i++) (void)hipStreamSynchronize(q[i]);   // (a persistent kernel may still be running on an error path; nullptr = the null stream, drained too)
    if (fd >= 0) { (void)flock(fd, LOCK_UN); close(fd); }
    if (dev_mu) dev_mu->unlock();
  }
};

int PhaseHost::ld_blocks(const PhaseInputs& in, int region, std::vector<int32_t>* off, std::vector<int32_t>* snps, hipStream_t s, std::string* err) {
  off->assign(1, 0); snps->clear();
  for (const ChainDesc& d : chain_desc) {
    if (d.slot != region) continue;
    const int c0 = in.cand_region_off[region];
    int32_t info[2] = {0, 0};
    auto chk = [&](hipError_t e) { if (e != hipSuccess && err) *err = hipGetErrorString(e); return e == hipSuccess; };
    if (!chk(hipMemcpyAsync(info, chain_dev.blk_info + 2 * region, 8, hipMemcpyDeviceToHost, s)) || !chk(hipStreamSynchronize(s))) return LCR_E_DEVICE;
    const int nb = info[0];
    if (nb == 0) return LCR_OK;
    std::vector<int32_t> ptr(nb + 1);
    if (!chk(hipMemcpyAsync(ptr.data(), chain_dev.blk_ptr + c0 + region, (size_t)(nb + 1) * 4, hipMemcpyDeviceToHost, s)) || !chk(hipStreamSynchronize(s))) return LCR_E_DEVICE;
    std::vector<int32_t> nodes(ptr[nb]);
    if (!chk(hipMemcpyAsync(nodes.data(), chain_dev.blk_nodes + c0, (size_t)ptr[nb] * 4, hipMemcpyDeviceToHost, s)) || !chk(hipStreamSynchronize(s))) return LCR_E_DEVICE;
    for (int b = nb - 1; b >= 0; b--) {   // kosaraju_scc emits the blocks in descending order of their smallest node
      snps->insert(snps->end(), nodes.begin() + ptr[b], nodes.begin() + ptr[b + 1]);
      off->push_back((int32_t)snps->size());
    }
    return LCR_OK;
  }
  return LCR_OK;   // not a chain region: no blocks are built (phase.rs:1097-1122 never looks at them)
}

#define PCHK_TO(err_, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { if (err_) *(err_) = std::string(#expr) + ": " + hipGetErrorString(e_); return LCR_E_DEVICE; } } while (0)
#define PCHK(expr) PCHK_TO(c.err, expr)   // (in the steps of run())
#define RCHK(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)
// collects what the last run() left in flight: waits for its queues, fetches the tie census, copies the candidates' updated
// records and the objectives out of the pinned blocks k4_post wrote (the per-row results are read in place)
int PhaseHost::settle(std::string* err) {
  if (!pending) return LCR_OK;
  pending = false;
  PCHK_TO(err, hipStreamSynchronize(side));
  PCHK_TO(err, hipMemcpyAsync(h_census.p, d_tie.p, TIE_NCTR * 8, hipMemcpyDeviceToHost, q_first));   // (`side` is drained: every kernel that counts is done or ahead in the first queue)
  PCHK_TO(err, hipStreamSynchronize(q_first));
  PCHK_TO(err, hipGetLastError());
  memcpy(tie_census, h_census.p, TIE_NCTR * 8);
  uint8_t* const h_r = h_res.as<uint8_t>();
  const long long* const h_obj = (const long long*)(h_cand_obj.as<uint8_t>() + pend.hc_obj);
  std::vector<lcr_candidate>& cand = *pend.cand;
  for (int g = 0; g < pend.ng; g++) {
    const int c0 = pend.cand_off[g], S = pend.cand_off[g + 1] - c0;
    if (S == 0) continue;
    memcpy(cand.data() + c0, h_cand_obj.as<lcr_candidate>() + c0, (size_t)S * sizeof(lcr_candidate));
    objective[g] = (double)h_obj[g] / FX_SCALE;
  }
  r_haplotag = (int8_t*)(h_r + pend.res_tag); r_assignment = h_r + pend.res_asg; r_phase_set = (uint32_t*)(h_r + pend.res_ps);
  return LCR_OK;
}

// the repair pass of the enumeration branch (k4_enum_redo): per launch queue a list of REDO_CAP restarts, REDO_GRID workgroups
constexpr uint32_t REDO_CAP = 8192, REDO_GRID = 512;
constexpr uint32_t ENUM_STREAM_PER_WAVE = 2;   // restarts per wave of the streaming class (k4_enum_reg; 3, 4 measured: noise)

// The values of one run() call, shared by its steps; it lives in run()'s frame.
struct PhaseCall {
  const PhaseInputs& in; const lcr_params& prm; std::string* const err;
  const hipStream_t sq;   // the caller's stream: the fills and the staging kernel, the host waits for the sizes there
  const int ng, nrow, ncand; const int64_t nnz; const size_t nnz1, nc1, nr1; const bool prof;
  std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
  bool async_mode = false; hipStream_t stream = nullptr;   // the stage's first queue: the caller's stream, or main_q under async_phase
  // state: sigma[n_rows] | delta[n_cand] | eta[n_cand] | obj[n_regions] (8-byte aligned); one copy per queue
  size_t st_sig = 0, st_del = 0, st_eta = 0, st_obj = 0, st_bytes = 0;
  // results of the device epilogue in pinned host memory: phase set u32 | haplotag | assignment, and candidate mirror | objectives
  size_t res_ps = 0, res_tag = 0, res_asg = 0, res_bytes = 0, hc_obj = 0;
  PhaseDev P{}, Pc{};     // the enumeration and the chain regions (each with its own copy of the state arrays)
  PostIn pin{}, pinc{}; PostLut plut;   // k4_post / k4_gpost of the enumeration and of the chain regions
  StageIn si{}; StageOut so{};
  int64_t grid_min = 0; StageStat* stat = nullptr;   // per-region sizes, written by k4_stage into pinned host memory
  std::vector<int32_t> enum_slots, chain_slots, gpost_slots, gstage_slots;
  std::vector<uint8_t> grid_post;   // per region: k4_gpost
  uint32_t post_lds = 0;
  size_t gp_S = 1, gp_rows = 1, gp_E = 1;   // largest region image of k4_gpost
  GridLock grid_lock;   // held from the first persistent launch until run() returns (all queues are drained by then)
  PhaseCall(const PhaseInputs& in_, const lcr_params& prm_, hipStream_t user_stream, std::string* err_, bool prof_)
      : in(in_), prm(prm_), err(err_), sq(user_stream), ng(in_.n_regions), nrow(in_.n_rows), ncand(in_.cand_region_off[in_.n_regions]),
        nnz(in_.nnz), nnz1((size_t)std::max<int64_t>(nnz, 1)), nc1((size_t)std::max(ncand, 1)), nr1((size_t)std::max(nrow, 1)), prof(prof_) {}
  void lap(const char* what) { if (!prof) return; auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[phase] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count()); t_last = t; }
  int lock_grid(const PhaseHost& h) {   // the device lock of the persistent launches, taken by the first of them
    const std::string e = grid_lock.acquire(h.lock_dir, stream, h.side, h.aux);
    if (!e.empty() && err) *err = "device lock of the persistent launches: " + e;
    return e.empty() ? LCR_OK : LCR_E_DEVICE;
  }
};

int PhaseHost::run(const PhaseInputs& in, const lcr_params& prm, hipStream_t user_stream, std::string* err) {
  RCHK(settle(err));   // (a previous call nobody asked about: its pinned blocks are rewritten below)
  HT("phase");
  // Two queues: `stream` stages the phase matrices and runs the enumeration regions (S <= max_enum_snps) with their
  // post-phase kernel; `side` runs the chain regions (S > max_enum_snps): LD blocks, LD-seeded start, block-flip pass
  // and perturbation rounds in ONE kernel per region class (k4_grid.hip: a workgroup per region, or all CUs on one
  // large region), then their post-phase kernel.  The host only sizes buffers and launches.
  PhaseCall c(in, prm, user_stream, err, dbg.prof != 0);
  objective.assign(c.ng, 0.0);
  RCHK(open_queues(c));
  RCHK(size_buffers(c));
  RCHK(sample(c));
  RCHK(stage(c));
  RCHK(classify(c));
  RCHK(wait_sizes(c));
  // Order of the two queues' launches: the enumeration tiles (thousands of four-wave workgroups) and the chain regions'
  // sixteen-wave workgroups (a CU's worth of LDS and wave slots each) compete for the same CUs, and whoever is launched
  // second only finds room as the first drains.  The enumeration goes first: its host preparation ends ~50 us earlier that
  // way, and its kernel + k4_enum_resolve + k4_post are the critical path (round 4: C3 2.48 -> 2.44 ms, C4 5.59 -> 5.57).
  RCHK(launch_enum(c));
  HT("ph:enum_q");
  RCHK(launch_chain(c));
  c.lap("enum launch");
  RCHK(launch_gpost(c));
  c.lap("chain launch");
  if (!mark_pending(c)) return LCR_OK;
  PCHK_TO(err, hipStreamSynchronize(side));
  c.lap("chain kernels");
  RCHK(settle(err));
  c.lap("enumeration kernels");
  if (c.prof) RCHK(report_prof(c));
  c.lap("results");
  return LCR_OK;
}

// async_phase (opt-in): everything is queued on the stage's OWN first queue, behind what the caller's stream holds now (the
// fragment stage's kernels), and the call returns without waiting.  Default: the caller's stream, results collected before the
// call returns -- measured on C3 (profiles/r05_async_phase.txt): the next batch's pileup then time-shares the CUs with the
// restarts (K0 214 -> 385 us, k4_enum_reg<32> 647 -> 1142 us), the resolve / post-phase tails stay exposed because the next
// lcr_candidates has to wait for this stage anyway, and a fourth stream of the process pushes `side` and `aux` onto one hardware
// queue: 2.19 -> 2.12 ms per step, and the pileup kernels' own durations (the roofline's measurement) grow by half.
int PhaseHost::open_queues(PhaseCall& c) {
  c.async_mode = dbg.async_phase != 0;
  if (c.async_mode && !main_q) PCHK(hipStreamCreateWithFlags(&main_q, hipStreamNonBlocking));
  if (!ev_user) { PCHK(hipEventCreateWithFlags(&ev_user, hipEventDisableTiming)); PCHK(hipEventCreateWithFlags(&ev_gate[0], hipEventDisableTiming)); PCHK(hipEventCreateWithFlags(&ev_gate[1], hipEventDisableTiming)); }
  gate_set[0] = gate_set[1] = false;
  c.stream = c.async_mode ? main_q : c.sq;
  // (round 6) the staging kernel and the fills in front of it stay on the CALLER's queue (c.sq) -- right behind the fragment stage's
  // kernels, no queue-to-queue hand-over in front of them (16 us on this platform) --, the host waits for the sizes there, and the
  // stage's own queue picks up behind an event that is long complete when the first restarts are queued
  q_first = c.stream;
  if (!side) {
    PCHK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    PCHK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
    PCHK(hipEventCreateWithFlags(&ev_csr, hipEventDisableTiming));
    PCHK(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking));
    PCHK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    PCHK(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
  }
  return LCR_OK;
}

// device and pinned buffers of the call, the kernels' argument blocks, and the stage's fills in one launch
int PhaseHost::size_buffers(PhaseCall& c) {
  const int ng = c.ng; const size_t nnz1 = c.nnz1, nc1 = c.nc1, nr1 = c.nr1;
  const HostLut& L = hlut();
  PCHK(d_reg.reserve((size_t)std::max(ng, 1) * sizeof(RegionDev)));
  PCHK(d_prow_ptr.reserve((nr1 + ng + 1) * 4)); PCHK(d_pcol.reserve(nnz1 * 4)); PCHK(d_pval.reserve(nnz1));
  PCHK(d_ccol_ptr.reserve((nc1 + ng + 1) * 4)); PCHK(d_crow.reserve(nnz1 * 4)); PCHK(d_cval.reserve(nnz1));
  PCHK(d_snp.reserve(nc1 * 3 + 16)); PCHK(d_snp_const.reserve(nc1 * 4 * sizeof(long long))); PCHK(d_cur.reserve(nc1 * 4));
  PCHK(d_prow_src.reserve(nr1 * 4));
  c.st_sig = 0; c.st_del = (nr1 + 15) & ~(size_t)15; c.st_eta = c.st_del + ((nc1 + 15) & ~(size_t)15);
  c.st_obj = c.st_eta + ((nc1 + 15) & ~(size_t)15); c.st_bytes = c.st_obj + (size_t)std::max(ng, 1) * 8;
  PCHK(d_st_enum.reserve(c.st_bytes + 16)); PCHK(d_st_chain.reserve(c.st_bytes + 16));
  PCHK(h_stat.reserve((size_t)std::max(ng, 1) * sizeof(StageStat)));
  // k4_post writes its results into pinned host memory itself (every row belongs to a region with candidates, fragment.rs:24-26,
  // so every row is written)
  c.res_ps = 0; c.res_tag = nr1 * 4; c.res_asg = nr1 * 5; c.res_bytes = nr1 * 6;
  c.hc_obj = (nc1 * sizeof(lcr_candidate) + 15) & ~(size_t)15;
  PCHK(h_res.reserve(c.res_bytes)); PCHK(h_cand_obj.reserve(c.hc_obj + (size_t)std::max(ng, 1) * 8));
  PCHK(d_read_rec.reserve(nr1 * 12));   // per-row results once more, as records in HBM (lcr_get_read_records_device)
  uint8_t* d_res = nullptr; uint8_t* d_hc = nullptr;   // device-side addresses of the two pinned blocks
  PCHK(hipHostGetDevicePointer((void**)&d_res, h_res.p, 0));
  PCHK(hipHostGetDevicePointer((void**)&d_hc, h_cand_obj.p, 0));

  PhaseDev& P = c.P;
  P.reg = d_reg.as<RegionDev>();
  P.prow_ptr = d_prow_ptr.as<int32_t>(); P.pcol = d_pcol.as<int32_t>(); P.pval = d_pval.as<uint8_t>();
  P.ccol_ptr = d_ccol_ptr.as<int32_t>(); P.crow = d_crow.as<int32_t>(); P.cval = d_cval.as<uint8_t>();
  P.snp_const = d_snp_const.as<long long>();
  P.snp_fp = d_snp.as<uint8_t>(); P.snp_vt = d_snp.as<int8_t>() + nc1; P.snp_cons = d_snp.as<uint8_t>() + 2 * nc1;
  P.st_sigma = d_st_enum.as<int8_t>() + c.st_sig; P.st_delta = d_st_enum.as<int8_t>() + c.st_del; P.st_eta = d_st_enum.as<int8_t>() + c.st_eta;
  P.st_obj = (long long*)(d_st_enum.as<int8_t>() + c.st_obj);
  P.lut = L.dev;
  PostLut& plut = c.plut;
  for (int q = 0; q < 31; q++) { plut.le[q] = L.le[q]; plut.l1e[q] = L.l1e[q]; }
  plut.p_homref = L.p_homref; plut.p_homvar = L.p_homvar; plut.log_theta = L.log_theta; plut.log2 = L.log2;
  PCHK(d_lut64.reserve(sizeof(PostLut))); PCHK(d_tie.reserve(TIE_NCTR * 8)); PCHK(h_census.reserve(TIE_NCTR * 8));
  if (!lut64_ready) { PCHK(hipMemcpyAsync(d_lut64.p, &plut, sizeof(PostLut), hipMemcpyHostToDevice, c.sq)); PCHK(hipStreamSynchronize(c.sq)); lut64_ready = true; }
  // the stage's fills in ONE launch in front of the staging kernel (the host's wait for the sizes ends with that kernel, and every command
  // between it and the first restart is idle GPU time): the tie census, the result state, the enumeration branch's best objective seen per
  // region (0x8080...: far below any objective) and the repair lists' counts (the pairs behind them are written before they are read)
  PCHK(d_en_rbest.reserve((size_t)std::max(ng, 1) * 8 + 64));
  if (dbg.tie_arith >= 3) PCHK(d_en_redo.reserve(2 * (16 + 8 * (size_t)REDO_CAP) + 64));
  { void* const fp[4] = {d_tie.p, d_st_enum.p, d_en_rbest.p, d_en_redo.p};
    const int fv[4] = {0, 0, 0x80, 0};
    const size_t fs[4] = {TIE_NCTR * 8, ng ? c.st_bytes : 0, (size_t)ng * 8, dbg.tie_arith >= 3 ? 2 * (16 + 8 * (size_t)REDO_CAP) : 0};
    PCHK(lcr_fill_multi_async(4, fp, fv, fs, c.sq)); }
  P.lut64 = d_lut64.as<PostLut>(); P.tie_ctr = d_tie.as<unsigned long long>(); P.tie_arith = dbg.tie_arith; P.enum_elide = dbg.enum_elide;

  c.Pc = P;
  c.Pc.st_sigma = d_st_chain.as<int8_t>() + c.st_sig; c.Pc.st_delta = d_st_chain.as<int8_t>() + c.st_del; c.Pc.st_eta = d_st_chain.as<int8_t>() + c.st_eta;
  c.Pc.st_obj = (long long*)(d_st_chain.as<int8_t>() + c.st_obj);
  const PhaseInputs& in = c.in; const lcr_params& prm = c.prm;
  c.pin = PostIn{in.d_row_ptr, in.d_col, in.d_val, in.d_row_links, const_cast<lcr_candidate*>(in.d_cand), in.d_cand_off,
                 in.d_row_region_off, in.d_start0, P.st_sigma, P.st_delta, P.st_eta, (int8_t*)(d_res + c.res_tag), d_res + c.res_asg,
                 (uint32_t*)(d_res + c.res_ps), d_read_rec.as<uint32_t>(), P.st_obj, (long long*)(d_hc + c.hc_obj), (lcr_candidate*)d_hc,
                 prm.min_linkers, prm.max_enum_snps, prm.seed, prm.read_assign_cutoff, prm.min_phase_score, nullptr, P.reg, d_prow_src.as<int32_t>()};
  c.pinc = c.pin;
  c.pinc.st_sigma = c.Pc.st_sigma; c.pinc.st_delta = c.Pc.st_delta; c.pinc.st_eta = c.Pc.st_eta; c.pinc.st_obj = c.Pc.st_obj;
  return LCR_OK;
}

// Down-sampling (thread.rs:144-151): a region applies when it has at least ds_depth fragment rows (all rows of lcr_get_fragmat, empty
// ones included) -- or, with the caller's own bytes, when one of its rows is unsampled (a region whose rows are all sampled behaves as
// with the feature off).  k4_sample writes the bytes of the regions that apply, the others' are 1.  No region applies: nothing is
// launched and every kernel gets null pointers -- exactly the call with the feature off.
int PhaseHost::sample(PhaseCall& c) {
  const PhaseInputs& in = c.in;
  ds_applied.assign((size_t)std::max(c.ng, 1), 0); ds_any = false;
  ds_ng = (int32_t)c.ng; ds_nrow = (int32_t)c.nrow;
  if (!in.ds_rows && in.ds_depth == 0) return LCR_OK;
  PCHK(h_smp_slots.reserve((size_t)std::max(c.ng, 1) * 4));
  int32_t* const slots = h_smp_slots.as<int32_t>();
  int n = 0;
  for (int g = 0; g < c.ng; g++) {
    const int r0 = in.row_region_off[g], F = in.row_region_off[g + 1] - r0;
    bool app = false;
    if (in.ds_rows) app = F > 0 && memchr(in.ds_rows + r0, 0, (size_t)F) != nullptr;
    else app = F > 0 && (uint32_t)F >= in.ds_depth;
    if (app) { ds_applied[g] = 1; slots[n++] = g; }
  }
  if (!n) return LCR_OK;
  ds_any = true;
  PCHK(d_sampled.reserve(c.nr1)); PCHK(h_sampled.reserve(c.nr1)); PCHK(d_prow_ord.reserve(c.nr1 * 4));
  if (in.ds_rows) {
    memcpy(h_sampled.p, in.ds_rows, (size_t)c.nrow);
    PCHK(hipMemcpyAsync(d_sampled.p, h_sampled.p, (size_t)c.nrow, hipMemcpyHostToDevice, c.sq));
  } else {
    int32_t* d_slots = nullptr;
    PCHK(hipHostGetDevicePointer((void**)&d_slots, slots, 0));
    PCHK(lcr_fill_async(d_sampled.p, 1, (size_t)c.nrow, c.sq));
    launch_k4_sample(n, d_slots, in.d_row_region_off, in.d_start0, in.ds_depth, in.ds_seed, d_sampled.as<uint8_t>(), c.sq);
    PCHK(hipGetLastError());
    PCHK(hipMemcpyAsync(h_sampled.p, d_sampled.p, (size_t)c.nrow, hipMemcpyDeviceToHost, c.sq));   // (complete when the host has the staging kernel's sizes)
  }
  c.P.draw_ord = c.Pc.draw_ord = d_prow_ord.as<int32_t>();
  c.pin.sampled = c.pinc.sampled = d_sampled.as<uint8_t>();
  return LCR_OK;
}

// k4_stage on the caller's queue -- launched before the host sorts the regions into their kernel classes (the device would idle for
// that long); the per-region sizes arrive in pinned host memory
int PhaseHost::stage(PhaseCall& c) {
  const PhaseInputs& in = c.in;
  c.grid_min = dbg.grid_min >= 0 ? dbg.grid_min : (1 << 17);   // chain regions with at least this many phase entries get all CUs (tests: 0 = every region)
  c.stat = h_stat.as<StageStat>();
  c.si = StageIn{in.d_row_ptr, in.d_col, in.d_val, in.d_row_links, in.d_cand, in.d_cand_off, in.d_row_region_off, in.d_start0,
                 c.prm.min_linkers, c.prm.max_enum_snps, c.prm.seed, std::max<int64_t>(c.grid_min, 1), ds_any ? d_sampled.as<uint8_t>() : nullptr};
  if (!c.ng) return LCR_OK;
  StageStat* d_stat = nullptr;   // the per-region sizes go straight into pinned host memory (no copy behind the staging kernels)
  PCHK(hipHostGetDevicePointer((void**)&d_stat, c.stat, 0));
  c.so = StageOut{d_reg.as<RegionDev>(), d_stat, d_prow_ptr.as<int32_t>(), d_pcol.as<int32_t>(), d_pval.as<uint8_t>(),
                  d_ccol_ptr.as<int32_t>(), d_crow.as<int32_t>(), d_cval.as<uint8_t>(), d_snp.as<uint8_t>(), d_snp.as<int8_t>() + c.nc1,
                  d_snp.as<uint8_t>() + 2 * c.nc1, d_snp_const.as<long long>(), d_cur.as<int32_t>(), d_prow_src.as<int32_t>(),
                  ds_any ? d_prow_ord.as<int32_t>() : nullptr};
  launch_k4_stage((int32_t)c.ng, c.sq, c.si, c.so, hlut().dev);
  PCHK(hipGetLastError());
  HT("  ph:stage_q");
  return LCR_OK;
}

// enumeration (S <= max_enum_snps) and chain regions; the post-phase epilogue of every region: k4_post (a workgroup per region, the
// region in LDS) where it fits its LDS image, else k4_gpost (all CUs on the region).  The regions' sizes are on the host already
// (lcr_fragments), so this is known before anything is queued.
int PhaseHost::classify(PhaseCall& c) {
  const PhaseInputs& in = c.in;
  for (int g = 0; g < c.ng; g++) {
    const int S = in.snps(g);
    if (S == 0) continue;
    if ((uint32_t)S <= c.prm.max_enum_snps) c.enum_slots.push_back(g); else c.chain_slots.push_back(g);
  }
  c.grid_post.assign(c.ng, 0);
  for (int g = 0; g < c.ng; g++) {
    const int S = in.snps(g);
    if (S == 0) continue;
    const int nr_g = in.row_region_off[g + 1] - in.row_region_off[g];
    const int64_t E_all = in.region_e_off[g + 1] - in.region_e_off[g];
    if (E_all > INT_MAX - 64) { if (c.err) *c.err = "a region's fragment matrix has more than 2^31 entries"; return LCR_E_ARG; }
    if (E_all >= std::max<int64_t>(c.grid_min, 1)) c.gstage_slots.push_back(g);
    bool fits = !(nr_g > POST_MAX_ROWS || E_all > POST_MAX_ENTRIES || S > POST_MAX_SNPS);
    uint32_t need = 0;
    if (fits) { need = post_layout(nr_g, (uint32_t)E_all, S).total; if (need > 64 * 1024) fits = false; }
    if (!fits || (c.grid_min == 0 && (uint32_t)S > c.prm.max_enum_snps)) {
      c.grid_post[g] = 1; c.gpost_slots.push_back(g);
      c.gp_S = std::max(c.gp_S, (size_t)S); c.gp_rows = std::max(c.gp_rows, (size_t)nr_g); c.gp_E = std::max(c.gp_E, (size_t)E_all);
    } else c.post_lds = std::max(c.post_lds, need);
  }
  return LCR_OK;
}

// queue `side`: the large regions' staging with all CUs; then the host waits for the per-region sizes
int PhaseHost::wait_sizes(PhaseCall& c) {
  hipStream_t const sq = c.sq;
  PCHK(hipEventRecord(ev_in, sq));
  PCHK(hipStreamWaitEvent(side, ev_in, 0));
  if (c.ng) {
    if (!c.gstage_slots.empty()) {   // large regions: all CUs on one region at a time (every persistent launch goes to `side`)
      RCHK(c.lock_grid(*this));
      PCHK(d_grid_ctl.reserve((4 + 16) * sizeof(GridCtl))); PCHK(d_grid_tot.reserve((size_t)(3 * std::max(1, k4_grid_blocks()) + 1) * 4 + 64));
      for (int g : c.gstage_slots) PCHK(k4_stage_launch_grid(c.si, c.so, hlut().dev, g, d_grid_ctl.as<GridCtl>(), d_grid_tot.as<int32_t>(), side));
      PCHK(hipEventRecord(ev_join, side));
      PCHK(hipStreamWaitEvent(sq, ev_join, 0));
    }
    PCHK(hipEventRecord(ev_csr, sq));   // the chain kernels on `side` read the staged matrices
  }
  if (c.async_mode) { PCHK(hipEventRecord(ev_user, sq)); PCHK(hipStreamWaitEvent(c.stream, ev_user, 0)); }
  HT("ph:presync");
  if (c.ng) PCHK(hipStreamSynchronize(sq));
  HT("ph:synced");
  c.lap("stage + sizes");
  const size_t clk_bytes = ((size_t)(c.ng + 1) * 16 + 2 * 1024) * 8;   // phase_prof: k4_post's step clocks, then the chain kernels' (launch_chain)
  if (c.prof) { PCHK(d_prof_clk.reserve(clk_bytes)); PCHK(hipMemsetAsync(d_prof_clk.p, 0, clk_bytes, c.stream)); c.pin.dbg_clk = c.pinc.dbg_clk = d_prof_clk.as<long long>(); }
  return LCR_OK;
}

// enumeration regions: all restarts in one launch per class, then k4_enum_resolve per class (the winner's state is taken from what its
// restart left; only the global-memory class re-runs its winner)
int PhaseHost::launch_enum(PhaseCall& c) {
  if (c.enum_slots.empty()) return LCR_OK;
  const PhaseInputs& in = c.in; const int ng = c.ng; const StageStat* const stat = c.stat;
  std::vector<int32_t>& enum_slots = c.enum_slots; PhaseDev& P = c.P; hipStream_t const stream = c.stream;
  // heaviest regions first (tiles are started in grid order: the kernel's tail should be the light ones; the post-phase
  // kernel's workgroups follow the same order)
  // (this block is on the critical path -- the device idles between k4_stage and the first restart: one sort of packed keys,
  // one layout computation per region, no allocation beyond the lists themselves: 48 -> ~10 us for C3's 366 regions)
  {
    std::vector<uint64_t>& key = enum_keys;   // descending E, ties in ascending region order (= the stable sort it replaces)
    key.resize(enum_slots.size());
    for (size_t k = 0; k < enum_slots.size(); k++) key[k] = ((uint64_t)(0xffffffffu - (uint32_t)stat[enum_slots[k]].E) << 32) | (uint32_t)enum_slots[k];
    std::sort(key.begin(), key.end());
    for (size_t k = 0; k < enum_slots.size(); k++) enum_slots[k] = (int32_t)(uint32_t)key[k];
  }
  HT("en:sorted");
  int32_t max_state = 0;
  for (int g : enum_slots) max_state = std::max(max_state, stat[g].R + 2 * in.snps(g));
  const int32_t stride = (max_state + 63) & ~63;
  P.scratch_stride = stride;
  const bool force_big = dbg.enum_force_big != 0;        // test hooks: exercise the fallback kernels
  const bool force_stream = dbg.enum_force_stream != 0;
  // kernel classes: CL_BITS = k4_enum_bits (eight restarts per wave as bit states) where its image (a sigma byte per row and wave)
  // fits LDS; CL_STREAM = k4_enum_reg (one restart per wave, the entries streamed from LDS) for the LDS-resident regions beyond that
  // image, in a launch of its own beside CL_BITS (behind it on one queue they were 0.68 ms of the C4 share's critical path);
  // CL_BIG = k4_enum_big, global memory (matrix larger than the LDS budget)
  enum { CL_STREAM, CL_BITS, CL_BIG, NCLS };
  std::vector<EnumSpan> spans[NCLS];
  spans[CL_STREAM].reserve(enum_slots.size()); spans[CL_BITS].reserve(enum_slots.size());
  size_t n_t[NCLS] = {0, 0, 0};   // tiles per class = grid of the class's kernel
  const uint32_t per_of[NCLS] = {ENUM_STREAM_PER_WAVE * ENUM_WAVES, ENUM_BITS_PER, 1u};
  std::vector<int64_t>& job_base = enum_job_base; std::vector<int64_t>& st_base = enum_st_base;   // st_base: first word of the region's saved restart states
  job_base.assign(ng, 0); st_base.assign(ng, 0);
  int64_t nj = 0, st_words = 0, big_words = 0, big_emax = 0;
  uint32_t lds_need[NCLS] = {0, 0, 0}, res_lds[NCLS] = {0, 0, 0};   // (res_lds: k4_enum_resolve's image of the class's largest region)
  // enumeration regions with the device epilogue: those of the bit-state class are post-processed on its queue right behind its
  // resolve kernel, beside the streaming class's; the others behind everything on `stream`
  std::vector<int32_t> post_slots, post_slots_b, post_slots_c;   // (c: the global-memory class, behind its winners' second launch)
  post_slots.reserve(enum_slots.size());
  for (int g : enum_slots) {
    const int S = in.snps(g);
    const StageStat& st = stat[g];
    const EnumLayout EL_stream = enum_layout(st.R, st.E), EL_bits = enum_layout(st.R, st.E, true, (uint32_t)std::min(S, 32));
    const bool use_bits = !force_stream && S <= 31 && EL_bits.total <= ENUM_LDS_MAX;
    const EnumLayout EL = use_bits ? EL_bits : EL_stream;
    const uint32_t RL = resolve_layout((uint32_t)st.R, (uint32_t)st.E, (uint32_t)S).total;
    int cls = CL_BIG;
    if (!force_big && st.R < 65536 && st.E < 65536 && S <= 31 && EL.total <= ENUM_LDS_MAX && RL <= ENUM_LDS_MAX && st.max_rows <= 64)
      cls = use_bits ? CL_BITS : CL_STREAM;
    //  the saved restart states of the LDS classes are allocated up front: a raised max_enum_snps (2^20 restarts x
    // R / 64 + 3 words) goes to the global-memory class instead, whose states are kept only inside a budget
    if (cls != CL_BIG && (int64_t)((uint64_t)1 << std::min(S, 62)) * enum_state_words((uint32_t)st.R) > ((int64_t)1 << 27)) cls = CL_BIG;
    if (cls != CL_BIG) { lds_need[cls] = std::max(lds_need[cls], EL.total); res_lds[cls] = std::max(res_lds[cls], RL); }
    job_base[g] = nj;
    const uint64_t n = 1ull << S;
    // saved restart states: every region of the LDS classes; of the global-memory class while they fit a budget of 2^26 words
    // (512 MB -- beyond it that region's equal-objective restarts fall to "first maximum", counted as unresolved)
    st_base[g] = -1;
    if (cls != CL_BIG) { st_base[g] = st_words; st_words += (int64_t)n * enum_state_words((uint32_t)st.R); }
    else if ((int64_t)n * enum_state_words((uint32_t)st.R) <= ((int64_t)1 << 26) - big_words) {
      st_base[g] = st_words; st_words += (int64_t)n * enum_state_words((uint32_t)st.R); big_words += (int64_t)n * enum_state_words((uint32_t)st.R);
      big_emax = std::max<int64_t>(big_emax, st.E);
    }
    if (n_t[cls] + (n + per_of[cls] - 1) / per_of[cls] > 0x7fffffffull) { if (c.err) *c.err = "too many enumeration restarts for one launch"; return LCR_E_ARG; }
    spans[cls].push_back({g, (uint32_t)n_t[cls]});
    n_t[cls] += (size_t)((n + per_of[cls] - 1) / per_of[cls]);
    nj += (int64_t)n;
    if (!c.grid_post[g]) (cls == CL_BITS ? post_slots_b : (cls == CL_BIG ? post_slots_c : post_slots)).push_back(g);
    if (c.prof && cls == CL_BIG) fprintf(stderr, "[phase]   global-memory enumeration region %d: R %d E %d S %d max_rows %d max_n %d, LDS image %u B\n", g, st.R, st.E, S, st.max_rows, st.max_n, EL.total);
  }
  if (c.prof) fprintf(stderr, "[phase]   enumeration classes: bit states %zu regions / %zu tiles, streaming %zu / %zu, global %zu / %zu\n",
                      spans[CL_BITS].size(), n_t[CL_BITS], spans[CL_STREAM].size(), n_t[CL_STREAM], spans[CL_BIG].size(), n_t[CL_BIG]);
  // one upload: spans of every class | job_base | slots | post slots ; then job objectives and winners
  size_t n_w[NCLS], s_off[NCLS], n_spans = 0;
  for (int k = 0; k < NCLS; k++) { n_w[k] = spans[k].size(); s_off[k] = n_spans; n_spans += n_w[k]; }
  const size_t ns = enum_slots.size(), nps_a = post_slots.size(), nps_b = post_slots_b.size(), nps_c = post_slots_c.size(), nps = nps_a + nps_b + nps_c;
  const size_t off_jb_al = (n_spans * sizeof(EnumSpan) + 7) & ~(size_t)7;
  const size_t off_sb = off_jb_al + (size_t)ng * 8;   // st_base
  const size_t up_bytes = off_sb + (size_t)ng * 8 + (ns + nps) * 4;
  HT("en:classes");
  PCHK(d_en_st.reserve((size_t)std::max<int64_t>(st_words, 1) * 8));
  PCHK(d_en_job.reserve(up_bytes + 64));
  PCHK(d_en_obj.reserve((size_t)nj * 8 + (size_t)ng * 8 + (size_t)ng * 8 + 64));   // objectives | winners | tiles done | best objective seen per region
  PCHK(h_en_up.reserve(up_bytes + 64));   // pinned: the upload is queued, not staged
  uint8_t* const up = h_en_up.as<uint8_t>();
  for (int k = 0; k < NCLS; k++) memcpy(up + s_off[k] * sizeof(EnumSpan), spans[k].data(), n_w[k] * sizeof(EnumSpan));
  memcpy(up + off_jb_al, job_base.data(), (size_t)ng * 8);
  memcpy(up + off_sb, st_base.data(), (size_t)ng * 8);
  memcpy(up + off_sb + (size_t)ng * 8, enum_slots.data(), ns * 4);
  memcpy(up + off_sb + (size_t)ng * 8 + ns * 4, post_slots.data(), nps_a * 4);
  memcpy(up + off_sb + (size_t)ng * 8 + (ns + nps_a) * 4, post_slots_b.data(), nps_b * 4);
  memcpy(up + off_sb + (size_t)ng * 8 + (ns + nps_a + nps_b) * 4, post_slots_c.data(), nps_c * 4);
  PCHK(hipMemcpyAsync(d_en_job.p, up, up_bytes, hipMemcpyHostToDevice, stream));
  HT("en:up_q");
  const EnumSpan* d_sp = d_en_job.as<EnumSpan>();
  const int64_t* d_jb = (const int64_t*)(d_en_job.as<uint8_t>() + off_jb_al);
  const int64_t* d_sb = (const int64_t*)(d_en_job.as<uint8_t>() + off_sb);
  const int32_t* d_sl = (const int32_t*)(d_en_job.as<uint8_t>() + off_sb + (size_t)ng * 8);
  const int32_t* d_psl = d_sl + ns;
  long long* d_obj = d_en_obj.as<long long>();
  uint32_t* d_win = (uint32_t*)(d_obj + nj);
  const size_t n_big_blocks = std::max(n_t[CL_BIG], n_w[CL_BIG]);
  // the repair pass (tie classes 2 / 4 met by a fast kernel's restart): per launch queue a list of REDO_CAP restarts and REDO_GRID
  // workgroups' worth of state scratch + score scratch (2 doubles per row), behind the global-memory class's own
  const bool full_ties = dbg.tie_arith >= 3;
  int32_t max_rows_any = 1;
  for (int g : enum_slots) max_rows_any = std::max(max_rows_any, stat[g].R);
  const int64_t qstride = ((int64_t)2 * max_rows_any + 15) & ~(int64_t)15;
  const size_t n_scr_blocks = n_big_blocks + 2 * (size_t)REDO_GRID;
  PCHK(d_en_scr.reserve((size_t)stride * n_scr_blocks + 64));
  P.scratch = d_en_scr.as<int8_t>();
  if (full_ties) PCHK(d_en_qrow.reserve((size_t)qstride * n_scr_blocks * 8 + 64));
  uint32_t* const redo_a = full_ties ? d_en_redo.as<uint32_t>() : nullptr;                          // the streaming class (first queue)
  uint32_t* const redo_b = full_ties ? d_en_redo.as<uint32_t>() + 4 + 2 * REDO_CAP : nullptr;       // the bit-state class (`aux`)
  double* const qrow_all = full_ties ? d_en_qrow.as<double>() : nullptr;
  auto launch_redo = [&](uint32_t* redo, int which, hipStream_t q) {
    if (!redo) return;
    const size_t b0 = n_big_blocks + (size_t)which * REDO_GRID;
    launch_k4_enum_redo(REDO_GRID, q, P, redo, REDO_CAP, d_en_scr.as<int8_t>() + (size_t)stride * b0, stride, qrow_all + (size_t)qstride * b0, qstride,
                        d_jb, d_obj, d_sb, d_en_st.as<unsigned long long>(),
                        // (the matrix in LDS where it fits -- not for the streaming class's queue: its matrices are the largest, and that
                        // launch runs beside the bit-state kernel, where 512 workgroups asking for 64 KB each wait for it to drain even
                        // when the list is empty: 5 us -> 0.98 ms on the C4 share)
                        which == 0 ? 0u : (uint32_t)std::max(0, dbg.redo_lds));
  };
  // the classes touch disjoint regions: the streaming class on `stream`, the bit-state and global-memory classes beside it on `aux`
  // (their tails overlap)
  long long* const d_rbest = d_en_rbest.as<long long>();   // (filled in front of the staging kernel)
  unsigned long long* const d_st = d_en_st.as<unsigned long long>();
  const uint32_t post_lds = c.post_lds; const PostIn& pin = c.pin; const PostLut& plut = c.plut;
  auto launch = [&](const size_t* cnt, const uint32_t* win) -> hipError_t {
    const bool fork = cnt[CL_STREAM] && (cnt[CL_BITS] || cnt[CL_BIG]);
    hipStream_t const qb = fork ? aux : stream;
    hipError_t e = hipSuccess;
    if (fork) { if ((e = hipEventRecord(ev_fork, stream)) != hipSuccess) return e; if ((e = hipStreamWaitEvent(aux, ev_fork, 0)) != hipSuccess) return e; }
    // per class all restarts, then `prob > largest_prob` over each region's restarts from the objectives, signatures and states they
    // left (phase.rs:1113-1119; ties between configurations of maximal objective by their f64 sums) -- a workgroup per region -- and
    // the post-phase kernel of the class's regions, each behind its own restarts on its own queue
    if (cnt[CL_STREAM]) {   // (first: the largest matrices have the longest restarts)
      launch_k4_enum_reg((unsigned)cnt[CL_STREAM], lds_need[CL_STREAM], stream, P, d_sp + s_off[CL_STREAM], (int32_t)n_w[CL_STREAM], per_of[CL_STREAM], d_jb, d_obj, d_sb, d_st, d_rbest, redo_a, REDO_CAP);
      if (!win) {
        launch_redo(redo_a, 0, stream);
        launch_k4_enum_resolve((unsigned)n_w[CL_STREAM], res_lds[CL_STREAM], stream, P, d_sp + s_off[CL_STREAM], d_jb, d_obj, d_sb, d_st);
      }
    }
    if (cnt[CL_BITS]) launch_k4_enum_bits((unsigned)cnt[CL_BITS], lds_need[CL_BITS], qb, P, d_sp + s_off[CL_BITS], (int32_t)n_w[CL_BITS], per_of[CL_BITS], d_jb, d_obj, d_sb, d_st, d_rbest, redo_b, REDO_CAP);
    if (!win && c.async_mode) {   // (the dense part of the stage ends here on both queues: the next batch's pileup waits for these)
      if (cnt[CL_STREAM]) { if ((e = hipEventRecord(ev_gate[0], stream)) != hipSuccess) return e; gate_set[0] = true; }
      if (fork && cnt[CL_BITS]) { if ((e = hipEventRecord(ev_gate[1], qb)) != hipSuccess) return e; gate_set[1] = true; }
      else if (!fork && cnt[CL_BITS]) { if ((e = hipEventRecord(ev_gate[0], stream)) != hipSuccess) return e; gate_set[0] = true; }
    }
    if (!win) {
      // eight waves per region: the slowest region (most rows) sets the kernel's length, and every row sweep of the
      // epilogue is a pass of <threads> rows (148 -> 103 us on C3)
      if (nps_a && (e = launch_k4_post(2 * LCR_BLOCK, (unsigned)nps_a, post_lds, stream, pin, d_psl, (int32_t)nps_a, plut)) != hipSuccess) return e;
      if (cnt[CL_BITS]) { launch_redo(redo_b, 1, qb); launch_k4_enum_resolve((unsigned)n_w[CL_BITS], res_lds[CL_BITS], qb, P, d_sp + s_off[CL_BITS], d_jb, d_obj, d_sb, d_st); }
      if (nps_b && (e = launch_k4_post(2 * LCR_BLOCK, (unsigned)nps_b, post_lds, qb, pin, d_psl + nps_a, (int32_t)nps_b, plut)) != hipSuccess) return e;
    }
    if (cnt[CL_BIG]) launch_k4_enum_big((unsigned)cnt[CL_BIG], qb, P, d_sp + s_off[CL_BIG], (int32_t)n_w[CL_BIG], per_of[CL_BIG], d_jb, d_obj, win, d_sb, d_st, qrow_all, qstride);
    if (fork) { if ((e = hipEventRecord(ev_join, aux)) != hipSuccess) return e; if ((e = hipStreamWaitEvent(stream, ev_join, 0)) != hipSuccess) return e; }
    return e;
  };
  PCHK(launch(n_t, nullptr));
  HT("en:launched");
  if (n_w[CL_BIG]) {   // the global-memory class: its own resolve kernel (equal objectives by the f64 sums) and the winners' second launch
    const size_t only_big[NCLS] = {0, 0, n_w[CL_BIG]};
    const int64_t tstride = (big_emax + 63) & ~(int64_t)63;
    PCHK(d_en_terms.reserve((size_t)std::max<int64_t>(tstride, 64) * n_w[CL_BIG] * 8 + 64));
    launch_k4_enum_resolve_big((int32_t)n_w[CL_BIG], stream, P, d_sp + s_off[CL_BIG], d_jb, d_obj, d_sb, d_st, d_win, d_en_terms.as<double>(), tstride);
    PCHK(launch(only_big, d_win));
  }
  if (nps_c) PCHK(launch_k4_post(2 * LCR_BLOCK, (unsigned)nps_c, post_lds, stream, pin, d_psl + nps_a + nps_b, (int32_t)nps_c, plut));
  PCHK(hipGetLastError());
  return LCR_OK;
}

// chain regions on queue `side` (their own copy of the state arrays): a region whose phase matrix is far beyond one CU gets all of
// them (persistent launch with grid barriers); the others run side by side, one workgroup each.  LCR_GRID_MIN_ENTRIES moves the
// boundary (tests: 0 = every region).
int PhaseHost::launch_chain(PhaseCall& c) {
  chain_forms.clear();
  if (c.chain_slots.empty()) { chain_desc.clear(); return LCR_OK; }
  const PhaseInputs& in = c.in; const int ng = c.ng; const StageStat* const stat = c.stat;
  const size_t nnz1 = c.nnz1, nc1 = c.nc1, nr1 = c.nr1;
  std::vector<int32_t> wide, big;
  const bool grid_generic = dbg.grid_generic != 0;   // test hook
  bool w_fits_limbs = true;   // (the batched rounds split w into a 23-bit and a signed limb; w < 0 for q < 4)
  for (int q = 0; q < 31; q++) w_fits_limbs = w_fits_limbs && std::llabs(c.P.lut.f1e[q] - c.P.lut.fe[q]) < (1ll << 45);
  for (int g : c.chain_slots) ((int64_t)stat[g].E >= c.grid_min ? big : wide).push_back(g);
  // longest first: a batch with more chain regions than CUs runs them in two generations (one sixteen-wave workgroup
  // per CU), and the workgroups are started in launch order -- the second generation should be the short regions
  // (cost ~ entries x rounds, rounds ~ SNPs / 4)
  std::stable_sort(wide.begin(), wide.end(), [&](int a, int b) {
    return (int64_t)stat[a].E * (in.snps(a) + 8) > (int64_t)stat[b].E * (in.snps(b) + 8);
  });
  const int n_small = (int)wide.size(), n_big = (int)big.size(), nc = n_small + n_big;
  const int grid_waves = std::max(1, k4_grid_blocks()) * 16;
  std::vector<ChainDesc> desc(nc);
  int64_t tbl_cells = 0, adj_n = 0, part_n = 0, term_n = 0;
  int32_t max_state = 0;
  for (int k = 0; k < nc; k++) {
    const int g = k < n_small ? wide[k] : big[k - n_small];
    const int S = in.snps(g);
    ChainDesc& d = desc[k];
    d.slot = g; d.W = std::max(1, std::min(stat[g].W, S)); d.fast_lds = 0;
    d.batch_lds = 0; d.term_off = 0;
    if (k < n_small) { d.term_off = (int32_t)std::min<int64_t>(term_n, INT32_MAX); term_n += stat[g].E; }
    if (k >= n_small && !grid_generic) {
      const size_t need = k4_grid_fast_lds(stat[g].R, S); if (need <= (size_t)K4_GRID_FAST_LDS_MAX) d.fast_lds = (int32_t)need;
      const size_t need_b = k4_grid_batch_lds(S); if (dbg.spec_batch && w_fits_limbs && need_b <= (size_t)K4_GRID_FAST_LDS_MAX) d.batch_lds = (int32_t)need_b;
    }
    d.tbl_off = tbl_cells; tbl_cells += (int64_t)S * d.W;
    d.adj_off = adj_n; adj_n += 2 * (int64_t)S * d.W;
    d.n_parts = k < n_small ? 16 : (int32_t)std::max<int64_t>(16, std::min<int64_t>(grid_waves, (int64_t)(1 << 23) / S));
    d.part_off = part_n; part_n += (int64_t)d.n_parts * S;
    if (k < n_small) max_state = std::max(max_state, stat[g].R + 2 * S);
  }
  // post-phase: device epilogue for the chain regions that fit it
  std::vector<int32_t> post_slots;
  for (int k = 0; k < nc; k++) if (!c.grid_post[desc[k].slot]) post_slots.push_back(desc[k].slot);
  const size_t nps = post_slots.size();
  const size_t desc_bytes = ((size_t)nc * sizeof(ChainDesc) + 15) & ~(size_t)15;
  PCHK(h_ch_up.reserve(desc_bytes + nps * 4 + 64));
  PCHK(d_ch_desc.reserve(desc_bytes + 64)); PCHK(d_ch_slots.reserve(nps * 4 + 64));
  memcpy(h_ch_up.p, desc.data(), (size_t)nc * sizeof(ChainDesc));
  memcpy(h_ch_up.as<uint8_t>() + desc_bytes, post_slots.data(), nps * 4);
  PCHK(d_ch_tbl.reserve((size_t)tbl_cells * 8 + 64)); PCHK(d_ch_adj.reserve((size_t)adj_n * 4 + 64)); PCHK(d_ch_part.reserve((size_t)part_n * 4 + 64));
  const size_t ni = nc1 + (size_t)ng + 1;   // per-SNP int32 arrays: adj_ptr, blk_ptr (ni each), blk_of, blk_pos, blk_nodes, queue (nc1), stack (2 nc1)
  PCHK(d_ch_snpi.reserve((2 * ni + 6 * nc1) * 4 + 64)); PCHK(d_ch_snpb.reserve(3 * nc1 + 64)); PCHK(d_ch_q.reserve(2 * nc1 * 8 + 64));
  PCHK(d_ch_info.reserve((size_t)std::max(ng, 1) * 8 + 64)); PCHK(d_ch_rowi.reserve(nr1 * 4 + 64)); PCHK(d_ch_enti.reserve(2 * nnz1 * 4 + 64));
  PCHK(d_ch_work.reserve(c.st_bytes + 64)); PCHK(d_ch_macc.reserve(nc1 * 8 + 64)); PCHK(d_ch_sig.reserve((2 * (nr1 / 64 + (size_t)ng + 2)) * 8 + 64)); PCHK(d_grid_ctl.reserve((4 + 16) * sizeof(GridCtl)));
  ChainDev C{};
  {   // speculative half-rounds of the all-CU regions: lanes x (sigma words | delta, eta bytes | result) of the largest such region
    size_t ng_max = 1, s_max = 16;
    for (int k = n_small; k < nc; k++) { const int g = desc[k].slot; ng_max = std::max(ng_max, (size_t)(stat[g].R + 63) / 64 + 1); s_max = std::max(s_max, (size_t)in.snps(g)); }
    const size_t s8 = (s_max + 15) & ~(size_t)15, lanes = (size_t)std::max(1, dbg.spec_lanes);
    PCHK(d_spec_sig.reserve(lanes * ng_max * 8 + 64)); PCHK(d_spec_de.reserve(lanes * 2 * s8 + 64)); PCHK(d_spec_res.reserve(lanes * 8 + 64));
    C.spec_sig = d_spec_sig.as<unsigned long long>(); C.spec_de = d_spec_de.as<int8_t>(); C.spec_res = d_spec_res.as<long long>();
    C.spec_lanes = (int32_t)lanes; C.spec_ng = (int32_t)ng_max; C.spec_s8 = (int32_t)s8;
    size_t e_max = 0, g4_max = 0, r_max = 0, sb_max = 0;   // packed entries of the largest all-CU region with device-coherent rounds
    for (int k = n_small; k < nc; k++) if (desc[k].fast_lds || desc[k].batch_lds) e_max = std::max(e_max, (size_t)stat[desc[k].slot].E);
    for (int k = n_small; k < nc; k++) if (desc[k].batch_lds) {
      const int g = desc[k].slot;
      g4_max = std::max(g4_max, ((size_t)stat[g].E + 3 * (size_t)stat[g].R + 3) / 4); r_max = std::max(r_max, (size_t)stat[g].R);
      sb_max = std::max(sb_max, (size_t)in.snps(g));
    }
    if (g4_max) {   // batched rounds: groups | unit pointers | sigma bytes | SNP masks | barrier payload
      auto al = [](size_t x) { return (x + 63) / 64 * 64; };
      const size_t nb = r_max / 64 + 2;   // blocks of 64 sorted rows; the groups: every row padded to its block's longest (<= 64 (S / 4 + 1) more)
      g4_max += 64 * (sb_max / 4 + 2) + 64;
      const size_t o_up = (g4_max + 4) * 16, o_bs = o_up + al(nb * 8), o_pm = o_bs + al(nb * 8), o_iv = o_pm + al(r_max * 4 + 256), o_sig = o_iv + al(r_max * 4 + 256),
                   o_m = o_sig + al(r_max + 64), o_ctl = o_m + al((sb_max + 2) * 4);
      PCHK(d_bt.reserve(o_ctl + K4_GRID_BATCH_CTL_BYTES + 64));
      uint8_t* bp = d_bt.as<uint8_t>();
      C.bt_pk4 = (uint32_t*)bp; C.bt_up4 = (int32_t*)(bp + o_up); C.bt_bs32 = (uint32_t*)(bp + o_bs); C.bt_perm = (int32_t*)(bp + o_pm); C.bt_inv = (int32_t*)(bp + o_iv);
      C.bt_sig8 = bp + o_sig; C.bt_m32 = (uint32_t*)(bp + o_m); C.bt_ctl = bp + o_ctl;
      C.bt_cap4 = (int64_t)g4_max; C.spec_batch = 1;
    }
    C.pk_cap = (int64_t)e_max;
    if (e_max) { PCHK(d_pk.reserve(2 * (e_max + 8) * 4 + 64)); C.pk_csr = d_pk.as<uint32_t>(); C.pk_csc = C.pk_csr + (e_max + 8); }
  }
  c.Pc.scratch = nullptr; c.Pc.scratch_stride = 0; c.Pc.lds_state = 0; c.Pc.lds_mat = 0;
  C.P = c.Pc;
  C.desc = d_ch_desc.as<ChainDesc>();
  C.row_ptr = in.d_row_ptr; C.col = in.d_col; C.val = in.d_val;
  C.cand = in.d_cand; C.cand_off = in.d_cand_off; C.row_region_off = in.d_row_region_off;
  C.prow_src = d_prow_src.as<int32_t>();
  C.ld_tbl = d_ch_tbl.as<uint32_t>(); C.ld_adj = d_ch_adj.as<int32_t>(); C.part_cnt = d_ch_part.as<int32_t>();
  int32_t* si32 = d_ch_snpi.as<int32_t>();
  C.adj_ptr = si32; C.blk_ptr = si32 + ni; C.blk_of = si32 + 2 * ni; C.blk_pos = C.blk_of + nc1; C.blk_nodes = C.blk_pos + nc1;
  C.queue = C.blk_nodes + nc1; C.stack = C.queue + nc1;
  C.seen = d_ch_snpb.as<uint8_t>(); C.ld_ok = C.seen + nc1; C.new_hap = (int8_t*)(C.ld_ok + nc1);
  C.qs = d_ch_q.as<double>(); C.qfs = C.qs + nc1;
  C.blk_info = d_ch_info.as<int32_t>();
  C.flipcol = d_ch_rowi.as<int32_t>(); C.erow = d_ch_enti.as<int32_t>(); C.cent = C.erow + nnz1;
  C.w_sigma = d_ch_work.as<int8_t>() + c.st_sig; C.w_delta = d_ch_work.as<int8_t>() + c.st_del; C.w_eta = d_ch_work.as<int8_t>() + c.st_eta;
  C.macc = d_ch_macc.as<unsigned long long>(); C.ctl = d_grid_ctl.as<GridCtl>(); C.spec_ctl = d_grid_ctl.as<GridCtl>() + 4; C.sig_words = d_ch_sig.as<unsigned long long>();
  const HostLut& L = hlut();
  for (int q = 0; q < 31; q++) { C.le[q] = L.le[q]; C.l1e[q] = L.l1e[q]; }
  C.p_homref = L.p_homref; C.p_homvar = L.p_homvar; C.log_theta = L.log_theta; C.log2 = L.log2;
  if (dbg.chain_ties && dbg.tie_arith >= 3 && n_small && term_n < INT32_MAX) {
    PCHK(d_tie_terms.reserve((size_t)term_n * 16 + 64)); C.tie_terms = d_tie_terms.as<double>();
    PCHK(d_tie_flag.reserve((size_t)std::max(ng, 1) * 4 + 64)); PCHK(d_tie_q.reserve((2 * nr1 + 2 * nc1) * 8 + 64)); PCHK(d_tie_ch.reserve(2 * nc1 + 64));
    C.tie_flag = d_tie_flag.as<int32_t>(); C.tie_qrow = d_tie_q.as<double>(); C.tie_qsnp = C.tie_qrow + 2 * nr1; C.tie_ch = d_tie_ch.as<int8_t>();
  }
  if (c.prof) { C.dbg = d_prof_clk.as<long long>() + (size_t)ng * 16; PCHK(hipMemsetAsync(C.dbg, 0, (16 + 2 * 1024) * 8, side)); }   // 16 step timers + per-workgroup sigma / delta step times
  chain_dev = C; chain_desc = desc;   // (lcr_get_ld_blocks reads the blocks back)
  PCHK(hipStreamWaitEvent(side, ev_csr, 0));
  PCHK(hipMemcpyAsync(d_ch_desc.p, h_ch_up.p, (size_t)nc * sizeof(ChainDesc), hipMemcpyHostToDevice, side));
  if (nps) PCHK(hipMemcpyAsync(d_ch_slots.p, h_ch_up.as<uint8_t>() + desc_bytes, nps * 4, hipMemcpyHostToDevice, side));
  // the working state lives in dynamic LDS when it fits, with room behind it for the largest matrix of the class
  auto launch_class = [&](const std::vector<int32_t>& regs, int first, int32_t mstate, size_t lds_budget) -> hipError_t {
    if (regs.empty()) return hipSuccess;
    ChainDev Ck = C;
    const int32_t stride = (mstate + 63) & ~63;
    const size_t dyn_state = (size_t)stride <= lds_budget * 3 / 4 ? (size_t)stride : 0;
    Ck.P.scratch_stride = stride; Ck.P.lds_state = dyn_state ? 1 : 0;
    uint32_t want = 0;
    for (int g : regs) {
      const uint32_t m = matview_bytes(stat[g].R, in.snps(g), stat[g].E);
      if (dyn_state && dyn_state + m + 64 <= lds_budget) want = std::max(want, m);
    }
    Ck.P.lds_mat = (int32_t)want;
    if (c.prof) {   // the forms k4_chain_wg takes from these values (k4_grid.hip, cross_optimize in k4_dev.h, ld_pair_table)
      for (size_t k = 0; k < regs.size(); k++) {
        const int g = regs[k], S = in.snps(g);
        const bool mat = dyn_state && matview_bytes(stat[g].R, S, stat[g].E) <= want;
        const bool cols = S <= CROSS_MACC, rows = cols && stat[g].R <= K4_CHAIN_STAGE_BYTES / 8;
        const bool tbl = S < 32768 && stat[g].E_all < 65536 &&
                         8ull * (uint64_t)S * (uint64_t)desc[first + k].W + 4ull * (uint64_t)stat[g].E_all + 16 <= (uint64_t)K4_CHAIN_STAGE_BYTES;
        char line[256];
        snprintf(line, sizeof(line), "chain region %d: scope workgroup, state %s, matrix %s, cross_optimize %s, constants %s, pair table %s", g,
                 dyn_state ? "LDS" : "global", mat ? "LDS" : "global", rows ? "rows_balanced" : cols ? "cols_balanced" : "plain",
                 S <= K4_CHAIN_SCN ? "LDS" : "global", tbl ? "LDS" : "global");
        chain_forms.push_back(line);
      }
    }
    return k4_chain_launch_wg(Ck, first, (int)regs.size(), dyn_state + (size_t)want, side);
  };
  PCHK(launch_class(wide, 0, max_state, 64 * 1024));
  if (n_big) RCHK(c.lock_grid(*this));
  if (c.prof) for (int k = 0; k < n_big; k++) {   // all CUs: state, matrix, constants and pair table in global memory, cross_optimize_scope
    char line[256];
    snprintf(line, sizeof(line), "chain region %d: scope all-CU, state global, matrix global, cross_optimize grid, constants global, pair table global", desc[n_small + k].slot);
    chain_forms.push_back(line);
  }
  for (int k = 0; k < n_big; k++) PCHK(k4_chain_launch_grid(C, n_small + k, (size_t)std::max(desc[n_small + k].fast_lds, desc[n_small + k].batch_lds), side));
  if (nps) {
    // 33 KB of static stage buffers + up to 64 KB of region image
    // more chain regions than CUs (a sixteen-wave workgroup has a CU to itself): eight waves, two regions per CU --
    // one generation of workgroups instead of two
    const bool half = ((int)nps > std::max(1, k4_grid_blocks()) || dbg.post_half /* test hook */) && c.post_lds <= 56 * 1024;
    PCHK(launch_k4_post(half ? CHAIN_THREADS / 2 : CHAIN_THREADS, (unsigned)nps, c.post_lds, side, c.pinc, d_ch_slots.as<int32_t>(), (int32_t)nps, c.plut));
  }
  PCHK(hipGetLastError());
  return LCR_OK;
}

// post-phase steps of the regions beyond k4_post's LDS image: all CUs on one region at a time, on `side`
int PhaseHost::launch_gpost(PhaseCall& c) {
  if (c.gpost_slots.empty()) return LCR_OK;
  RCHK(c.lock_grid(*this));
  const int grid_waves = std::max(1, k4_grid_blocks()) * 16;
  PostScratch ps{};
  ps.n_parts = (int32_t)std::max<int64_t>(16, std::min<int64_t>(grid_waves, (int64_t)(1 << 23) / (int64_t)c.gp_S));
  const size_t S8 = (c.gp_S + 8) & ~(size_t)7, R8 = (c.gp_rows + 8) & ~(size_t)7, E8 = (c.gp_E + 8) & ~(size_t)7;
  PCHK(d_gp_snp.reserve(S8 * (3 * 8 + 4 * 4 + 4 + 2 * 4) + R8 * (4 + 5 + 4) + 64 + 64));   // per SNP: 3 doubles, 4 + 2 int32, 4 bytes; per row: rptr, fdirt + 5 bytes
  PCHK(d_gp_ent.reserve(E8 * (3 * 4 + 1) + 64));
  PCHK(d_gp_part.reserve((size_t)ps.n_parts * c.gp_S * 4 + 64));
  PCHK(d_grid_ctl.reserve((4 + 16) * sizeof(GridCtl)));
  uint8_t* p = d_gp_snp.as<uint8_t>();
  ps.sps = (double*)p; p += 8 * S8; ps.rpa = (double*)p; p += 8 * S8; ps.rpb = (double*)p; p += 8 * S8;
  ps.sflags = (uint32_t*)p; p += 4 * S8; ps.soflags = (uint32_t*)p; p += 4 * S8; ps.parent = (int32_t*)p; p += 4 * S8; ps.ccptr = (int32_t*)p; p += 4 * S8;
  ps.rptr = (int32_t*)p; p += 4 * R8;
  ps.shap = (int8_t*)p; p += S8; ps.sgt = (int8_t*)p; p += S8; ps.svt = (int8_t*)p; p += S8; ps.rcode = p; p += S8;
  ps.tag = (int8_t*)p; p += R8; ps.asg = p; p += R8; ps.fp = p; p += R8; ps.lok = p; p += R8; ps.dirty = p; p += R8;
  ps.fdirt = (int32_t*)p; p += 4 * R8; ps.minf = (int32_t*)p; p += 4 * S8; ps.ndraw = (int32_t*)p; p += 4 * S8; ps.gwords = (int32_t*)p; p += 64;
  uint8_t* q = d_gp_ent.as<uint8_t>();
  ps.ecol = (int32_t*)q; q += 4 * E8; ps.erow = (int32_t*)q; q += 4 * E8; ps.cent = (int32_t*)q; q += 4 * E8; ps.ev = q;
  ps.pcnt = d_gp_part.as<int32_t>();
  ps.ctl = d_grid_ctl.as<GridCtl>() + 1;
  bool waited = false;
  for (int g : c.gpost_slots) {
    const bool chain = (uint32_t)c.in.snps(g) > c.prm.max_enum_snps;
    if (!chain && !waited) {   // an enumeration region: its winner is materialised on `stream`
      PCHK(hipEventRecord(ev_fork, c.stream));
      PCHK(hipStreamWaitEvent(side, ev_fork, 0));
      waited = true;
    }
    PCHK(k4_post_launch_grid(chain ? c.pinc : c.pin, ps, g, c.plut, side));
  }
  return LCR_OK;
}

// Everything is queued: the results become pending.  Returns false when run() returns now -- settle() collects them when somebody
// asks --, true when it has to wait for them (synchronous mode, persistent launches or phase_prof).
bool PhaseHost::mark_pending(PhaseCall& c) {
  const PhaseInputs& in = c.in;
  pend.ng = c.ng;
  pend.cand_off.assign(in.cand_region_off, in.cand_region_off + c.ng + 1);
  pend.res_ps = c.res_ps; pend.res_tag = c.res_tag; pend.res_asg = c.res_asg; pend.hc_obj = c.hc_obj; pend.cand = in.cand;
  pending = true;
  HT("ph:ret");
  if (g_lcr_host_trace) lcr_host_trace_flush();
  return !(c.async_mode && !c.prof && !c.grid_lock.held);
}

// phase_prof: the enumeration regions' sizes, the steps of the last chain launch and of k4_post / k4_gpost (every queue is drained)
int PhaseHost::report_prof(PhaseCall& c) {
  const PhaseInputs& in = c.in; const int ng = c.ng; const StageStat* const stat = c.stat;
  if (!c.enum_slots.empty()) {   // share sizes of the enumeration regions (entries per lane decide the kernel class)
    std::vector<int> mn; uint64_t jobs[3] = {0, 0, 0};
    for (int g : c.enum_slots) {
      mn.push_back(stat[g].max_n);
      jobs[stat[g].max_n <= 32 ? 0 : stat[g].max_n <= 48 ? 1 : 2] += 1ull << in.snps(g);
    }
    std::sort(mn.begin(), mn.end());
    fprintf(stderr, "[phase]   enumeration regions: %zu, entries per lane min %d median %d p90 %d max %d; restarts with <= 32: %llu, 33-48: %llu, > 48: %llu\n",
            mn.size(), mn.front(), mn[mn.size() / 2], mn[mn.size() * 9 / 10], mn.back(), (unsigned long long)jobs[0], (unsigned long long)jobs[1], (unsigned long long)jobs[2]);
  }
  for (const std::string& f : chain_forms) fprintf(stderr, "[phase]   %s\n", f.c_str());
  if (chain_dev.dbg && !chain_desc.empty()) {   // steps of the last grid-scope chain launch
    const ChainDesc& last = chain_desc.back();
    long long clk[16];
    PCHK(hipMemcpy(clk, chain_dev.dbg, sizeof(clk), hipMemcpyDeviceToHost));
    static const char* nm[] = {"ordered column index", "pair table", "LD graph", "components + seed", "cross_optimize A", "block flip", "perturbation rounds"};
    fprintf(stderr, "[phase]     chain steps of %s\n", last.fast_lds ? "the last all-CU launch" : "the last launch (one-workgroup form: its first region)");
    for (int k = 0; k < 7; k++) fprintf(stderr, "[phase]     grid chain: %-24s %9.1f us\n", nm[k], (double)(clk[k + 1] - clk[k]) / 100.0);
    if (!last.fast_lds) {
      fprintf(stderr, "[phase]     one-workgroup chain: %lld cross_optimize calls, %lld iterations\n", clk[14], clk[15]);
      static const char* nm3[] = {"setup", "sigma sweep", "row decisions", "delta sweep", "SNP decisions", "objective"};
      for (int k = 0; k < 6; k++) fprintf(stderr, "[phase]     one-workgroup cross_optimize: %-16s %8.1f us in total\n", nm3[k], (double)clk[8 + k] / 100.0);
    } else {   // per-workgroup work time of the two half steps (own work, without the barriers)
      std::vector<long long> wg(2 * 1024);
      PCHK(hipMemcpy(wg.data(), chain_dev.dbg + 16, wg.size() * 8, hipMemcpyDeviceToHost));
      const int nb = std::max(1, k4_grid_blocks());
      for (int h = 0; h < 2; h++) {
        std::vector<std::pair<long long, int>> t;
        for (int k = 0; k < nb && k < 1024; k++) t.push_back({wg[h * 1024 + k], k});
        std::sort(t.begin(), t.end());
        const double it = (double)std::max<long long>(clk[15], 1) * 100.0;
        fprintf(stderr, "[phase]     grid chain rounds: %s step per workgroup and iteration: min %.1f (wg %d)  median %.1f  p90 %.1f  max %.1f us (wg %d)\n",
                h ? "delta" : "sigma", t.front().first / it, t.front().second, t[t.size() / 2].first / it, t[t.size() * 9 / 10].first / it, t.back().first / it, t.back().second);
        if (dbg.prof > 1) { for (int k = 0; k < nb && k < 1024; k++) fprintf(stderr, "%s%.1f", k % 16 ? " " : "\n[phase]       ", wg[h * 1024 + k] / it); fprintf(stderr, "\n"); }
      }
    }
    fprintf(stderr, "[phase]     grid chain: %lld iterations in the rounds\n", clk[15]);
    if (last.batch_lds && clk[14] && chain_dev.bt_ctl) {   // rows by their number of groups (BatchCtl::hist at byte 128)
      unsigned hist[256];
      PCHK(hipMemcpy(hist, (const uint8_t*)chain_dev.bt_ctl + 128, sizeof(hist), hipMemcpyDeviceToHost));
      std::string line;
      for (int l = 0; l < 256; l++) if (hist[l]) line += " " + std::to_string(l) + ":" + std::to_string(hist[l]);
      fprintf(stderr, "[phase]     grid chain rounds (batched): rows by groups%s\n", line.c_str());
    }
    if (last.batch_lds && clk[14]) fprintf(stderr, "[phase]     grid chain rounds (batched): %lld groups of four het-site entries incl. padding (%d rows, %d entries)\n", clk[14], stat[last.slot].R, stat[last.slot].E);
    static const char* nm2[] = {"stage delta/eta", "sigma step (workgroup 0)", "barrier 1", "stage sigma / invalidate", "delta step (workgroup 0)", "barrier 2"};
    for (int k = 0; k < 6; k++) fprintf(stderr, "[phase]     grid chain rounds: %-26s %9.1f us per iteration\n", nm2[k], (double)clk[8 + k] / 100.0 / (double)std::max<long long>(clk[15], 1));
  }
  // steps of k4_post: the slowest workgroup of each kind of region, and the median total; then the regions that took k4_gpost
  std::vector<long long> clk((size_t)ng * 16);
  PCHK(hipMemcpy(clk.data(), c.pin.dbg_clk, clk.size() * 8, hipMemcpyDeviceToHost));
  auto steps = [&](int g, const char* const* nm) {
    for (int k = 0; k < 9; k++) fprintf(stderr, "[phase]     %-30s %7.1f us\n", nm[k], (double)(clk[(size_t)g * 16 + k + 1] - clk[(size_t)g * 16 + k]) / 100.0);
  };
  static const char* nm[] = {"stage rows", "stage entries + column index", "reads_hap", "snp_hap", "reads_hap + snp_hap", "rescue x2",
                             "reads_hap + snp_hap", "phase_set", "write back"};
  for (int chain = 0; chain < 2; chain++) {
    std::vector<std::pair<long long, int>> tot;
    for (int g = 0; g < ng; g++) {
      const int S = in.snps(g);
      if (S == 0 || c.grid_post[g] || ((uint32_t)S > c.prm.max_enum_snps) != (chain == 1)) continue;
      tot.push_back({clk[(size_t)g * 16 + 9] - clk[(size_t)g * 16], g});
    }
    if (tot.empty()) continue;
    std::sort(tot.begin(), tot.end());
    const int g = tot.back().second;
    fprintf(stderr, "[phase]   k4_post %s regions: %zu workgroups, median %.1f us, slowest %.1f us (region %d: %d rows, %d entries, %d SNPs)\n",
            chain ? "chain" : "enumeration", tot.size(), (double)tot[tot.size() / 2].first / 100.0, (double)tot.back().first / 100.0, g,
            in.row_region_off[g + 1] - in.row_region_off[g], stat[g].E_all, in.snps(g));
    steps(g, nm);
  }
  static const char* nm_g[] = {"stage rows + entries", "column index", "reads_hap", "snp_hap", "reads_hap + snp_hap", "rescue x2",
                               "reads_hap + snp_hap", "phase_set", "write back"};
  for (int g = 0; g < ng; g++) {
    if (!c.grid_post[g]) continue;
    fprintf(stderr, "[phase]   k4_gpost region %d: %.1f us\n", g, (double)(clk[(size_t)g * 16 + 9] - clk[(size_t)g * 16]) / 100.0);
    steps(g, nm_g);
    fprintf(stderr, "[phase]     rescue rounds: RNA-edit list %lld, low-fraction list %lld\n", clk[(size_t)g * 16 + 11], clk[(size_t)g * 16 + 12]);
  }
  return LCR_OK;
}

#undef RCHK
#undef PCHK
#undef PCHK_TO

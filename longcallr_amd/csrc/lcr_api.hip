// lcr_api.hip — C ABI (include/lcr.h) over the HIP kernels: context lifecycle, the block cache, the fill kernels, timing and debug
// switches, the phase stage's entry and getters, region discovery.  Batch binding is lcr_batch.hip, the pileup stage lcr_pileup.hip,
// the candidate / import / fragment stages lcr_calls.hip; the context itself is lcr_ctx.h.
// There is NO CPU fallback: every stage launches HIP kernels and fails with LCR_E_DEVICE otherwise.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>

#include "lcr_ctx.h"

// ---- block cache (lcr_dev.h): freed device / page-locked blocks per device, first fit in size order
namespace {
struct BlockCache {
  std::mutex mu;
  std::multimap<size_t, void*> blocks[2][16];   // [host][device]: capacity -> block
  size_t held[2][16] = {};
  size_t limit[2] = {(size_t)24 << 30, (size_t)2 << 30};   // bytes kept per device: HBM blocks, page-locked host blocks
};
BlockCache& block_cache() { static BlockCache* c = new BlockCache(); return *c; }   // (never destroyed: contexts may outlive static destructors)
}  // namespace
void* lcr_cache_take(int host, size_t want, size_t* cap) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  BlockCache& bc = block_cache();
  std::lock_guard<std::mutex> g(bc.mu);
  auto& m = bc.blocks[host ? 1 : 0][dev];
  auto it = m.lower_bound(want);
  if (it == m.end() || it->first > 2 * want + (1u << 20)) return nullptr;
  void* p = it->second;
  *cap = it->first;
  bc.held[host ? 1 : 0][dev] -= it->first;
  m.erase(it);
  return p;
}
bool lcr_cache_put(int host, void* p, size_t cap) {
  int dev = 0;
  if (!p || hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return false;
  BlockCache& bc = block_cache();
  std::lock_guard<std::mutex> g(bc.mu);
  const int h = host ? 1 : 0;
  if (bc.held[h][dev] + cap > bc.limit[h]) return false;
  bc.blocks[h][dev].emplace(cap, p);
  bc.held[h][dev] += cap;
  return true;
}

int g_lcr_own_fill = 1;
namespace {
__global__ void __launch_bounds__(256) lcr_fill_kernel(uint8_t* p, uint32_t word, size_t head, size_t n16, size_t tail) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
  if (t < head) p[t] = (uint8_t)word;
  uint4* const body = reinterpret_cast<uint4*>(p + head);
  const uint4 w = make_uint4(word, word, word, word);
  for (size_t i = t; i < n16; i += nt) body[i] = w;
  if (t < tail) p[head + 16 * n16 + t] = (uint8_t)word;
}
}
namespace {
struct FillRanges { uint8_t* p[4]; size_t head[4], n16[4], tail[4]; uint32_t word[4]; };
__global__ void __launch_bounds__(256) lcr_fill_multi_kernel(FillRanges r) {
  const int k = blockIdx.y;
  uint8_t* const p = r.p[k];
  if (!p) return;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
  const uint32_t word = r.word[k];
  if (t < r.head[k]) p[t] = (uint8_t)word;
  uint4* const body = reinterpret_cast<uint4*>(p + r.head[k]);
  const uint4 w = make_uint4(word, word, word, word);
  for (size_t i = t; i < r.n16[k]; i += nt) body[i] = w;
  if (t < r.tail[k]) p[r.head[k] + 16 * r.n16[k] + t] = (uint8_t)word;
}
}
// up to four fills in one launch (every launch of its own costs ~5 us of queue time on this platform)
hipError_t lcr_fill_multi_async(int n, void* const* ptrs, const int* bytes_val, const size_t* sizes, hipStream_t s) {
  if (!g_lcr_own_fill) { for (int k = 0; k < n; k++) if (sizes[k]) { const hipError_t e = hipMemsetAsync(ptrs[k], bytes_val[k], sizes[k], s); if (e != hipSuccess) return e; } return hipSuccess; }
  FillRanges r{};
  size_t most = 0;
  int m = 0;
  for (int k = 0; k < n && m < 4; k++) {
    if (!sizes[k]) continue;
    const size_t mis = (size_t)((uintptr_t)ptrs[k] & 15), head = std::min(sizes[k], mis ? 16 - mis : 0), n16 = (sizes[k] - head) / 16;
    const uint32_t b = (uint32_t)(bytes_val[k] & 255);
    r.p[m] = (uint8_t*)ptrs[k]; r.head[m] = head; r.n16[m] = n16; r.tail[m] = sizes[k] - head - 16 * n16; r.word[m] = b | (b << 8) | (b << 16) | (b << 24);
    most = std::max(most, n16); m++;
  }
  if (!m) return hipSuccess;
  const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((most + 255) / 256, 1024));
  hipLaunchKernelGGL(lcr_fill_multi_kernel, dim3(blocks, (unsigned)m), dim3(256), 0, s, r);
  return hipGetLastError();
}

hipError_t lcr_fill_async(void* p, int byte, size_t bytes, hipStream_t s) {
  if (!bytes) return hipSuccess;
  if (!g_lcr_own_fill) return hipMemsetAsync(p, byte, bytes, s);
  const size_t mis = (size_t)((uintptr_t)p & 15), head = std::min(bytes, mis ? 16 - mis : 0), n16 = (bytes - head) / 16, tail = bytes - head - 16 * n16;
  const uint32_t b = (uint32_t)(byte & 255), word = b | (b << 8) | (b << 16) | (b << 24);
  const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((n16 + 255) / 256, 2048));
  hipLaunchKernelGGL(lcr_fill_kernel, dim3(blocks), dim3(256), 0, s, (uint8_t*)p, word, head, n16, tail);
  return hipGetLastError();
}

int g_lcr_host_trace = 0;
namespace {
struct HtMark { const char* tag; std::chrono::steady_clock::time_point t; };
thread_local std::vector<HtMark> g_ht;
}
void lcr_host_trace_mark(const char* tag) { g_ht.push_back({tag, std::chrono::steady_clock::now()}); }
void lcr_host_trace_flush() {
  if (g_ht.empty()) return;
  std::string line = "[host]";
  char buf[96];
  for (const HtMark& m : g_ht) { snprintf(buf, sizeof buf, " %s %.1f", m.tag, std::chrono::duration<double, std::micro>(m.t - g_ht[0].t).count()); line += buf; }
  fprintf(stderr, "%s\n", line.c_str());
  g_ht.clear();
}

extern "C" {

const char* lcr_version(void) { return "liblcr 0.1 (gfx950)"; }

int lcr_release_cached_memory(void) {   // every block the cache holds goes back to the runtime (all devices)
  BlockCache& bc = block_cache();
  std::lock_guard<std::mutex> g(bc.mu);
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (int dev = 0; dev < 16; dev++) {
    if (bc.blocks[0][dev].empty() && bc.blocks[1][dev].empty()) continue;
    (void)hipSetDevice(dev);
    for (auto& kv : bc.blocks[0][dev]) (void)hipFree(kv.second);
    for (auto& kv : bc.blocks[1][dev]) (void)hipHostFree(kv.second);
    bc.blocks[0][dev].clear(); bc.blocks[1][dev].clear();
    bc.held[0][dev] = bc.held[1][dev] = 0;
  }
  (void)hipSetDevice(cur);
  return LCR_OK;
}
int lcr_set_cache_limits(int64_t device_bytes, int64_t host_bytes) {   // per device; 0 = keep nothing (every block is freed when it is given back)
  if (device_bytes < 0 || host_bytes < 0) return LCR_E_ARG;
  BlockCache& bc = block_cache();
  std::lock_guard<std::mutex> g(bc.mu);
  bc.limit[0] = (size_t)device_bytes; bc.limit[1] = (size_t)host_bytes;
  return LCR_OK;
}

int lcr_params_preset(int preset, lcr_params* o) {
  if (!o || preset < 0 || preset > 3) return LCR_E_ARG;
  memset(o, 0, sizeof *o);
  const bool ont = preset >= 2;  // main.rs:272-396
  o->platform = ont ? LCR_PLATFORM_ONT : LCR_PLATFORM_HIFI;
  o->min_baseq = 10; o->dist_to_end = ont ? 20 : 40; o->polya_len = 5;
  o->min_depth = ont ? 10 : 6; o->max_depth = 50000; o->min_qual = 2;
  o->dense_win = 100; o->min_dense_cnt = 5; o->low_cnt_cut = 10; o->min_linkers = 1; o->max_enum_snps = 10;
  o->ld_weight_threshold = 1;
  o->use_strand_bias = (preset == 0 || preset == 2) ? 1 : 0;
  o->min_af = ont ? 0.20f : 0.15f; o->min_af_intron = 0.0f; o->low_frac_cut = 0.05f;
  o->min_phase_score = ont ? 13.0f : 11.0f;
  o->read_assign_cutoff = 0.0; o->seed = 2025;
  return LCR_OK;
}

int lcr_ctx_create(int device, lcr_ctx** out) {
  if (!out) return LCR_E_ARG;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return LCR_E_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return LCR_E_DEVICE;
  lcr_ctx* c = new lcr_ctx();
  c->device = device;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return LCR_E_DEVICE; }
  c->own_stream = true;
  for (int k = 0; k < LCR_NTIMERS; k++)
    for (int j = 0; j < 2; j++)
      if (hipEventCreate(&c->ev[k][j]) != hipSuccess) { lcr_ctx_destroy(c); return LCR_E_DEVICE; }
  for (hipEvent_t* e : {&c->ev_ctl, &c->ev_sv, &c->ev_cand, &c->ev_nnz, &c->ev_imp, &c->ev_genes})
    if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) { lcr_ctx_destroy(c); return LCR_E_DEVICE; }
  for (CallState* st : c->post_calls()) {
    if (hipEventCreateWithFlags(&st->ev, hipEventDisableTiming) != hipSuccess) { lcr_ctx_destroy(c); return LCR_E_DEVICE; }
    for (hipEvent_t& e : st->ev_t) if (hipEventCreate(&e) != hipSuccess) { lcr_ctx_destroy(c); return LCR_E_DEVICE; }
  }
  *out = c;
  return LCR_OK;
}

void lcr_ctx_destroy(lcr_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)c->phase.settle(nullptr);   // (an lcr_phase whose results nobody collected: its queues are drained before anything is freed)
  for (hipStream_t q : {c->phase.main_q, c->phase.side, c->phase.aux}) if (q) (void)hipStreamSynchronize(q);
  (void)hipStreamSynchronize(c->stream);
  if (c->up_stream) (void)hipStreamSynchronize(c->up_stream);
  for (auto& u : c->up) if (u.ev) (void)hipEventDestroy(u.ev);
  if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
  for (hipEvent_t e : {c->ev_nnz, c->ev_cand, c->ev_sv, c->ev_ctl, c->ev_imp, c->ev_genes}) if (e) (void)hipEventDestroy(e);
  for (CallState* st : c->post_calls()) for (hipEvent_t e : {st->ev, st->ev_t[0], st->ev_t[1]}) if (e) (void)hipEventDestroy(e);
  for (int k = 0; k < 2 * lcr_ctx::UP_LANES; k++) if (c->ev_up[k]) (void)hipEventDestroy(c->ev_up[k]);
  for (hipEvent_t e : c->ev_mask_t) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev_unpack_t) if (e) (void)hipEventDestroy(e);
  c->phase.release();
  for (int k = 0; k < LCR_NTIMERS; k++) for (int j = 0; j < 2; j++) if (c->ev[k][j]) (void)hipEventDestroy(c->ev[k][j]);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;   // (every queue is drained: the buffers give their blocks back)
}

const char* lcr_last_error(const lcr_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int lcr_ctx_set_stream(lcr_ctx* c, void* s) {
  if (!c) return LCR_E_ARG;
  (void)hipSetDevice(c->device);
  { int rc = phase_settle(c); if (rc) return rc; }
  if (c->own_stream && c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
  if (s) { c->stream = (hipStream_t)s; c->own_stream = false; }
  else { HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
  return LCR_OK;
}

int lcr_ctx_sync(lcr_ctx* c) {
  if (!c) return LCR_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LCR_OK;
}

int lcr_enable_timing(lcr_ctx* c, int on) { if (!c) return LCR_E_ARG; c->timing = on != 0; return LCR_OK; }

int lcr_kernel_ms(lcr_ctx* c, int k, float* ms) {
  if (!c || !ms || k < 0 || k >= LCR_NTIMERS) return LCR_E_ARG;
  if (!c->ev_valid[k]) return LCR_E_STATE;
  HIPCHK(c, hipEventSynchronize(c->ev[k][1]));
  HIPCHK(c, hipEventElapsedTime(ms, c->ev[k][0], c->ev[k][1]));
  return LCR_OK;
}

int lcr_pileup_bytes(lcr_ctx* c, int64_t* bytes) {
  if (!c || !bytes) return LCR_E_ARG;
  int64_t staged = 0;   // (a lean tally: 48 bytes per staged survivor instead of the planes)
  const int rc = pile_staged_bytes(c, &staged);
  *bytes = c->pileup_bytes + staged;
  return rc;
}

int lcr_pileup_records(lcr_ctx* c, int64_t* items, int64_t* records) {
  if (!c || !items || !records) return LCR_E_ARG;
  if (c->stage < ST_PILED) { c->err = "lcr_pileup_records before lcr_pileup"; return LCR_E_STATE; }
  *items = c->pile_items; *records = c->pile_recs;
  return LCR_OK;
}

int lcr_pileup_stage_bytes(lcr_ctx* c, int64_t* bytes) {
  if (!c || !bytes) return LCR_E_ARG;
  int64_t staged = 0;
  const int rc = pile_staged_bytes(c, &staged);
  *bytes = c->stage_bytes + staged;
  return rc;
}

int lcr_phase(lcr_ctx* c, const lcr_params* p) {
  if (!c || !p) return LCR_E_ARG;
  if (c->stage < ST_FRAGGED) { c->err = "lcr_phase before lcr_fragments"; return LCR_E_STATE; }
  if (c->cand_used) { c->err = "lcr_phase after lcr_phase: the phase stage has rewritten the candidate records; run the candidate stage again"; return LCR_E_STATE; }
  if (p->ld_weight_threshold != 1) { c->err = "ld_weight_threshold must be 1: SNPFrag::phase is only ever called with 1 (thread.rs:166)"; return LCR_E_ARG; }
  const bool ds_on = c->ds_rows_set || c->ds_depth > 0;
  if (ds_on && !(p->read_assign_cutoff > 0.0)) { c->err = "down-sampling needs read_assign_cutoff > 0: the last read assignment must not depend on the sign of an unsampled row's haplotag"; return LCR_E_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = frag_settle(c); if (rc) return rc; }
  PhaseInputs in;
  in.ds_depth = c->ds_depth; in.ds_seed = c->ds_seed; in.ds_rows = c->ds_rows_set ? c->ds_rows.data() : nullptr;
  c->ds_rows_set = false;   // (for this lcr_phase only)
  in.n_regions = c->bv.n_regions; in.n_rows = c->n_rows; in.nnz = c->nnz;
  in.row_region_off = c->h_row_region_off.data(); in.cand_region_off = c->h_cand_off.data();
  in.region_start0 = c->h_start0.data();
  in.region_e_off = c->h_nnz.as<int64_t>();
  in.d_row_ptr = c->row_ptr.as<int64_t>(); in.d_col = c->col.as<int32_t>(); in.d_val = c->val.as<uint8_t>();
  in.d_row_links = c->row_links.as<uint32_t>();
  in.cand = &c->h_cand;
  in.d_cand = c->d_cand.as<lcr_candidate>(); in.d_cand_off = c->d_cand_off.as<int32_t>();
  in.d_row_region_off = c->row_region_off.as<int32_t>(); in.d_start0 = c->bv.start0;
  Timer t(c, LCR_K_PHASE);
  c->cand_used = true;   // (from here on the post-phase kernels may rewrite the records: an error part of the way through included)
  int rc = c->phase.run(in, *p, c->stream, &c->err);
  if (rc) {   // (an error part of the way through an asynchronous stage leaves kernels queued that read the candidate / fragment buffers)
    if (c->phase.q_first) (void)hipStreamSynchronize(c->phase.q_first);
    if (c->phase.side) (void)hipStreamSynchronize(c->phase.side);
    if (c->phase.aux) (void)hipStreamSynchronize(c->phase.aux);
    return rc;
  }
  c->stage = ST_PHASED;
  c->res_valid = true; c->res_ng = c->bv.n_regions;
  c->phase_slot = c->bound_slot >= 0 ? c->bound_slot : (c->bound_host ? -2 : -1);
  return LCR_OK;
}

int lcr_set_downsample(lcr_ctx* c, uint32_t depth, uint64_t seed) {
  if (!c) return LCR_E_ARG;
  c->ds_depth = depth; c->ds_seed = seed;
  return LCR_OK;
}

int lcr_set_downsample_rows(lcr_ctx* c, int32_t mem, int32_t n_rows, const uint8_t* sampled) {
  if (!c || (mem != LCR_MEM_HOST && mem != LCR_MEM_DEVICE)) return LCR_E_ARG;
  if (c->stage < ST_FRAGGED || c->cand_used) { c->err = "lcr_set_downsample_rows names the rows of a fragment stage: call it between lcr_fragments and lcr_phase"; return LCR_E_STATE; }
  if (n_rows != c->n_rows || (n_rows > 0 && !sampled)) { c->err = "lcr_set_downsample_rows: one byte per fragment row of lcr_get_fragmat"; return LCR_E_ARG; }
  c->ds_rows.resize((size_t)n_rows);
  if (n_rows > 0) {
    if (mem == LCR_MEM_HOST) memcpy(c->ds_rows.data(), sampled, (size_t)n_rows);
    else { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipMemcpy(c->ds_rows.data(), sampled, (size_t)n_rows, hipMemcpyDeviceToHost)); }
  }
  for (uint8_t& b : c->ds_rows) b = b ? 1 : 0;
  c->ds_rows_set = true;
  return LCR_OK;
}

int lcr_get_downsample(lcr_ctx* c, lcr_downsample_info* out) {
  if (!c || !out) return LCR_E_ARG;
  if (!c->res_valid) { c->err = "lcr_get_downsample: no phase results (call it after lcr_phase and before the next candidate stage)"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }   // (the asynchronous stage: the bytes' copy is queued with it)
  out->n_regions = c->phase.ds_ng; out->n_rows = c->phase.ds_nrow;   // (of that lcr_phase, not of a later fragment stage)
  out->region_applied = c->phase.ds_applied.data();
  out->sampled = c->phase.ds_any ? c->phase.h_sampled.as<uint8_t>() : nullptr;
  out->dev_sampled = c->phase.ds_any ? c->phase.d_sampled.as<uint8_t>() : nullptr;
  return LCR_OK;
}

int lcr_discover_regions(lcr_ctx* c, int32_t mem, int32_t n_reads, const int32_t* ref_start, const int32_t* ref_end,
                         int64_t contig_len, lcr_region_list* out) {
  return lcr_discover_regions_truncated(c, mem, n_reads, ref_start, ref_end, contig_len, 0, 0, out, nullptr);
}

int lcr_discover_regions_truncated(lcr_ctx* c, int32_t mem, int32_t n_reads, const int32_t* ref_start, const int32_t* ref_end,
                                   int64_t contig_len, int32_t truncation, uint32_t truncation_coverage, lcr_region_list* out, int64_t* n_truncated) {
  if (!c || !out || n_reads < 0 || contig_len < 0 || contig_len > 0x7FFFFFF0ll) return LCR_E_ARG;
  if (n_truncated) *n_truncated = 0;
  const uint32_t cap = truncation ? truncation_coverage : UINT32_MAX;   // util.rs:294-296: depth > cap breaks a region like depth == 0
  HIPCHK(c, hipSetDevice(c->device));
  c->rl_start0.clear(); c->rl_len.clear(); c->rl_max.clear();
  out->n_regions = 0; out->start0 = nullptr; out->len = nullptr; out->max_cov = nullptr;
  if (n_reads == 0 || contig_len == 0) return LCR_OK;
  const int32_t *d_s = ref_start, *d_e = ref_end;
  if (mem == LCR_MEM_HOST) {
    HIPCHK(c, c->rd_start.reserve((size_t)n_reads * 4)); HIPCHK(c, c->rd_end.reserve((size_t)n_reads * 4));
    { int rc2 = upload_bytes(c, c->rd_start.p, ref_start, (size_t)n_reads * 4); if (rc2) return rc2; rc2 = upload_bytes(c, c->rd_end.p, ref_end, (size_t)n_reads * 4); if (rc2) return rc2; }
    d_s = c->rd_start.as<int32_t>(); d_e = c->rd_end.as<int32_t>();
  }
  // the window of the contig that reads cover at all (host spans: one loop here; device spans: one small reduction)
  int64_t w_lo = contig_len, w_hi = 0;
  if (mem == LCR_MEM_HOST) {
    for (int32_t r = 0; r < n_reads; r++) {
      const int64_t s = ref_start[r], e = std::min<int64_t>(ref_end[r], contig_len);
      if (s >= 0 && s < e) { w_lo = std::min(w_lo, s); w_hi = std::max(w_hi, e); }
    }
  } else {
    HIPCHK(c, c->rd_cnt.reserve(16));
    int32_t init[2] = {INT_MAX, 0}, got[2] = {INT_MAX, 0};
    HIPCHK(c, hipMemcpyAsync(c->rd_cnt.p, init, 8, hipMemcpyHostToDevice, c->stream));
    launch_k5_span_window(d_s, d_e, n_reads, contig_len, c->rd_cnt.as<int32_t>(), c->stream);
    HIPCHK(c, hipMemcpyAsync(got, c->rd_cnt.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (got[1] > 0) { w_lo = got[0]; w_hi = got[1]; }
  }
  if (w_hi <= w_lo) return LCR_OK;   // no valid span
  const int64_t full_len = contig_len;
  contig_len = w_hi - w_lo;          // from here on positions are relative to w_lo
  const size_t nd = (size_t)contig_len + 2;
  HIPCHK(c, c->rd_diff.reserve(nd * 4)); HIPCHK(c, c->rd_ex.reserve((nd + 1) * 4));
  HIPCHK(c, hipMemsetAsync(c->rd_diff.p, 0, nd * 4, c->stream));
  launch_k5_span_diff(d_s, d_e, n_reads, full_len, w_lo, c->rd_diff.as<uint32_t>(), c->stream);
  launch_scan_i32(c->scan_tmp, (const int32_t*)c->rd_diff.p, c->rd_ex.as<int32_t>(), (int32_t)nd, nullptr, c->stream);
  const int32_t nb = (int32_t)((contig_len + 1023) / 1024);
  HIPCHK(c, c->rd_cnt.reserve(((size_t)nb + 1) * 4)); HIPCHK(c, c->rd_off.reserve(((size_t)nb + 2) * 4));
  // rd_off: nb offsets, [nb] the number of islands, [nb + 1] the columns above the cap (counted only while truncation is on)
  uint32_t* d_trunc = truncation ? c->rd_off.as<uint32_t>() + nb + 1 : nullptr;
  if (d_trunc) HIPCHK(c, hipMemsetAsync(d_trunc, 0, 4, c->stream));
  launch_k5_bounds(false, c->rd_ex.as<int32_t>(), contig_len, cap, nb, c->rd_cnt.as<int32_t>(), nullptr, nullptr, nullptr, nullptr, 0, d_trunc, c->stream);
  launch_scan_i32(c->scan_tmp, c->rd_cnt.as<int32_t>(), c->rd_off.as<int32_t>(), nb, c->rd_off.as<int32_t>() + nb, c->stream);
  int32_t tot[2] = {0, 0};      // islands, columns above the cap
  HIPCHK(c, hipMemcpyAsync(tot, c->rd_off.as<int32_t>() + nb, d_trunc ? 8 : 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  const int32_t n_isl = tot[0];
  if (n_truncated) *n_truncated = (int64_t)(uint32_t)tot[1];
  if (n_isl == 0) return LCR_OK;
  const int32_t n_keys = 2 * n_isl + 1;     // (n_isl <= window / 2 + 1 < 2^30)
  HIPCHK(c, c->rd_s.reserve((size_t)n_isl * 4)); HIPCHK(c, c->rd_e.reserve((size_t)n_isl * 4)); HIPCHK(c, c->rd_max.reserve((size_t)n_keys * 4));
  HIPCHK(c, hipMemsetAsync(c->rd_max.p, 0, (size_t)n_keys * 4, c->stream));
  launch_k5_bounds(true, c->rd_ex.as<int32_t>(), contig_len, cap, nb, nullptr, c->rd_off.as<int32_t>(), c->rd_s.as<int32_t>(), c->rd_e.as<int32_t>(),
                   c->rd_max.as<uint32_t>(), n_keys, nullptr, c->stream);
  std::vector<int32_t> hs(n_isl), he(n_isl);
  std::vector<uint32_t> hm(n_keys);
  HIPCHK(c, hipMemcpyAsync(hs.data(), c->rd_s.p, (size_t)n_isl * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(he.data(), c->rd_e.p, (size_t)n_isl * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hm.data(), c->rd_max.p, (size_t)n_keys * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  // util.rs:287-330: cursors and max_coverage are reset only when a region is emitted, and a region is
  // emitted only if region_end > region_start: a single-column island stays pending and becomes the
  // start of the region that ends with the next island (the gap between them included).  max_coverage runs over
  // every column since the last emission, breaks included: the breaks in front of the island (hm[2 i]), then the
  // island and the break that closes it (hm[2 i + 1]) -- the column at which the reference emits.
  uint32_t running = 0;
  int64_t pend = -1;
  for (int i = 0; i < n_isl; i++) {
    hs[i] += (int32_t)w_lo; he[i] += (int32_t)w_lo;   // back to contig positions
    running = std::max(running, std::max(hm[2 * i], hm[2 * i + 1]));
    if (pend < 0) pend = hs[i];
    if ((int64_t)he[i] > pend) {
      c->rl_start0.push_back(pend); c->rl_len.push_back((int32_t)(he[i] - pend + 1)); c->rl_max.push_back(running);
      pend = -1; running = 0;
    }
  }
  out->n_regions = (int32_t)c->rl_start0.size();
  out->start0 = c->rl_start0.data(); out->len = c->rl_len.data(); out->max_cov = c->rl_max.data();
  return LCR_OK;
}

int lcr_get_phase_result(lcr_ctx* c, lcr_phase_result* out) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED) { c->err = "lcr_get_phase_result before lcr_phase"; return LCR_E_STATE; }
  { int rc = phase_settle(c); if (rc) return rc; }
  out->n_rows = c->n_rows; out->n_regions = c->bv.n_regions;
  out->haplotag = c->phase.r_haplotag; out->assignment = c->phase.r_assignment;
  out->phase_set = c->phase.r_phase_set; out->objective = c->phase.objective.data();
  return LCR_OK;
}

int lcr_get_read_records_device(lcr_ctx* c, const lcr_read_record** dev_rec, int32_t* n_rows) {
  if (!c || !dev_rec || !n_rows) return LCR_E_ARG;
  if (c->stage < ST_PHASED) { c->err = "lcr_get_read_records_device before lcr_phase"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }
  static_assert(sizeof(lcr_read_record) == 12, "lcr_read_record is 12 bytes");
  *dev_rec = c->phase.d_read_rec.as<lcr_read_record>();
  *n_rows = c->n_rows;
  return LCR_OK;
}

// The pipelined consumer's getter: everything the last lcr_phase produced, valid although the NEXT batch has been bound
// (lcr_load_batch / lcr_bind_batch) and its pileup queued -- none of those touch the buffers named here -- until the next lcr_candidates.
int lcr_collect_phase(lcr_ctx* c, lcr_phase_collected* out) {
  if (!c || !out) return LCR_E_ARG;
  if (!c->res_valid) { c->err = "lcr_collect_phase: no phase results (call it after lcr_phase and before the next lcr_candidates)"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }
  out->n_regions = c->res_ng; out->n_rows = c->n_rows; out->n_cand = (int32_t)c->h_cand.size(); out->pad_ = 0;
  out->cand = c->h_cand.data(); out->cand_region_off = c->h_cand_off.data(); out->row_region_off = c->h_row_region_off.data();
  out->haplotag = c->phase.r_haplotag; out->assignment = c->phase.r_assignment; out->phase_set = c->phase.r_phase_set;
  out->objective = c->phase.objective.data();
  out->dev_cand = c->d_cand.as<lcr_candidate>(); out->dev_read_rec = c->phase.d_read_rec.as<lcr_read_record>();
  return LCR_OK;
}

int lcr_ctx_set_async_phase(lcr_ctx* c, int on) {
  if (!c) return LCR_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  { int rc = phase_settle(c); if (rc) return rc; }
  c->phase.dbg.async_phase = on != 0;
  if (on) {   // the stage's four queues need hardware queues of their own: the runtime's default of 4 per process maps two of them onto one
    const char* q = getenv("GPU_MAX_HW_QUEUES");
    if (!q || atoi(q) < 8) {
      c->err = "asynchronous phase stage: GPU_MAX_HW_QUEUES is unset or below 8 in this process's environment -- the HIP runtime then shares hardware queues "
               "between the stage's streams (results are the same, the overlap is lost); export GPU_MAX_HW_QUEUES=8 before the process starts";
      return LCR_W_HW_QUEUES;
    }
  }
  return LCR_OK;
}

int lcr_ctx_set_lock_dir(lcr_ctx* c, const char* dir) {
  if (!c || !dir) return LCR_E_ARG;
  c->phase.lock_dir = dir;
  return LCR_OK;
}

int lcr_debug_set(lcr_ctx* c, const char* key, int64_t value) {
  if (!c || !key) return LCR_E_ARG;
  PhaseDebug& d = c->phase.dbg;
  const std::string k(key);
  if (k == "phase_prof") d.prof = (int)value;
  else if (k == "grid_min_entries") d.grid_min = value;
  else if (k == "grid_generic") d.grid_generic = (int)value;
  else if (k == "post_half") d.post_half = (int)value;
  else if (k == "enum_force_big") d.enum_force_big = (int)value;
  else if (k == "enum_force_stream") d.enum_force_stream = (int)value;
  else if (k == "enum_elide") d.enum_elide = value != 0;
  else if (k == "async_phase") d.async_phase = value != 0;
  else if (k == "host_trace") g_lcr_host_trace = value != 0;
  else if (k == "own_fill") g_lcr_own_fill = value != 0;
  else if (k == "fill_selftest") {   // lcr_fill_async / lcr_fill_multi_async against the host on every alignment of both ends (a test hook: returns LCR_E_DEVICE on a difference)
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = 4096;
    DevBuf buf;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{c->stream};   // (destroyed before `buf`: no fill is in flight when it is freed)
    HIPCHK(c, buf.reserve(4 * N));
    std::vector<uint8_t> host(4 * N), want(4 * N);
    for (size_t off = 0; off < 18; off++)
      for (size_t len : {(size_t)0, (size_t)1, (size_t)15, (size_t)16, (size_t)17, (size_t)255, (size_t)1000 + off, (size_t)2049}) {
        HIPCHK(c, hipMemsetAsync(buf.p, 0xAB, 4 * N, c->stream));
        std::fill(want.begin(), want.end(), (uint8_t)0xAB);
        uint8_t* base = buf.as<uint8_t>();
        HIPCHK(c, lcr_fill_async(base + off, 0x5C, len, c->stream));
        std::fill(want.begin() + off, want.begin() + off + len, (uint8_t)0x5C);
        void* const ptrs[4] = {base + N + off, base + 2 * N + 3, nullptr, base + 3 * N + off};
        const int vals[4] = {0x80, 0, 7, 0xFF};
        const size_t sizes[4] = {len, 33, 0, len / 2};
        HIPCHK(c, lcr_fill_multi_async(4, ptrs, vals, sizes, c->stream));
        std::fill(want.begin() + N + off, want.begin() + N + off + len, (uint8_t)0x80);
        std::fill(want.begin() + 2 * N + 3, want.begin() + 2 * N + 3 + 33, (uint8_t)0);
        std::fill(want.begin() + 3 * N + off, want.begin() + 3 * N + off + len / 2, (uint8_t)0xFF);
        HIPCHK(c, hipMemcpyAsync(host.data(), buf.p, 4 * N, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (host != want) { c->err = "fill_selftest: a fill kernel wrote other bytes than asked (offset " + std::to_string(off) + ", length " + std::to_string(len) + ")"; return LCR_E_DEVICE; }
      }
  }
  else if (k == "chain_ties") d.chain_ties = value != 0;
  else if (k == "redo_lds") d.redo_lds = (int)std::max<int64_t>(0, std::min<int64_t>(value, 128 * 1024));
  else if (k == "tie_arith") d.tie_arith = (int)std::max<int64_t>(0, std::min<int64_t>(value, 3));   // (3 = the default: all four classes in the enumeration branch)
  else if (k == "timing_mask") c->timing_mask = (uint32_t)value;
  else if (k == "hist_tiles") c->dbg_hist_tiles = value > 0 ? 1 : value < 0 ? -1 : 0;
  else if (k == "k3_hits") c->dbg_k3_hits = value != 0;
  else if (k == "k3_list_blocks") c->dbg_k3_list_blocks = (int)std::max<int64_t>(0, std::min<int64_t>(value, 65536));
  else if (k == "fuse_filter") c->dbg_fuse_filter = value != 0;
  else if (k == "spec_compact") c->dbg_spec_compact = value != 0;
  else if (k == "lean_planes") c->dbg_lean_planes = value != 0;
  else if (k == "fold_indels") c->dbg_fold_indels = value != 0;
  else if (k == "poison_planes") c->dbg_poison_planes = value != 0;
  else if (k == "iso_hash_bits") c->dbg_iso_hash_bits = (int)std::max<int64_t>(0, std::min<int64_t>(value, 64));
  else if (k == "ends_hash_bits") c->dbg_ends_hash_bits = (int)std::max<int64_t>(0, std::min<int64_t>(value, 32));
  else if (k == "ir_hash_bits") c->dbg_ir_hash_bits = (int)std::max<int64_t>(0, std::min<int64_t>(value, 32));
  else if (k == "indel_hash_bits") c->dbg_indel_hash_bits = (int)std::max<int64_t>(0, std::min<int64_t>(value, 32));
  else if (k == "grid_spec_batch") d.spec_batch = (int)value;
  else if (k == "grid_spec_lanes") d.spec_lanes = (int)std::max<int64_t>(1, std::min<int64_t>(value, 16));
  else { c->err = "lcr_debug_set: unknown key " + k; return LCR_E_ARG; }
  return LCR_OK;
}

int lcr_get_ld_blocks(lcr_ctx* c, int32_t region, int32_t* n_blocks, const int32_t** block_off, const int32_t** snp_idx) {
  if (!c || !n_blocks || !block_off || !snp_idx) return LCR_E_ARG;
  if (c->stage < ST_PHASED) { c->err = "lcr_get_ld_blocks before lcr_phase"; return LCR_E_STATE; }
  if (region < 0 || region >= c->bv.n_regions) { c->err = "lcr_get_ld_blocks: no such region"; return LCR_E_ARG; }
  { int rc = phase_settle(c); if (rc) return rc; }
  PhaseInputs in;
  in.n_regions = c->bv.n_regions;
  in.cand_region_off = c->h_cand_off.data();
  const int rc = c->phase.ld_blocks(in, region, &c->ld_off, &c->ld_snps, c->stream, &c->err);
  if (rc != LCR_OK) return rc;
  *n_blocks = (int32_t)c->ld_off.size() - 1; *block_off = c->ld_off.data(); *snp_idx = c->ld_snps.data();
  return LCR_OK;
}

int lcr_get_tie_census(lcr_ctx* c, uint64_t out[8]) {
  if (!c || !out) return LCR_E_ARG;
  if (c->stage < ST_PHASED) { c->err = "lcr_get_tie_census before lcr_phase"; return LCR_E_STATE; }
  { int rc = phase_settle(c); if (rc) return rc; }
  for (int i = 0; i < 8; i++) out[i] = i < TIE_NCTR ? (uint64_t)c->phase.tie_census[i] : 0;
  return LCR_OK;
}

}  // extern "C"

// lcr_batch.hip — binding a batch: host uploads, the asynchronous input path, and the load-time kernels of K0 (region and tile tables,
// packed read headers, the flat op space).  lcr_load_batch / lcr_load_batch_async / lcr_bind_batch of include/lcr.h, and their forms for
// a batch whose bases are still BAM nibbles (lcr_load_batch_packed / _async, lcr_unpack_bases): the same code with one array exchanged.
#include <atomic>
#include <thread>

#include "lcr_ctx.h"

// Host -> device copy of a caller's (pageable) array on the context's stream.  Page-locked sources (hipHostMalloc / hipHostRegister: what
// lcr_load_batch_async asks for) go straight to the DMA engines.  Pageable ones are staged through page-locked buffers of the context,
// 8 MB at a time: the runtime's own path for them pins the caller's pages chunk by chunk, and on this stack (ROCm 7, MI355X) a device memory
// fault inside that path (rocr VMFaultHandler under hsaCopyStagedOrPinned / addPinnedMem, the caller still inside hipMemcpyAsync) aborted one
// test-suite run in five -- in torch's own .to() as well as here.  Small copies (<= 64 KB) are staged by the runtime itself either way.
int upload_bytes(lcr_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t q) {
  if (!q) q = c->stream;
  if (bytes <= 64 * 1024) { HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, q)); return LCR_OK; }
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, src) == hipSuccess && at.type == hipMemoryTypeHost) {
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, q));
    return LCR_OK;
  }
  (void)hipGetLastError();   // (an unregistered pointer is reported as an error by some runtimes)
  constexpr size_t CH = 8u << 20;
  // one staging lane = two buffers + their events; large uploads run UP_LANES lanes on threads of their own (one thread's memcpy is
  // ~10 GB/s against the link's 50: 33 ms instead of 21 per C3 batch with a single lane)
  const int lanes = bytes >= (64u << 20) ? lcr_ctx::UP_LANES : 1;
  for (int k = 0; k < 2 * lanes; k++) {
    HIPCHK(c, c->h_up[k].reserve(CH));
    if (!c->ev_up[k]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_up[k], hipEventDisableTiming));
  }
  const size_t n_ch = (bytes + CH - 1) / CH;
  std::atomic<int> bad{0};
  auto lane_fn = [&](int w) {
    (void)hipSetDevice(c->device);
    int use = 0;
    for (size_t i = (size_t)w; i < n_ch && !bad.load(std::memory_order_relaxed); i += (size_t)lanes, use ^= 1) {
      const int k = 2 * w + use;
      const size_t off = i * CH, n = std::min(CH, bytes - off);
      hipError_t e = c->up_busy[k] ? hipEventSynchronize(c->ev_up[k]) : hipSuccess;
      if (e == hipSuccess) {
        memcpy(c->h_up[k].p, (const uint8_t*)src + off, n);
        e = hipMemcpyAsync((uint8_t*)dst + off, c->h_up[k].p, n, hipMemcpyHostToDevice, q);
      }
      if (e == hipSuccess) e = hipEventRecord(c->ev_up[k], q);
      if (e != hipSuccess) { bad.store((int)e); return; }
      c->up_busy[k] = true;
    }
  };
  if (lanes == 1) lane_fn(0);
  else {
    std::vector<std::thread> th;
    try { for (int w = 1; w < lanes; w++) th.emplace_back(lane_fn, w); } catch (...) { }   // (no thread to be had: their chunks are taken below)
    const int started = (int)th.size() + 1;
    lane_fn(0);
    for (auto& t : th) t.join();
    for (int w = started; w < lanes; w++) lane_fn(w);
  }
  if (bad.load()) { c->err = std::string("host upload: ") + hipGetErrorString((hipError_t)bad.load()); return LCR_E_DEVICE; }
  return LCR_OK;
}

namespace {

// ---- the 16 arrays of a batch, once.  Position in the list = slot in lcr_ctx::in_[] / UploadSlot::buf[]; the caller's pointer lies in
// lcr_reads or lcr_regions (an UploadSlot's device-resident header has the same fields); the device address goes to a field of BatchView.
enum BatchCount { N_READS, N_BASES, N_CIGAR, N_REGIONS, N_REGIONS_1, N_COLS };
struct BatchArray { bool of_regions; size_t src; size_t elem; BatchCount count; size_t view; };
#define RD_ARRAY(field, count, view) {false, offsetof(lcr_reads, field), sizeof(*((const lcr_reads*)nullptr)->field), count, offsetof(BatchView, view)}
#define RG_ARRAY(field, count) {true, offsetof(lcr_regions, field), sizeof(*((const lcr_regions*)nullptr)->field), count, offsetof(BatchView, field)}
const BatchArray BATCH_ARRAYS[16] = {
  RD_ARRAY(pos, N_READS, pos), RD_ARRAY(seq_len, N_READS, seq_len), RD_ARRAY(lead_clip, N_READS, lead), RD_ARRAY(trail_clip, N_READS, trail),
  RD_ARRAY(flags, N_READS, flags), RD_ARRAY(seq_off, N_READS, seq_off), RD_ARRAY(cig_off, N_READS, cig_off), RD_ARRAY(n_cig, N_READS, n_cig),
  RD_ARRAY(bases, N_BASES, bases), RD_ARRAY(quals, N_BASES, quals), RD_ARRAY(cigar, N_CIGAR, cigar),
  RG_ARRAY(start0, N_REGIONS), RG_ARRAY(len, N_REGIONS), RG_ARRAY(col_off, N_REGIONS_1), RG_ARRAY(read_begin, N_REGIONS_1), RG_ARRAY(ref, N_COLS),
};
#undef RD_ARRAY
#undef RG_ARRAY

size_t array_bytes(const BatchArray& a, const lcr_reads* rd, const lcr_regions* rg, int64_t n_cols) {
  int64_t n = 0;
  switch (a.count) {
    case N_READS: n = rd->n_reads; break;
    case N_BASES: n = rd->n_bases; break;
    case N_CIGAR: n = rd->n_cigar; break;
    case N_REGIONS: n = rg->n_regions; break;
    case N_REGIONS_1: n = (int64_t)rg->n_regions + 1; break;
    case N_COLS: n = n_cols; break;
  }
  return (size_t)n * a.elem;
}
// the pointer field at byte `off` of a header struct (lcr_reads / lcr_regions / BatchView)
const void* get_ptr(const void* obj, size_t off) { const void* p; memcpy(&p, (const char*)obj + off, sizeof p); return p; }
void set_ptr(void* obj, size_t off, const void* p) { memcpy((char*)obj + off, &p, sizeof p); }
const void* array_src(const BatchArray& a, const lcr_reads* rd, const lcr_regions* rg) { return get_ptr(a.of_regions ? (const void*)rg : (const void*)rd, a.src); }
constexpr int A_SEQ_LEN = 1, A_SEQ_OFF = 5, A_BASES = 8;   // places in BATCH_ARRAYS

// ---- a packed batch (lcr_reads_packed) is its plain header without bases, plus what stands in their place
struct PackedSrc { const uint64_t* pack_off; const uint8_t* seq4; int64_t n_pack; };
lcr_reads plain_header(const lcr_reads_packed* p) {
  lcr_reads r{};
  r.mem = p->mem; r.n_reads = p->n_reads; r.n_bases = p->n_bases; r.n_cigar = p->n_cigar;
  r.pos = p->pos; r.seq_len = p->seq_len; r.lead_clip = p->lead_clip; r.trail_clip = p->trail_clip; r.flags = p->flags;
  r.seq_off = p->seq_off; r.cig_off = p->cig_off; r.n_cig = p->n_cig; r.quals = p->quals; r.cigar = p->cigar;
  return r;
}
// the three layout rules of include/lcr.h on a host batch, in front of any work (a device batch: the same test in k0_unpack)
int check_packed_host(lcr_ctx* c, const lcr_reads* rd, const PackedSrc& pk) {
  if (pk.n_pack < 0 || rd->n_bases < 0) { c->err = "packed batch: negative n_pack / n_bases"; return LCR_E_ARG; }
  const int nr = rd->n_reads;
  if (nr && (!rd->seq_len || !rd->seq_off || !pk.pack_off || (pk.n_pack && !pk.seq4))) { c->err = "packed batch: null array"; return LCR_E_ARG; }
  for (int r = 0; r < nr; r++) {
    const int64_t L = rd->seq_len[r];
    const uint64_t so = rd->seq_off[r], po = pk.pack_off[r];
    if (L < 0 || so > (uint64_t)rd->n_bases || (uint64_t)L > (uint64_t)rd->n_bases - so || po > (uint64_t)pk.n_pack ||
        (uint64_t)((L + 1) >> 1) > (uint64_t)pk.n_pack - po) {
      c->err = "packed batch: read " + std::to_string(r) + " leaves bases (seq_off + seq_len > n_bases), seq4 (pack_off + (seq_len + 1) / 2 > n_pack) or has a negative length";
      return LCR_E_ARG;
    }
  }
  return LCR_OK;
}
// the unpack kernel on queue q, with its verdict word cleared (every earlier launch that could raise it has been waited for) and, when
// timing is on, its two events (lcr_unpack_ms)
int queue_unpack(lcr_ctx* c, int32_t nr, const int32_t* seq_len, const uint64_t* seq_off, const uint64_t* pack_off, const uint8_t* seq4, int64_t n_pack,
                 uint8_t* out, int64_t n_bases, hipStream_t q) {
  HIPCHK(c, c->h_unpack_bad.reserve(64));
  *c->h_unpack_bad.as<int32_t>() = 0;
  if (nr == 0) return LCR_OK;
  int32_t* d_bad = nullptr;
  HIPCHK(c, c->h_unpack_bad.dev(&d_bad));
  if (c->timing && !c->ev_unpack_t[0]) for (hipEvent_t& e : c->ev_unpack_t) HIPCHK(c, hipEventCreate(&e));
  if (c->timing) HIPCHK(c, hipEventRecord(c->ev_unpack_t[0], q));
  launch_k0_unpack(nr, seq_len, seq_off, pack_off, seq4, n_pack, out, n_bases, d_bad, q);
  if (c->timing) { HIPCHK(c, hipEventRecord(c->ev_unpack_t[1], q)); c->unpack_timed = true; }
  HIPCHK(c, hipGetLastError());
  return LCR_OK;
}

// BatchView's 16 input pointers: the caller's own arrays (LCR_MEM_DEVICE) or copies in in_[] queued on the context's stream.  pk: a packed
// host batch -- its nibbles are copied and unpacked into in_[] where a plain batch's bases are copied (seq_len and seq_off are queued by then).
int bind_arrays(lcr_ctx* c, const lcr_reads* rd, const lcr_regions* rg, const PackedSrc* pk) {
  for (int i = 0; i < 16; i++) {
    const BatchArray& a = BATCH_ARRAYS[i];
    const void* p = array_src(a, rd, rg);
    if (rd->mem != LCR_MEM_DEVICE && pk && i == A_BASES) {
      const uint64_t* d_po = nullptr; const uint8_t* d_s4 = nullptr;
      HIPCHK(c, c->in_[i].reserve(std::max<size_t>((size_t)rd->n_bases, 1)));
      { const int rc = upload(c, c->in_pack_off, pk->pack_off, (size_t)rd->n_reads, &d_po, LCR_MEM_HOST); if (rc) return rc; }
      { const int rc = upload(c, c->in_seq4, pk->seq4, (size_t)pk->n_pack, &d_s4, LCR_MEM_HOST); if (rc) return rc; }
      { const int rc = queue_unpack(c, rd->n_reads, c->in_[A_SEQ_LEN].as<int32_t>(), c->in_[A_SEQ_OFF].as<uint64_t>(), d_po, d_s4, pk->n_pack,
                                    c->in_[i].as<uint8_t>(), rd->n_bases, c->stream); if (rc) return rc; }
      p = c->in_[i].p;
    } else if (rd->mem != LCR_MEM_DEVICE) {
      const size_t bytes = array_bytes(a, rd, rg, c->n_cols);
      HIPCHK(c, c->in_[i].reserve(std::max<size_t>(bytes, 1)));
      if (bytes) { const int rc = upload_bytes(c, c->in_[i].p, p, bytes); if (rc) return rc; }
      p = c->in_[i].p;
    }
    set_ptr(&c->bv, a.view, p);
  }
  return LCR_OK;
}

// host copies of the small per-region arrays (start0, len, col_off, read_begin).  A device-resident batch: one kernel writes the four
// into pinned host memory, one wait; the same launch and the same wait bring the geometry of the flat op space into h_order (first op,
// end of the last read's ops, "CIGARs lie back to back") and the regions' first tiles.
int fetch_region_tables(lcr_ctx* c, const lcr_reads* rd, const lcr_regions* rg) {
  const int nr = rd->n_reads, ng = rg->n_regions;
  c->h_start0.assign(ng, 0); c->h_len.assign(ng, 0); c->h_col_off.assign(ng + 1, 0); c->h_read_begin.assign(ng + 1, 0);
  if (rd->mem == LCR_MEM_HOST) {
    if (ng) { memcpy(c->h_start0.data(), rg->start0, ng * sizeof(int64_t)); memcpy(c->h_len.data(), rg->len, ng * sizeof(int32_t)); }
    memcpy(c->h_col_off.data(), rg->col_off, (ng + 1) * sizeof(int64_t));
    memcpy(c->h_read_begin.data(), rg->read_begin, (ng + 1) * sizeof(int32_t));
    return LCR_OK;
  }
  const size_t o1 = (size_t)ng * 8, o2 = o1 + (size_t)(ng + 1) * 8, o3 = o2 + (size_t)ng * 4, tot = o3 + (size_t)(ng + 1) * 4;
  HIPCHK(c, c->h_stage[0].reserve(tot + 16));
  HIPCHK(c, c->first_tile.reserve((ng + 1) * 4));
  uint8_t* st = c->h_stage[0].as<uint8_t>();
  uint8_t* dst = nullptr;   // the pinned buffer as the device sees it
  HIPCHK(c, c->h_stage[0].dev(&dst));
  HIPCHK(c, c->h_order.reserve(64));
  memset(c->h_order.p, 0, 64);
  { int32_t* d_flag = nullptr; HIPCHK(c, c->h_order.dev(&d_flag));
    Timer t(c, LCR_K_BIND_TABLE);
    launch_k0_bind_a(rg->start0, rg->len, rg->col_off, rg->read_begin, ng, c->first_tile.as<int32_t>(), (int64_t*)dst,
                     (int32_t*)(dst + o2), (int64_t*)(dst + o1), (int32_t*)(dst + o3), rd->cig_off, rd->n_cig, nr, rd->n_cigar, d_flag, c->stream); }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  if (ng) { memcpy(c->h_start0.data(), st, ng * sizeof(int64_t)); memcpy(c->h_len.data(), st + o2, ng * sizeof(int32_t)); }
  memcpy(c->h_col_off.data(), st + o1, (ng + 1) * sizeof(int64_t));
  memcpy(c->h_read_begin.data(), st + o3, (ng + 1) * sizeof(int32_t));
  return LCR_OK;
}

int check_region_tables(lcr_ctx* c, int nr, int ng) {
  if (c->h_read_begin[ng] != nr || c->h_col_off[0] != 0) { c->err = "read_begin/col_off inconsistent"; return LCR_E_ARG; }
  for (int g = 0; g < ng; g++)
    if (c->h_len[g] < 0 || c->h_col_off[g + 1] - c->h_col_off[g] != c->h_len[g] || c->h_read_begin[g + 1] < c->h_read_begin[g]) {
      c->err = "region table inconsistent"; return LCR_E_ARG;
    }
  c->n_cols = c->h_col_off[ng];
  // (tile column origins and the intron difference array are indexed with int32)
  if (c->n_cols + ng + 1 > (int64_t)INT32_MAX) { c->err = "batch too large: columns + regions must stay below 2^31; split it"; return LCR_E_ARG; }
  return LCR_OK;
}

// tile table: tiles never cross a region; the host only needs the tile count, the table is built on the device.  Also the per-read
// tables K0 derives (BatchView::read_rend / read_region / region_first_tile, the packed headers).
int reserve_tile_tables(lcr_ctx* c, int mem) {
  BatchView& b = c->bv;
  const int nr = b.n_reads, ng = b.n_regions;
  c->h_region_first_tile.assign(ng + 1, 0);
  for (int g = 0; g < ng; g++) c->h_region_first_tile[g + 1] = c->h_region_first_tile[g] + (c->h_len[g] + LCR_TILE - 1) / LCR_TILE;
  c->n_tiles = c->h_region_first_tile[ng];
  HIPCHK(c, c->tile_region.reserve(std::max<size_t>(c->n_tiles, 1) * 4));
  HIPCHK(c, c->tile_col0.reserve(std::max<size_t>(c->n_tiles, 1) * 4));
  HIPCHK(c, c->first_tile.reserve((ng + 1) * 4));
  if (mem == LCR_MEM_HOST)   // (a device-resident batch had its prefix sums computed with the region fetch: fetch_region_tables)
    launch_k0_region_setup(b.start0, b.len, b.col_off, b.read_begin, ng, c->first_tile.as<int32_t>(), nullptr, nullptr, nullptr, nullptr, c->stream);
  HIPCHK(c, c->read_rend.reserve(std::max<size_t>(nr, 1) * 4));
  b.read_rend = c->read_rend.as<int32_t>();
  HIPCHK(c, c->read_region.reserve(std::max(nr, 1) * 4));
  b.read_region = c->read_region.as<int32_t>();
  b.region_first_tile = c->first_tile.as<int32_t>(); b.error_flag = nullptr;   // set by lcr_pileup
  HIPCHK(c, c->read_bin.reserve(std::max<size_t>(nr, 1) * sizeof(ReadBin)));
  return LCR_OK;
}

// ---- the flat op space of K0 (k0_ops.hip): ops [cig0, cig0 + n_ops) of bv.cigar, read after read.  Checks the caller's cig_off / n_cig
// (on the host for a host batch; k0_cig_check's verdict, waited for in fetch_region_tables, for a device-resident one) and copies
// CIGARs that do not lie back to back once.  Leaves h_order's order flag cleared for k0_bind_b.
int bind_op_space(lcr_ctx* c, const lcr_reads* rd) {
  BatchView& b = c->bv;
  const int nr = rd->n_reads;
  bool contiguous = true, cig_oob = false;
  uint64_t cig0 = 0, cig_end = 0, cig_total = 0;
  if (rd->mem == LCR_MEM_HOST) {
    HIPCHK(c, c->h_order.reserve(64));
    // (a device-resident batch bound before this one returned without a wait: its k0_pack may still be about to raise the flag)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memset(c->h_order.p, 0, 64);
    if (nr) { cig0 = rd->cig_off[0]; cig_end = rd->cig_off[nr - 1] + rd->n_cig[nr - 1]; }
    for (int r = 0; r + 1 < nr && contiguous; r++) contiguous = rd->cig_off[r + 1] == rd->cig_off[r] + rd->n_cig[r];
    for (int r = 0; r < nr; r++) {   // (any layout: every read's ops inside the caller's array; the total in 64 bits)
      cig_total += rd->n_cig[r];
      cig_oob |= rd->cig_off[r] > (uint64_t)rd->n_cigar || (uint64_t)rd->n_cig[r] > (uint64_t)rd->n_cigar - rd->cig_off[r];
    }
  } else {
    const uint64_t* g = reinterpret_cast<const uint64_t*>(c->h_order.as<uint8_t>() + 16);   // written by k0_cig_check, waited for in fetch_region_tables
    contiguous = c->h_order.as<int32_t>()[1] == 0;
    cig_oob = c->h_order.as<int32_t>()[2] != 0;
    cig0 = g[0]; cig_end = g[1];
  }
  if (cig_oob) { c->err = "cig_off / n_cig reach beyond n_cigar"; return LCR_E_ARG; }
  // (every read lies inside [0, n_cigar): a total beyond 2^31 needs n_cigar beyond it or overlapping reads -- the scan below is int32)
  if (!contiguous && (rd->n_cigar > 0x7FFFFFF0ll || cig_total > 0x7FFFFFF0ull)) { c->err = "batch too large: CIGAR ops must stay below 2^31; split it"; return LCR_E_ARG; }
  if (!contiguous) {   // the ABI allows any cig_off: copy the CIGARs back to back once (rare; every producer here is contiguous)
    HIPCHK(c, c->cig_new_off32.reserve(((size_t)nr + 2) * 4));
    HIPCHK(c, c->cig_off_new.reserve(std::max<size_t>(nr, 1) * 8));
    int32_t* total = c->cig_new_off32.as<int32_t>() + nr;
    launch_scan_i32(c->scan_tmp, (const int32_t*)b.n_cig, c->cig_new_off32.as<int32_t>(), nr, total, c->stream);
    int32_t h_total = 0;
    HIPCHK(c, hipMemcpyAsync(&h_total, total, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h_total < 0) { c->err = "batch too large: CIGAR ops must stay below 2^31; split it"; return LCR_E_ARG; }
    HIPCHK(c, c->cig_compact.reserve(std::max<size_t>((size_t)h_total, 1) * 4));
    launch_k0_cig_compact(b.cigar, b.cig_off, b.n_cig, c->cig_new_off32.as<int32_t>(), nr, c->cig_compact.as<uint32_t>(),
                          c->cig_off_new.as<uint64_t>(), c->stream);
    b.cigar = c->cig_compact.as<uint32_t>(); b.cig_off = c->cig_off_new.as<uint64_t>();
    cig0 = 0; cig_end = (uint64_t)h_total;
  }
  if (cig_end < cig0 || cig_end - cig0 > 0xFFF00000ull || (contiguous && cig_end > (uint64_t)std::max<int64_t>(rd->n_cigar, 0))) {
    c->err = "cig_off / n_cig inconsistent with n_cigar, or more than 2^32 CIGAR ops in one batch"; return LCR_E_ARG;
  }
  c->cig0 = cig0; c->n_ops = (uint32_t)(cig_end - cig0);
  *c->h_order.as<int32_t>() = 0;   // (the previous batch's k0_pack finished long ago: every lcr_pileup waits behind it)
  return LCR_OK;
}

// ONE launch: read -> region and tile tables, the packed read headers, the order check, the op blocks' first reads (k0_bind_b)
int queue_bind_tables(lcr_ctx* c) {
  int32_t* d_flag = nullptr;
  HIPCHK(c, c->h_order.dev(&d_flag));
  const int opb = launch_k0_opb();
  const int32_t n_blocks = (int32_t)(((uint64_t)c->n_ops + opb - 1) / opb);
  HIPCHK(c, c->blk_first_read.reserve(((size_t)n_blocks + 2) * 4));
  Timer t(c, LCR_K_BIND);
  launch_k0_bind_b(c->bv, c->read_bin.as<ReadBin>(), d_flag, c->read_region.as<int32_t>(), c->n_tiles, c->tile_region.as<int32_t>(), c->tile_col0.as<int32_t>(),
                   c->cig0, opb, n_blocks, c->blk_first_read.as<int32_t>(), c->stream);
  return LCR_OK;
}

// lcr_load_batch, and lcr_load_batch_packed with pk: the packed form differs in where the bases come from and in nothing else
int load_common(lcr_ctx* c, const lcr_reads* rd_in, const lcr_regions* rg, const PackedSrc* pk) {
  lcr_reads rd_ = *rd_in;
  const lcr_reads* rd = &rd_;
  if (rd->n_reads < 0 || rg->n_regions < 0 || rd->mem != rg->mem || (pk && rd->mem != LCR_MEM_HOST && rd->mem != LCR_MEM_DEVICE)) { c->err = "bad batch header"; return LCR_E_ARG; }
  if (pk && rd->mem == LCR_MEM_HOST) { const int rc = check_packed_host(c, rd, *pk); if (rc) return rc; }
  if (pk && rd->mem == LCR_MEM_DEVICE && (pk->n_pack < 0 || rd->n_bases < 0)) { c->err = "packed batch: negative n_pack / n_bases"; return LCR_E_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  // a device-resident batch may be bound (and its pileup queued) while the previous batch's phase stage is still running: nothing
  // here or in lcr_pileup touches what that stage reads.  A host batch is copied into the context's staging buffers, which hold
  // the previous batch's region table: the stage has to be done first.  So it has for a packed device batch, which is unpacked into
  // the one buffer that may hold the bases of the batch whose stage is in flight.
  if (rd->mem == LCR_MEM_HOST || pk) { int rc = phase_settle(c); if (rc) return rc; }
  rewind_to(c, ST_NONE);   // (from here on the host tables, BatchView and -- a host batch -- in_[] are rewritten)
  c->bound_slot = -1;
  c->bound_host = rd->mem == LCR_MEM_HOST;
  const int nr = rd->n_reads, ng = rg->n_regions, mem = rd->mem;
  int rc;
  if (pk && mem == LCR_MEM_DEVICE) {   // the unpack in front of the one wait of fetch_region_tables, which delivers its verdict too
    HIPCHK(c, c->unpacked.reserve(std::max<size_t>((size_t)rd->n_bases, 1)));
    if ((rc = queue_unpack(c, nr, rd->seq_len, rd->seq_off, pk->pack_off, pk->seq4, pk->n_pack, c->unpacked.as<uint8_t>(), rd->n_bases, c->stream))) return rc;
    rd_.bases = c->unpacked.as<uint8_t>();
  }
  if ((rc = fetch_region_tables(c, rd, rg))) return rc;
  if (pk && mem == LCR_MEM_DEVICE && *c->h_unpack_bad.as<int32_t>()) {
    c->err = "packed batch: a read leaves bases (seq_off + seq_len > n_bases), seq4 (pack_off + (seq_len + 1) / 2 > n_pack) or has a negative length";
    return LCR_E_ARG;
  }
  if ((rc = check_region_tables(c, nr, ng))) return rc;
  c->n_bases = rd->n_bases; c->n_cigar = rd->n_cigar;
  c->bv.n_reads = nr; c->bv.n_regions = ng; c->bv.n_bases = rd->n_bases;
  if ((rc = bind_arrays(c, rd, rg, pk))) return rc;
  if ((rc = reserve_tile_tables(c, mem))) return rc;
  if ((rc = bind_op_space(c, rd))) return rc;
  if ((rc = queue_bind_tables(c))) return rc;
  // host batch: the caller's arrays are free again when this returns; device batch: no wait, the next stage queues
  // behind these kernels on the same stream (the arrays stay the caller's to keep alive, include/lcr.h)
  if (mem == LCR_MEM_HOST) HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  c->stage = ST_LOADED;
  return LCR_OK;
}

// lcr_load_batch_async, and lcr_load_batch_packed_async with pk: the nibbles cross the link in place of the bases, and the unpack kernel
// writes the slot's bases on the upload stream in front of the slot's event
int load_async_common(lcr_ctx* c, const lcr_reads* rd, const lcr_regions* rg, int32_t slot, const PackedSrc* pk) {
  if (slot < 0 || slot > 1) { c->err = "lcr_load_batch_async: slot must be 0 or 1"; return LCR_E_ARG; }
  if (rd->mem != LCR_MEM_HOST || rg->mem != LCR_MEM_HOST) { c->err = "lcr_load_batch_async takes LCR_MEM_HOST batches (a device-resident batch needs no upload)"; return LCR_E_ARG; }
  if (rd->n_reads < 0 || rg->n_regions < 0 || rd->n_bases < 0 || rd->n_cigar < 0) { c->err = "bad batch header"; return LCR_E_ARG; }
  if (pk) { const int rc = check_packed_host(c, rd, *pk); if (rc) return rc; }
  HIPCHK(c, hipSetDevice(c->device));
  // a phase stage in flight reads the region table of ITS batch: it has to be done only if that batch lives in the slot rewritten here
  // (two slots alternate: batch k + 1 is uploaded while batch k's stage runs -- lcr_collect_phase fetches batch k's results afterwards)
  if (c->phase.pending && c->phase_slot == slot) { int rc = phase_settle(c); if (rc) return rc; }
  if (!c->up_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking));
  lcr_ctx::UploadSlot& u = c->up[slot];
  if (!u.ev) HIPCHK(c, hipEventCreateWithFlags(&u.ev, hipEventDisableTiming));
  if (c->bound_slot == slot) {   // the bound batch lives in this slot: its kernels must be done before it is overwritten
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rewind_to(c, ST_NONE);
    c->bound_slot = -1;
  }
  u.filled = false;
  const int nr = rd->n_reads, ng = rg->n_regions;
  int64_t n_cols = 0;
  if (ng) { if (!rg->col_off) { c->err = "col_off missing"; return LCR_E_ARG; } n_cols = rg->col_off[ng]; }
  if (n_cols < 0) { c->err = "region table inconsistent"; return LCR_E_ARG; }
  u.rd = lcr_reads{}; u.rg = lcr_regions{};
  u.rd.mem = LCR_MEM_DEVICE; u.rg.mem = LCR_MEM_DEVICE;
  u.rd.n_reads = nr; u.rd.n_bases = rd->n_bases; u.rd.n_cigar = rd->n_cigar; u.rg.n_regions = ng;
  for (int i = 0; i < 16; i++) {   // the slot's header names the copies: a device-resident batch for lcr_bind_batch
    const BatchArray& a = BATCH_ARRAYS[i];
    const void* src = array_src(a, rd, rg);
    const size_t bytes = array_bytes(a, rd, rg, n_cols);
    HIPCHK(c, u.buf[i].reserve(std::max<size_t>(bytes, 1)));
    if (bytes && !(pk && i == A_BASES)) {
      if (!src) { c->err = "lcr_load_batch_async: null array"; return LCR_E_ARG; }
      { const int rc2 = upload_bytes(c, u.buf[i].p, src, bytes, c->up_stream); if (rc2) return rc2; }   // (page-locked arrays: asynchronous; pageable ones are staged)
    }
    set_ptr(a.of_regions ? (void*)&u.rg : (void*)&u.rd, a.src, u.buf[i].p);
  }
  if (pk) {
    HIPCHK(c, u.pack_off.reserve(std::max<size_t>(nr, 1) * 8));
    HIPCHK(c, u.seq4.reserve(std::max<size_t>((size_t)pk->n_pack, 1)));
    if (nr) { const int rc2 = upload_bytes(c, u.pack_off.p, pk->pack_off, (size_t)nr * 8, c->up_stream); if (rc2) return rc2; }
    if (pk->n_pack) { const int rc2 = upload_bytes(c, u.seq4.p, pk->seq4, (size_t)pk->n_pack, c->up_stream); if (rc2) return rc2; }
    { const int rc2 = queue_unpack(c, nr, u.buf[A_SEQ_LEN].as<int32_t>(), u.buf[A_SEQ_OFF].as<uint64_t>(), u.pack_off.as<uint64_t>(), u.seq4.as<uint8_t>(),
                                   pk->n_pack, u.buf[A_BASES].as<uint8_t>(), rd->n_bases, c->up_stream); if (rc2) return rc2; }
  }
  HIPCHK(c, hipEventRecord(u.ev, c->up_stream));
  u.filled = true;
  return LCR_OK;
}

}  // namespace

extern "C" {

int lcr_load_batch(lcr_ctx* c, const lcr_reads* rd, const lcr_regions* rg) {
  if (!c || !rd || !rg) return LCR_E_ARG;
  return load_common(c, rd, rg, nullptr);
}

int lcr_load_batch_packed(lcr_ctx* c, const lcr_reads_packed* rp, const lcr_regions* rg) {
  if (!c || !rp || !rg) return LCR_E_ARG;
  const lcr_reads rd = plain_header(rp);
  const PackedSrc pk{rp->pack_off, rp->seq4, rp->n_pack};
  return load_common(c, &rd, rg, &pk);
}

int lcr_load_batch_async(lcr_ctx* c, const lcr_reads* rd, const lcr_regions* rg, int32_t slot) {
  if (!c || !rd || !rg) return LCR_E_ARG;
  return load_async_common(c, rd, rg, slot, nullptr);
}

int lcr_load_batch_packed_async(lcr_ctx* c, const lcr_reads_packed* rp, const lcr_regions* rg, int32_t slot) {
  if (!c || !rp || !rg) return LCR_E_ARG;
  const lcr_reads rd = plain_header(rp);
  const PackedSrc pk{rp->pack_off, rp->seq4, rp->n_pack};
  return load_async_common(c, &rd, rg, slot, &pk);
}

int lcr_unpack_bases(lcr_ctx* c, int32_t n_reads, const int32_t* seq_len, const uint64_t* seq_off, const uint64_t* pack_off, const uint8_t* seq4,
                     int64_t n_pack, uint8_t* bases_out, int64_t n_bases) {
  if (!c) return LCR_E_ARG;
  if (n_reads < 0 || n_pack < 0 || n_bases < 0) { c->err = "lcr_unpack_bases: negative size"; return LCR_E_ARG; }
  if (n_reads && (!seq_len || !seq_off || !pack_off || (n_pack && !seq4) || (n_bases && !bases_out))) { c->err = "lcr_unpack_bases: null array"; return LCR_E_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  { const int rc = queue_unpack(c, n_reads, seq_len, seq_off, pack_off, seq4, n_pack, bases_out, n_bases, c->stream); if (rc) return rc; }
  if (n_reads == 0) return LCR_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  if (*c->h_unpack_bad.as<int32_t>()) {
    c->err = "lcr_unpack_bases: a read leaves bases_out (seq_off + seq_len > n_bases), seq4 (pack_off + (seq_len + 1) / 2 > n_pack) or has a negative length";
    return LCR_E_ARG;
  }
  return LCR_OK;
}

int lcr_unpack_ms(lcr_ctx* c, float* ms) {
  if (!c || !ms) return LCR_E_ARG;
  if (!c->timing || !c->unpack_timed) { c->err = "lcr_unpack_ms: no unpack kernel with timing enabled"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(c->ev_unpack_t[1]));
  HIPCHK(c, hipEventElapsedTime(ms, c->ev_unpack_t[0], c->ev_unpack_t[1]));
  return LCR_OK;
}

int lcr_bind_batch(lcr_ctx* c, int32_t slot) {
  if (!c) return LCR_E_ARG;
  if (slot < 0 || slot > 1) { c->err = "lcr_bind_batch: slot must be 0 or 1"; return LCR_E_ARG; }
  lcr_ctx::UploadSlot& u = c->up[slot];
  if (!u.filled) { c->err = "lcr_bind_batch before lcr_load_batch_async on this slot"; return LCR_E_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamWaitEvent(c->stream, u.ev, 0));   // the ctx stream continues behind the slot's upload
  const int rc = lcr_load_batch(c, &u.rd, &u.rg);      // (device-resident form: region tables fetched with one wait; the upload is complete when it returns)
  if (rc == LCR_OK) c->bound_slot = slot;
  return rc;
}

int lcr_host_alloc(size_t bytes, void** out) {
  if (!out) return LCR_E_ARG;
  *out = nullptr;
  return hipHostMalloc(out, std::max<size_t>(bytes, 1), hipHostMallocDefault) == hipSuccess ? LCR_OK : LCR_E_NOMEM;
}
void lcr_host_free(void* p) { if (p) (void)hipHostFree(p); }
int lcr_host_register(void* p, size_t bytes) {
  if (!p || !bytes) return LCR_E_ARG;
  return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? LCR_OK : LCR_E_DEVICE;
}
int lcr_host_unregister(void* p) { return p && hipHostUnregister(p) == hipSuccess ? LCR_OK : LCR_E_ARG; }

}  // extern "C"

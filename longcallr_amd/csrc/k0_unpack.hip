// k0_unpack.hip — BAM 4-bit bases -> the ASCII bases the stages read, in HBM (lcr_load_batch_packed, lcr_load_batch_packed_async,
// lcr_unpack_bases of include/lcr.h).  A streaming kernel: n_pack bytes in, n_bases bytes out.
//
// One wave per read.  A read's output range [seq_off, seq_off + seq_len) starts anywhere: up to 15 bases by single bytes bring the
// address to a 16-byte boundary (the head), then every lane writes 16-base pieces with one aligned 16-byte store, 64 pieces = 1 024
// bases per round of the wave, then up to 15 single bases (the tail).  Head and tail take one pass: lanes 0-15 and 16-31.  The source of
// a piece is unaligned -- and when the head is odd it starts on a low nibble and spans 9 bytes --: three aligned dwords around it,
// funnel-shifted, where those twelve bytes lie inside the caller's seq4 array; byte loads inside the read's own range at the array's
// two edges.  (Measured and rejected, DESIGN.md section 1h: one 8-byte load per lane with the third dword taken from the next lane.)  Nothing outside a read's range is written; a read whose ranges leave the arrays is skipped whole before any address is
// formed from its offsets, and raises the verdict word.
#include "k0_unpack.h"
#include "lcr_dev.h"

namespace {

__global__ __launch_bounds__(LCR_BLOCK) void k0_unpack(int32_t nr, const int32_t* __restrict__ seq_len, const uint64_t* __restrict__ seq_off,
                                                       const uint64_t* __restrict__ pack_off, const uint8_t* __restrict__ seq4, int64_t n_pack,
                                                       uint8_t* __restrict__ out, int64_t n_bases, int32_t* bad /* pinned host memory */) {
  const int64_t r = ((int64_t)blockIdx.x * LCR_BLOCK + threadIdx.x) / LCR_WAVE;
  const int lane = threadIdx.x & (LCR_WAVE - 1);
  if (r >= nr) return;
  const int64_t L = seq_len[r];
  const uint64_t so = seq_off[r], po = pack_off[r];
  // the guard, in 64 bits, in front of every use of the offsets (n_pack, n_bases >= 0: the launcher's callers)
  if (L < 0 || so > (uint64_t)n_bases || (uint64_t)L > (uint64_t)n_bases - so || po > (uint64_t)n_pack ||
      (uint64_t)((L + 1) >> 1) > (uint64_t)n_pack - po) {
    if (lane == 0) *bad = 1;
    return;
  }
  uint8_t* o = out + so;
  const uint8_t* s = seq4 + po;
  const int64_t head = min(L, (int64_t)((16u - (uint32_t)((uintptr_t)o & 15u)) & 15u));
  const int64_t nbody = (L - head) >> 4;
  const int64_t t0 = head + (nbody << 4);
  {   // head (lanes 0-15) and tail (lanes 16-31): one base per lane
    const int64_t i = lane < 16 ? lane : t0 + (lane - 16);
    const bool on = lane < 16 ? lane < head : (lane < 32 && i < L);
    if (on) { const uint32_t v = s[i >> 1]; o[i] = unpack_nt16((i & 1) ? (v & 15u) : (v >> 4)); }
  }
  const int odd = (int)(head & 1);   // every piece of the read starts on the same nibble parity
  const uintptr_t a_lo = (uintptr_t)seq4, a_hi = (uintptr_t)seq4 + (uint64_t)n_pack;
  for (int64_t p = lane; p < nbody; p += LCR_WAVE) {
    const int64_t i = head + (p << 4);
    const uint8_t* sp = s + (i >> 1);   // bytes sp[0 .. 7], and sp[8] when odd, belong to the read
    const uintptr_t a = (uintptr_t)sp & ~(uintptr_t)3;
    uint64_t x; uint32_t b8;
    if (a >= a_lo && a + 12 <= a_hi) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(a);
      const uint32_t sh = (uint32_t)((uintptr_t)sp & 3u);
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
      x = (uint64_t)__builtin_amdgcn_alignbyte(w1, w0, sh) | ((uint64_t)__builtin_amdgcn_alignbyte(w2, w1, sh) << 32);
      b8 = (w2 >> (8u * sh)) & 0xffu;
    } else {
      x = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) x |= (uint64_t)sp[k] << (8 * k);
      b8 = odd ? sp[8] : 0u;
    }
    uint32_t q[4];
    unpack16(x, b8, odd, q);
    *reinterpret_cast<uint4*>(o + i) = make_uint4(q[0], q[1], q[2], q[3]);
  }
}

}  // namespace

void launch_k0_unpack(int32_t nr, const int32_t* seq_len, const uint64_t* seq_off, const uint64_t* pack_off, const uint8_t* seq4, int64_t n_pack,
                      uint8_t* out, int64_t n_bases, int32_t* bad, hipStream_t s) {
  if (nr <= 0) return;
  const unsigned blocks = (unsigned)(((int64_t)nr * LCR_WAVE + LCR_BLOCK - 1) / LCR_BLOCK);
  k0_unpack<<<blocks, LCR_BLOCK, 0, s>>>(nr, seq_len, seq_off, pack_off, seq4, n_pack, out, n_bases, bad);
}

// k0_unpack.h — BAM's 4-bit base codes -> ASCII: the arithmetic of k0_unpack.hip's 16-base piece and of its single bases.  Host and
// device: tests/packed_main.cpp runs the same functions on the CPU against a nibble-by-nibble expansion.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define UNPACK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define UNPACK_HD inline
#endif

// "=ACMGRSVTWYHKDBN" as four little-endian dwords: the table lives in registers (literals), not in memory
#define UNPACK_NT0 0x4d43413du   // = A C M
#define UNPACK_NT1 0x56535247u   // G R S V
#define UNPACK_NT2 0x48595754u   // T W Y H
#define UNPACK_NT3 0x4e42444bu   // K D B N

// the letter of one code
UNPACK_HD uint8_t unpack_nt16(uint32_t k) {
  const uint64_t lo = ((uint64_t)UNPACK_NT1 << 32) | UNPACK_NT0, hi = ((uint64_t)UNPACK_NT3 << 32) | UNPACK_NT2;
  return (uint8_t)(((k & 8u) ? hi : lo) >> (8u * (k & 7u)));
}

// byte k of the result = byte sel_k (0..7) of hi:lo  (v_perm_b32 with selectors below 8)
UNPACK_HD uint32_t unpack_perm8(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const uint64_t pool = ((uint64_t)hi << 32) | lo;
  uint32_t r = 0;
  for (int k = 0; k < 4; k++) r |= (uint32_t)((pool >> (8u * ((sel >> (8 * k)) & 7u))) & 0xffu) << (8 * k);
  return r;
#endif
}

// 16 bases as four dwords of ASCII.  odd == 0: the 16 nibbles of the 8 source bytes x (byte 0 in bits 0-7), high nibble first.
// odd == 1: the piece starts on a low nibble and spans 9 source bytes: nibbles 1 .. 16 of x and b8 (the ninth byte).
UNPACK_HD void unpack16(uint64_t x, uint32_t b8, int odd, uint32_t out[4]) {
  const uint64_t M = 0x0f0f0f0f0f0f0f0full;
  if (odd) x = ((x & M) << 4) | (((x >> 12) | ((uint64_t)b8 << 52)) & M);   // byte k = low nibble of byte k, high nibble of byte k + 1
#pragma unroll
  for (int d = 0; d < 4; d++) {
    const uint32_t h = (uint32_t)(x >> (16 * d)) & 0xffffu;
    const uint32_t t = (h & 0xffu) | ((h & 0xff00u) << 8);                          // the two source bytes in bytes 0 and 2
    const uint32_t n = ((t >> 4) & 0x000f000fu) | ((t & 0x000f000fu) << 8);          // the codes of bases 4d .. 4d + 3, one per byte
    const uint32_t s = n & 0x07070707u;
    const uint32_t lo = unpack_perm8(UNPACK_NT1, UNPACK_NT0, s), hi = unpack_perm8(UNPACK_NT3, UNPACK_NT2, s);
    const uint32_t m = ((n >> 3) & 0x01010101u) * 0xffu;                            // 0xff in the bytes whose code is 8 .. 15
    out[d] = (hi & m) | (lo & ~m);
  }
}

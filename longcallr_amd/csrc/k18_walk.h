// k18_walk.h — the gap walk of a read and the normalisation of a small indel over its equivalent placements (k18_indels.hip; the contract
// is lcr_indels', include/lcr.h).  k6_walk.h's walk sees N ops only and no query offsets; this one is a walk of its own.
#pragma once
#include "lcr_dev.h"

#ifdef __HIPCC__
// A C G T of either case -> 0..3, every other byte -> -1
__device__ __forceinline__ int k18_code(uint8_t c) {
  c &= 0xdfu;
  return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
}

// Sixteen lanes per read (one DPP row; four reads per wave64), ops spread over the lanes as in row16_walk_junctions.  Two row scans per round
// of 16 ops: the reference-consuming lengths (M D N = X) and the query-consuming ones (M I S = X; the walk starts at query offset 0, so a
// leading S counts and H does not), each with a carry between rounds.  A first pass over the ops sums rend, which decides whether an I or D
// has an aligned base behind it.  Every lane of a row takes the same branches and has to call.
//   gap(s, len, op, q, k) -> bool  runs in the lane of every gap: an N op of length >= 1, or an I / D op of length >= 1 with pos < s and
//        s + Lr < rend.  s: the contig column at the op; q: the offset of the op's first base in the read's bases; k: the gap's index in
//        the read (walk order).  It answers whether the gap is an event.
//   edge(col, d)  runs once per end of an aligned block (M = X D cover, only an N of length >= 1 breaks a block): d = +1 at the block's
//        first column, -1 at the column behind its last.
// *n_gap, *n_ev: the read's gaps and events; *rend: pos + all reference-consuming lengths (row-uniform).
template <class Gap, class Edge>
__device__ __forceinline__ void row16_walk_gaps(const BatchView& b, int r, Gap gap, Edge edge, int* n_gap, int* n_ev, int* rend_out) {
  const int lane = threadIdx.x & 63, l16 = lane & 15, rbase = lane & 48;
  const uint32_t ncig = b.n_cig[r];
  const uint32_t* __restrict__ cg = b.cigar + b.cig_off[r];
  const int pos = b.pos[r];
  int part = 0;
  for (uint32_t c = l16; c < ncig; c += 16) {
    const uint32_t w = cg[c];
    const int op = w & 15;
    part += (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? (int)(w >> 4) : 0;
  }
  const int rend = pos + __shfl(row16_incl_scan(part), rbase + 15, 64);
  int ref_cur = pos, q_cur = 0, ng = 0, ne = 0;
  int prev_kind = 2;   // of the last covering / N op in front of this round: 1 covers, 2 N; nothing yet counts as an N
  for (uint32_t c0 = 0; c0 < ncig; c0 += 16) {
    const uint32_t w = c0 + l16 < ncig ? cg[c0 + l16] : 0u;   // (a padding word is a 0-length M)
    const int op = w & 15, len = (int)(w >> 4);
    const bool cov = len >= 1 && (op == 0 || op == 2 || op == 7 || op == 8);
    const bool isn = len >= 1 && op == 3;
    const int dr = (cov || isn) ? len : 0;
    const int dq = (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) ? len : 0;
    const int ir = row16_incl_scan(dr), iq = row16_incl_scan(dq);
    const int s = ref_cur + ir - dr, q = q_cur + iq - dq;
    const int lr = op == 1 ? 0 : len;
    const bool is_gap = isn || (len >= 1 && (op == 1 || op == 2) && s > pos && (long long)s + lr < (long long)rend);
    const unsigned int below = (1u << l16) - 1u;
    const unsigned int mg = (unsigned int)(__ballot(is_gap) >> rbase) & 0xffffu;
    bool ev = false;
    if (is_gap) ev = gap(s, len, op, q, ng + __popc(mg & below));
    const unsigned int me = (unsigned int)(__ballot(ev) >> rbase) & 0xffffu;
    ng += __popc(mg); ne += __popc(me);
    const unsigned int mc = (unsigned int)(__ballot(cov) >> rbase) & 0xffffu;
    const unsigned int mn = (unsigned int)(__ballot(isn) >> rbase) & 0xffffu;
    const unsigned int before = (mc | mn) & below;
    const int pk = before ? (((mc >> (31 - __clz((int)before))) & 1u) ? 1 : 2) : prev_kind;
    if (cov && pk == 2) edge(s, 1);
    if (isn && pk == 1) edge(s, -1);
    const unsigned int all = mc | mn;
    if (all) prev_kind = ((mc >> (31 - __clz((int)all))) & 1u) ? 1 : 2;
    ref_cur += __shfl(ir, rbase + 15, 64);
    q_cur += __shfl(iq, rbase + 15, 64);
  }
  if (l16 == 0 && prev_kind == 1) edge(ref_cur, -1);
  *n_gap = ng; *n_ev = ne; *rend_out = ref_cur;
}

#define K18_MAX_SHIFT 1024

// The leftmost equivalent placement of an event inside the window [w0, w1) whose reference is wref (wref[0] = column w0).  type 0 DEL of
// len columns from s, type 1 INS of len bases (seq: 2 bits per base, first base lowest) in front of column s; *seq is rotated along.
// Preconditions: w0 + 1 <= s, and s + len <= w1 (DEL) or s <= w1 (INS).  A reference letter outside ACGT stops the shift; so do
// K18_MAX_SHIFT steps.
__device__ __forceinline__ long long k18_left_shift(const uint8_t* __restrict__ wref, long long w0, int type, long long s, int len, uint32_t* seq) {
  const int top = 2 * (len - 1);
  const uint32_t mask = len >= 16 ? ~0u : ((1u << (2 * len)) - 1u);
  uint32_t q = *seq;
  for (int step = 0; step < K18_MAX_SHIFT && s > w0 + 1; step++) {
    const int a = k18_code(wref[s - 1 - w0]);
    if (a < 0) break;
    if (type == 0) { if (a != k18_code(wref[s + len - 1 - w0])) break; }
    else { if ((uint32_t)a != ((q >> top) & 3u)) break; q = ((q << 2) & mask) | (uint32_t)a; }
    s--;
  }
  *seq = q;
  return s;
}

// The rightmost one, from the left-shifted form: for the extent only
__device__ __forceinline__ long long k18_right_shift(const uint8_t* __restrict__ wref, long long w0, long long w1, int type, long long s, int len, uint32_t seq) {
  const int top = 2 * (len - 1);
  for (int step = 0; step < K18_MAX_SHIFT; step++) {
    if (type == 0 ? s + len >= w1 : s >= w1) break;
    const int a = k18_code(wref[s - w0]);
    if (a < 0) break;
    if (type == 0) { if (a != k18_code(wref[s + len - w0])) break; }
    else { if ((uint32_t)a != (seq & 3u)) break; seq = (seq >> 2) | ((uint32_t)a << top); }
    s++;
  }
  return s;
}
#endif

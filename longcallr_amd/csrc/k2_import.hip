// k2_import.hip — the candidate stage of a caller that brings its own sites: SNPFrag::import_external_candidates
// (candidate.rs:530-613, called by thread.rs:107-116 with min_variant_qual = 0.0) on the pileup planes of the bound batch.
// Sites (pos0 ascending and unique, genotype code 0-4 of vcf.rs:440-446, QUAL as f32) are a flat list over the batch; a region
// takes the sites inside its columns [start0, start0 + len).  One wave per region: two binary searches for its slice, then the
// slice 64 sites at a time, kept sites ranked by ballot.  count -> exclusive scan (launch_scan_i32) -> emit.
#include "lcr_dev.h"
#include "k2_eval.h"

namespace {

// a site becomes a record: genotype 1 / 2 / 3 and a quality that is not below 0 (NaN is kept: `NaN < 0.0` is false, candidate.rs:550)
__device__ __forceinline__ bool site_kept(uint8_t gt, float q) { return gt >= 1 && gt <= 3 && !(q < 0.f); }

// first index in [lo, hi) with pos0[i] >= x
__device__ __forceinline__ int32_t lower_bound_i64(const int64_t* __restrict__ pos0, int32_t lo, int32_t hi, int64_t x) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (pos0[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(LCR_BLOCK)
k2_import_count(const int64_t* __restrict__ start0, const int32_t* __restrict__ len, int32_t n_regions, const int64_t* __restrict__ pos0,
                const uint8_t* __restrict__ gt, const float* __restrict__ qual, int32_t n_sites, int32_t* __restrict__ count) {
  const int g = (int)((blockIdx.x * (unsigned)LCR_BLOCK + threadIdx.x) / LCR_WAVE), lane = threadIdx.x & (LCR_WAVE - 1);
  if (g >= n_regions) return;
  const int32_t lo = lower_bound_i64(pos0, 0, n_sites, start0[g]);
  const int32_t hi = lower_bound_i64(pos0, lo, n_sites, start0[g] + len[g]);
  int32_t n = 0;
  for (int32_t i0 = lo; i0 < hi; i0 += LCR_WAVE) {
    const int32_t i = i0 + lane;
    n += __popcll(__ballot(i < hi && site_kept(gt[i], qual[i])));
  }
  if (lane == 0) count[g] = n;
}

// candidate.rs:545-600 for every kept site of region g, written at cand_off[g] + rank into the device records and the pinned host mirror
__global__ void __launch_bounds__(LCR_BLOCK)
k2_import_emit(const int64_t* __restrict__ start0, const int32_t* __restrict__ len, const int64_t* __restrict__ col_off,
               const uint8_t* __restrict__ ref, const int32_t* __restrict__ region_first_tile, const int32_t* __restrict__ tile_fill,
               int32_t n_regions, int64_t n_cols, const uint32_t* __restrict__ planes,
               const int64_t* __restrict__ pos0, const uint8_t* __restrict__ gt, const float* __restrict__ qual, int32_t n_sites,
               const int32_t* __restrict__ cand_off, lcr_candidate* __restrict__ out, lcr_candidate* __restrict__ h_cand, int32_t* __restrict__ h_off) {
  const int g = (int)((blockIdx.x * (unsigned)LCR_BLOCK + threadIdx.x) / LCR_WAVE), lane = threadIdx.x & (LCR_WAVE - 1);
  if (g >= n_regions) return;
  const int64_t s0 = start0[g];
  const int32_t lo = lower_bound_i64(pos0, 0, n_sites, s0);
  const int32_t hi = lower_bound_i64(pos0, lo, n_sites, s0 + len[g]);
  int32_t base = cand_off[g];
  if (lane == 0 && h_off) { h_off[g] = base; if (g == n_regions - 1) h_off[n_regions] = cand_off[n_regions]; }
  for (int32_t i0 = lo; i0 < hi; i0 += LCR_WAVE) {
    const int32_t i = i0 + lane;
    const uint8_t code = i < hi ? gt[i] : 0;
    const float q = i < hi ? qual[i] : 0.f;
    const bool keep = i < hi && site_kept(code, q);
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int64_t col = pos0[i] - s0, gc = col_off[g] + col;
      // a tile without records has no counts, and lcr_pileup has not written its planes (what lies there is an earlier batch's)
      const bool covered = tile_fill[region_first_tile[g] + (int32_t)(col / LCR_TILE)] != 0;
      uint32_t cnt[4];
#pragma unroll
      for (int k = 0; k < 4; k++) cnt[k] = covered ? planes[(size_t)k * n_cols + gc] : 0u;
      lcr_candidate r{};
      r.pos = pos0[i];
      r.region = g;
      r.ref_base = ref[gc];
      two_major(cnt, r.ref_base, &r.allele1, &r.cnt1, &r.allele2, &r.cnt2);   // (get_two_major_alleles(bf.ref_base): the byte as stored)
      r.depth = cnt[0] + cnt[1] + cnt[2] + cnt[3];
      r.af1 = (float)r.cnt1 / (float)r.depth;   // (f32: 0 / 0 = NaN at a column without A/C/G/T, as in the reference)
      r.af2 = (float)r.cnt2 / (float)r.depth;
      r.qual = r.gq = (double)q;
      if (code == 1) { r.variant_type = 1; r.genotype = 0; r.flags = LCR_F_HET | LCR_F_FOR_PHASING; }
      else if (code == 2) { r.variant_type = 2; r.genotype = -1; r.flags = LCR_F_HOM | LCR_F_FOR_PHASING; }
      else { r.variant_type = 3; r.genotype = -1; r.flags = LCR_F_HOM; }
      const int32_t slot = base + __popcll(m & ((1ull << lane) - 1ull));
      const uint4* src = reinterpret_cast<const uint4*>(&r);
      uint4* d = reinterpret_cast<uint4*>(out + slot);
#pragma unroll
      for (int w = 0; w < (int)(sizeof(lcr_candidate) / 16); w++) d[w] = src[w];
      if (h_cand) {
        uint4* h = reinterpret_cast<uint4*>(h_cand + slot);
#pragma unroll
        for (int w = 0; w < (int)(sizeof(lcr_candidate) / 16); w++) h[w] = src[w];
      }
    }
    base += __popcll(m);
  }
}

// contract of device-resident sites (host ones are checked on the host): ascending unique positions, codes 0-4.  *bad = 1 on a violation.
__global__ void __launch_bounds__(LCR_BLOCK)
k2_import_check(const int64_t* __restrict__ pos0, const uint8_t* __restrict__ gt, int32_t n_sites, int32_t* __restrict__ bad) {
  const int32_t i = (int32_t)(blockIdx.x * LCR_BLOCK + threadIdx.x);
  if (i >= n_sites) return;
  if (gt[i] > 4 || (i > 0 && pos0[i - 1] >= pos0[i])) *bad = 1;   // (every writer stores the same value: a plain store)
}

}  // namespace

static_assert(sizeof(lcr_candidate) % 16 == 0, "k2_import_emit writes 16-byte words");

void launch_k2_import_count(const BatchView& b, const int64_t* pos0, const uint8_t* gt, const float* qual, int32_t n_sites, int32_t* count, hipStream_t s) {
  const int ng = b.n_regions, wpb = LCR_BLOCK / LCR_WAVE;
  if (ng > 0) hipLaunchKernelGGL(k2_import_count, dim3((ng + wpb - 1) / wpb), dim3(LCR_BLOCK), 0, s, b.start0, b.len, ng, pos0, gt, qual, n_sites, count);
}

void launch_k2_import_emit(const BatchView& b, int64_t n_cols, const uint32_t* planes, const int32_t* tile_fill, const int64_t* pos0, const uint8_t* gt, const float* qual,
                           int32_t n_sites, const int32_t* cand_off, lcr_candidate* out, hipStream_t s, lcr_candidate* h_cand, int32_t* h_off) {
  const int ng = b.n_regions, wpb = LCR_BLOCK / LCR_WAVE;
  if (ng > 0) hipLaunchKernelGGL(k2_import_emit, dim3((ng + wpb - 1) / wpb), dim3(LCR_BLOCK), 0, s, b.start0, b.len, b.col_off, b.ref, b.region_first_tile, tile_fill, ng, n_cols, planes,
                                 pos0, gt, qual, n_sites, cand_off, out, h_cand, h_off);
}

void launch_k2_import_check(const int64_t* pos0, const uint8_t* gt, int32_t n_sites, int32_t* bad, hipStream_t s) {
  if (n_sites > 0) hipLaunchKernelGGL(k2_import_check, dim3((n_sites + LCR_BLOCK - 1) / LCR_BLOCK), dim3(LCR_BLOCK), 0, s, pos0, gt, n_sites, bad);
}

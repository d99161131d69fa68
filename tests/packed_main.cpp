// packed_main.cpp — lcr_bam_batch against lcr_bam_batch_packed (longcallr_amd/csrc/lcr_bam.cpp, pure host C++) in a stand-alone host
// program: built by tests/test_packed_host.py together with lcr_bam.cpp under -fsanitize=address,undefined and run as a child process.
//   packed_main <bam> <min_mapq> <min_read_length> <n_regions> <start0 len>...     (regions on the first contig that has records)
// Both calls are made for the regions given; the plain call's arrays are copied (the handle reuses its buffers), then every array the
// two share is compared, pack_off is checked to lie back to back, and the nibbles are expanded here, one base at a time, against the
// plain call's bases.  The arithmetic of the GPU kernel's 16-base piece (csrc/k0_unpack.h) runs over every read too.  Exit status 0 and
// "ok" iff everything agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/lcr.h"
#include "../longcallr_amd/csrc/k0_unpack.h"

static int fail(const char* what, long i) { printf("mismatch: %s at %ld\n", what, i); return 1; }

template <class T> static std::vector<T> copy_of(const T* p, size_t n) { return n ? std::vector<T>(p, p + n) : std::vector<T>(); }

int main(int argc, char** argv) {
  if (argc < 5) { printf("usage\n"); return 2; }
  lcr_bam* b = nullptr;
  if (lcr_bam_open(argv[1], 2, &b) != LCR_OK) { printf("open: %s\n", b ? lcr_bam_last_error(b) : "no handle"); return 2; }
  const lcr_read_filter flt{(uint8_t)atoi(argv[2]), atoi(argv[3]), 0.5f};
  const int ng = atoi(argv[4]);
  if (argc != 5 + 2 * ng) { printf("usage\n"); return 2; }
  std::vector<int64_t> start0(ng); std::vector<int32_t> len(ng);
  for (int g = 0; g < ng; g++) { start0[g] = atoll(argv[5 + 2 * g]); len[g] = atoi(argv[6 + 2 * g]); }
  int32_t n_ref = 0; const char* const* names = nullptr; const int64_t* lens = nullptr;
  if (lcr_bam_refs(b, &n_ref, &names, &lens) != LCR_OK) return 2;
  int32_t ref_id = -1;
  for (int32_t r = 0; r < n_ref && ref_id < 0; r++) {
    int32_t n = 0; const int32_t *s = nullptr, *e = nullptr;
    if (lcr_bam_spans(b, r, &flt, &n, &s, &e) != LCR_OK) { printf("spans: %s\n", lcr_bam_last_error(b)); return 2; }
    if (n) ref_id = r;
  }
  if (ref_id < 0) { printf("no records\n"); return 2; }

  lcr_reads rd; const int32_t* rb = nullptr; const uint64_t* noff = nullptr; const char* nm = nullptr;
  if (lcr_bam_batch(b, ref_id, &flt, ng, start0.data(), len.data(), &rd, &rb, &noff, &nm) != LCR_OK) { printf("batch: %s\n", lcr_bam_last_error(b)); return 2; }
  const size_t nr = (size_t)rd.n_reads;
  const int64_t n_bases = rd.n_bases, n_cigar = rd.n_cigar;
  const auto pos = copy_of(rd.pos, nr), seq_len = copy_of(rd.seq_len, nr), lead = copy_of(rd.lead_clip, nr), trail = copy_of(rd.trail_clip, nr);
  const auto flags = copy_of(rd.flags, nr);
  const auto seq_off = copy_of(rd.seq_off, nr), cig_off = copy_of(rd.cig_off, nr);
  const auto n_cig = copy_of(rd.n_cig, nr);
  const auto bases = copy_of(rd.bases, (size_t)n_bases), quals = copy_of(rd.quals, (size_t)n_bases);
  const auto cigar = copy_of(rd.cigar, (size_t)n_cigar);
  const auto read_begin = copy_of(rb, (size_t)ng + 1);
  const auto name_off = copy_of(noff, nr + 1);
  const auto name_blob = copy_of(nm, nr ? (size_t)noff[nr] : 0);

  lcr_reads_packed pk; rb = nullptr; noff = nullptr; nm = nullptr;
  if (lcr_bam_batch_packed(b, ref_id, &flt, ng, start0.data(), len.data(), &pk, &rb, &noff, &nm) != LCR_OK) { printf("packed: %s\n", lcr_bam_last_error(b)); return 2; }
  if (pk.mem != LCR_MEM_HOST || (size_t)pk.n_reads != nr || pk.n_bases != n_bases || pk.n_cigar != n_cigar) return fail("header", 0);
  if (memcmp(rb, read_begin.data(), ((size_t)ng + 1) * 4) != 0) return fail("read_begin", 0);
  if (nr && (memcmp(noff, name_off.data(), (nr + 1) * 8) != 0 || memcmp(nm, name_blob.data(), name_blob.size()) != 0)) return fail("names", 0);
  uint64_t po = 0;
  static const char NT16[] = "=ACMGRSVTWYHKDBN";
  for (size_t r = 0; r < nr; r++) {
    if (pk.pos[r] != pos[r] || pk.seq_len[r] != seq_len[r] || pk.lead_clip[r] != lead[r] || pk.trail_clip[r] != trail[r] || pk.flags[r] != flags[r] ||
        pk.seq_off[r] != seq_off[r] || pk.cig_off[r] != cig_off[r] || pk.n_cig[r] != n_cig[r])
      return fail("per-read arrays", (long)r);
    if (pk.pack_off[r] != po) return fail("pack_off not back to back", (long)r);
    const int32_t L = seq_len[r];
    const uint8_t* s = pk.seq4 + po;
    for (int32_t i = 0; i < L; i++) {
      const uint8_t v = s[i >> 1];
      const uint8_t want = (uint8_t)NT16[(i & 1) ? (v & 15) : (v >> 4)];
      if (want != bases[seq_off[r] + (uint64_t)i]) return fail("base", (long)(seq_off[r] + (uint64_t)i));
      if (unpack_nt16((i & 1) ? (v & 15u) : (uint32_t)(v >> 4)) != want) return fail("unpack_nt16", i);
    }
    // the kernel's piece: 16 bases from base i0, for an even and an odd first base
    for (int32_t i0 = 0; i0 + 16 <= L; i0 += 13) {
      uint64_t x = 0;
      for (int k = 0; k < 8; k++) x |= (uint64_t)s[(i0 >> 1) + k] << (8 * k);
      const uint32_t b8 = (i0 & 1) ? s[(i0 >> 1) + 8] : 0u;
      uint32_t q[4];
      unpack16(x, b8, i0 & 1, q);
      if (memcmp(q, bases.data() + seq_off[r] + (uint64_t)i0, 16) != 0) return fail("unpack16", (long)(seq_off[r] + (uint64_t)i0));
    }
    po += ((uint64_t)L + 1) / 2;
  }
  if ((uint64_t)pk.n_pack != po) return fail("n_pack", (long)po);
  if (n_bases && memcmp(pk.quals, quals.data(), (size_t)n_bases) != 0) return fail("quals", 0);
  if (n_cigar && memcmp(pk.cigar, cigar.data(), (size_t)n_cigar * 4) != 0) return fail("cigar", 0);
  lcr_bam_close(b);
  printf("ok %zu reads %lld bases\n", nr, (long long)n_bases);
  return 0;
}

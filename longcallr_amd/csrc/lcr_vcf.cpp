// lcr_vcf.cpp — the VCF reader of a run with user-provided candidates (longcallR -v): replaces
// get_genotype_quality_phase_from_vcf (src/vcf.rs:400-462, htslib bcf::Reader) on the host (no GPU code in this file).
//
// What is kept from the reference, by line:
//   * for every record and every sample whose GT has exactly two alleles (vcf.rs:420-423; a haploid `1`, a lone `.` are skipped):
//     allele n -> n, a missing allele -> 3 (vcf.rs:424-438), then (0,0) -> 0, (0,1) | (1,0) -> 1, (1,1) -> 2, (1,2) | (2,1) -> 3,
//     anything else -> 4 (vcf.rs:440-446);
//   * the value is inserted into contig -> 0-based POS, so a later sample or a later record at that position overwrites the
//     earlier one, a code 4 included (vcf.rs:448-455);
//   * quality = record.qual() as f32, NaN for a missing QUAL; the phase bit, REF and ALT are not used (an indel is a site at its POS).
// Beside the reference's three values every site keeps REF, ALT and the phase bit of its winning record and sample for
// lcr_vcf_contig_alleles (the loaders of allele_specific/longcallR-ase.py read them), and the sample's FORMAT PS integer for
// lcr_vcf_contig_phase_sets (the phase sets lcr_haplotag tags reads with); lcr_vcf_contig does not see them.
// Input: plain text, or gzip / BGZF (a sequence of gzip members, every member is inflated), parsed as it is read.  BCF input is refused, and so is a
// record with samples but no GT key in its FORMAT (the reference panics there: `genotypes().expect`); a sites-only record has no
// samples and yields nothing, as the reference's loop over zero samples does.
#include "../../include/lcr.h"

#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

struct lcr_vcf {
  std::string err;
  struct Contig {
    std::vector<int64_t> pos0;
    std::vector<uint8_t> gt;
    std::vector<float> qual;
    std::vector<uint8_t> ref, alt, phase;   // lcr_vcf_contig_alleles: parallel to the three above
    std::vector<uint32_t> ps;               // lcr_vcf_contig_phase_sets: FORMAT PS of the winning record and sample, 0 = none
  };
  std::vector<std::string> names;          // in the order of their first record
  std::vector<const char*> name_ptrs;
  std::vector<Contig> contigs;
  std::unordered_map<std::string, int32_t> index;
};

namespace {

// one GT value: "0/1", "1|2", "./.", "1", "." -> number of alleles and the reference's code (missing allele = 3)
// *phase (diploid GTs): 0 = unphased, 1 = 0|1, 2 = 1|0, 3 = phased with other alleles
int gt_code(const char* s, const char* e, int* n_alleles, int* phase) {
  int n = 0, a[2] = {0, 0};
  bool bar = false;
  *phase = 0;
  const char* p = s;
  while (p < e) {
    int v;
    if (*p == '.') { v = 3; p++; }
    else if (*p >= '0' && *p <= '9') { v = 0; while (p < e && *p >= '0' && *p <= '9') { v = v * 10 + (*p - '0'); if (v > 1000000) v = 1000000; p++; } }
    else { *n_alleles = -1; return 4; }
    if (n < 2) a[n] = v;
    n++;
    if (p < e) { if (*p != '/' && *p != '|') { *n_alleles = -1; return 4; } bar = *p == '|'; p++; if (p == e) { *n_alleles = -1; return 4; } }
  }
  *n_alleles = n;
  if (n != 2) return 4;
  if (bar) *phase = (a[0] == 0 && a[1] == 1) ? 1 : (a[0] == 1 && a[1] == 0) ? 2 : 3;
  if (a[0] == 0 && a[1] == 0) return 0;
  if ((a[0] == 0 && a[1] == 1) || (a[0] == 1 && a[1] == 0)) return 1;
  if (a[0] == 1 && a[1] == 1) return 2;
  if ((a[0] == 1 && a[1] == 2) || (a[0] == 2 && a[1] == 1)) return 3;
  return 4;
}

struct Entry { int64_t pos0; uint32_t seq; uint8_t gt; float qual; uint8_t ref, alt, phase; uint32_t ps; };

// a sample's PS subfield: an unsigned 32-bit decimal integer, anything else (".", empty, a sign, letters, overflow) -> 0
uint32_t ps_value(const char* s, const char* e) {
  if (s == e) return 0;
  uint64_t v = 0;
  for (const char* p = s; p < e; p++) {
    if (*p < '0' || *p > '9') return 0;
    v = v * 10 + (uint64_t)(*p - '0');
    if (v > 0xffffffffull) return 0;
  }
  return (uint32_t)v;
}

// Lines are parsed as the (inflated) bytes arrive: what is held is one input chunk, one output chunk, the partial line between
// them and one entry per record that yields a site -- not the file, nor its inflated text.
struct Parser {
  lcr_vcf* h;
  std::vector<std::vector<Entry>> ent;   // per contig, in record order
  std::string pending;                   // bytes after the last complete line
  size_t line_no = 0;
  uint32_t seq = 0;
  bool checked = false;

  explicit Parser(lcr_vcf* h_) : h(h_) {}

  bool check_magic() {
    checked = true;
    if (pending.compare(0, 3, "BCF") == 0) { h->err = "BCF input is not supported: convert it to VCF (bcftools view -Oz)"; return false; }
    if (pending.compare(0, 16, "##fileformat=VCF") != 0) { h->err = "not a VCF file (no ##fileformat=VCF line)"; return false; }
    return true;
  }

  bool line(const char* s, const char* e) {
    line_no++;
    if (e > s && e[-1] == '\r') e--;
    if (s == e || *s == '#') return true;
    const char* col[10];
    int nc = 1;
    col[0] = s;
    for (const char* p = s; p < e && nc < 10; p++) if (*p == '\t') col[nc++] = p + 1;
    auto end_of = [&](int k) { if (k + 1 < nc) return col[k + 1] - 1; const char* t = col[k]; while (t < e && *t != '\t') t++; return t; };
    if (nc < 8) { h->err = "line " + std::to_string(line_no) + ": fewer than 8 columns"; return false; }
    if (nc <= 9) return true;   // sites only (no FORMAT, or FORMAT without samples): no samples, no sites
    char* pe = nullptr;
    const long long pos = strtoll(col[1], &pe, 10);
    if (pe != end_of(1) || pos < 1) { h->err = "line " + std::to_string(line_no) + ": bad POS"; return false; }
    float qual;
    if (end_of(5) - col[5] == 1 && col[5][0] == '.') qual = std::numeric_limits<float>::quiet_NaN();
    else {
      const std::string qs(col[5], end_of(5));
      char* qe = nullptr;
      qual = strtof(qs.c_str(), &qe);
      if (qe != qs.c_str() + qs.size()) { h->err = "line " + std::to_string(line_no) + ": bad QUAL"; return false; }
    }
    // index of GT among the FORMAT keys
    int gt_key = -1, ps_key = -1;   // (PS: optional, for lcr_vcf_contig_phase_sets)
    { int k = 0; const char* p = col[8]; const char* fe = end_of(8);
      while (p <= fe) {
        const char* q = p; while (q < fe && *q != ':') q++;
        if (q - p == 2 && p[0] == 'G' && p[1] == 'T' && gt_key < 0) gt_key = k;
        if (q - p == 2 && p[0] == 'P' && p[1] == 'S' && ps_key < 0) ps_key = k;
        k++; p = q + 1;
      } }
    if (gt_key < 0) { h->err = "line " + std::to_string(line_no) + ": no GT key in FORMAT (genotypes are required)"; return false; }
    const std::string chrom(col[0], end_of(0));
    auto it = h->index.find(chrom);
    int32_t ci;
    if (it == h->index.end()) {
      ci = (int32_t)h->names.size();
      h->index.emplace(chrom, ci);
      h->names.push_back(chrom);
      ent.emplace_back();
    } else ci = it->second;
    // samples in order; each one with a diploid GT overwrites the record's value, so only the last of them counts
    int last = -1, last_phase = 0;
    uint32_t last_ps = 0;
    for (const char* smp = col[9]; smp <= e;) {
      const char* se = smp; while (se < e && *se != '\t') se++;
      // the sample's GT subfield (a sample with fewer subfields has a missing GT: one allele, skipped)
      const char* p = smp;
      int f = 0;
      while (f < gt_key && p < se) { if (*p == ':') f++; p++; }
      if (f == gt_key) {
        const char* q = p; while (q < se && *q != ':') q++;
        int n_alleles = 0, phase = 0;
        const int code = gt_code(p, q, &n_alleles, &phase);
        if (n_alleles == 2) {
          last = code; last_phase = phase; last_ps = 0;
          if (ps_key >= 0) {   // the same sample's PS subfield
            const char* a = smp;
            int g = 0;
            while (g < ps_key && a < se) { if (*a == ':') g++; a++; }
            if (g == ps_key) { const char* b = a; while (b < se && *b != ':') b++; last_ps = ps_value(a, b); }
          }
        }
      }
      smp = se + 1;
    }
    if (last >= 0) {
      // REF's byte when REF is one base; the first ALT's byte when every ALT allele is one base
      const uint8_t ref = end_of(3) - col[3] == 1 ? (uint8_t)col[3][0] : 0;
      uint8_t alt = end_of(4) > col[4] ? (uint8_t)col[4][0] : 0;
      for (const char* a = col[4]; a <= end_of(4);) {
        const char* ae = a; while (ae < end_of(4) && *ae != ',') ae++;
        if (ae - a != 1) alt = 0;
        a = ae + 1;
      }
      ent[ci].push_back(Entry{(int64_t)pos - 1, seq++, (uint8_t)last, qual, ref, alt, (uint8_t)last_phase, last_ps});
    }
    return true;
  }

  bool feed(const char* data, size_t n) {
    pending.append(data, n);
    if (!checked) { if (pending.size() < 16) return true; if (!check_magic()) return false; }
    size_t at = 0;
    for (;;) {
      const size_t nl = pending.find('\n', at);
      if (nl == std::string::npos) break;
      if (!line(pending.data() + at, pending.data() + nl)) return false;
      at = nl + 1;
    }
    pending.erase(0, at);
    return true;
  }

  bool finish() {
    if (!checked && !check_magic()) return false;
    if (!pending.empty() && !line(pending.data(), pending.data() + pending.size())) return false;
    pending.clear();
    std::vector<std::string> names;
    names.swap(h->names);
    h->index.clear();
    for (size_t ci = 0; ci < ent.size(); ci++) {
      std::vector<Entry>& v = ent[ci];
      if (v.empty()) continue;   // (records whose samples all lack a diploid GT: no site, no contig)
      h->index.emplace(names[ci], (int32_t)h->names.size());
      h->names.push_back(names[ci]);
      h->contigs.emplace_back();
      std::sort(v.begin(), v.end(), [](const Entry& a, const Entry& b) { return a.pos0 != b.pos0 ? a.pos0 < b.pos0 : a.seq < b.seq; });
      lcr_vcf::Contig& c = h->contigs.back();
      for (size_t i = 0; i < v.size(); i++) {
        if (i + 1 < v.size() && v[i + 1].pos0 == v[i].pos0) continue;   // the last value at a position wins
        c.pos0.push_back(v[i].pos0); c.gt.push_back(v[i].gt); c.qual.push_back(v[i].qual);
        c.ref.push_back(v[i].ref); c.alt.push_back(v[i].alt); c.phase.push_back(v[i].phase);
        c.ps.push_back(v[i].ps);
      }
      std::vector<Entry>().swap(v);
    }
    for (const std::string& n : h->names) h->name_ptrs.push_back(n.c_str());
    return true;
  }
};

// the file through the parser: plain text as read, gzip / BGZF inflated member after member (every member, the empty
// end-of-file block included), 1 MiB of input and 256 KiB of output at a time
int read_stream(FILE* f, Parser& ps, std::string* err) {
  std::vector<unsigned char> in(1 << 20), out(1 << 18);
  size_t n = fread(in.data(), 1, in.size(), f);
  const bool gz = n >= 2 && in[0] == 0x1f && in[1] == 0x8b;
  if (!gz) {
    while (n > 0) {
      if (!ps.feed((const char*)in.data(), n)) return LCR_E_ARG;
      n = fread(in.data(), 1, in.size(), f);
    }
  } else {
    z_stream z{};
    if (inflateInit2(&z, 15 + 16) != Z_OK) { *err = "zlib: inflateInit2 failed"; return LCR_E_ARG; }
    z.next_in = in.data();
    z.avail_in = (uInt)n;
    bool mid = false;   // inside a member that has not ended yet
    for (;;) {
      if (z.avail_in == 0) {
        n = fread(in.data(), 1, in.size(), f);
        if (n == 0) break;
        z.next_in = in.data();
        z.avail_in = (uInt)n;
      }
      z.next_out = out.data();
      z.avail_out = (uInt)out.size();
      mid = true;
      const int rc = inflate(&z, Z_NO_FLUSH);
      const size_t got = out.size() - z.avail_out;
      if (got && !ps.feed((const char*)out.data(), got)) { inflateEnd(&z); return LCR_E_ARG; }
      if (rc == Z_STREAM_END) { mid = false; inflateReset(&z); continue; }   // the next member
      if (rc == Z_OK || (rc == Z_BUF_ERROR && z.avail_in == 0)) continue;
      *err = std::string("zlib: ") + (z.msg ? z.msg : "inflate failed");
      inflateEnd(&z);
      return LCR_E_ARG;
    }
    inflateEnd(&z);
    if (mid) { *err = "truncated gzip stream"; return LCR_E_ARG; }
  }
  if (ferror(f)) { *err = "read error"; return LCR_E_ARG; }
  return ps.finish() ? LCR_OK : LCR_E_ARG;
}

}  // namespace

extern "C" {

int lcr_vcf_open(const char* path, int32_t n_threads, lcr_vcf** out) {
  (void)n_threads;
  if (!path || !out) return LCR_E_ARG;
  lcr_vcf* h = new (std::nothrow) lcr_vcf();
  *out = h;   // returned even on failure so that lcr_vcf_last_error can explain; the caller closes it
  if (!h) return LCR_E_NOMEM;
  FILE* f = fopen(path, "rb");
  if (!f) { h->err = std::string("cannot open ") + path; return LCR_E_ARG; }
  int rc;
  try {
    Parser ps(h);
    rc = read_stream(f, ps, &h->err);
  } catch (const std::bad_alloc&) {
    h->err = "out of memory";
    rc = LCR_E_NOMEM;
  }
  fclose(f);
  return rc;
}

void lcr_vcf_close(lcr_vcf* h) { delete h; }

const char* lcr_vcf_last_error(const lcr_vcf* h) { return h ? h->err.c_str() : "null handle"; }

int lcr_vcf_contigs(lcr_vcf* h, int32_t* n, const char* const** names) {
  if (!h || !n || !names) return LCR_E_ARG;
  *n = (int32_t)h->names.size();
  *names = h->name_ptrs.data();
  return LCR_OK;
}

int lcr_vcf_contig(lcr_vcf* h, const char* name, int32_t* n, const int64_t** pos0, const uint8_t** genotype, const float** qual) {
  if (!h || !name || !n || !pos0 || !genotype || !qual) return LCR_E_ARG;
  auto it = h->index.find(name);
  if (it == h->index.end()) { *n = 0; *pos0 = nullptr; *genotype = nullptr; *qual = nullptr; return LCR_OK; }
  const lcr_vcf::Contig& c = h->contigs[it->second];
  *n = (int32_t)c.pos0.size();
  *pos0 = c.pos0.data(); *genotype = c.gt.data(); *qual = c.qual.data();
  return LCR_OK;
}

int lcr_vcf_contig_alleles(lcr_vcf* h, const char* name, int32_t* n, const uint8_t** ref, const uint8_t** alt, const uint8_t** phase) {
  if (!h || !name || !n || !ref || !alt || !phase) return LCR_E_ARG;
  auto it = h->index.find(name);
  if (it == h->index.end()) { *n = 0; *ref = nullptr; *alt = nullptr; *phase = nullptr; return LCR_OK; }
  const lcr_vcf::Contig& c = h->contigs[it->second];
  *n = (int32_t)c.pos0.size();
  *ref = c.ref.data(); *alt = c.alt.data(); *phase = c.phase.data();
  return LCR_OK;
}

int lcr_vcf_contig_phase_sets(lcr_vcf* h, const char* name, int32_t* n, const uint32_t** ps) {
  if (!h || !name || !n || !ps) return LCR_E_ARG;
  auto it = h->index.find(name);
  if (it == h->index.end()) { *n = 0; *ps = nullptr; return LCR_OK; }
  const lcr_vcf::Contig& c = h->contigs[it->second];
  *n = (int32_t)c.ps.size();
  *ps = c.ps.data();
  return LCR_OK;
}

}  // extern "C"

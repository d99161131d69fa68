"""Allele-specific expression without a GPU: the host arithmetic of longcallr_amd/ase.py (beta-binomial test, the three TSV texts, the
filter mode's drop rule, the VCF loaders on lcr_vcf_contig_alleles), the plain-Python restatement of the lcr_ase contract
(tests/ase_ref.py) on a hand-worked instance, and the layout of the new ABI structs and their INTEGRATION.md binding."""
import ctypes as C
import gzip
import math
import os
import re

import numpy as np
import pytest

import ase_ref
from longcallr_amd import _abi, _lib, ase, asj, build, vcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# Closed forms are met to the rounding of lgamma: a pmf value is exp of a sum of ten lgamma values of up to ~6e3 (alpha + beta = 998 at
# rho = 0.001, n up to 2 000), each good to about an ulp of that magnitude (9e-13): a few 1e-12 relative, so 1e-10 with a margin.
LG = 1e-10


# ---- 1. the beta-binomial test -----------------------------------------------------------------------------------------------------
def test_mu_rho_as_written():
    a, b = ase.convert_mu_rho_to_alpha_beta(0.5, 0.001)
    assert a == b == 0.5 * ((1 - 0.001) / 0.001 - 1) and a == pytest.approx(499.0, rel=1e-12)
    a, b = ase.convert_mu_rho_to_alpha_beta(0.25, 0.1)
    assert (a, b) == (0.25 * 8.0, 0.75 * 8.0)


@pytest.mark.parametrize("rho", [0.001, 0.05, 0.3])
def test_betabinom_closed_forms(rho):
    a, _ = ase.convert_mu_rho_to_alpha_beta(0.5, rho)
    assert ase.betabinom_two_sided(0, 1, 0.5, rho) == pytest.approx(1.0, rel=LG) and ase.betabinom_two_sided(1, 1, 0.5, rho) == pytest.approx(1.0, rel=LG)
    # n = 2, alpha = beta = a: pmf(0) = pmf(2) = (a + 1) / (2 (2a + 1)), pmf(1) = a / (2a + 1): the larger for a > 1, the smaller below
    pmf = [(a + 1) / (2 * (2 * a + 1)), a / (2 * a + 1), (a + 1) / (2 * (2 * a + 1))]
    assert (pmf[1] > pmf[0]) == (a > 1)
    for k in range(3):
        assert ase.betabinom_two_sided(k, 2, 0.5, rho) == pytest.approx(sum(x for x in pmf if x <= pmf[k]), rel=LG), k
    assert ase.betabinom_two_sided(0, 0, 0.5, rho) == 1.0
    for n in (3, 10, 57, 400):
        for k in (0, 1, n // 3, n // 2):
            assert ase.betabinom_two_sided(k, n, 0.5, rho) == pytest.approx(ase.betabinom_two_sided(n - k, n, 0.5, rho), rel=LG)
    # without symmetry (mu != 0.5) the mirror image does not count
    assert ase.betabinom_two_sided(1, 10, 0.3, rho) != pytest.approx(ase.betabinom_two_sided(9, 10, 0.3, rho), rel=1e-3)


def test_betabinom_against_scipy():
    """relative 1e-9, the tolerance of the asj host tests against a closed form; the largest deviation seen over these cases is printed"""
    st = pytest.importorskip("scipy.stats")
    worst = 0.0
    for mu, rho in ((0.5, 0.001), (0.5, 0.02), (0.3, 0.001), (0.5, 0.3)):
        a, b = ase.convert_mu_rho_to_alpha_beta(mu, rho)
        for n in (1, 2, 3, 10, 57, 100, 333, 1000, 2000):
            pmf = st.betabinom(n, a, b).pmf(np.arange(n + 1))
            for k in sorted({0, 1, n // 4, n // 2 - 1 if n > 2 else 0, n // 2, (3 * n) // 5, n}):
                want = min(float(pmf[pmf <= pmf[k] * (1.0 + 1e-7)].sum()), 1.0)
                got = ase.betabinom_two_sided(k, n, mu, rho)
                if want > 1e-300:
                    worst = max(worst, abs(got - want) / want)
                assert got == pytest.approx(want, rel=1e-9, abs=1e-300), (mu, rho, n, k)
    print("largest relative deviation from scipy.stats.betabinom: %.3g" % worst)


# ---- 2. the three tables --------------------------------------------------------------------------------------------------------------
def _rec(rows):
    a = np.zeros(len(rows), dtype=_abi.ASE_DTYPE)
    for i, r in enumerate(rows):
        for k, v in r.items():
            a[k][i] = v
        a["region"][i] = i
    return a


def test_tsv_texts():
    rec = _rec([dict(phase_set=1001, n_phase_sets=2, h1=30, h2=10, n_sites=3, h1_pat=20, h1_mat=1, h2_pat=0, h2_mat=7),
                dict(phase_set=2001, n_phase_sets=1, h1=4, h2=5),                       # 9 < min_support: not written, not adjusted over
                dict(),                                                                  # no counting row
                dict(phase_set=4001, n_phase_sets=1, h1=5, h2=5)])
    start0, length = np.array([100, 1000, 2000, 3000]), np.array([500, 600, 700, 800])
    rec2 = _rec([dict(phase_set=77, n_phase_sets=1, h1=0, h2=12, h2_mat=12, n_sites=1)])
    tables = [("chrA", rec, start0, length), ("chrB", rec2, np.array([9]), np.array([10]))]
    p = [ase.betabinom_two_sided(30, 40, 0.5, 0.001), ase.betabinom_two_sided(5, 10, 0.5, 0.001), ase.betabinom_two_sided(0, 12, 0.5, 0.001)]
    adj = asj.bh_adjust(p)          # over the three written rows only
    assert p[1] == pytest.approx(1.0, rel=LG) and adj[1] == p[1] and adj[0] != p[0]
    text = ase.format_tsv(tables, min_support=10, overdispersion=0.001)
    assert text == ("#Gene_name\tChr\tPS\tH1\tH2\tP_value\n"
                    "chrA:101-600\tchrA\t1001\t30\t10\t%s\n"
                    "chrA:3001-3800\tchrA\t4001\t5\t5\t%s\n"
                    "chrB:10-19\tchrB\t77\t0\t12\t%s\n" % tuple(float(x) for x in adj))
    pm = ase.format_tsv(tables, min_support=10, overdispersion=0.001, patmat=True).split("\n")
    assert pm[0] == "#Gene_name\tChr\tPS\tH1\tH2\tP_value\tH1_Paternal\tH1_Maternal\tH2_Paternal\tH2_Maternal"
    assert pm[1] == "chrA:101-600\tchrA\t1001\t30\t10\t%s\t20\t1\t0\t7" % float(adj[0])
    assert pm[3] == "chrB:10-19\tchrB\t77\t0\t12\t%s\t0\t0\t0\t12" % float(adj[2]) and pm[4] == "" and len(pm) == 5
    # min_support 0 writes every region; a region without a phase set prints "."
    low = ase.format_tsv(tables[:1], min_support=0).split("\n")
    assert len(low) == 6 and low[3] == "chrA:2001-2700\tchrA\t.\t0\t0\t%s" % float(asj.bh_adjust([p[0], ase.betabinom_two_sided(4, 9), 1.0, p[1]])[2])
    # the filter mode: a dropped region is not written and not adjusted over
    keep = np.array([True, True, True, False])
    flt = ase.format_tsv([("chrA", rec, start0, length, keep)], min_support=10).split("\n")
    assert flt[0] == ase.HEADER and flt[1] == "chrA:101-600\tchrA\t1001\t30\t10\t%s" % p[0] and flt[2] == "" and len(flt) == 3
    assert ase.format_tsv([]) == ase.HEADER + "\n"


# ---- 3. the filter mode's drop rule ---------------------------------------------------------------------------------------------------
def _cand(rows):
    a = np.zeros(len(rows), dtype=_abi.CAND_DTYPE)
    for i, r in enumerate(rows):
        base = dict(ref_base=ord("A"), allele1=ord("A"), allele2=ord("G"), variant_type=1, haplotype=1, phase_score=20.0, phase_set=1001,
                    flags=_abi.F_HET | _abi.F_FOR_PHASING, depth=100, af1=0.6, af2=0.4, region=0)
        base.update(r)
        for k, v in base.items():
            a[k][i] = v
    return a


def test_filter_drop_rule():
    p39, p40 = ase.betabinom_two_sided(39, 100), ase.betabinom_two_sided(40, 100)
    assert p39 < 0.05 < p40                                   # the cases below stand on this
    assert int(100 * float(vcf._f2(np.float32(0.396)))) == 40 and int(100 * 0.396) == 39
    rec = _rec([dict(phase_set=1001, h1=20, h2=20)] * 8)
    cands = _cand([
        dict(region=0, pos=10, af2=0.394),                    # prints 0.39 -> 39 of 100: significant, kept
        dict(region=1, pos=20, af2=0.396),                    # prints 0.40 -> 40 of 100 (the raw value would give 39): dropped
        dict(region=2, pos=30, af2=0.394),                    # not in the DNA set: dropped
        dict(region=3, pos=40, af2=0.394, phase_set=999),     # another phase set: dropped
        dict(region=4, pos=50, af2=0.0, depth=9),             # below min_support, however skewed: dropped
        dict(region=5, pos=60, af2=0.394, phase_score=5.0),   # LowQual, not PASS: dropped
        dict(region=6, pos=70, depth=0, af2=float("nan")),    # skipped ...
        dict(region=6, pos=71, allele1=ord("G"), allele2=ord("A"), af1=0.2, af2=0.8),   # ... the ALT is allele1: af1 counts, kept
        dict(region=7, pos=80, af2=0.1, flags=_abi.F_HET | _abi.F_DENSE)])              # dense: dropped
    dna = np.array([10, 20, 40, 50, 60, 70, 71, 80], np.int64)
    keep = ase.filter_regions(rec, cands, dna, min_phase_score=11.0, min_support=10, overdispersion=0.001)
    assert keep.tolist() == [True, False, False, False, False, False, True, False]
    assert ase.filter_regions(rec, cands, np.zeros(0, np.int64), 11.0).tolist() == [False] * 8
    assert ase.filter_regions(rec, cands[:0], dna, 11.0).tolist() == [False] * 8


# ---- 4. the restatement on a hand-worked instance -------------------------------------------------------------------------------------
def test_restatement_by_hand():
    """One region, six rows, three candidates (0 and 1 PASS phased het in set 101, 2 in set 202).  val = q | p << 5 | code << 6.

      row  hap  ps   entries (candidate: base q)                 pat / mat at sites 0 (pat A, mat G) and 1 (pat T, mat C)
      0    1    101  0: A 30, 1: T 30                            2 / 0  paternal
      1    1    101  0: A 30, 1: C 30                            1 / 1  no vote
      2    2    101  0: G 30, 1: T 12                            0 / 1  maternal (q 12 < 13 is not seen; at min_baseq 12: 1 / 1)
      3    2    101  (none)                                      no vote
      4    2    202  0: A 30                                     another phase set: takes no part in the votes
      5    0    101  0: G 30                                     unassigned: takes no part at all
    phase sets: 101 has 4 counting rows, 202 has 1: phase_set 101 of 2, h1 2, h2 2, n_sites 2."""
    def v(base, q, p=0):
        return q | p << 5 | "ACGT".index(base) << 6
    fm = dict(row_region_off=np.array([0, 6]), row_ptr=np.array([0, 2, 4, 6, 6, 7, 8]),
              col=np.array([0, 1, 0, 1, 0, 1, 0, 0]), val=np.array([v("A", 30, 1), v("T", 30), v("A", 30, 1), v("C", 30, 1), v("G", 30), v("T", 12), v("A", 30, 1), v("G", 30)]))
    asg, ps = np.array([1, 1, 2, 2, 2, 0]), np.array([101, 101, 101, 101, 202, 101])
    cands = _cand([dict(pos=500, ref_base=ord("A"), allele1=ord("A"), allele2=ord("G"), phase_set=101),
                   dict(pos=600, ref_base=ord("C"), allele1=ord("T"), allele2=ord("C"), phase_set=101),
                   dict(pos=700, phase_set=202)])
    parental = {500: ("A", "G"), 600: ("T", "C"), 700: ("A", "G"), 900: ("A", "C")}
    got = ase_ref.regions(fm, asg, ps, cands, [0, 3], parental, 13, 11.0)
    assert got.tolist() == [(0, 101, 2, 2, 2, 2, 1, 0, 0, 1)]
    assert ase_ref.regions(fm, asg, ps, cands, [0, 3], parental, 12, 11.0).tolist() == [(0, 101, 2, 2, 2, 2, 1, 0, 0, 0)]   # row 2: 1 / 1 now
    assert ase_ref.regions(fm, asg, ps, cands, [0, 3], None, 13, 11.0).tolist() == [(0, 101, 2, 2, 2, 0, 0, 0, 0, 0)]
    assert ase_ref.regions(fm, asg, ps, cands, [0, 3], parental, 13, 21.0).tolist() == [(0, 101, 2, 2, 2, 0, 0, 0, 0, 0)]   # no PASS site
    # equal counts: the smaller value
    ps2 = np.array([101, 101, 50, 50, 202, 101])
    assert ase_ref.regions(fm, asg, ps2, cands, [0, 3], None).tolist() == [(0, 50, 3, 0, 2, 0, 0, 0, 0, 0)]
    assert ase.eligible_candidates(cands, got, 11.0).tolist() == [True, True, False]


# ---- 5. lcr_vcf_contig_alleles ------------------------------------------------------------------------------------------------------
VCF_TEXT = "\n".join(["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"] + ["\t".join(r) for r in [
    ("chr1", "100", ".", "A", "G", "30", "PASS", ".", "GT", "0|1"),
    ("chr1", "200", ".", "C", "T", "31", "PASS", ".", "GT:DP", "1|0:9"),
    ("chr1", "300", ".", "G", "A", "32", "PASS", ".", "GT", "0/1"),
    ("chr1", "400", ".", "AT", "A", "33", "PASS", ".", "GT", "0|1"),          # an indel
    ("chr1", "500", ".", "A", "G,TTT", "34", "PASS", ".", "GT", "1|2"),       # one long ALT allele
    ("chr1", "600", ".", "A", "C", "35", "PASS", ".", "GT", "0|1"),
    ("chr2", "50", ".", "T", "C", ".", "PASS", ".", "GT", "0|1"),
    ("chr1", "600", ".", "A", "T", "36", "PASS", ".", "GT", "1|0"),           # a later record at the same position wins
    ("chr1", "700", ".", "G", "C,T", "37", "PASS", ".", "GT", "1/1"),
    ("chr1", "800", ".", "T", "A", "38", "PASS", ".", "GT", "1|1"),
    ("chr1", "900", ".", "C", "G", "39", "PASS", ".", "GT", "0/1\t1|0")]]) + "\n"    # two samples: the last one's GT and phase


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


@pytest.mark.parametrize("gz", [False, True])
def test_vcf_contig_alleles(lib, tmp_path, gz):
    text = VCF_TEXT.replace("FORMAT\tS\n", "FORMAT\tS\tS2\n")
    path = str(tmp_path / ("a.vcf.gz" if gz else "a.vcf"))
    if gz:
        with gzip.open(path, "wb") as f:
            f.write(text.encode())
    else:
        open(path, "w").write(text)
    al = vcf.read_sites(path, alleles=True)
    assert list(al) == ["chr1", "chr2"]
    pos, gt, _, ref, alt, ph = al["chr1"]
    assert pos.tolist() == [99, 199, 299, 399, 499, 599, 699, 799, 899]
    assert gt.tolist() == [1, 1, 1, 1, 3, 1, 2, 2, 1]
    assert bytes(ref) == b"ACG\0AAGTC" and bytes(alt) == b"GTAA\0TCAG"
    assert ph.tolist() == [1, 2, 0, 1, 3, 2, 0, 3, 2]
    assert [al["chr2"][k].tolist() for k in (0, 1, 3, 4, 5)] == [[49], [1], [ord("T")], [ord("C")], [1]]
    # lcr_vcf_contig's own arrays on the same file: what they were
    sites = vcf.read_sites(path)
    assert sites["chr1"][0].tolist() == pos.tolist() and sites["chr1"][1].tolist() == gt.tolist()
    assert sites["chr1"][2].tolist() == [30.0, 31.0, 32.0, 33.0, 34.0, 36.0, 37.0, 38.0, 39.0]
    assert sites["chr2"][0].tolist() == [49] and sites["chr2"][1].tolist() == [1] and math.isnan(sites["chr2"][2][0])
    # the script's two loaders
    p, pat, mat = ase.parental_sites(path, "chr1")
    assert p.tolist() == [99, 199, 599, 899] and bytes(pat) == b"GCAC" and bytes(mat) == b"ATTG"
    assert ase.dna_het_sites(path, "chr1").tolist() == [99, 199, 299, 599, 899]
    both = ase.parental_sites(path)
    assert sorted(both) == ["chr1", "chr2"] and both["chr2"][0].tolist() == [49] and bytes(both["chr2"][1]) == b"C" and bytes(both["chr2"][2]) == b"T"
    assert ase.parental_sites(path, "chrX")[0].size == 0 and ase.dna_het_sites(path, "chrX").size == 0
    # a contig the file does not name
    m = C.c_int32(7)
    r, a, q = C.c_void_p(), C.c_void_p(), C.c_void_p()
    h = C.c_void_p()
    assert lib.lcr_vcf_open(path.encode(), 0, C.byref(h)) == 0
    assert lib.lcr_vcf_contig_alleles(h, b"nope", C.byref(m), C.byref(r), C.byref(a), C.byref(q)) == 0 and m.value == 0
    assert lib.lcr_vcf_contig_alleles(h, None, C.byref(m), C.byref(r), C.byref(a), C.byref(q)) == -1
    lib.lcr_vcf_close(h)


# ---- 6. layouts and bindings ------------------------------------------------------------------------------------------------------------
def _c_layout(tmp_path, structs):
    """{struct: [field]} -> {"struct": sizeof, "struct.field": offsetof} from gcc on include/lcr.h"""
    lines = ['#include "lcr.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(){"]
    for name, fields in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in fields]
    lines.append("return 0;}")
    src, exe = tmp_path / "asz.c", tmp_path / "asz"
    src.write_text("\n".join(lines))
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    return {k: int(v) for k, v in (l.split() for l in os.popen(str(exe)).read().strip().split("\n"))}


FIELDS = {"lcr_ase_params": ["min_baseq", "min_phase_score"],
          "lcr_ase_region": ["region", "phase_set", "n_phase_sets", "h1", "h2", "n_sites", "h1_pat", "h1_mat", "h2_pat", "h2_mat"],
          "lcr_ase_list": ["n_regions", "rec", "dev_rec"]}


def test_ase_struct_layouts_match_the_header(tmp_path):
    got = _c_layout(tmp_path, FIELDS)
    assert list(_abi.ASE_DTYPE.names) == FIELDS["lcr_ase_region"] and [n for n, _ in _abi.LcrAseList._fields_] == FIELDS["lcr_ase_list"]
    assert got["lcr_ase_region"] == 40 == _abi.ASE_DTYPE.itemsize
    assert got["lcr_ase_params"] == C.sizeof(_abi.LcrAseParams) == 8 and got["lcr_ase_list"] == C.sizeof(_abi.LcrAseList)
    for f in FIELDS["lcr_ase_region"]:
        assert got["lcr_ase_region." + f] == _abi.ASE_DTYPE.fields[f][1], f
    for f in FIELDS["lcr_ase_list"]:
        assert got["lcr_ase_list." + f] == getattr(_abi.LcrAseList, f).offset, f
    for f in FIELDS["lcr_ase_params"]:
        assert got["lcr_ase_params." + f] == getattr(_abi.LcrAseParams, f).offset, f
    assert _abi.K_ASE == _abi.K_JUNCTIONS + 1 == _abi.NKERNELS - 1
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcr.h")).read(), flags=re.S)
    assert re.search(r"LCR_K_JUNCTIONS\s*,\s*LCR_K_ASE\s*,\s*LCR_NKERNELS", hdr)


def test_integration_md_binding_matches_the_header(tmp_path):
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [re.sub(r"//[^\n]*", "", b) for b in re.findall(r"```rust(.*?)```", md, flags=re.S)]
    fns = set(re.findall(r"pub fn (lcr_\w+)", "".join(blocks)))
    assert {"lcr_ase", "lcr_get_ase", "lcr_vcf_contig_alleles"} <= fns & set(_lib.SYMBOLS)
    prim = {"i32": 4, "u32": 4, "f32": 4}
    got = _c_layout(tmp_path, FIELDS)
    for name, want_fields in FIELDS.items():
        m = [x for x in (re.search(r"pub struct %s\s*\{(.*?)\}" % name, b, flags=re.S) for b in blocks) if x]
        assert len(m) == 1, name
        fields = [(a, b.strip()) for a, b in re.findall(r"pub (\w+):\s*([^,}]+)", m[0].group(1))]
        assert [a for a, _ in fields] == want_fields
        off, align = 0, 1
        for f, ty in fields:      # C layout rules
            sz = 8 if ty.startswith("*") else prim[ty]
            off = (off + sz - 1) // sz * sz
            assert got["%s.%s" % (name, f)] == off, (name, f)
            off += sz
            align = max(align, sz)
        assert got[name] == (off + align - 1) // align * align, name
    # the argument list of lcr_ase as the header has it
    sig = re.search(r"pub fn lcr_ase\((.*?)\)\s*->\s*i32", "".join(blocks), flags=re.S).group(1)
    assert [a.strip().split(":")[1].strip() for a in sig.split(",")] == ["*mut lcr_ctx", "*const lcr_ase_params", "i32", "i32", "*const i64", "*const u8", "*const u8"]

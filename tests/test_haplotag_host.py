"""The host side of haplotagging against a phased VCF (no GPU): the VCF reader's PS array, vcf.haplotag_sites' keep rule, the layout of
lcr_haplotag_site, the plain-Python restatement of the contract (tests/haplotag_ref.py) on a row worked by hand, the merge of per-gene
records whose phase sets span regions, and the command line's --haplotag without -v."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import haplotag_ref
from longcallr_amd import _abi, _lib, ase, build, vcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"


def rec(chrom, pos, ref, alt, fmt, sample):
    return "%s\t%d\t.\t%s\t%s\t30\tPASS\t.\t%s\t%s\n" % (chrom, pos, ref, alt, fmt, sample)


VCF_TEXT = HEAD + "".join([
    rec("c1", 10, "A", "C", "GT:PS", "0|1:7"),              # PS present
    rec("c1", 20, "C", "G", "GT:PS", "1|0:."),              # PS "."
    rec("c1", 30, "G", "T", "GT", "0|1"),                   # no PS key
    rec("c1", 40, "T", "A", "GT:PS", "0|1:x7"),             # not an integer
    rec("c1", 50, "A", "G", "GT:PS", "0|1:4294967296"),     # beyond 32 bits
    rec("c1", 60, "A", "G", "GT:PS", "0|1:4294967295"),     # the largest value
    rec("c1", 70, "A", "G", "GT:DP:PS", "0|1:12:9"),        # PS behind another key
    rec("c1", 80, "A", "G", "GT:DP:PS", "0|1:12"),          # a sample with fewer subfields than keys
    rec("c1", 90, "A", "G", "GT:PS", "0|1:5"),
    rec("c1", 90, "A", "T", "PS:GT", "11:1|0"),             # a later record at the same position overwrites; PS in front of GT
    rec("c1", 100, "A", "G", "PS:GT", "13:1/0"),            # an unphased GT keeps its PS value: the reader does not judge
    rec("c1", 110, "A", "G", "GT:PS", "0|1:-3"),            # a sign
    rec("c2", 5, "a", "g", "GT:PS", "0|1:21"),
])


def test_phase_sets_of_the_reader(lib, tmp_path):
    p = tmp_path / "in.vcf"
    p.write_text(VCF_TEXT)
    gz = tmp_path / "in.vcf.gz"
    with gzip.open(gz, "wt") as f:
        f.write(VCF_TEXT)
    for path in (p, gz):
        s = vcf.read_sites(str(path), alleles=True, phase_sets=True)
        assert sorted(s) == ["c1", "c2"] and all(len(v) == 7 for v in s.values())
        pos, gt, q, ref, alt, ph, ps = s["c1"]
        assert ps.dtype == np.uint32 and pos.tolist() == [9, 19, 29, 39, 49, 59, 69, 79, 89, 99, 109]
        #                      7   .  none x7  2^32  2^32-1     9  short  later  13  -3
        assert ps.tolist() == [7, 0, 0, 0, 0, 4294967295, 9, 0, 11, 13, 0]
        assert chr(alt[8]) == "T" and gt[8] == 1 and ph[8] == 2 and ph[9] == 0      # the later record at 90 won, with its PS
        assert s["c2"][6].tolist() == [21]
        # without the switch nothing changes; the two switches are independent
        assert len(vcf.read_sites(str(path))["c1"]) == 3 and len(vcf.read_sites(str(path), alleles=True)["c1"]) == 6
        only = vcf.read_sites(str(path), phase_sets=True)["c1"]
        assert len(only) == 4 and only[3].tolist() == ps.tolist()
    # a contig the file does not name: n = 0
    h = C.c_void_p()
    assert lib.lcr_vcf_open(os.fsencode(str(p)), 0, C.byref(h)) == 0
    n, ptr = C.c_int32(5), C.c_void_p()
    assert lib.lcr_vcf_contig_phase_sets(h, b"nope", C.byref(n), C.byref(ptr)) == 0 and n.value == 0
    assert lib.lcr_vcf_contig_phase_sets(h, None, C.byref(n), C.byref(ptr)) == -1
    lib.lcr_vcf_close(h)


def test_later_record_overwrites_the_phase_set(lib, tmp_path):
    p = tmp_path / "two.vcf"
    p.write_text(HEAD + rec("c1", 10, "A", "C", "GT:PS", "0|1:7") + rec("c1", 10, "A", "C", "GT:PS", "1|0:8")
                 + rec("c1", 20, "A", "C", "GT:PS", "0|1:7") + rec("c1", 20, "A", "C", "GT", "0|1"))
    pos, gt, q, ref, alt, ph, ps = vcf.read_sites(str(p), alleles=True, phase_sets=True)["c1"]
    assert pos.tolist() == [9, 19] and ph.tolist() == [2, 1] and ps.tolist() == [8, 0]


def test_haplotag_sites_keep_rule_and_fallback_set():
    b = lambda s: np.frombuffer(s, np.uint8)
    #             kept      kept       hom   unphased  phase 3  indel ref  indel alt  N      kept (lower case)
    pos = np.array([100,    200,       300,  400,      500,     600,       700,       800,   900], np.int64)
    gt = np.array([1,       1,         2,    1,        1,       1,         1,         1,     1], np.uint8)
    ph = np.array([1,       2,         1,    0,        3,       1,         1,         1,     2], np.uint8)
    ref = b(b"AC" b"G" b"T" b"A" b"\0" b"A" b"N" b"g")
    alt = b(b"CG" b"T" b"A" b"C" b"A" b"\0" b"A" b"t")
    ps = np.array([0, 77, 5, 5, 5, 5, 5, 5, 0], np.uint32)
    p, h1, h2, s = vcf.haplotag_sites((pos, gt, np.zeros(9, np.float32), ref, alt, ph, ps))
    assert p.tolist() == [100, 200, 900] and p.dtype == np.int64 and s.dtype == np.uint32
    assert bytes(h1) == b"AGT" and bytes(h2) == b"CCG"      # 0|1: REF on haplotype 1; 1|0: ALT on haplotype 1
    assert s.tolist() == [101, 77, 101]                      # no PS: the 1-based position of the contig's first kept site
    # when the first record is dropped the fallback names the first KEPT one; nothing kept: empty arrays
    p2, _, _, s2 = vcf.haplotag_sites((pos[2:], gt[2:], np.zeros(7, np.float32), ref[2:], alt[2:], ph[2:], ps[2:]))
    assert p2.tolist() == [900] and s2.tolist() == [901]
    p3, h13, _, s3 = vcf.haplotag_sites((pos[2:8], gt[2:8], np.zeros(6, np.float32), ref[2:8], alt[2:8], ph[2:8], ps[2:8]))
    assert p3.size == 0 and h13.dtype == np.uint8 and s3.size == 0


def test_site_record_layout_matches_the_header(tmp_path):
    fields = ["match_fx", "total_fx", "n_h1", "n_h2", "n_h1_match", "n_h2_match"]
    src = tmp_path / "hs.c"
    src.write_text('#include "lcr.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu", sizeof(lcr_haplotag_site));'
                   + "".join('printf(" %%zu", offsetof(lcr_haplotag_site, %s));' % f for f in fields) + "return 0;}")
    exe = tmp_path / "hs"
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = [int(x) for x in os.popen(str(exe)).read().split()]
    assert got[0] == 32 == _abi.HAPSITE_DTYPE.itemsize
    assert got[1:] == [_abi.HAPSITE_DTYPE.fields[f][1] for f in fields] == [0, 8, 16, 20, 24, 28]
    assert {"lcr_haplotag", "lcr_get_haplotag_sites", "lcr_haplotag_ms", "lcr_vcf_contig_phase_sets"} <= set(_lib.SYMBOLS)


def test_table_rounding_cannot_depend_on_the_mode():
    """llround(x * 2^40) of the 62 table entries: no product lies within 1e-6 of a half, so every rounding mode to nearest agrees"""
    fr = haplotag_ref.lut_fractions()
    assert len(fr) == 62 and min(abs(f - 0.5) for f in fr) > 1e-6
    assert haplotag_ref.FE[0] == haplotag_ref.FE[1] and haplotag_ref.F1E[0] == haplotag_ref.F1E[1]      # q = 0 as q = 1
    assert (haplotag_ref.FE[30], haplotag_ref.F1E[30]) == (-3298534883328, -477750748)
    assert (haplotag_ref.FE[20], haplotag_ref.F1E[20]) == (-2199023255552, -4799154293)


def hand_row():
    """Three candidates at 10, 20, 30 (REF A, C, G) and one row with an entry at each: A q30, C q30, G q20.  Sites: h1 = REF at the first
    two, h1 = T / h2 = G at the third -- so the row shows h1, h1, h2."""
    cands = np.zeros(3, _abi.CAND_DTYPE)
    cands["pos"] = [10, 20, 30]
    cands["ref_base"] = [ord("A"), ord("c"), ord("G")]        # (lower case in the reference: compared upper-cased)
    cands["variant_type"] = 1
    cands["flags"] = _abi.F_HET | _abi.F_FOR_PHASING
    val = [30 | 32 | (0 << 6), 30 | 32 | (1 << 6), 20 | 32 | (2 << 6)]
    fm = dict(row_ptr=np.array([0, 3], np.int64), col=np.array([0, 1, 2], np.int32), val=np.array(val, np.uint8))
    sites = (np.array([10, 20, 30], np.int64), np.frombuffer(b"ACT", np.uint8), np.frombuffer(b"CGG", np.uint8), np.array([11, 11, 11], np.uint32))
    return fm, cands, sites


def test_restatement_on_a_hand_computed_row():
    fm, cands, sites = hand_row()
    # A1 = 2 f1e[30] + fe[20], A2 = 2 fe[30] + f1e[20]
    a1, a2 = 2 * -477750748 + -2199023255552, 2 * -3298534883328 + -4799154293
    assert (a1, a2, a1 - a2, a1 + a2) == (-2199978757048, -6601868920949, 4401890163901, -8801847677997)
    assert 0.5001 < (a1 - a2) / -(a1 + a2) < 0.5002
    r = haplotag_ref.haplotag(fm, cands, sites, 1, 0.5001)
    assert (r["haplotag"].tolist(), r["assignment"].tolist(), r["phase_set"].tolist()) == ([1], [1], [11])
    assert r["cand"]["haplotype"].tolist() == [1, 1, -1] and r["cand"]["phase_set"].tolist() == [11, 11, 11]
    assert not (r["cand"]["flags"] & _abi.F_NON_SELECTED).any()
    # the row is on haplotype 1: its bases at the first two sites are haplotype 1's allele, at the third they are not
    assert r["site"].tolist() == [(-477750748, -3299012634076, 1, 0, 1, 0), (-477750748, -3299012634076, 1, 0, 1, 0),
                                  (-2199023255552, -2203822409845, 1, 0, 0, 0)]
    assert r["cand"]["phase_score"].tolist() == [haplotag_ref.PHASE_SCORE_CONST] * 3        # no row of haplotype 2 anywhere
    # the cutoff just above the row's margin, min_linkers above its entries, no sites: unassigned, site records zero
    for kw in (dict(min_linkers=1, cutoff=0.5002), dict(min_linkers=4, cutoff=0.0)):
        u = haplotag_ref.haplotag(fm, cands, sites, **kw)
        assert (u["haplotag"].tolist(), u["assignment"].tolist(), u["phase_set"].tolist()) == ([0], [0], [0]) and not u["site"]["n_h1"].any()
        assert u["cand"]["haplotype"].tolist() == [1, 1, -1]
    n = haplotag_ref.haplotag(fm, cands, None, 1, 0.0)
    assert not n["assignment"].any() and (n["cand"]["flags"] & _abi.F_NON_SELECTED).all() and not n["cand"]["haplotype"].any()
    # two phase sets, 2 entries against 1: only the larger set's entries are summed; 1 against 1 plus a tie: the smaller value
    s2 = sites[:3] + (np.array([11, 11, 5], np.uint32),)
    t = haplotag_ref.haplotag(fm, cands, s2, 1, 0.0)
    assert t["phase_set"].tolist() == [11] and t["site"]["n_h1"].tolist() == [1, 1, 0] and t["assignment"].tolist() == [1]
    s3 = sites[:3] + (np.array([11, 5, 0xFFFFFFFF], np.uint32),)
    t = haplotag_ref.haplotag(fm, cands, s3, 1, 0.0)
    assert t["phase_set"].tolist() == [5] and t["site"]["n_h1"].tolist() == [0, 1, 0]
    # an exact tie is no evidence, whatever the cutoff: one h1 and one h2 entry of equal quality
    fm2 = dict(row_ptr=np.array([0, 2], np.int64), col=np.array([0, 1], np.int32), val=np.array([30 | 32, 30 | (0 << 6)], np.uint8))
    s4 = (sites[0], np.frombuffer(b"ACT", np.uint8), np.frombuffer(b"CAG", np.uint8), sites[3])     # the second site: h1 = C (REF), h2 = A
    t = haplotag_ref.haplotag(fm2, cands, s4, 1, 0.0)
    assert t["assignment"].tolist() == [0] and t["phase_set"].tolist() == [0]


def test_merge_gene_records_with_shared_phase_sets():
    p = np.zeros(5, _abi.AGENE_DTYPE)
    p["region"] = [0, 1, 2, 2, 3]
    p["gene"] = [4, 4, 4, 9, 9]
    p["phase_set"] = [50, 70, 50, 70, 70]
    p["h1"] = [3, 5, 3, 1, 2]
    p["h2"] = [0, 0, 1, 1, 0]
    p["n_sites"] = [1, 2, 3, 1, 1]
    p["h1_pat"] = [1, 0, 2, 0, 0]
    p["n_phase_sets"] = 1
    old = ase.merge_gene_records(p)
    assert old.tolist() == ase.merge_gene_records(p, shared_phase_sets=False).tolist()
    assert [(int(r["gene"]), int(r["phase_set"]), int(r["h1"]), int(r["h2"]), int(r["region"])) for r in old] == [(4, 70, 5, 0, 1), (9, 70, 1, 1, 2)]
    new = ase.merge_gene_records(p, shared_phase_sets=True)
    # gene 4: set 50 sums to 6 + 1 = 7 rows and beats set 70's 5; gene 9: set 70 sums to 3 + 1
    assert [(int(r["gene"]), int(r["phase_set"]), int(r["h1"]), int(r["h2"]), int(r["n_sites"]), int(r["h1_pat"]), int(r["region"]), int(r["n_phase_sets"]))
            for r in new] == [(4, 50, 6, 1, 4, 3, 0, 3), (9, 70, 3, 1, 2, 0, 2, 2)]
    rec, kept = ase.merge_gene_records(p, np.array([0, 1, 1, 0, 0], bool), shared_phase_sets=True)
    assert rec.tolist() == new.tolist() and kept.tolist() == [True, False]
    assert ase.merge_gene_records(np.zeros(0, _abi.AGENE_DTYPE), shared_phase_sets=True).size == 0


def test_command_line_haplotag_needs_an_input_vcf(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_pipeline.py"), "-b", "x.bam", "-f", "x.fa", "-o", str(tmp_path / "o.vcf"),
                        "--haplotag"], capture_output=True, text=True)
    assert r.returncode != 0 and "--haplotag needs -v" in r.stderr
    from longcallr_amd import pipeline
    with pytest.raises(ValueError, match="haplotag needs input_vcf"):
        pipeline.run("x.bam", "x.fa", str(tmp_path / "o.vcf"), haplotag=True)

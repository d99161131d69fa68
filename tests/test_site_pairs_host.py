"""K19 lcr_site_pairs without a GPU: the contract's worked instance through the plain-Python restatement (tests/site_pairs_ref.py) against
hand-written numbers; pairs.cells, the orientation / agreement rules and pairs.mnv_records on hand-made records against hand-derived
results and against the restatement; the structs' layout against gcc; the pipeline's and the command line's option checks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import site_pairs_ref as ref
from longcallr_amd import _abi, asj, pairs, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, G = 0, 2
MIN_PS = 8.0


def cand(pos, ref_base="A", alt="G", vt=1, hap=1, ps=100, flags=_abi.F_HET | _abi.F_FOR_PHASING, region=0, score=20.0, qual=50.9, depth=20, a1=None):
    """a het site carries (ref, alt) as its two alleles, a homozygous one (alt, ref)"""
    s = np.zeros(1, dtype=_abi.CAND_DTYPE)
    s["pos"], s["region"], s["ref_base"], s["variant_type"], s["haplotype"], s["phase_set"] = pos, region, ord(ref_base), vt, hap, ps
    s["allele1"], s["allele2"] = (ord(a1 if a1 is not None else ref_base), ord(alt)) if vt == 1 else (ord(alt), ord(ref_base))
    s["flags"], s["phase_score"], s["qual"], s["depth"], s["genotype"] = flags, score, qual, depth, 0 if vt == 1 else -1
    return s


def hom(pos, ref_base="A", alt="G", flags=_abi.F_HOM, **kw):
    return cand(pos, ref_base, alt, vt=2, hap=0, ps=0, flags=flags, score=0.0, **kw)


def val(base, q=30, ref_base="A"):
    return ("ACGT".index(base) << 6) | (32 if base == ref_base else 0) | q


def csr(rows):
    """[{candidate: value}] -> row_ptr, col, val"""
    row_ptr, col, v = [0], [], []
    for r in rows:
        for c in sorted(r):
            col.append(c)
            v.append(r[c])
        row_ptr.append(len(col))
    return np.array(row_ptr, np.int64), np.array(col, np.int32), np.array(v, np.uint8)


def worked(site11_hom=False):
    """the header's instance: sites at columns 10, 11, 13, 40 (candidates 0..3), rows r0..r2; r1 / r2 carry the reference base at 40"""
    cands = np.concatenate([cand(10), hom(11) if site11_hom else cand(11), cand(13), cand(40)])
    rows = [{0: val("A"), 1: val("A"), 2: val("A"), 3: val("A")},
            {0: val("G"), 1: val("G"), 3: val("A")},                       # a third base at 13: no entry
            {0: val("G"), 1: val("G", 5), 2: val("G"), 3: val("A")}]
    return cands, csr(rows)


def as_tuples(rec):
    """[(a, b, n_rows, n_lowq, {(x, y): n})]"""
    return [(int(r["a"]), int(r["b"]), int(r["n_rows"]), int(r["n_lowq"]), {(x, y): int(r["n"][x][y]) for x in range(4) for y in range(4) if r["n"][x][y]})
            for r in rec]


WORKED_WANT = {
    ("all", 2, 3, 13): ([(0, 1, 3, 1, {(A, A): 1, (G, G): 1}), (0, 2, 2, 0, {(A, A): 1, (G, G): 1}), (1, 2, 2, 1, {(A, A): 1})], [0, 2, 3, 3, 3], 4),
    ("all", 2, 2, 13): ([(0, 1, 3, 1, {(A, A): 1, (G, G): 1}), (1, 2, 2, 1, {(A, A): 1})], [0, 1, 2, 2, 2], 4),
    ("phased", 1, 0, 13): ([(0, 2, 2, 0, {(A, A): 1, (G, G): 1}), (2, 3, 2, 0, {(A, A): 1, (G, A): 1})], [0, 1, 1, 2, 2], 3),
}


@pytest.mark.parametrize("key", sorted(WORKED_WANT))
def test_worked_instance(key):
    mode, K, D, q = key
    cands, (row_ptr, col, v) = worked(site11_hom=mode == "phased")
    rec, off, n_el = ref.site_pairs(row_ptr, col, v, cands, mode, K, D, q)
    want_rec, want_off, want_el = WORKED_WANT[key]
    assert as_tuples(rec) == want_rec and off.tolist() == want_off and n_el == want_el
    assert (rec["n"].reshape(len(rec), 16).sum(axis=1) + rec["n_lowq"]).tolist() == rec["n_rows"].tolist()


def test_ranks_regions_and_empty_pairs():
    """a dense candidate between eligible ones takes no partner slot; no pair across a region boundary; a pair no row holds has a zero record"""
    cands = np.concatenate([cand(5), cand(6, flags=_abi.F_DENSE | _abi.F_HET), cand(7), cand(9, region=1), cand(10, region=1)])
    rows = [{0: val("A"), 2: val("G")}, {3: val("A")}, {4: val("C")}, {}]
    rec, off, n_el = ref.site_pairs(*csr(rows), cands, "all", 1, 0, 13)
    assert as_tuples(rec) == [(0, 2, 1, 0, {(A, G): 1}), (3, 4, 0, 0, {})] and off.tolist() == [0, 1, 1, 1, 2, 2] and n_el == 4
    rec, off, _ = ref.site_pairs(*csr(rows), cands, "all", 8, 1, 13)      # 5 -> 7 is two apart
    assert as_tuples(rec) == [(3, 4, 0, 0, {})] and off.tolist() == [0, 0, 0, 0, 1, 1]
    rec, off, n_el = ref.site_pairs(*csr([]), cands[:0], "all", 2, 2, 13)
    assert rec.size == 0 and off.tolist() == [0] and n_el == 0


# ---- pairs.py on hand-made records --------------------------------------------------------------------------------------------------------
def record(a, b, lowq=0, **cells_):
    """cells_: e.g. AC=5 -> n[A][C] = 5"""
    r = np.zeros(1, dtype=_abi.SITE_PAIR_DTYPE)
    r["a"], r["b"], r["n_lowq"] = a, b, lowq
    for k, n in cells_.items():
        r["n"][0]["ACGT".index(k[0])]["ACGT".index(k[1])] = n
    r["n_rows"] = int(r["n"].sum()) + lowq
    return r


#            0 / 1 a cis het pair; 2 / 3 a trans pair; 4 / 5 a 1/1 pair; 6 / 7 a mixed run; 8 - 10 three sites with one weak pair; 11 - 14 a chain of four;
#            15 / 16 a cis pair two apart, set 300, around a lower-case reference base; 17 a site whose two alleles both differ from the reference
MNV_CANDS = np.concatenate([
    cand(100, "A", "G", hap=1, ps=77, qual=41.2, depth=30), cand(101, "C", "T", hap=1, ps=77, qual=35.9, depth=25),
    cand(200, "A", "G", hap=1, ps=77), cand(201, "C", "T", hap=-1, ps=77),
    hom(300, "A", "G", qual=60.0, depth=12), hom(301, "C", "T", qual=70.0, depth=14),
    cand(400, "A", "G", hap=1, ps=77), hom(401, "C", "T"),
    cand(500, "A", "G", hap=-1, ps=77), cand(501, "C", "T", hap=-1, ps=77), cand(502, "G", "A", hap=-1, ps=77),
    cand(600, "A", "G", hap=1, ps=77), cand(601, "C", "T", hap=1, ps=77), cand(602, "G", "A", hap=1, ps=77), cand(603, "T", "C", hap=1, ps=77),
    cand(700, "A", "G", hap=-1, ps=300), cand(702, "C", "T", hap=-1, ps=300),
    cand(800, "A", "G", a1="C", hap=1, ps=77)])
MNV_RECORDS = np.concatenate([
    record(0, 1, lowq=2, AC=5, GT=6), record(2, 3, AT=5, GC=6), record(4, 5, GT=10, GC=1), record(6, 7, AT=3, GT=9),
    record(8, 9, AC=4, GT=7), record(8, 10, AG=4, GA=2), record(9, 10, CG=4, TA=7),
    record(11, 12, AC=5, GT=5), record(11, 13, AG=5, GA=4, AC=1), record(12, 13, CG=5, TA=5), record(12, 14, CC=5, TT=5), record(13, 14, GT=5, AC=5),
    record(15, 16, AC=3, GT=3), record(16, 17, CA=2, CC=3, CG=4, TC=1)])
MNV_REFSEQ = "".join({100: "A", 101: "C", 300: "A", 301: "C", 600: "A", 601: "C", 602: "G", 700: "A", 701: "t", 702: "C"}.get(p, "N") for p in range(900))
# (index 0 of MNV_REFSEQ is position 0)
MNV_WANT = [(100, "AC", "GT", 35, "0|1", 77, 25, [100, 101], (6, 0, 0, 5)),
            (300, "AC", "GT", 60, "1/1", None, 12, [300, 301], (10, 1, 0, 0)),
            (600, "ACG", "GTA", 50, "0|1", 77, 20, [600, 601, 602], (4, 0, 0, 5)),
            (700, "ATC", "GTT", 50, "1|0", 300, 20, [700, 702], (3, 0, 0, 3))]


def test_cells_orientation_and_agreement():
    c, r = MNV_CANDS, MNV_RECORDS
    assert pairs.cells(r[0], c[0], c[1]) == (5, 0, 0, 6, 0) == ref.cells(r[0], c[0], c[1])
    assert pairs.cells(r[1], c[2], c[3]) == (0, 5, 6, 0, 0)
    assert pairs.cells(r[2], c[4], c[5]) == (0, 0, 1, 10, 0)
    # site 17: reference A, alleles C and G -- the main VCF prints C, so G is a third base there
    assert pairs.ref_alt(c[17]) == ("A", "C") and pairs.cells(r[13], c[16], c[17]) == (2, 3, 0, 1, 4) == ref.cells(r[13], c[16], c[17])
    for k, rec in enumerate(r):
        assert pairs.cells(rec, c[int(rec["a"])], c[int(rec["b"])]) == ref.cells(rec, c[int(rec["a"])], c[int(rec["b"])]), k
    assert [pairs.orientation(*x) for x in ((5, 0, 0, 6), (0, 5, 6, 0), (3, 3, 3, 3), (0, 0, 0, 0))] == ["cis", "trans", "tie", "tie"]
    assert pairs.phase_check(c[0], c[1], "cis") == "agree" and pairs.phase_check(c[0], c[1], "trans") == "disagree"
    assert pairs.phase_check(c[2], c[3], "trans") == "agree" and pairs.phase_check(c[2], c[3], "cis") == "disagree"
    assert pairs.phase_check(c[0], c[1], "tie") == "." and pairs.phase_check(c[4], c[5], "cis") == "." and pairs.phase_check(c[6], c[7], "cis") == "."
    assert pairs.phase_check(c[14], c[15], "cis") == "."       # two phase sets


def test_pairs_tsv():
    text = pairs.format_pairs_tsv([("chr1", MNV_CANDS, MNV_RECORDS)], 10, MIN_PS)
    assert text == ref.format_pairs_tsv([("chr1", MNV_CANDS, MNV_RECORDS)], 10, MIN_PS)
    lines = [l.split("\t") for l in text.splitlines()]
    assert lines[0] == pairs.HEADER_PAIRS.split("\t") and len(lines[0]) == 21
    body = lines[1:]
    # counted rows >= 10: the pairs (0,1) 11, (2,3) 11, (4,5) 11, (6,7) 12, (8,9) 11, (9,10) 11, the chain's five with 10, (16,17) 10; not (8,10) 6 and (15,16) 6
    assert [(l[1], l[2]) for l in body] == [("101", "102"), ("201", "202"), ("301", "302"), ("401", "402"), ("501", "502"), ("502", "503"),
                                            ("601", "602"), ("601", "603"), ("602", "603"), ("602", "604"), ("603", "604"), ("703", "801")]
    assert body[0][3:19] == ["A", "G", "C", "T", "0|1", "0|1", "77", "77", "5", "0", "0", "6", "0", "2", "cis", "agree"]
    assert body[1][7:9] == ["0|1", "1|0"] and body[1][17:19] == ["trans", "agree"]
    assert body[2][7:11] == ["1/1", "1/1", ".", "."] and body[2][17:19] == ["cis", "."]
    assert body[7][11:19] == ["5", "0", "0", "4", "1", "0", "cis", "agree"]       # (11,13): C is a third base at 603 -> other
    assert body[9][17:19] == ["trans", "disagree"]                                # (12,14): the reads contradict the phase
    assert body[11][11:17] == ["2", "3", "0", "1", "4", "0"] and body[11][18] == "."
    p = [asj.fisher_two_sided([[int(l[11]), int(l[12])], [int(l[13]), int(l[14])]]) for l in body]
    assert [float(l[19]) for l in body] == p and [float(l[20]) for l in body] == asj.bh_adjust(p).tolist()
    assert pairs.format_pairs_tsv([], 10) == pairs.HEADER_PAIRS + "\n"
    assert len(pairs.format_pairs_tsv([("chr1", MNV_CANDS, MNV_RECORDS)], 0, MIN_PS).splitlines()) == 1 + len(MNV_RECORDS)


def test_callable_is_the_writers_pass_line():
    variants = [MNV_CANDS[i:i + 1] for i in range(len(MNV_CANDS))]
    variants += [cand(1, flags=_abi.F_DENSE | _abi.F_HET), cand(2, flags=_abi.F_NON_SELECTED | _abi.F_HET), cand(3, score=1.0),
                 hom(4, flags=_abi.F_NON_SELECTED | _abi.F_RNA_EDIT | _abi.F_HOM), hom(5, flags=_abi.F_NON_SELECTED | _abi.F_HOM), cand(6, vt=0), cand(7, alt="A")]
    got = [pairs.callable_gt(s[0], MIN_PS) for s in variants]
    assert got == [ref.vcf_callable(s[0], "c", MIN_PS) for s in variants]
    assert got[-7:] == [None, None, None, None, "1/1", None, None] and set(got) == {None, "0|1", "1|0", "1/1"}


def test_mnv_records():
    got = pairs.mnv_records(MNV_CANDS, MNV_RECORDS, None, MNV_REFSEQ, 0, MIN_PS, 2, 3, 0.8, 2)
    assert [(m["pos0"], m["ref"], m["alt"], m["qual"], m["gt"], m["ps"], m["dp"], m["sites"], m["rb"]) for m in got] == MNV_WANT
    assert ref.mnv_records(MNV_CANDS, MNV_RECORDS, None, MNV_REFSEQ, 0, MIN_PS, 2, 3, 0.8, 2) == MNV_WANT
    # the same reference as an array that starts at position 50
    arr = np.frombuffer(MNV_REFSEQ[50:].encode(), np.uint8)
    assert pairs.mnv_records(MNV_CANDS, MNV_RECORDS, None, arr, 50, MIN_PS, 2, 3, 0.8, 2) == got
    # the thresholds: the weak pair (8,10) has aa = 2 of 6 -- merged once both bounds let it through; a distance of 1 drops the pair two apart
    loose = pairs.mnv_records(MNV_CANDS, MNV_RECORDS, None, MNV_REFSEQ, 0, MIN_PS, 2, 2, 0.3, 2)
    assert [m["pos0"] for m in loose] == [100, 300, 500, 600, 700] and loose[2]["alt"] == "GTA" and loose[2]["gt"] == "1|0" and loose[2]["rb"] == (2, 0, 0, 4)
    assert [m["pos0"] for m in pairs.mnv_records(MNV_CANDS, MNV_RECORDS, None, MNV_REFSEQ, 0, MIN_PS, 1, 3, 0.8, 2)] == [100, 300, 600]
    assert [m["pos0"] for m in pairs.mnv_records(MNV_CANDS, MNV_RECORDS, None, MNV_REFSEQ, 0, MIN_PS, 2, 7, 0.8, 2)] == [300]
    # a run of one partner: the chain of four is cut into two pairs
    k1 = pairs.mnv_records(MNV_CANDS, MNV_RECORDS, None, MNV_REFSEQ, 0, MIN_PS, 2, 3, 0.8, 1)
    assert [(m["pos0"], m["sites"]) for m in k1 if m["pos0"] >= 600 and m["pos0"] < 700] == [(600, [600, 601]), (602, [602, 603])]
    assert ref.mnv_records(MNV_CANDS, MNV_RECORDS, None, MNV_REFSEQ, 0, MIN_PS, 2, 3, 0.8, 1) == [
        (m["pos0"], m["ref"], m["alt"], m["qual"], m["gt"], m["ps"], m["dp"], m["sites"], m["rb"]) for m in k1]
    text, n = pairs.format_mnv_vcf([("chr2", got[2:]), ("chr1", got[:2])], ["chr1", "chr2"])
    assert n == 4 and text.splitlines() == [
        "chr1\t101\t.\tAC\tGT\t35\tPASS\tRDS=mnv;SITES=101,102;RB=6,0,0,5\tGT:PS:DP\t0|1:77:25",
        "chr1\t301\t.\tAC\tGT\t60\tPASS\tRDS=mnv;SITES=301,302;RB=10,1,0,0\tGT:PS:DP\t1/1:.:12",
        "chr2\t601\t.\tACG\tGTA\t50\tPASS\tRDS=mnv;SITES=601,602,603;RB=4,0,0,5\tGT:PS:DP\t0|1:77:20",
        "chr2\t701\t.\tATC\tGTT\t50\tPASS\tRDS=mnv;SITES=701,703;RB=3,0,0,3\tGT:PS:DP\t1|0:300:20"]


def test_instances_exercise_every_class():
    recs = [ref.site_pairs(*worked()[1], worked()[0], "all", 2, 3, 13)[0]]
    cands = np.concatenate([cand(9, region=1), cand(10, region=1)])
    recs.append(ref.site_pairs(*csr([{0: val("A")}, {1: val("C")}]), cands, "all", 1, 0, 13)[0])
    rec = np.concatenate(recs)
    assert rec["n"].any() and rec["n_lowq"].any() and (rec["n_rows"] == 0).any() and (rec["n_rows"] > 0).any()
    assert any(pairs.cells(r, MNV_CANDS[int(r["a"])], MNV_CANDS[int(r["b"])])[4] > 0 for r in MNV_RECORDS)       # an "other" base
    assert MNV_RECORDS["n_lowq"].any()


# ---- layout and option checks -------------------------------------------------------------------------------------------------------------
def test_layout_against_gcc(tmp_path):
    fields = [("lcr_site_pair", f) for f in ("a", "b", "n_rows", "n_lowq", "n")] + [("lcr_site_pair_params", f) for f in ("mode", "max_partners", "max_dist", "min_baseq")] \
        + [("lcr_site_pair_list", f) for f in ("n_cand", "n_eligible", "n_pairs", "pad_", "pair", "pair_off", "dev_pair", "dev_pair_off")]
    body = "".join('printf("%%zu\\n", offsetof(%s, %s));' % sf for sf in fields)
    src = tmp_path / "sp.c"
    src.write_text('#include "lcr.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu %%zu %%zu %%d %%d %%d\\n", sizeof(lcr_site_pair), '
                   'sizeof(lcr_site_pair_params), sizeof(lcr_site_pair_list), LCR_PAIRS_ALL, LCR_PAIRS_PHASED, LCR_PAIRS_MAX_PARTNERS);%s return 0;}' % body)
    exe = tmp_path / "sp"
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = [int(x) for x in os.popen(str(exe)).read().split()]
    assert got[:6] == [_abi.SITE_PAIR_DTYPE.itemsize, C.sizeof(_abi.LcrSitePairParams), C.sizeof(_abi.LcrSitePairList), _abi.PAIRS_ALL, _abi.PAIRS_PHASED,
                       _abi.PAIRS_MAX_PARTNERS] and got[0] == 80
    want = [_abi.SITE_PAIR_DTYPE.fields[f][1] for f in ("a", "b", "n_rows", "n_lowq", "n")]
    want += [getattr(_abi.LcrSitePairParams, f).offset for f in ("mode", "max_partners", "max_dist", "min_baseq")]
    want += [getattr(_abi.LcrSitePairList, f).offset for f in ("n_cand", "n_eligible", "n_pairs", "pad_", "pair", "pair_off", "dev_pair", "dev_pair_off")]
    assert got[6:] == want
    assert _abi.SITE_PAIR_DTYPE["n"].shape == (4, 4)


@pytest.mark.parametrize("bad", [dict(pairs_partners=0), dict(pairs_partners=9), dict(pairs_partners=1.5), dict(pairs_partners=True), dict(pairs_min_count=-1),
                                 dict(pairs_min_baseq=31), dict(pairs_min_baseq=-1), dict(mnv_max_dist=0), dict(mnv_min_count=-1),
                                 dict(mnv_min_frac=1.5), dict(mnv_min_frac=-0.1), dict(mnv_min_frac=float("nan"))])
@pytest.mark.parametrize("which", ["pairs_out", "mnv_out"])
def test_pipeline_rejects_bad_values(tmp_path, which, bad):
    with pytest.raises(ValueError, match=list(bad)[0]):
        pipeline.run(str(tmp_path / "no.bam"), str(tmp_path / "no.fa"), str(tmp_path / "out.vcf"), **{which: str(tmp_path / "o")}, **bad)
    assert not list(tmp_path.iterdir())


def test_command_line_refuses_bad_values(tmp_path):
    for flag, v in (("--pairs-partners", "9"), ("--pairs-min-baseq", "31"), ("--mnv-max-dist", "0"), ("--mnv-min-frac", "1.5")):
        cmd = [sys.executable, os.path.join(ROOT, "tools", "run_pipeline.py"), "-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"),
               "-o", str(tmp_path / "out.vcf"), "--pairs-out", str(tmp_path / "p.tsv"), flag, v]
        p = subprocess.run(cmd, capture_output=True, text=True)
        assert p.returncode == 2 and flag in p.stderr and not (tmp_path / "out.vcf").exists(), flag

"""The host side of lcr_site_counts without a GPU: the record's layout against the header, the contract's worked instance through its
plain-Python restatement (tests/site_counts_ref.py), ase.format_sites_tsv on hand-made records, and the command line's refusal."""
import os
import subprocess
import sys

import numpy as np

import site_counts_ref as ref
from longcallr_amd import _abi, ase, asj, vcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, C_, G, T = 0, 1, 2, 3


def test_struct_layout_matches_the_header(tmp_path):
    names = ["phase_set", "n_phase_sets", "n_entries", "n_lowq", "n"]
    src = tmp_path / "sc.c"
    src.write_text('#include "lcr.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu",sizeof(lcr_site_count),'
                   'sizeof(lcr_site_count_params),sizeof(((lcr_site_count*)0)->n));'
                   + "".join('printf(" %%zu",offsetof(lcr_site_count,%s));' % f for f in names) + 'printf("\\n");return 0;}')
    exe = tmp_path / "sc"
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = [int(x) for x in os.popen(str(exe)).read().split()]
    import ctypes as C
    want = [_abi.SITE_COUNT_DTYPE.itemsize, C.sizeof(_abi.LcrSiteCountParams), 48] + [_abi.SITE_COUNT_DTYPE.fields[f][1] for f in names]
    assert got == want and got[0] == 64 and got[1] == 4
    assert _abi.SITE_COUNT_DTYPE.fields["n"][0].shape == (3, 4)      # n[k][b], row-major as the C array


# ---- the worked instance of the contract: one site, reference base A, seven entries, one per row --------------------------------------
ROWS = [(1, 100, A, 30), (1, 100, G, 30), (2, 100, G, 12), (2, 200, G, 30), (2, 200, A, 30), (0, 0, A, 20), (1, 0, G, 30)]


def worked(cand_ps, min_baseq):
    row_ptr = list(range(len(ROWS) + 1))
    col = [0] * len(ROWS)
    val = [(b << 6) | q for _, _, b, q in ROWS]
    return ref.site_counts(row_ptr, col, val, [r[0] for r in ROWS], [r[1] for r in ROWS], [cand_ps], min_baseq)[0]


def cells(rec):
    return [[int(x) for x in row] for row in rec["n"]]


def test_worked_instance():
    r = worked(0, 13)       # unphased: 100 and 200 tie 2 : 2 -> the smaller
    assert (int(r["phase_set"]), int(r["n_phase_sets"]), int(r["n_entries"]), int(r["n_lowq"])) == (100, 2, 7, 1)
    assert cells(r) == [[2, 0, 2, 0], [1, 0, 1, 0], [0, 0, 0, 0]]
    r = worked(0, 0)        # everything counts: 100 wins 3 : 2
    assert (int(r["phase_set"]), int(r["n_phase_sets"]), int(r["n_entries"]), int(r["n_lowq"])) == (100, 2, 7, 0)
    assert cells(r) == [[2, 0, 2, 0], [1, 0, 1, 0], [0, 0, 1, 0]]
    r = worked(200, 13)     # the candidate's own set
    assert (int(r["phase_set"]), int(r["n_phase_sets"]), int(r["n_entries"]), int(r["n_lowq"])) == (200, 2, 7, 1)
    assert cells(r) == [[2, 0, 2, 0], [0, 0, 0, 0], [1, 0, 1, 0]]
    for rec in (worked(0, 13), worked(0, 0), worked(200, 13), worked(300, 30)):
        assert int(rec["n"].sum()) + int(rec["n_lowq"]) == int(rec["n_entries"])
    r = worked(300, 13)     # a set none of the rows is in: both haplotype rows are zero
    assert int(r["phase_set"]) == 300 and cells(r) == [[3, 0, 3, 0], [0, 0, 0, 0], [0, 0, 0, 0]]


def test_restatement_without_entries():
    out = ref.site_counts([0, 0, 0], [], [], [1, 2], [5, 5], [0, 77], 13)
    assert out.dtype == _abi.SITE_COUNT_DTYPE and out["phase_set"].tolist() == [0, 77] and not out["n_entries"].any() and not out["n"].any()
    assert len(ref.site_counts([0], [], [], [], [], [], 13)) == 0


# ---- format_sites_tsv on hand-made records --------------------------------------------------------------------------------------------
def cand(pos, ref_base, a1, a2, vt=1, flags=0, ps=0, hap=1, score=20.0, gt=0, af1=0.5, af2=0.5, depth=40):
    c = np.zeros(1, dtype=_abi.CAND_DTYPE)
    c["pos"], c["ref_base"], c["allele1"], c["allele2"] = pos, ord(ref_base), ord(a1), ord(a2)
    c["variant_type"], c["flags"], c["phase_set"], c["haplotype"], c["phase_score"], c["genotype"] = vt, flags, ps, hap, score, gt
    c["af1"], c["af2"], c["depth"], c["gq"], c["qual"] = af1, af2, depth, 30.0, 50.0
    return c


def rec(ps, other, h1, h2, n_sets=1):
    r = np.zeros(1, dtype=_abi.SITE_COUNT_DTYPE)
    r["phase_set"], r["n_phase_sets"] = ps, n_sets
    r["n"][0] = [other, h1, h2]
    r["n_entries"] = int(r["n"].sum())
    return r


def hand_table():
    cs = [cand(99, "A", "A", "G", ps=100, hap=1),                                   # 0: PASS 0|1, 12 reads on the haplotypes
          cand(199, "c", "C", "T", ps=100, hap=-1),                                 # 1: a lower-case reference base, 1|0
          cand(299, "A", "A", "G", ps=100),                                         # 2: support 9: dropped
          cand(399, "A", "A", "G", ps=100),                                         # 3: support 10: kept
          cand(499, "A", "C", "G", vt=3, flags=_abi.F_NON_SELECTED, gt=0),          # 4: triallelic 1/2: two alt cells summed, PS "."
          cand(599, "A", "A", "A", ps=100),                                         # 5: no ALT: the writer prints no line
          cand(699, "A", "A", "G", vt=1, flags=_abi.F_NON_SELECTED | _abi.F_RNA_EDIT)]   # 6: RnaEdit 0/1
    rs = [rec(100, [1, 0, 2, 0], [6, 0, 1, 0], [0, 0, 5, 0]),
          rec(100, [0, 3, 0, 0], [0, 2, 0, 9], [0, 8, 0, 1]),
          rec(100, [50, 0, 50, 0], [4, 0, 0, 0], [0, 0, 5, 0]),
          rec(100, [0, 0, 0, 0], [5, 0, 0, 0], [0, 0, 5, 0]),
          rec(0, [7, 6, 5, 0], [0, 0, 0, 0], [0, 0, 0, 0]),
          rec(100, [0, 0, 0, 0], [30, 0, 0, 0], [30, 0, 0, 0]),
          rec(77, [0, 0, 0, 0], [10, 0, 1, 0], [2, 0, 9, 0])]
    return np.concatenate(cs), np.concatenate(rs)


def test_format_sites_tsv():
    cands, recs = hand_table()
    text = ase.format_sites_tsv([("chr1", cands, recs)], min_support=10, overdispersion=0.001, min_phase_score=11.0)
    lines = text.split("\n")
    assert lines[0] == ase.HEADER_SITES and lines[0].split("\t") == [
        "#Chr", "Pos", "Ref", "Alt", "Filter", "GT", "PS", "H1_ref", "H1_alt", "H2_ref", "H2_alt", "Other_ref", "Other_alt",
        "P_ase", "P_ase_adj", "P_hap", "P_hap_adj"] and lines[-1] == ""
    rows = [l.split("\t") for l in lines[1:-1]]
    # candidate 2 (support 9) and 5 (no line) are absent; 4 has no read on a haplotype, so it is dropped at any positive min_support
    assert [r[1] for r in rows] == ["100", "200", "400", "700"]
    assert rows[0][:13] == ["chr1", "100", "A", "G", "PASS", "0|1", "100", "6", "1", "0", "5", "1", "2"]
    # (the writer compares the bytes, so it prints C as the ALT of c; the counts take the C cell as the reference's)
    assert rows[1][:13] == ["chr1", "200", "c", "C", "PASS", "1|0", "100", "2", "9", "8", "1", "3", "0"]
    assert rows[2][:13] == ["chr1", "400", "A", "G", "PASS", "0|1", "100", "5", "0", "0", "5", "0", "0"]
    assert rows[3][:13] == ["chr1", "700", "A", "G", "RnaEdit", "0/1", "77", "10", "1", "2", "9", "0", "0"]
    tables = [(6, 1, 0, 5), (2, 9, 8, 1), (5, 0, 0, 5), (10, 1, 2, 9)]
    p_ase = [ase.betabinom_two_sided(a1 + a2, r1 + a1 + r2 + a2, 0.5, 0.001) for r1, a1, r2, a2 in tables]
    p_hap = [asj.fisher_two_sided([[r1, a1], [r2, a2]]) for r1, a1, r2, a2 in tables]
    assert [float(r[13]) for r in rows] == p_ase and [float(r[15]) for r in rows] == p_hap
    assert [float(r[14]) for r in rows] == asj.bh_adjust(p_ase).tolist() and [float(r[16]) for r in rows] == asj.bh_adjust(p_hap).tolist()
    assert len(set(p_ase)) > 1 and asj.bh_adjust(p_hap).tolist() != p_hap      # (the adjustment moves something)
    assert text == ref.format_rows([("chr1", cands, recs)], 10, 0.001, 11.0)
    # min_support 0 writes every candidate with a line: the triallelic one with both alternate cells summed and "." for PS 0
    rows0 = [l.split("\t") for l in ase.format_sites_tsv([("chr1", cands, recs)], 0, 0.001, 11.0).split("\n")[1:-1]]
    assert [r[1] for r in rows0] == ["100", "200", "300", "400", "500", "700"]
    assert rows0[4][:13] == ["chr1", "500", "A", "C,G", "Multiallelic", "1/2", ".", "0", "0", "0", "0", "7", "11"]
    assert float(rows0[4][13]) == 1.0 and float(rows0[4][15]) == 1.0
    # the edge: 9 reads against 10
    assert rows0[2][7:11] == ["4", "0", "0", "5"] and rows0[3][7:11] == ["5", "0", "0", "5"]
    # the writer's min_phase_score decides Filter and GT: below it candidate 0 is a LowQual 0/1
    low = ase.format_sites_tsv([("chr1", cands[:1], recs[:1])], 10, 0.001, 25.0).split("\n")[1].split("\t")
    assert low[4:6] == ["LowQual", "0/1"]
    # two tables: rows in the order given, one adjustment over all of them
    two = ase.format_sites_tsv([("chr1", cands[:2], recs[:2]), ("chr2", cands[3:4], recs[3:4])], 10, 0.001, 11.0).split("\n")[1:-1]
    assert [l.split("\t")[0] for l in two] == ["chr1", "chr1", "chr2"]
    assert [float(l.split("\t")[14]) for l in two] == asj.bh_adjust(p_ase[:3]).tolist()
    assert ase.format_sites_tsv([], 10) == ase.HEADER_SITES + "\n"
    assert vcf.format_records(cands[5:6], "chr1", 11.0) == ""


def test_command_line_refuses_a_threshold_above_30(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_pipeline.py"), "-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"),
           "-o", str(tmp_path / "out.vcf"), "--ase-sites-out", str(tmp_path / "s.tsv"), "--ase-sites-min-baseq", "31"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 2 and "--ase-sites-min-baseq" in p.stderr and not (tmp_path / "out.vcf").exists()

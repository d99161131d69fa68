"""The host side of lcr_isoforms without a GPU: the records' layout against the header, the contract's worked instance through its
plain-Python restatement (tests/isoforms_ref.py) with hand-written expected values, the arms of the contract at pos == a and rend == e,
isoforms.chains / isoforms.format_tsv, and the argument plumbing of pipeline.run and the command line."""
import ctypes as C
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import isoforms_ref as ref
from longcallr_amd import _abi, isoforms, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = ("h1_absent", "h1_present", "h2_absent", "h2_present")


def test_struct_layout_matches_the_header(tmp_path):
    iso_f = list(_abi.ISOFORM_DTYPE.names)
    lst_f = ["n_regions", "n_isoforms", "n_chain", "n_rows", "iso", "iso_region_off", "chain", "row_isoform", "dev_iso", "dev_chain", "dev_row_isoform"]
    src = tmp_path / "iso.c"
    src.write_text('#include "lcr.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu",sizeof(lcr_isoform),'
                   'sizeof(lcr_isoform_list),sizeof(lcr_isoform_params));'
                   + "".join('printf(" %%zu",offsetof(lcr_isoform,%s));' % f for f in iso_f)
                   + "".join('printf(" %%zu",offsetof(lcr_isoform_list,%s));' % f for f in lst_f) + 'printf("\\n");return 0;}')
    exe = tmp_path / "iso"
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = [int(x) for x in os.popen(str(exe)).read().split()]
    want = ([_abi.ISOFORM_DTYPE.itemsize, C.sizeof(_abi.LcrIsoformList), C.sizeof(_abi.LcrIsoformParams)]
            + [_abi.ISOFORM_DTYPE.fields[f][1] for f in iso_f] + [getattr(_abi.LcrIsoformList, f).offset for f in lst_f])
    assert got == want and got[:3] == [64, 72, 8]


# ---- the worked instance of the contract ------------------------------------------------------------------------------------------------
WORKED = [("20M30N20M40N20M", 1), ("20M30N20M40N20M", 2), ("20M30N20M40N20M", 1), ("20M30N20M40N20M50N10M", 2), ("20M30N80M", 1),
          ("20M30N20M40N20M", 0), ("130M", 1), ("20M30N25M35N20M", 2)]       # R1 .. R8: CIGAR, class
A = [(1020, 30), (1070, 40)]
B = A + [(1130, 50)]
Cc = [(1020, 30)]
D = [(1020, 30), (1075, 35)]
#              chain  extent        n_reads n_h1 n_h2  cells
WORKED_WANT = [(Cc, (1020, 1050), (1, 1, 0), (0, 3, 0, 3)),
               (A, (1020, 1110), (3, 2, 1), (1, 2, 1, 2)),
               (B, (1020, 1180), (1, 0, 1), (0, 0, 0, 1)),
               (D, (1020, 1110), (1, 0, 1), (3, 0, 2, 1))]


def seq_len(cigar):
    import re
    return sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MIS=X")


def worked_batch(cigars=None):
    cigars = [c for c, _ in WORKED] if cigars is None else cigars
    reads = [dict(pos=1000, seq="A" * seq_len(c), qual=30, cigar=c, region=0) for c in cigars]
    return helpers.mk_batch(reads, [(1000, "A" * 300)])


def worked(min_count, min_junctions=1):
    b = worked_batch()
    n = len(WORKED)
    return ref.isoforms(b, [0, n], list(range(n)), [c for _, c in WORKED], [7] * n, min_count, min_junctions)


def summary(rec, pool):
    return [(ch, (int(r["start0"]), int(r["end0"])), (int(r["n_reads"]), int(r["n_h1"]), int(r["n_h2"])), tuple(int(r[f]) for f in CELLS))
            for r, ch in zip(rec, isoforms.chains(rec, pool))]


def test_worked_instance():
    rec, off, pool, row_iso = worked(1)
    assert summary(rec, pool) == WORKED_WANT            # the order is C, A, B, D
    assert off.tolist() == [0, 4] and rec["region"].tolist() == [0] * 4 and rec["n_junc"].tolist() == [1, 2, 3, 2]
    assert rec["chain_first"].tolist() == [0, 1, 3, 6] and pool.size == 8
    assert rec["phase_set"].tolist() == [7] * 4 and rec["n_phase_sets"].tolist() == [1] * 4
    assert row_iso.tolist() == [1, 1, 1, 2, 0, -1, -1, 3]       # R6 is unassigned, R7 has no junction
    # min_count 2: only A is kept, with the same four cells -- the rows of chains that are not kept still count
    rec2, off2, pool2, row2 = worked(2)
    assert summary(rec2, pool2) == [WORKED_WANT[1]] and off2.tolist() == [0, 1]
    assert row2.tolist() == [0, 0, 0, -1, -1, -1, -1, -1]
    # min_junctions 2: R5 (one junction) takes no part, neither as a chain nor as a spanning row
    rec3, _, pool3, row3 = worked(1, 2)
    assert [s[0] for s in summary(rec3, pool3)] == [A, B, D] and summary(rec3, pool3)[0][3] == (0, 2, 1, 2)
    assert row3.tolist() == [0, 0, 0, 1, -1, -1, -1, 2]
    with pytest.raises(ValueError):
        worked(1, 0)


def one_region(cigars, pos, cls, ps, min_count=1, min_junctions=1):
    reads = [dict(pos=p, seq="A" * seq_len(c), qual=30, cigar=c, region=0) for c, p in zip(cigars, pos)]
    b = helpers.mk_batch(reads, [(1000, "A" * 400)])
    n = len(cigars)
    return ref.isoforms(b, [0, n], list(range(n)), cls, ps, min_count, min_junctions)


def test_arms_at_the_ends_of_a_read():
    """pos == a (a CIGAR that begins with N) and rend == e (one that ends with N) span; one base short on either side does not"""
    cig = ["20M30N20M", "30N20M", "20M30N", "20M29N21M", "21M29N20M"]
    pos = [1000, 1020, 1000, 1000, 1000]
    rec, off, pool, row_iso = one_region(cig, pos, [1, 2, 1, 2, 1], [5] * 5)
    ch = isoforms.chains(rec, pool)
    assert ch == [[(1020, 29)], [(1020, 30)], [(1021, 29)]]
    k = ch.index([(1020, 30)])
    assert int(rec["n_reads"][k]) == 3 and row_iso.tolist() == [1, 1, 1, 0, 2]
    # [1020, 1050): the read at 1020 starts AT a, the third ends AT e: both span and are present; (1020, 29) and (1021, 29) lie inside: absent
    assert tuple(int(rec[f][k]) for f in CELLS) == (1, 2, 1, 1)
    # a read that starts one base inside the extent, or ends one base short of it, is neither
    rec, _, pool, _ = one_region(["20M30N20M", "29N20M", "21M28N"], [1000, 1021, 1000], [1, 2, 2], [5] * 3)
    k = isoforms.chains(rec, pool).index([(1020, 30)])
    assert tuple(int(rec[f][k]) for f in CELLS) == (0, 1, 0, 0)


def test_restatement_rules():
    # a zero-length N is no junction; I S H consume nothing, D = X do
    rec, _, pool, row_iso = one_region(["2H3S10=5D5X0N2I10N5M0N5M20N5M", "20M10N10M20N5M"], [1000, 1000], [1, 2], [1, 1])
    assert isoforms.chains(rec, pool) == [[(1020, 10), (1040, 20)]] and int(rec["n_reads"][0]) == 2 and row_iso.tolist() == [0, 0]
    # phase sets: the most rows win, a tie goes to the smaller value, 0 is a value like any other
    cig = ["20M30N20M"] * 6
    rec, _, _, _ = one_region(cig, [1000] * 6, [1, 2, 1, 2, 1, 2], [9, 9, 0, 0, 4, 4])
    assert (int(rec["phase_set"][0]), int(rec["n_phase_sets"][0]), int(rec["n_reads"][0])) == (0, 3, 6)
    assert tuple(int(rec[f][0]) for f in CELLS) == (0, 1, 0, 1) and (int(rec["n_h1"][0]), int(rec["n_h2"][0])) == (3, 3)
    rec, _, _, _ = one_region(cig, [1000] * 6, [1, 2, 1, 2, 1, 1], [9, 9, 3, 4, 4, 4])
    assert (int(rec["phase_set"][0]), int(rec["n_phase_sets"][0])) == (4, 3) and tuple(int(rec[f][0]) for f in CELLS) == (0, 2, 0, 1)
    # an exon-skipping read and junctions that straddle a or e: absent; introns outside the extent on either side: present
    cig = ["50M30N20M40N60M", "50M30N20M40N60M", "50M90N60M", "50M30N20M45N55M", "45M35N20M40N60M", "10M10N30M30N20M40N20M10N30M"]
    rec, _, pool, _ = one_region(cig, [1000] * 6, [1, 1, 2, 2, 2, 1], [1] * 6, min_count=2)
    assert isoforms.chains(rec, pool) == [[(1050, 30), (1100, 40)]]
    assert tuple(int(rec[f][0]) for f in CELLS) == (0, 3, 3, 0)


# ---- isoforms.format_tsv ---------------------------------------------------------------------------------------------------------------
def test_format_tsv_worked_instance():
    rec, off, pool, _ = worked(1)
    text = isoforms.format_tsv([("chr7", rec, pool, [1000], [300])], min_count=1)
    ln2, b_sor, d_sor = repr(math.log(2.0)), repr(math.log(2.0 + 0.5)), repr(math.log(8.0 / 3.0 + 3.0 / 8.0))
    assert text == (
        "#Isoform\tRegion\tN_junctions\tChain\tReads\tH1_reads\tH2_reads\tPhase_set\tHap1_absent\tHap1_present\tHap2_absent\tHap2_present\tP_value\tSOR\n"
        "chr7:1021-1050\tchr7:1001-1300\t1\t1021-1050\t1\t1\t0\t7\t0\t3\t0\t3\t1.0\t" + ln2 + "\n"
        "chr7:1021-1110\tchr7:1001-1300\t2\t1021-1050,1071-1110\t3\t2\t1\t7\t1\t2\t1\t2\t1.0\t" + ln2 + "\n"
        "chr7:1021-1180\tchr7:1001-1300\t3\t1021-1050,1071-1110,1131-1180\t1\t0\t1\t7\t0\t0\t0\t1\t1.0\t" + b_sor + "\n"
        "chr7:1021-1110\tchr7:1001-1300\t2\t1021-1050,1076-1110\t1\t0\t1\t7\t3\t0\t2\t1\t1.0\t" + d_sor + "\n")
    # rows whose four cells sum to less than min_count are not written: B's single spanning row
    assert [ln.split("\t")[3] for ln in isoforms.format_tsv([("chr7", rec, pool, [1000], [300])], min_count=2).splitlines()[1:]] == [
        "1021-1050", "1021-1050,1071-1110", "1021-1050,1076-1110"]
    assert isoforms.format_tsv([]) == text.splitlines()[0] + "\n"


def test_format_tsv_adjusts_over_the_written_rows_only():
    rec = np.zeros(3, dtype=_abi.ISOFORM_DTYPE)
    pool = np.array([(100 << 32) | 10, (100 << 32) | 20, (300 << 32) | 5, (100 << 32) | 30], dtype=np.uint64)
    for k, (n, first, cells, ps) in enumerate([(1, 0, (20, 0, 0, 20), 0), (2, 1, (1, 1, 1, 0), 3), (1, 3, (5, 5, 5, 5), 8)]):
        rec[k]["region"], rec[k]["n_junc"], rec[k]["chain_first"], rec[k]["phase_set"] = k % 2, n, first, ps
        ch = isoforms.chains(rec[k:k + 1], pool)[0]
        rec[k]["start0"], rec[k]["end0"] = ch[0][0], ch[-1][0] + ch[-1][1]
        rec[k]["n_reads"], rec[k]["n_h1"], rec[k]["n_h2"] = sum(cells), cells[0] + cells[1], cells[2] + cells[3]
        for f, v in zip(CELLS, cells):
            rec[k][f] = v
    rows = [ln.split("\t") for ln in isoforms.format_tsv([("c", rec, pool, [50, 60], [500, 600])], min_count=10).splitlines()[1:]]
    assert [r[0] for r in rows] == ["c:101-110", "c:101-130"] and [r[1] for r in rows] == ["c:51-550", "c:51-550"]
    assert [r[7] for r in rows] == [".", "8"] and [r[3] for r in rows] == ["101-110", "101-130"]
    # Fisher's p of the complete separation is 2 / C(40, 20), above the G-test's; over the TWO written rows its adjusted value is twice
    # that (three rows would make it three times that); the balanced table stays 1
    assert float(rows[0][12]) == pytest.approx(2.0 * 2.0 / math.comb(40, 20), rel=1e-9) and float(rows[1][12]) == 1.0
    assert float(rows[0][13]) == pytest.approx(math.log(441.0 + 1.0 / 441.0), rel=1e-12)


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------
def test_pipeline_arguments():
    sig = inspect.signature(pipeline.run).parameters
    assert (sig["isoforms_out"].default, sig["isoform_min_count"].default, sig["isoform_min_junctions"].default) == (None, 10, 1)
    for kw in (dict(isoform_min_junctions=0), dict(isoform_min_count=-1), dict(isoform_min_junctions=1.5)):
        with pytest.raises(ValueError):
            pipeline.run("no.bam", "no.fa", "no.vcf", isoforms_out="no.tsv", **kw)


def test_command_line_arguments():
    tool = os.path.join(ROOT, "tools", "run_pipeline.py")
    r = subprocess.run([sys.executable, tool, "-b", "x.bam", "-f", "x.fa", "-o", "x.vcf", "--isoforms-out", "x.tsv", "--isoform-min-junctions", "0"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--isoform-min-junctions" in r.stderr
    h = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and "--isoforms-out" in h.stdout and "--isoform-min-count" in h.stdout

"""The host side of lcr_intron_retention without a GPU: the records' layout against the header, the three symbols in the built library, the
contract's worked instance through its plain-Python restatement (tests/retention_ref.py) with hand-written expected values,
retention.format_tsv, and the argument plumbing of pipeline.run and the command line."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers
import retention_ref as ref
from longcallr_amd import _abi, _lib, pipeline, retention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = ("h1_spliced", "h1_retained", "h2_spliced", "h2_retained")
COUNTS = ("n_spliced", "n_retained", "n_other")


def test_struct_layout_matches_the_header(tmp_path):
    rec_f = [f for f in _abi.RETAINED_INTRON_DTYPE.names]
    lst_f = ["n_regions", "n_introns", "n_rows", "n_part", "n_retained_total", "intron", "intron_region_off", "row_retained", "dev_intron",
             "dev_row_retained"]
    par_f = ["min_count", "anchor", "pad_"]
    src = tmp_path / "ret.c"
    src.write_text('#include "lcr.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu",sizeof(lcr_retained_intron),'
                   'sizeof(lcr_retention_list),sizeof(lcr_retention_params));'
                   + "".join('printf(" %%zu",offsetof(lcr_retained_intron,%s));' % f for f in rec_f)
                   + "".join('printf(" %%zu",offsetof(lcr_retention_list,%s));' % f for f in lst_f)
                   + "".join('printf(" %%zu",offsetof(lcr_retention_params,%s));' % f for f in par_f) + 'printf("\\n");return 0;}')
    exe = tmp_path / "ret"
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = [int(x) for x in os.popen(str(exe)).read().split()]
    want = ([_abi.RETAINED_INTRON_DTYPE.itemsize, C.sizeof(_abi.LcrRetentionList), C.sizeof(_abi.LcrRetentionParams)]
            + [_abi.RETAINED_INTRON_DTYPE.fields[f][1] for f in rec_f] + [getattr(_abi.LcrRetentionList, f).offset for f in lst_f]
            + [getattr(_abi.LcrRetentionParams, f).offset for f in par_f])
    assert got == want and got[:3] == [56, 64, 16]
    assert rec_f == ["region", "motif", "pad_", "start0", "len", "n_spliced", "n_retained", "n_other", "phase_set", "n_phase_sets", "h1_spliced",
                     "h1_retained", "h2_spliced", "h2_retained"]
    # the header carries the contract above the declarations
    hdr = open(os.path.join(ROOT, "include", "lcr.h")).read()
    k = hdr.index("int lcr_intron_retention(")
    for word in ("SPLICED", "RETAINED", "OTHER", "ties to the smallest value", "row_retained", "Not here:", "partial retention", "anchor > 4096"):
        assert word in hdr[hdr.index("Allele-specific intron retention (K17)"):k], word


def test_symbols_resolve():
    lib = _lib.load()                    # (no GPU is touched by loading it)
    for name in ("lcr_intron_retention", "lcr_get_intron_retention", "lcr_intron_retention_ms"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    # before lcr_phase nothing changes: a NULL context is an argument error, not a crash
    assert lib.lcr_intron_retention(None, None) == -1 and lib.lcr_get_intron_retention(None, None) == -1 and lib.lcr_intron_retention_ms(None, None) == -1


# ---- the worked instance of the contract: region [1000, 1400), min_count = 2, anchor = 10; all reads start at window column 0 ------------
WORKED = [(0, "50M100N50M60N40M", 1),
          (0, "50M100N50M60N40M", 2),
          (0, "50M100N150M", 1),
          (0, "200M60N40M", 2),
          (0, "300M", 2),
          (0, "155M", 1),
          (0, "50M90N160M", 1),
          (0, "50M100N50M60N40M", 0),
          (0, "100M20D80M60N40M", 2)]
#                 s    l   (spliced, retained, other)  (h1_spliced, h1_retained, h2_spliced, h2_retained)
WORKED_WANT = [(1050, 100, (3, 3, 2), (2, 0, 1, 3)),
               (1200, 60, (4, 3, 0), (1, 2, 3, 1))]
WORKED_ROW_RETAINED = [0, 0, 1, 1, 2, 0, 1, 0, 1]


def seq_len(cigar):
    return sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MIS=X")


def batch_of(reads, start0=1000, length=400):
    """reads: [(column, CIGAR, class)] of one region"""
    return helpers.mk_batch([dict(pos=start0 + col, seq="A" * seq_len(c), qual=30, cigar=c, region=0) for col, c, _ in reads], [(start0, "A" * length)])


def run_ref(reads, min_count, anchor, ps=None, **kw):
    n = len(reads)
    return ref.intron_retention(batch_of(reads, **kw), [0, n], list(range(n)), [r[2] for r in reads], [7] * n if ps is None else ps, min_count, anchor)


def summary(rec):
    return [(int(r["start0"]), int(r["len"]), tuple(int(r[f]) for f in COUNTS), tuple(int(r[f]) for f in CELLS)) for r in rec]


def test_worked_instance():
    rec, off, row_retained, tot = run_ref(WORKED, 2, 10)
    assert rec.dtype == _abi.RETAINED_INTRON_DTYPE and summary(rec) == WORKED_WANT
    assert off.tolist() == [0, 2] and rec["region"].tolist() == [0, 0] and not rec["pad_"].any() and rec["motif"].tolist() == [0, 0]
    assert rec["phase_set"].tolist() == [7, 7] and rec["n_phase_sets"].tolist() == [1, 1]
    assert row_retained.tolist() == WORKED_ROW_RETAINED and tot == dict(n_part=8, n_retained=6)
    # the class of every read, by hand
    b = batch_of(WORKED)
    cls = lambda s, l, a: "".join(ref.classify(ref.read_structure(b, i), s, l, a) or "-" for i in range(9) if WORKED[i][2])
    assert cls(1050, 100, 10) == "SSSRROOR" and cls(1200, 60, 10) == "SSRSR-RS"      # read 6 ends at 1155: it does not reach intron B
    # anchor 50: A's retained rows are unchanged, B's all become OTHER (every read ends at 1300 < 1310)
    rec50, _, row50, tot50 = run_ref(WORKED, 2, 50)
    assert summary(rec50) == [(1050, 100, (3, 3, 2), (2, 0, 1, 3)), (1200, 60, (4, 0, 3), (1, 0, 3, 0))]
    assert row50.tolist() == [0, 0, 0, 1, 1, 0, 0, 0, 1] and tot50 == dict(n_part=8, n_retained=3)
    # min_count 1 keeps the junction of one read; min_count 0 is 1
    rec1, _, _, _ = run_ref(WORKED, 1, 10)
    assert [(s[0], s[1]) for s in summary(rec1)] == [(1050, 90), (1050, 100), (1200, 60)] and summary(rec1)[0][2] == (1, 4, 3)
    assert run_ref(WORKED, 0, 10)[0].tobytes() == rec1.tobytes()
    with pytest.raises(ValueError):
        run_ref(WORKED, 1, 4097)


def test_restatement_rules():
    # blocks: M = X D cover, I S H and zero-length ops change nothing, an N op of length >= 1 ends a block
    b = batch_of([(5, "2H3S10M2I5=0N5X0M10D4M7N0D6M3S", 1)])
    assert ref.read_structure(b, 0) == (1005, 1052, [(1039, 7)], [(1005, 1039), (1046, 1052)])
    # the anchor's two edges, one column each way
    base = [(0, "50M20N50M", 1), (0, "50M20N50M", 2)]
    at = lambda col, cig, a: summary(run_ref(base + [(col, cig, 1)], 2, a)[0])[0][2]
    assert at(40, "40M", 10) == (2, 1, 0) and at(41, "39M", 10) == (2, 0, 1)          # bs == s - a; one column short
    assert at(0, "80M", 10) == (2, 1, 0) and at(0, "79M", 10) == (2, 0, 1)            # be == e + a; one column short
    assert at(50, "20M", 0) == (2, 1, 0) and at(51, "19M", 0) == (2, 0, 1)            # a == 0: the block is the intron itself
    # s - a < 0 is covered by no row
    rec, _, row, _ = run_ref([(3, "2M5N20M", 1), (3, "2M5N20M", 2), (0, "30M", 1)], 2, 6, start0=0, length=100)
    assert summary(rec) == [(5, 5, (2, 0, 1), (1, 0, 1, 0))] and row.tolist() == [0, 0, 0]
    assert summary(run_ref([(3, "2M5N20M", 1), (3, "2M5N20M", 2), (0, "30M", 1)], 2, 5, start0=0, length=100)[0])[0][2] == (2, 1, 0)
    # OTHER's causes: another acceptor, another donor, a nested junction inside [s - a, e + a), a read ending inside the intron
    for cig in ("50M30N40M", "40M30N50M", "50M5D5N60M", "60M", "55M3N62M"):
        assert at(0, cig, 10) == (2, 0, 1), cig
    assert at(0, "30M15N75M", 10) == (2, 0, 1) and at(0, "30M15N75M", 5) == (2, 1, 0)   # an N op ending at 1045: inside [s - 10, ...), outside [s - 5, ...)
    assert at(0, "30M5N85M", 10) == (2, 1, 0)                                           # ... and one that ends in front of s - a
    # phase sets over SPLICED and RETAINED rows only: most rows, ties to the smallest value, 0 a value like any other
    reads = [(0, "50M20N50M", 1 + k % 2) for k in range(4)] + [(0, "120M", 1), (0, "120M", 2), (0, "60M", 1), (0, "60M", 1), (0, "60M", 1)]
    rec, _, _, _ = run_ref(reads, 2, 10, ps=[9, 9, 4, 4, 0, 0, 4, 4, 4])
    assert (int(rec["phase_set"][0]), int(rec["n_phase_sets"][0])) == (0, 3) and summary(rec)[0][2:] == ((4, 2, 3), (0, 1, 0, 1))
    rec, _, _, _ = run_ref(reads, 2, 10, ps=[9, 9, 4, 4, 4, 9, 2, 2, 2])
    assert (int(rec["phase_set"][0]), int(rec["n_phase_sets"][0])) == (4, 2) and summary(rec)[0][3] == (1, 1, 1, 0)
    # an intron held only by untagged reads is not kept; untagged reads count nowhere
    rec, _, row, tot = run_ref([(0, "50M20N50M", 0)] * 3 + [(0, "120M", 1)], 1, 10)
    assert rec.size == 0 and row.tolist() == [0] * 4 and tot == dict(n_part=1, n_retained=0)
    # the motif on the window's reference
    b = helpers.mk_batch([dict(pos=1000, seq="A" * 20, qual=30, cigar="10M6N10M", region=0)] * 2, [(1000, "A" * 10 + "gtCCag" + "A" * 10)])
    assert ref.intron_retention(b, [0, 2], [0, 1], [1, 2], [1, 1], 2, 0)[0]["motif"].tolist() == [1]


# ---- retention.format_tsv -----------------------------------------------------------------------------------------------------------
def test_format_tsv_worked_instance():
    rec, _, _, _ = run_ref(WORKED, 2, 10)
    text = retention.format_tsv([("chr7", rec, [1000], [400])], min_count=1)
    sor = lambda *cells: str(retention.sor(*cells))       # (asj's own function: its values are pinned in test_asj_host.py)
    rows = [ln.split("\t") for ln in text.splitlines()]
    assert rows[0] == ["#Intron", "Region", "Motif", "Spliced", "Retained", "Other", "Phase_set", "Hap1_spliced", "Hap1_retained", "Hap2_spliced",
                       "Hap2_retained", "PIR_h1", "PIR_h2", "P_value", "SOR"]
    assert rows[1][:13] == ["chr7:1051-1150", "chr7:1001-1400", ".", "3", "3", "2", "7", "2", "0", "1", "3", "0.0", "0.75"]
    assert rows[2][:13] == ["chr7:1201-1260", "chr7:1001-1400", ".", "4", "3", "0", "7", "1", "2", "3", "1", str(2 / 3), "0.25"]
    assert rows[1][14] == sor(2, 0, 1, 3) and rows[2][14] == sor(1, 2, 3, 1) and len(rows) == 3 and text.endswith("\n")
    assert all(0.0 < float(r[13]) <= 1.0 for r in rows[1:])
    # rows whose four cells sum to less than min_count, or whose retained cells to less than min_retained, are not written
    assert [ln.split("\t")[0] for ln in retention.format_tsv([("chr7", rec, [1000], [400])], min_count=7).splitlines()[1:]] == ["chr7:1201-1260"]
    rec50 = run_ref(WORKED, 2, 50)[0]
    assert [ln.split("\t")[0] for ln in retention.format_tsv([("chr7", rec50, [1000], [400])], 1, 1).splitlines()[1:]] == ["chr7:1051-1150"]
    assert len(retention.format_tsv([("chr7", rec50, [1000], [400])], 1, 0).splitlines()) == 3
    assert len(retention.format_tsv([("chr7", rec50, [1000], [400])], 1, 4).splitlines()) == 1
    assert retention.format_tsv([]) == text.splitlines()[0] + "\n"


def test_format_tsv_na_and_adjustment_over_the_written_rows():
    rec = np.zeros(4, dtype=_abi.RETAINED_INTRON_DTYPE)
    for k, (s, l, motif, cells, ps) in enumerate([(100, 50, 1, (20, 0, 0, 20), 0), (200, 40, 2, (1, 1, 1, 0), 3), (300, 30, 0, (5, 5, 5, 5), 8),
                                                  (400, 20, 1, (0, 0, 6, 6), 8)]):
        r = rec[k]
        r["region"], r["motif"], r["start0"], r["len"], r["phase_set"] = k % 2, motif, s, l, ps
        r["n_spliced"], r["n_retained"], r["n_other"] = cells[0] + cells[2] + 1, cells[1] + cells[3], 2
        for f, v in zip(CELLS, cells):
            r[f] = v
    rows = [ln.split("\t") for ln in retention.format_tsv([("c", rec, [50, 60], [500, 600])], min_count=10).splitlines()[1:]]
    assert [r[0] for r in rows] == ["c:101-150", "c:301-330", "c:401-420"] and [r[1] for r in rows] == ["c:51-550", "c:51-550", "c:61-660"]
    assert [r[2] for r in rows] == ["GT-AG", ".", "GT-AG"] and [r[6] for r in rows] == [".", "8", "8"] and [r[3] for r in rows] == ["21", "11", "7"]
    assert [(r[11], r[12]) for r in rows] == [("0.0", "1.0"), ("0.5", "0.5"), ("NA", "0.5")]             # a haplotype without a row: NA
    # Fisher's p of the complete separation is 2 / C(40, 20), above the G-test's; over the THREE written rows its adjusted value is three
    # times that (the unwritten row does not count); the balanced tables stay 1
    assert float(rows[0][13]) == pytest.approx(3.0 * 2.0 / math.comb(40, 20), rel=1e-9) and float(rows[1][13]) == 1.0 and float(rows[2][13]) == 1.0
    assert float(rows[0][14]) == pytest.approx(math.log(441.0 + 1.0 / 441.0), rel=1e-12)


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------
def test_pipeline_arguments():
    sig = inspect.signature(pipeline.run).parameters
    assert ((sig["retention_out"].default, sig["retention_min_count"].default, sig["retention_anchor"].default, sig["retention_min_retained"].default)
            == (None, 10, 10, 1))
    for kw in (dict(retention_anchor=4097), dict(retention_anchor=-1), dict(retention_min_count=-1), dict(retention_anchor=1.5),
               dict(retention_min_retained=-1), dict(retention_min_count=True)):
        with pytest.raises(ValueError):
            pipeline.run("no.bam", "no.fa", "no.vcf", retention_out="no.tsv", **kw)


def test_command_line_arguments():
    tool = os.path.join(ROOT, "tools", "run_pipeline.py")
    r = subprocess.run([sys.executable, tool, "-b", "x.bam", "-f", "x.fa", "-o", "x.vcf", "--retention-out", "x.tsv", "--retention-anchor", "5000"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--retention-anchor" in r.stderr
    h = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and all(f in h.stdout for f in ("--retention-out", "--retention-min-count", "--retention-anchor", "--retention-min-retained"))

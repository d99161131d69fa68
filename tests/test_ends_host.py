"""The host side of lcr_transcript_ends without a GPU: the records' layout against the header, the three symbols in the built library, the
contract's worked instance through its plain-Python restatement (tests/ends_ref.py) with hand-written expected values, the strand truth
table, ends.format_tsv, and the argument plumbing of pipeline.run and the command line."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ends_ref as ref
import helpers
from longcallr_amd import _abi, _lib, ends, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = ("h1_absent", "h1_present", "h2_absent", "h2_present")
PLUS, MINUS, NONE, PLUS_REV = (1, 0), (1, 1), (0, 0), (2, 1)     # (ts, rev): '+', '-', no tag on the forward strand, '+' as ts '-' on a reverse read


def test_struct_layout_matches_the_header(tmp_path):
    site_f = list(_abi.END_SITE_DTYPE.names)
    lst_f = ["n_regions", "n_sites", "n_rows", "n_part", "n_assigned", "site", "site_region_off", "row_site", "dev_site", "dev_row_site"]
    par_f = ["min_count", "window", "strand_mode", "pad_"]
    src = tmp_path / "ends.c"
    src.write_text('#include "lcr.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %d %d",sizeof(lcr_end_site),'
                   'sizeof(lcr_end_list),sizeof(lcr_end_params),LCR_ENDS_STRAND_TS,LCR_ENDS_STRAND_READ);'
                   + "".join('printf(" %%zu",offsetof(lcr_end_site,%s));' % f for f in site_f)
                   + "".join('printf(" %%zu",offsetof(lcr_end_list,%s));' % f for f in lst_f)
                   + "".join('printf(" %%zu",offsetof(lcr_end_params,%s));' % f for f in par_f) + 'printf("\\n");return 0;}')
    exe = tmp_path / "ends"
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = [int(x) for x in os.popen(str(exe)).read().split()]
    want = ([_abi.END_SITE_DTYPE.itemsize, C.sizeof(_abi.LcrEndList), C.sizeof(_abi.LcrEndParams), _abi.LCR_ENDS_STRAND_TS, _abi.LCR_ENDS_STRAND_READ]
            + [_abi.END_SITE_DTYPE.fields[f][1] for f in site_f] + [getattr(_abi.LcrEndList, f).offset for f in lst_f]
            + [getattr(_abi.LcrEndParams, f).offset for f in par_f])
    assert got == want and got[:5] == [64, 64, 16, 0, 1]
    assert site_f == ["region", "strand", "side", "kind", "pad_", "peak0", "min0", "max0", "n_reads", "n_h1", "n_h2", "n_peak", "phase_set",
                      "n_phase_sets", "h1_absent", "h1_present", "h2_absent", "h2_present"]
    # the header carries the contract above the declarations
    hdr = open(os.path.join(ROOT, "include", "lcr.h")).read()
    k = hdr.index("int lcr_transcript_ends(")
    for word in ("non-maximum suppression", "ties to the smallest value", "row_site", "Not here:", "strand_mode"):
        assert word in hdr[hdr.index("Allele-specific transcript ends (K16)"):k], word


def test_symbols_resolve():
    lib = _lib.load()                    # (no GPU is touched by loading it)
    for name in ("lcr_transcript_ends", "lcr_get_transcript_ends", "lcr_transcript_ends_ms"):
        assert getattr(lib, name) is not None
    # before lcr_phase nothing changes: a NULL context is an argument error, not a crash
    assert lib.lcr_transcript_ends(None, None) == -1 and lib.lcr_get_transcript_ends(None, None) == -1


def test_strand_truth_table():
    fl = lambda ts, rev: (ts << 1) | rev
    #                          (rev, ts): "ts" mode, "read" mode      1 = '+', 2 = '-', 0 = none
    table = {(0, 0): (0, 1), (1, 0): (0, 2), (0, 1): (1, 1), (1, 1): (2, 2), (0, 2): (2, 2), (1, 2): (1, 1)}
    for (rev, ts), (want_ts, want_read) in table.items():
        assert ref.strand(fl(ts, rev), "ts") == want_ts and ref.strand(fl(ts, rev), "read") == want_read, (rev, ts)


# ---- the worked instance of the contract: W = 2, min_count = 2 ---------------------------------------------------------------------------
#          column  CIGAR        class  (ts, rev)      left  right
WORKED = [(0, "60M", 1, PLUS),            # 1000  1059
          (0, "60M", 2, PLUS),            # 1000  1059
          (0, "120M", 1, PLUS),           # 1000  1119   reads through the 3' site at 1059
          (0, "60M", 1, NONE),            # no ts tag: takes part in "read" mode only
          (0, "60M", 0, PLUS),            # unassigned: never takes part
          (1, "59M", 1, PLUS),            # 1001  1059
          (2, "118M", 2, PLUS),           # 1002  1119
          (3, "20M30N10M", 2, PLUS),      # 1003  1062   its left end is a shoulder of a shoulder, its right end a site of one read
          (4, "56M", 1, MINUS),           # 1004  1059   the same right coordinate in another class
          (4, "56M", 2, MINUS),
          (5, "55M", 1, PLUS_REV)]        # 1005  1059   '+' from ts '-' on a reverse read; its left end is unassigned too
#               p  strand side kind  spread      n_reads n_h1 n_h2 n_peak  cells
WORKED_WANT = [(1000, 1, 0, 0, (1000, 1002), (5, 3, 2, 3), (0, 3, 0, 2)),      # TSS of '+'
               (1004, 2, 0, 1, (1004, 1004), (2, 1, 1, 2), (0, 1, 0, 1)),      # TES of '-'
               (1059, 1, 1, 1, (1059, 1059), (4, 3, 1, 4), (1, 3, 2, 1)),      # TES of '+': three reads cover its window
               (1059, 2, 1, 0, (1059, 1059), (2, 1, 1, 2), (0, 1, 0, 1)),      # TSS of '-'
               (1119, 1, 1, 1, (1119, 1119), (2, 1, 1, 2), (0, 1, 0, 1))]
WORKED_ROW_SITE = [[0, 2], [0, 2], [0, 4], [-1, -1], [-1, -1], [0, 2], [0, 4], [-1, -1], [1, 3], [1, 3], [-1, 2]]


def seq_len(cigar):
    return sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MIS=X")


def batch_of(reads, start0=1000, length=300):
    """reads: [(column, CIGAR, class, (ts, rev))] of one region"""
    return helpers.mk_batch([dict(pos=start0 + col, seq="A" * seq_len(c), qual=30, cigar=c, ts=sr[0], rev=sr[1], region=0) for col, c, _, sr in reads],
                            [(start0, "A" * length)])


def run_ref(reads, min_count, window, mode="ts", ps=None):
    n = len(reads)
    return ref.transcript_ends(batch_of(reads), [0, n], list(range(n)), [r[2] for r in reads], [7] * n if ps is None else ps, min_count, window, mode)


def summary(rec):
    return [(int(r["peak0"]), int(r["strand"]), int(r["side"]), int(r["kind"]), (int(r["min0"]), int(r["max0"])),
             (int(r["n_reads"]), int(r["n_h1"]), int(r["n_h2"]), int(r["n_peak"])), tuple(int(r[f]) for f in CELLS)) for r in rec]


def test_worked_instance():
    rec, off, row_site, tot = run_ref(WORKED, 2, 2)
    assert rec.dtype == _abi.END_SITE_DTYPE and summary(rec) == WORKED_WANT
    assert off.tolist() == [0, 5] and rec["region"].tolist() == [0] * 5 and not rec["pad_"].any()
    assert rec["phase_set"].tolist() == [7] * 5 and rec["n_phase_sets"].tolist() == [1] * 5
    assert row_site.tolist() == WORKED_ROW_SITE and tot == dict(n_part=9, n_assigned=15)
    # min_count 1 adds the site of one read at 1062; its window [1060, 1064] is covered by the two long reads
    rec1, off1, row1, tot1 = run_ref(WORKED, 1, 2)
    assert [s[0] for s in summary(rec1)] == [1000, 1004, 1059, 1059, 1062, 1119] and summary(rec1)[4][5:] == ((1, 0, 1, 1), (1, 0, 1, 1))
    assert row1[7].tolist() == [-1, 4] and tot1 == dict(n_part=9, n_assigned=16)       # the two shoulders of shoulders stay unassigned
    assert run_ref(WORKED, 0, 2)[0].tobytes() == rec1.tobytes()                        # min_count 0 is 1
    # "read" mode: the untagged forward read is a '+' read
    rec2, _, row2, tot2 = run_ref(WORKED, 2, 2, "read")
    assert tot2 == dict(n_part=10, n_assigned=17) and row2[3].tolist() == [0, 2]
    assert summary(rec2)[0][5] == (6, 4, 2, 4) and summary(rec2)[2][5] == (5, 4, 1, 5)
    # W = 0: every distinct coordinate of a class is a peak
    rec3, _, _, _ = run_ref(WORKED, 1, 0)
    assert [(s[0], s[1], s[2]) for s in summary(rec3)] == [(1000, 1, 0), (1001, 1, 0), (1002, 1, 0), (1003, 1, 0), (1004, 2, 0), (1005, 1, 0),
                                                           (1059, 1, 1), (1059, 2, 1), (1062, 1, 1), (1119, 1, 1)]
    with pytest.raises(ValueError):
        run_ref(WORKED, 1, 4097)


def test_restatement_rules():
    # the peak rule: equal counts W apart give one peak (the smaller), W + 1 apart two
    two = lambda gap: [(0, "50M", 1 + k % 2, PLUS) for k in range(3)] + [(gap, "%dM" % (90 - gap), 1 + k % 2, PLUS) for k in range(3)]
    rec, _, row_site, _ = run_ref(two(4), 1, 4)
    assert [(s[0], s[2], s[5][0]) for s in summary(rec)] == [(1000, 0, 6), (1049, 1, 3), (1089, 1, 3)] and (row_site[:, 0] == 0).all()
    rec, _, _, _ = run_ref(two(5), 1, 4)
    assert [(s[0], s[5][0]) for s in summary(rec) if s[2] == 0] == [(1000, 3), (1005, 3)]
    # (3, 5, 7) at x, x + W, x + 2 W: only the last is a peak, the middle one's ends are assigned to it, x's are unassigned
    reads = [(0, "90M", 1, PLUS)] * 3 + [(4, "86M", 2, PLUS)] * 5 + [(8, "82M", 1, PLUS)] * 7
    rec, _, row_site, tot = run_ref(reads, 1, 4)
    left = [s for s in summary(rec) if s[2] == 0]
    assert [(s[0], s[4], s[5]) for s in left] == [(1008, (1004, 1008), (12, 7, 5, 7))] and row_site[:3, 0].tolist() == [-1] * 3
    assert tot == dict(n_part=15, n_assigned=12 + 15)
    # an end exactly between two peaks goes to the smaller one
    reads = [(0, "90M", 1, PLUS)] * 2 + [(3, "87M", 2, PLUS)] + [(6, "84M", 1, PLUS)] * 2
    rec, _, row_site, _ = run_ref(reads, 1, 3)
    assert [(s[0], s[5][0]) for s in summary(rec) if s[2] == 0] == [(1000, 3), (1006, 2)] and row_site[2, 0] == 0
    # phase sets: the most rows win, a tie goes to the smaller value, 0 is a value like any other
    reads = [(0, "60M", 1 + k % 2, PLUS) for k in range(6)]
    rec, _, _, _ = run_ref(reads, 1, 2, ps=[9, 9, 0, 0, 4, 4])
    assert (int(rec["phase_set"][0]), int(rec["n_phase_sets"][0]), int(rec["n_reads"][0])) == (0, 3, 6) and summary(rec)[0][6] == (0, 1, 0, 1)
    rec, _, _, _ = run_ref(reads, 1, 2, ps=[9, 9, 3, 4, 4, 4])
    assert (int(rec["phase_set"][0]), int(rec["n_phase_sets"][0])) == (4, 3) and summary(rec)[0][6] == (0, 1, 0, 2)
    # a window reaching below column 0 is covered by no row; clips and insertions do not move an end
    b = helpers.mk_batch([dict(pos=0, seq="A" * 60, qual=30, cigar="3S50M2I3M2S", ts=1, region=0), dict(pos=1, seq="A" * 50, qual=30, cigar="50M", ts=1, region=0),
                          dict(pos=1, seq="A" * 50, qual=30, cigar="50M", ts=1, region=0)], [(0, "A" * 100)])
    rec, _, row_site, _ = ref.transcript_ends(b, [0, 3], [0, 1, 2], [1, 1, 2], [1, 1, 1], 2, 2)
    assert summary(rec) == [(1, 1, 0, 0, (0, 1), (3, 2, 1, 2), (0, 2, 0, 1)), (50, 1, 1, 1, (50, 52), (3, 2, 1, 2), (0, 2, 0, 1))]


# ---- ends.format_tsv -------------------------------------------------------------------------------------------------------------------
def test_format_tsv_worked_instance():
    rec, _, _, _ = run_ref(WORKED, 2, 2)
    text = ends.format_tsv([("chr7", rec, [1000], [300])], min_count=1)
    sor = lambda *cells: str(ends.sor(*cells))       # (asj's own function: its values are pinned in test_asj_host.py)
    assert text == (
        "#Site\tKind\tStrand\tRegion\tSpread\tReads\tPeak_reads\tH1_reads\tH2_reads\tPhase_set\tHap1_absent\tHap1_present\tHap2_absent\tHap2_present\tP_value\tSOR\n"
        "chr7:1001\tTSS\t+\tchr7:1001-1300\t1001-1003\t5\t3\t3\t2\t7\t0\t3\t0\t2\t1.0\t" + sor(0, 3, 0, 2) + "\n"
        "chr7:1005\tTES\t-\tchr7:1001-1300\t1005-1005\t2\t2\t1\t1\t7\t0\t1\t0\t1\t1.0\t" + sor(0, 1, 0, 1) + "\n"
        "chr7:1060\tTES\t+\tchr7:1001-1300\t1060-1060\t4\t4\t3\t1\t7\t1\t3\t2\t1\t1.0\t" + sor(1, 3, 2, 1) + "\n"
        "chr7:1060\tTSS\t-\tchr7:1001-1300\t1060-1060\t2\t2\t1\t1\t7\t0\t1\t0\t1\t1.0\t" + sor(0, 1, 0, 1) + "\n"
        "chr7:1120\tTES\t+\tchr7:1001-1300\t1120-1120\t2\t2\t1\t1\t7\t0\t1\t0\t1\t1.0\t" + sor(0, 1, 0, 1) + "\n")
    # rows whose four cells sum to less than min_count are not written
    assert [ln.split("\t")[0] for ln in ends.format_tsv([("chr7", rec, [1000], [300])], min_count=5).splitlines()[1:]] == ["chr7:1001", "chr7:1060"]
    assert ends.format_tsv([]) == text.splitlines()[0] + "\n"


def test_format_tsv_adjusts_over_the_written_rows_only():
    rec = np.zeros(3, dtype=_abi.END_SITE_DTYPE)
    for k, (p, strand, side, cells, ps) in enumerate([(100, 1, 0, (20, 0, 0, 20), 0), (200, 2, 0, (1, 1, 1, 0), 3), (300, 2, 1, (5, 5, 5, 5), 8)]):
        r = rec[k]
        r["region"], r["strand"], r["side"], r["kind"], r["peak0"], r["min0"], r["max0"], r["phase_set"] = k % 2, strand, side, int((strand == 1) != (side == 0)), p, p - 1, p + 2, ps
        r["n_reads"], r["n_h1"], r["n_h2"], r["n_peak"] = sum(cells), cells[0] + cells[1], cells[2] + cells[3], 1
        for f, v in zip(CELLS, cells):
            r[f] = v
    rows = [ln.split("\t") for ln in ends.format_tsv([("c", rec, [50, 60], [500, 600])], min_count=10).splitlines()[1:]]
    assert [r[0] for r in rows] == ["c:101", "c:301"] and [r[1] for r in rows] == ["TSS", "TSS"] and [r[2] for r in rows] == ["+", "-"]
    assert [r[3] for r in rows] == ["c:51-550", "c:51-550"] and [r[4] for r in rows] == ["100-103", "300-303"] and [r[9] for r in rows] == [".", "8"]
    # Fisher's p of the complete separation is 2 / C(40, 20), above the G-test's; over the TWO written rows its adjusted value is twice
    # that (three rows would make it three times that); the balanced table stays 1
    assert float(rows[0][14]) == pytest.approx(2.0 * 2.0 / math.comb(40, 20), rel=1e-9) and float(rows[1][14]) == 1.0
    assert float(rows[0][15]) == pytest.approx(math.log(441.0 + 1.0 / 441.0), rel=1e-12)


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------
def test_pipeline_arguments():
    sig = inspect.signature(pipeline.run).parameters
    assert (sig["ends_out"].default, sig["ends_min_count"].default, sig["ends_window"].default, sig["ends_strand"].default) == (None, 10, 10, "ts")
    for kw in (dict(ends_window=4097), dict(ends_min_count=-1), dict(ends_window=1.5), dict(ends_strand="both")):
        with pytest.raises(ValueError):
            pipeline.run("no.bam", "no.fa", "no.vcf", ends_out="no.tsv", **kw)


def test_command_line_arguments():
    tool = os.path.join(ROOT, "tools", "run_pipeline.py")
    r = subprocess.run([sys.executable, tool, "-b", "x.bam", "-f", "x.fa", "-o", "x.vcf", "--ends-out", "x.tsv", "--ends-window", "5000"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--ends-window" in r.stderr
    h = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and all(f in h.stdout for f in ("--ends-out", "--ends-min-count", "--ends-window", "--ends-strand"))

"""The host side of lcr_hap_coverage without a GPU: the records' layout against the header, the contract's worked instance through its
plain-Python restatement (tests/hap_coverage_ref.py), coverage.format_bedgraph / coverage.expand / the track writer on hand-made and
random segments, and the argument plumbing of pipeline.run and the command line."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import hap_coverage_ref as ref
from longcallr_amd import _abi, coverage, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, I, D, N, S, H, P, EQ, X = range(9)


def test_struct_layout_matches_the_header(tmp_path):
    seg_f, reg_f = ["region", "len", "start0", "n", "pad_"], ["region", "n_reads", "max_depth", "pad_", "bases"]
    lst_f = ["n_regions", "n_segments", "seg", "seg_region_off", "reg", "dev_seg", "dev_reg"]
    src = tmp_path / "hc.c"
    src.write_text('#include "lcr.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu",sizeof(lcr_hap_cov_segment),'
                   'sizeof(lcr_hap_cov_region),sizeof(lcr_hap_cov_list));'
                   + "".join('printf(" %%zu",offsetof(lcr_hap_cov_segment,%s));' % f for f in seg_f)
                   + "".join('printf(" %%zu",offsetof(lcr_hap_cov_region,%s));' % f for f in reg_f)
                   + "".join('printf(" %%zu",offsetof(lcr_hap_cov_list,%s));' % f for f in lst_f) + 'printf("\\n");return 0;}')
    exe = tmp_path / "hc"
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = [int(x) for x in os.popen(str(exe)).read().split()]
    want = ([_abi.HAP_COV_SEGMENT_DTYPE.itemsize, _abi.HAP_COV_REGION_DTYPE.itemsize, C.sizeof(_abi.LcrHapCovList)]
            + [_abi.HAP_COV_SEGMENT_DTYPE.fields[f][1] for f in seg_f] + [_abi.HAP_COV_REGION_DTYPE.fields[f][1] for f in reg_f]
            + [getattr(_abi.LcrHapCovList, f).offset for f in lst_f])
    assert got == want and got[:2] == [32, 56]
    assert _abi.HAP_COV_SEGMENT_DTYPE.fields["n"][0].shape == (3,) and _abi.HAP_COV_REGION_DTYPE.fields["bases"][0].base == np.dtype("<u8")


# ---- the worked instance of the contract ------------------------------------------------------------------------------------------------
WORKED_READS = [(1000, [(10, M)]), (1005, [(5, M), (10, N), (5, M)]), (1008, [(4, M), (2, D), (4, M)]), (1020, [(3, S), (5, M), (2, I), (5, M)])]
WORKED_CLS = [1, 2, 0, 1]
WORKED_SEGS = [(1000, 1005, (0, 1, 0)), (1005, 1008, (0, 1, 1)), (1008, 1010, (1, 1, 1)), (1010, 1018, (1, 0, 0)),
               (1020, 1025, (0, 1, 1)), (1025, 1030, (0, 1, 0))]


def test_worked_instance():
    d, nr = ref.dense(1000, 40, WORKED_READS, WORKED_CLS)
    assert [(s, s + ln, t) for _, ln, s, t in ref.encode(0, 1000, d)] == WORKED_SEGS
    assert [int(d[k].sum()) for k in range(3)] == [10, 20, 10] and [int(d[k].max()) for k in range(3)] == [1, 1, 1] and nr == [1, 2, 1]


def test_restatement_arms():
    # = X D cover, N does not; I S H P and zero-length ops change nothing; clipping on both sides; a block wholly outside
    assert ref.blocks(10, [(2, H), (3, S), (4, EQ), (0, N), (1, X), (2, I), (0, D), (3, D), (5, N), (0, M), (2, P), (2, M)]) == [(10, 14), (14, 15), (15, 18), (23, 25)]
    d, nr = ref.dense(100, 10, [(95, [(7, M), (1, N), (5, M)]), (50, [(10, M)]), (120, [(3, M)])], [1, 2, 0])
    assert d[1].tolist() == [1, 1, 0, 1, 1, 1, 1, 1, 0, 0] and not d[2].any() and not d[0].any() and nr == [1, 1, 1]
    assert ref.encode(3, 100, d) == [(3, 2, 100, (0, 1, 0)), (3, 5, 103, (0, 1, 0))]
    assert ref.encode(0, 0, np.zeros((3, 0), np.uint64)) == [] and ref.encode(0, 0, np.zeros((3, 5), np.uint64)) == []
    # classes: a row's assignment where it is 1 or 2; reads that are no row and rows with assignment 0 are class 0
    assert ref.classes(5, [0, 3, 5], [0, 2, 3], [0, 1, 3], [2, 0, 1]).tolist() == [2, 0, 0, 1, 0]


def segs_of(rows):
    out = np.zeros(len(rows), dtype=_abi.HAP_COV_SEGMENT_DTYPE)
    for j, (s, e, t) in enumerate(rows):
        out["start0"][j], out["len"][j], out["n"][j] = s, e - s, t
    return out


# ---- coverage.format_bedgraph, coverage.expand, the writer --------------------------------------------------------------------------------
def test_format_bedgraph_exact_text():
    segs = segs_of(WORKED_SEGS)
    assert coverage.format_bedgraph("chr7", segs, 1) == "chr7\t1000\t1010\t1\nchr7\t1020\t1030\t1\n"     # merged across unchanged class 1
    assert coverage.format_bedgraph("chr7", segs, 2) == "chr7\t1005\t1010\t1\nchr7\t1020\t1025\t1\n"     # zeros skipped
    assert coverage.format_bedgraph("chr7", segs, 0) == "chr7\t1008\t1018\t1\n"
    # a value change splits, a gap splits, equal values that abut merge; values beyond 16 bits print in full
    segs = segs_of([(0, 5, (0, 3, 0)), (5, 9, (1, 3, 0)), (9, 12, (1, 70000, 0)), (12, 13, (0, 0, 4)), (14, 20, (0, 70000, 4))])
    assert coverage.format_bedgraph("c", segs, 1) == "c\t0\t9\t3\nc\t9\t12\t70000\nc\t14\t20\t70000\n"
    assert coverage.format_bedgraph("c", segs, 2) == "c\t12\t13\t4\nc\t14\t20\t4\n"
    assert coverage.format_bedgraph("c", segs[:0], 1) == "" and coverage.format_bedgraph("c", segs[:1], 0) == ""


def test_expand_inverts_the_restatement():
    rng = np.random.default_rng(5)
    for trial in range(20):
        length = int(rng.integers(1, 300))
        start0 = int(rng.integers(0, 1 << 33))
        reads = []
        for _ in range(int(rng.integers(0, 12))):
            ops = [(int(rng.integers(0, 40)), int(rng.choice([M, I, D, N, S, EQ, X]))) for _ in range(int(rng.integers(1, 8)))]
            reads.append((start0 + int(rng.integers(-30, length + 10)), ops))
        cls = rng.integers(0, 3, len(reads)).tolist()
        d, _ = ref.dense(start0, length, reads, cls)
        rows = ref.encode(0, start0, d)
        back = coverage.expand(segs_of([(s, s + ln, t) for _, ln, s, t in rows]), start0, length)
        assert back.dtype == np.uint32 and back.shape == (3, length) and (back == d).all()
        for k in range(3):      # a track's lines add up to the class's bases
            total = sum((int(e) - int(s)) * int(v) for _, s, e, v in (l.split("\t") for l in coverage.format_bedgraph("c", segs_of([(s, s + ln, t) for _, ln, s, t in rows]), k).splitlines()))
            assert total == int(d[k].sum())
    with pytest.raises(ValueError):
        coverage.expand(segs_of([(5, 12, (1, 0, 0))]), 0, 10)


def test_track_writer_checks_the_order(tmp_path):
    w = coverage.TrackWriter(str(tmp_path / "t"))
    w.add_contig("chr1", segs_of(WORKED_SEGS))
    w.add_contig("chr2", segs_of([(5, 9, (2, 0, 0))]))
    w.close()
    assert (tmp_path / "t.h1.bedgraph").read_text() == "chr1\t1000\t1010\t1\nchr1\t1020\t1030\t1\n"
    assert (tmp_path / "t.h2.bedgraph").read_text() == "chr1\t1005\t1010\t1\nchr1\t1020\t1025\t1\n"
    assert (tmp_path / "t.unassigned.bedgraph").read_text() == "chr1\t1008\t1018\t1\nchr2\t5\t9\t2\n"
    assert w.bases == [18, 20, 10] and w.segments == 7
    for bad in ([(10, 20, (1, 0, 0)), (5, 8, (1, 0, 0))], [(10, 20, (1, 0, 0)), (15, 30, (2, 0, 0))]):       # out of order; overlapping
        w = coverage.TrackWriter(str(tmp_path / "bad"))
        with pytest.raises(ValueError):
            w.add_contig("chr1", segs_of(bad))
        w.close()


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def test_run_takes_the_prefix_and_refuses_a_bad_one(tmp_path):
    assert inspect.signature(pipeline.run).parameters["hap_coverage_out"].default is None
    for bad in ("", str(tmp_path / "missing_dir" / "cov"), str(tmp_path) + os.sep):
        with pytest.raises(ValueError, match="hap_coverage_out"):
            pipeline.run(str(tmp_path / "no.bam"), str(tmp_path / "no.fa"), str(tmp_path / "out.vcf"), hap_coverage_out=bad)
    with pytest.raises(FileNotFoundError):      # a good prefix gets as far as every run: to the missing .fai
        pipeline.run(str(tmp_path / "no.bam"), str(tmp_path / "no.fa"), str(tmp_path / "out.vcf"), hap_coverage_out=str(tmp_path / "cov"))
    assert not list(tmp_path.iterdir())


def test_command_line_option(tmp_path):
    tool = os.path.join(ROOT, "tools", "run_pipeline.py")
    cmd = [sys.executable, tool, "-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"), "-o", str(tmp_path / "out.vcf"),
           "--hap-coverage-out", str(tmp_path / "missing_dir" / "cov")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 2 and "--hap-coverage-out" in p.stderr and not (tmp_path / "out.vcf").exists()
    p = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "--hap-coverage-out PREFIX" in p.stdout

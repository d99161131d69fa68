"""Allele-specific junctions without a GPU: the host arithmetic of longcallr_amd/asj.py, the plain-Python restatement of the
lcr_junctions contract (tests/asj_ref.py) on a hand-worked instance, and the layout of the new ABI structs."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import asj_ref
import helpers
from longcallr_amd import _abi, asj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fisher_two_sided():
    assert asj.fisher_two_sided([[3, 0], [0, 3]]) == pytest.approx(0.1, abs=1e-12)
    assert asj.fisher_two_sided([[2, 0], [0, 2]]) == pytest.approx(1.0 / 3.0, abs=1e-12)
    assert asj.fisher_two_sided([[1, 1], [1, 1]]) == pytest.approx(1.0, abs=1e-12)
    assert asj.fisher_two_sided([[20, 0], [0, 20]]) == pytest.approx(2.0 / math.comb(40, 20), rel=1e-9)


def test_sor_g_test_bh():
    assert asj.sor(5, 5, 5, 5) == pytest.approx(math.log(2.0), abs=1e-15)
    assert asj.sor(3, 7, 3, 7) == pytest.approx(math.log(2.0), abs=1e-15)
    g, p = asj.g_test([[5, 5], [5, 5]])
    assert abs(p - 1.0) < 1e-6
    g, p = asj.g_test([[20, 0], [0, 20]])
    assert g > 50 and 0.0 <= p < 1e-10
    assert asj.bh_adjust([0.01, 0.04, 0.03, 0.005]).tolist() == pytest.approx([0.02, 0.04, 0.04, 0.02], abs=1e-12)
    assert asj.bh_adjust([]).size == 0
    assert asj.bh_adjust([0.9, 0.8]).tolist() == pytest.approx([0.9, 0.9], abs=1e-12)   # (monotone from the largest down, capped at 1)


def _junc(rows):
    a = np.zeros(len(rows), dtype=_abi.JUNC_DTYPE)
    for i, (g, s, l) in enumerate(rows):
        a["region"][i], a["start0"][i], a["len"][i] = g, s, l
    return a


def test_cluster_components():
    # A and B share a start, B and C share an end, D stands alone; E has A's start in ANOTHER region
    a = _junc([(0, 100, 50), (0, 100, 80), (0, 130, 50), (0, 300, 20), (1, 100, 50)])
    comp = asj.cluster(a)
    assert comp.tolist() == [0, 0, 0, 3, 4]
    assert len(set(comp[:4].tolist())) == 2


def six_read_batch():
    """One region at 100 with 300 columns, six reads (all rows), min_count = 2, min_junctions = 0.

      read  pos  CIGAR              junctions (s, l)        rend  assignment  ps
      r0    100  20M30N20M40N20M    (120, 30) (170, 40)     230   1           101
      r1    100  20M30N20M40N20M    (120, 30) (170, 40)     230   1           101
      r2    100  20M90N20M          (120, 90)               230   2           101
      r3    105  15M90N10M          (120, 90)               220   2           101
      r4    150  20M40N5M           (170, 40)               215   2           0
      r5    100  20M30N20M40N20M    (120, 30) (170, 40)     230   0           0      takes no part

    n_reads: (120, 30) = 2, (120, 90) = 2, (170, 40) = 3 (r0, r1, r4): all kept, in this order.
    (120, 30): overlap needs pos < 150 and rend > 120: r0, r1 present; r2, r3 absent; r4 starts AT 150: no overlap.
               one phase set, 101: h1_present 2, h2_absent 2.
    (120, 90): pos < 210 and rend > 120: r0, r1 absent (hap 1); r2, r3 present (hap 2); r4 absent (hap 2, ps 0).
               ps 101 has 4 rows, ps 0 has 1: phase set 101 of 2, h1_absent 2, h2_present 2 -- r4 is not counted.
    (170, 40): pos < 210 and rend > 170: r0, r1 present; r2, r3 absent; r4 present under ps 0.
               phase set 101 of 2: h1_present 2, h2_absent 2.
    motifs: window columns 20-21 "GT", 48-49 "AG", 70-71 "ct", 108-109 "ac":
               (120, 30) GT..AG = 1, (120, 90) GT..AC = 0, (170, 40) ct..ac = 2."""
    ref = ["A"] * 300
    ref[20:22] = "GT"; ref[48:50] = "AG"; ref[70:72] = "ct"; ref[108:110] = "ac"
    cig = ["20M30N20M40N20M", "20M30N20M40N20M", "20M90N20M", "15M90N10M", "20M40N5M", "20M30N20M40N20M"]
    pos = [100, 100, 100, 105, 150, 100]
    reads = [dict(pos=p, cigar=c, seq="A" * n, region=0) for p, c, n in zip(pos, cig, [60, 60, 40, 25, 25, 60])]
    order = sorted(range(6), key=lambda i: pos[i])
    b = helpers.mk_batch([reads[i] for i in order], [(100, "".join(ref))])
    asg = np.array([[1, 1, 2, 2, 2, 0][i] for i in order], np.uint8)
    ps = np.array([[101, 101, 101, 101, 0, 0][i] for i in order], np.uint32)
    return b, asg, ps


def test_restatement_on_six_reads():
    b, asg, ps = six_read_batch()
    rro, rread = np.array([0, 6], np.int32), np.arange(6, dtype=np.int32)
    rec, off = asj_ref.junctions(b, rro, rread, asg, ps, min_count=2, min_junctions=0)
    assert off.tolist() == [0, 3]
    got = [tuple(int(rec[f][i]) for f in ("region", "motif", "start0", "len", "n_reads", "phase_set", "n_phase_sets",
                                          "h1_absent", "h1_present", "h2_absent", "h2_present")) for i in range(3)]
    assert got == [(0, 1, 120, 30, 2, 101, 1, 0, 2, 2, 0),
                   (0, 0, 120, 90, 2, 101, 2, 2, 0, 0, 2),
                   (0, 2, 170, 40, 3, 101, 2, 0, 2, 2, 0)]
    # min_junctions = 1 leaves r0 / r1 only (r5 is unassigned): the two junctions they share, no row absent
    rec, off = asj_ref.junctions(b, rro, rread, asg, ps, min_count=2, min_junctions=1)
    assert [(int(r["start0"]), int(r["len"]), int(r["h1_present"]), int(r["h2_absent"])) for r in rec] == [(120, 30, 2, 0), (170, 40, 2, 0)]
    # min_count = 3 keeps (170, 40) alone
    rec, off = asj_ref.junctions(b, rro, rread, asg, ps, min_count=3, min_junctions=0)
    assert [(int(r["start0"]), int(r["len"])) for r in rec] == [(170, 40)]
    # the TSV of the first table: three junctions of one cluster ((120, 30) - (120, 90) share the start, (120, 90) - (170, 40) the end)
    rec, off = asj_ref.junctions(b, rro, rread, asg, ps, min_count=2, min_junctions=0)
    text = asj.format_tsv([("chrT", rec, b.start0, b.len)], min_count=2).split("\n")
    assert text[0] == asj.HEADER and len(text) == 5 and text[4] == ""
    f = text[2].split("\t")
    assert f[:8] == ["chrT:121-210", ".", "chrT:121-150", "101", "2", "0", "0", "2"] and f[10:] == [".", "False", "chrT:101-400"]
    p = [max(asj.fisher_two_sided(t), asj.g_test(t)[1]) for t in ([[0, 2], [2, 0]], [[2, 0], [0, 2]], [[0, 2], [2, 0]])]
    assert float(f[8]) == asj.bh_adjust(p)[1] and float(f[9]) == asj.sor(2, 0, 0, 2)
    assert text[1].split("\t")[11] == "True" and text[3].split("\t")[11] == "True"


def test_junction_struct_layouts_match_the_header(tmp_path):
    fields = [n for n in _abi.JUNC_DTYPE.names]
    lfields = [n for n, _ in _abi.LcrJunctionList._fields_]
    lines = ['#include "lcr.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(){",
             'printf("%zu %zu %zu\\n", sizeof(lcr_junction), sizeof(lcr_junction_list), sizeof(lcr_junction_params));']
    lines += ['printf("%%zu\\n", offsetof(lcr_junction, %s));' % f for f in fields]
    lines += ['printf("%%zu\\n", offsetof(lcr_junction_list, %s));' % f for f in lfields]
    lines += ['printf("%zu %zu\\n", offsetof(lcr_junction_params, min_count), offsetof(lcr_junction_params, min_junctions));', "return 0;}"]
    src, exe = tmp_path / "jsz.c", tmp_path / "jsz"
    src.write_text("\n".join(lines))
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = [int(x) for x in os.popen(str(exe)).read().split()]
    want = [48, C.sizeof(_abi.LcrJunctionList), C.sizeof(_abi.LcrJunctionParams)]
    want += [_abi.JUNC_DTYPE.fields[f][1] for f in fields]
    want += [getattr(_abi.LcrJunctionList, f).offset for f in lfields]
    want += [_abi.LcrJunctionParams.min_count.offset, _abi.LcrJunctionParams.min_junctions.offset]
    assert got == want and _abi.JUNC_DTYPE.itemsize == 48

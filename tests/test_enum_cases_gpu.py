"""The recipes of tests/enum_cases.py in front of the enumeration kernels: every case through test_gpu_parity.full_check (planes, candidates,
fragment matrix, sigma / delta / eta, the exact fixed-point objective, the VCF text, the F64-mode check; no bar of its own) in each form
the phase stage has for an enumeration region.  tests/test_enum_cases.py shows on the CPU that each case meets the limit it names.

  default   the class the region's size gives it.  A profiled run (LCR_PHASE_PROF=1): the library's report of its classes must be what
            enum_cases.predicted_class says -- a wrong restatement of the layouts fails here
  stream    LCR_ENUM_FORCE_STREAM=1: k4_enum_reg for every region whose streaming image fits
  big       LCR_ENUM_FORCE_BIG=1: k4_enum_big and k4_enum_resolve_big meet the same ties
and, on the tie cases, step elision off against on, the tie census (nothing unresolved, one census from k4_enum_bits and k4_enum_reg, the
oracle's counts), tie_arith = 2 against the oracle with its classes, and each region of the mixed batch alone against itself in the batch."""
import collections
import re

import numpy as np
import pytest

import enum_cases as ec
import test_gpu_parity as par
from longcallr_amd import _abi
from test_enum_step_elision_gpu import _run

pytestmark = pytest.mark.gpu

TIE_CASES = [n for n in ec.NAMES if n.startswith(("tq_", "tcap_", "redo_"))]
CLASS_LINE = re.compile(r"enumeration classes: bit states (\d+) regions / \d+ tiles, streaming (\d+) / \d+, global (\d+) / \d+")


def check(engine_cls, orc, name, **more):
    try:
        return par.full_check(engine_cls, orc, ec.batch(name), ec.params(name, **more))
    except AssertionError as e:
        raise AssertionError("%s: %s" % (name, e)) from e


def profiled_check(engine_cls, orc, monkeypatch, capfd, name, want):
    """full_check under LCR_PHASE_PROF=1; the one phase call's class report must count `want`'s classes"""
    monkeypatch.setenv("LCR_PHASE_PROF", "1")
    capfd.readouterr()
    check(engine_cls, orc, name)
    got = [tuple(int(x) for x in m) for m in CLASS_LINE.findall(capfd.readouterr().err)]
    n = collections.Counter(want)
    assert got == [(n["bits"], n["stream"], n["big"])], "%s: classes (bit states, streaming, global) %s, predicted %s" % (name, got, want)


@pytest.mark.parametrize("name", ec.NAMES)
def test_default_form_takes_the_predicted_class(engine_cls, orc, monkeypatch, capfd, name):
    profiled_check(engine_cls, orc, monkeypatch, capfd, name, ec.classes(name))
    if name == "class_mixed":
        assert collections.Counter(ec.classes(name)) == dict(bits=2, stream=1, big=1)


@pytest.mark.parametrize("name", [n for n in ec.NAMES if "stream" in ec.classes(n, force_stream=True) and ec.classes(n, force_stream=True) != ec.classes(n)])
def test_streaming_form(engine_cls, orc, monkeypatch, capfd, name):
    monkeypatch.setenv("LCR_ENUM_FORCE_STREAM", "1")
    profiled_check(engine_cls, orc, monkeypatch, capfd, name, ec.classes(name, force_stream=True))


@pytest.mark.parametrize("name", [n for n in ec.NAMES if set(ec.classes(n)) != {"big"}])
def test_global_memory_form(engine_cls, orc, monkeypatch, capfd, name):
    monkeypatch.setenv("LCR_ENUM_FORCE_BIG", "1")
    profiled_check(engine_cls, orc, monkeypatch, capfd, name, ["big"] * len(ec.classes(name)))


def _oracle_census(orc, name):
    regs = par.oracle_all(orc, ec.batch(name), ec.params(name))
    return np.sum([R.tie_census() for R in regs], axis=0)


@pytest.mark.parametrize("name", TIE_CASES + ["single_entry_rows", "tile_s8"])
def test_step_elision_and_the_tie_census(engine_cls, orc, name):
    """enum_elide 0 / 1 x enum_force_stream 0 / 1: one result, one census (as test_enum_step_elision_gpu.test_on_off_and_kernel_class) -- the
    queue of tied rows and its overflow paths, the batches of k4_enum_resolve and the repair pass leave the same bytes whichever kernel ran the
    restarts and whether or not unchanged steps were skipped.  Nothing is left unresolved, and the counts are the oracle's: sigma_f64 / sigma_flips
    its sigma ties at rows with an entry at a het site and those of them that flip (census [8], [4]; lcr_get_tie_census counts those rows
    only -- the identity holds on the tie batch of test_gpu_parity.test_enumeration_kernels_agree, where [0] also counts rows without one),
    delta_step_f64 its delta / eta ties and tie-only steps ([1] + [2]).  A restart of the repair list is run twice and counts the sigma ties of
    both runs (its delta / step counts are taken back, its sigma counts are not): with such restarts sigma_f64 lies between the oracle's
    count and twice that."""
    b, p = ec.batch(name), ec.params(name)
    runs = {(el, st): _run(engine_cls, b, p, el, st) for el in (0, 1) for st in (0, 1)}
    ref = runs[(1, 0)]
    for k, got in runs.items():
        assert got[0] == ref[0], "%s: results differ: (enum_elide, enum_force_stream) = %s" % (name, k)
        assert got[1] == ref[1], (name, k, got[1], ref[1])
    hc, oc = ref[1], _oracle_census(orc, name)
    print("%s: census %s, oracle %s" % (name, hc, oc.tolist()))
    assert hc["sigma_unresolved"] == 0 and hc["best_unresolved"] == 0 and hc["step_unresolved"] == 0 and hc["delta_unresolved"] == 0, hc
    assert hc["delta_step_f64"] == int(oc[1]) + int(oc[2]), (hc, oc.tolist())
    if int(oc[1]) + int(oc[2]) == 0:
        assert hc["sigma_f64"] == int(oc[8]) > 0 and hc["sigma_flips"] == int(oc[4]), (hc, oc.tolist())
    else:
        assert 0 < int(oc[8]) <= hc["sigma_f64"] <= 2 * int(oc[8]), (hc, oc.tolist())
    if name == "redo_over_grid":
        assert int(oc[2]) > ec.REDO_GRID


@pytest.mark.parametrize("name", ["tq_126", "tq_127", "tq_300"])
@pytest.mark.parametrize("stream", [0, 1], ids=["bits", "stream"])
def test_sigma_ties_alone(engine_cls, orc, monkeypatch, name, stream):
    """tie_arith = 2: the sigma ties by the f64 scores, equal objectives by the f64 sums, nothing else -- the oracle with these classes (the
    mechanism of test_gpu_parity.test_tie_arithmetic_switch).  No restart is run a second time at this level, so the census is the oracle's
    count for count: every tied row scored once ([8]), every flip of one ([4]), every tie-only step left as it is ([2]).  This is the check
    that cannot miss a tied row beyond the queue: in the region's RESULT a restart that lost such a row's flip is outvoted by the restarts
    that did not need it (tq_127 has one row beyond the queue, and it flips in about half of the restarts)."""
    monkeypatch.setenv("LCR_TIE_ARITH", "2")
    monkeypatch.setenv("LCR_ENUM_FORCE_STREAM", str(stream))
    monkeypatch.setitem(par.ORACLE_TIE_MASK, 0, orc.tie_mask(9, 1))
    check(engine_cls, orc, name)
    E = engine_cls(0, ec.params(name))
    E.load_batch(ec.batch(name)).run_all()
    hc = E.tie_census()
    E.close()
    oc = _oracle_census(orc, name)
    print("%s: census %s, oracle %s" % (name, hc, oc.tolist()))
    assert int(oc[4]) > 0 and int(oc[1]) == 0
    assert (hc["sigma_f64"], hc["sigma_flips"], hc["step_unresolved"]) == (int(oc[8]), int(oc[4]), int(oc[2])), (hc, oc.tolist())
    assert hc["sigma_unresolved"] == 0 and hc["delta_unresolved"] == 0 and hc["delta_step_f64"] == 0, hc


def _region_alone(b, g):
    rb, re_ = int(b.read_begin[g]), int(b.read_begin[g + 1])
    so, eo = int(b.seq_off[rb]), int(b.seq_off[re_ - 1] + b.seq_len[re_ - 1])
    co, ce = int(b.cig_off[rb]), int(b.cig_off[re_ - 1] + b.n_cig[re_ - 1])
    return _abi.ReadBatch(pos=b.pos[rb:re_], seq_len=b.seq_len[rb:re_], lead_clip=b.lead_clip[rb:re_], trail_clip=b.trail_clip[rb:re_],
                          flags=b.flags[rb:re_], seq_off=b.seq_off[rb:re_] - so, cig_off=b.cig_off[rb:re_] - co, n_cig=b.n_cig[rb:re_],
                          bases=b.bases[so:eo], quals=b.quals[so:eo], cigar=b.cigar[co:ce], start0=b.start0[g:g + 1], len=b.len[g:g + 1],
                          read_begin=[0, re_ - rb], ref=b.ref[int(b.col_off[g]):int(b.col_off[g + 1])])


def test_mixed_batch_composition(engine_cls):
    """each region of class_mixed alone in a batch gives the bytes it gives inside the mixed batch, whose launch is forked between the
    queues of the classes (the pattern of test_gpu_parity.test_batch_composition_independence)"""
    b, p = ec.batch("class_mixed"), ec.params("class_mixed")
    E = engine_cls(0, p)
    E.load_batch(b).run_all()
    c_all, off = E.candidates()
    pr_all, rro = E.phase_result(), E.fragmat()["row_region_off"]
    for g in range(b.n_regions):
        E1 = engine_cls(0, p)
        E1.load_batch(_region_alone(b, g)).run_all()
        c_one, pr = E1.candidates()[0], E1.phase_result()
        E1.close()
        sub = c_all[off[g]:off[g + 1]].copy()
        sub["region"] = 0
        assert sub.tobytes() == c_one.tobytes(), "candidates of region %d" % g
        for f in ("haplotag", "assignment", "phase_set"):
            assert np.array_equal(pr_all[f][rro[g]:rro[g + 1]], pr[f]), "%s of region %d" % (f, g)
        assert pr_all["objective"][g] == pr["objective"][0], "objective of region %d" % g
    E.close()

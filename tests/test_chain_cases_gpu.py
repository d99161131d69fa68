"""The recipes of tests/chain_cases.py in front of the chain kernels: every case through test_gpu_parity.full_check (planes, candidates,
fragment matrix, LD blocks, sigma / delta / eta, the exact fixed-point objective, the VCF text, the F64-mode check; no bar of its own) in each
form the phase stage has for a chain region.  tests/test_chain_cases.py shows on the CPU that each case meets the limit it names.

  default    the scope and form the region's size gives it.  A profiled run (LCR_PHASE_PROF=1): the library's report of every chain region's
             form must be what chain_cases.predicted_form says -- a wrong restatement of launch_chain's rules fails here
  all-CU     LCR_GRID_MIN_ENTRIES=0 against the oracle under orc.TIE_MASK_LIBLCR_GRID: the batched rounds, the side-by-side lanes
             (grid_spec_batch = 0 with 1 and 8 lanes) and the fenced barriers (grid_generic = 1); the heavy size-edge cases in the first only
and, on the tie cases, the tie census against the oracle's with chain_ties on and off, the batched rounds' tie list within and beyond its
capacity, the scope rule at grid_min = E and E + 1, and the small region of the mixed batches alone against itself in the batch."""
import functools
import re

import numpy as np
import pytest

import chain_cases as cc
import test_gpu_parity as par
from test_enum_cases_gpu import _region_alone

pytestmark = pytest.mark.gpu

FORM_LINE = re.compile(r"^\[phase\]   (chain region \d+: scope .*)$", re.M)
ALL_CU_FORMS = {"batched": {}, "lanes_1": {"LCR_GRID_SPEC_BATCH": "0", "LCR_GRID_SPEC_LANES": "1"},
                "lanes_8": {"LCR_GRID_SPEC_BATCH": "0", "LCR_GRID_SPEC_LANES": "8"}, "generic": {"LCR_GRID_GENERIC": "1"}}
SCOPE_FREE = [n for n in cc.NAMES if n != "scope"]


@functools.lru_cache(maxsize=None)
def _shapes(name):
    from oracle import orc
    orc.build()
    b, p = cc.batch(name), cc.params(name)
    out = []
    for g in range(b.n_regions):
        R = orc.Region(b, g, p).set_fast(1).pileup().candidates().fragments()
        out.append(cc.region_shape(R.fragmat(), R.cands()))
    return out


def check(engine_cls, orc, name, **more):
    try:
        return par.full_check(engine_cls, orc, cc.batch(name), cc.params(name, **more))
    except AssertionError as e:
        raise AssertionError("%s: %s" % (name, e)) from e


def profiled_check(engine_cls, orc, monkeypatch, capfd, name, grid_min=cc.GRID_MIN):
    """full_check under LCR_PHASE_PROF=1; the one phase call's report of its chain regions' forms must be the predicted one"""
    monkeypatch.setenv("LCR_PHASE_PROF", "1")
    capfd.readouterr()
    check(engine_cls, orc, name)
    got = sorted(FORM_LINE.findall(capfd.readouterr().err))
    want = sorted(cc.form_line(g, f) for g, f in enumerate(cc.forms(_shapes(name), grid_min)))
    assert got == want, "%s: the library reports %s, predicted %s" % (name, got, want)


@pytest.mark.parametrize("name", cc.NAMES)
def test_default_form_is_the_predicted_one(engine_cls, orc, monkeypatch, capfd, name):
    profiled_check(engine_cls, orc, monkeypatch, capfd, name)


@pytest.mark.parametrize("name,form", [(n, f) for n in SCOPE_FREE for f in ALL_CU_FORMS if f == "batched" or not cc.BY_NAME[n]["heavy"]])
def test_all_cu_forms(engine_cls, orc, monkeypatch, capfd, name, form):
    monkeypatch.setenv("LCR_GRID_MIN_ENTRIES", "0")
    for k, v in ALL_CU_FORMS[form].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setitem(par.ORACLE_TIE_MASK, 0, orc.TIE_MASK_LIBLCR_GRID)
    profiled_check(engine_cls, orc, monkeypatch, capfd, name, grid_min=0)


@pytest.mark.parametrize("side", ["all-CU", "workgroup"])
def test_scope_rule(engine_cls, orc, monkeypatch, capfd, side):
    """stat.E >= grid_min: the small region with grid_min_entries = E gets all CUs, with E + 1 one workgroup"""
    E = _shapes("scope")[0][2]
    grid_min = E if side == "all-CU" else E + 1
    monkeypatch.setenv("LCR_GRID_MIN_ENTRIES", str(grid_min))
    if side == "all-CU":
        monkeypatch.setitem(par.ORACLE_TIE_MASK, 0, orc.TIE_MASK_LIBLCR_GRID)
    assert cc.forms(_shapes("scope"), grid_min)[0]["scope"] == side
    profiled_check(engine_cls, orc, monkeypatch, capfd, "scope", grid_min=grid_min)


def _census(engine_cls, name):
    E = engine_cls(0, cc.params(name))
    E.load_batch(cc.batch(name)).run_all()
    hc = E.tie_census()
    E.close()
    return hc


def _oracle_census(orc, name):
    return np.sum([R.tie_census() for R in par.oracle_all(orc, cc.batch(name), cc.params(name))], axis=0)


@pytest.mark.parametrize("resolve", [1, 0])
@pytest.mark.parametrize("name", cc.TIE_CASES)
def test_ties_in_workgroup_scope(engine_cls, orc, monkeypatch, name, resolve):
    """as test_gpu_parity.test_chain_ties_of_classes_2_and_4: with chain_ties on the results are the oracle's with every class resolved, nothing
    is reported unresolved and the decided ties are its census count for count (the class-8 cases reach the ordered f64 sums: best_f64);
    with chain_ties = 0 the first pass's result stands -- the oracle's under chain mask 1 -- and the unresolved counts are ITS census.
    ties_2_4_matrix_global runs both instantiations of k4_chain_wg's body with the matrix in global memory."""
    monkeypatch.setenv("LCR_CHAIN_TIES", str(resolve))
    monkeypatch.setitem(par.ORACLE_TIE_MASK, 0, orc.TIE_MASK_LIBLCR if resolve else orc.TIE_MASK_LIBLCR_GRID)
    check(engine_cls, orc, name)
    hc, oc = _census(engine_cls, name), _oracle_census(orc, name)
    print("%s: census %s, oracle %s" % (name, hc, oc.tolist()))
    if resolve:
        assert hc["delta_unresolved"] == 0 and hc["step_unresolved"] == 0 and hc["sigma_unresolved"] == 0 and hc["best_unresolved"] == 0, hc
        assert hc["delta_step_f64"] == int(oc[1]) + int(oc[2]), (hc, oc.tolist())
        if name.startswith("class8_"):
            assert hc["best_f64"] > 0, hc
        else:
            assert int(oc[1]) + int(oc[2]) > 0
    else:
        assert hc["delta_unresolved"] == int(oc[1]) and hc["step_unresolved"] == int(oc[2]), (hc, oc.tolist())


@pytest.mark.parametrize("name", cc.TIE_QUEUE_CASES)
def test_batched_rounds_tie_list(engine_cls, orc, monkeypatch, name):
    """the batched all-CU rounds with more tied (row, state) pairs in a workgroup's sigma step than TIE_CAP, and with fewer: the oracle's
    results under the grid mask (test_all_cu_forms runs that too), no sigma tie unresolved, and at least the oracle's number of them decided
    -- the all-CU census counts the ties of speculative rounds that are discarded as well"""
    monkeypatch.setenv("LCR_GRID_MIN_ENTRIES", "0")
    monkeypatch.setitem(par.ORACLE_TIE_MASK, 0, orc.TIE_MASK_LIBLCR_GRID)
    check(engine_cls, orc, name)
    hc, oc = _census(engine_cls, name), _oracle_census(orc, name)
    print("%s: census %s, oracle %s" % (name, hc, oc.tolist()))
    assert hc["sigma_unresolved"] == 0 and hc["sigma_f64"] >= int(oc[8]) > 0, (hc, oc.tolist())


@pytest.mark.parametrize("name", ["mixed_state", "mixed_matrix"])
def test_mixed_batch_composition(engine_cls, name):
    """the small region alone gives the bytes it gives beside the large one, whose size moves the launch's state to global memory
    (mixed_state) or which runs without its matrix in LDS in the same launch (mixed_matrix)"""
    b, p = cc.batch(name), cc.params(name)
    alone, both = cc.forms(_shapes(name)[:1])[0], cc.forms(_shapes(name))[0]
    assert alone["state"] == "LDS" and alone["matrix"] == "LDS" and (both["state"] == "global") == (name == "mixed_state")
    E = engine_cls(0, p)
    E.load_batch(b).run_all()
    c_all, off = E.candidates()
    pr_all, rro = E.phase_result(), E.fragmat()["row_region_off"]
    E1 = engine_cls(0, p)
    E1.load_batch(_region_alone(b, 0)).run_all()
    c_one, pr = E1.candidates()[0], E1.phase_result()
    E1.close()
    assert c_all[off[0]:off[1]].tobytes() == c_one.tobytes()
    for f in ("haplotag", "assignment", "phase_set"):
        assert np.array_equal(pr_all[f][rro[0]:rro[1]], pr[f]), f
    assert pr_all["objective"][0] == pr["objective"][0]
    E.close()

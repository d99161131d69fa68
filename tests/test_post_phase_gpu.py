"""The recipes of tests/post_phase_cases.py in front of the kernels: every case through test_gpu_parity.full_check (planes, candidates,
fragment matrix, phase results, VCF text, the F64-mode check; no bar of its own) in each scope post_run (csrc/k4_post.h) is built for.
tests/test_post_phase_cases.py shows on the CPU that each case meets the branch it names, under both values of max_enum_snps used here.

  wg      k4_post, one workgroup per region (default)
  half    its eight-wave form (LCR_POST_HALF=1)
  grid    k4_gpost, all CUs on the region (LCR_GRID_MIN_ENTRIES=0).  Only a chain region goes there, so a case that is phased by
          enumeration runs with max_enum_snps below its number of sites (post_phase_cases.params(lowered=True)) -- and once more in
          the default scope with that value (wg-chain), the control of the grid run.  The oracle follows the parameter.
The grid runs are profiled runs (LCR_PHASE_PROF=1): the report says which regions took k4_gpost and how many rounds its rescue lists ran."""
import re

import pytest

import post_phase_cases as pc
import test_gpu_parity as par

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in pc.CASES]
LOWERED = [n for n in NAMES if pc.is_enumerated(n)]


def check(engine_cls, orc, name, lowered):
    try:
        return par.full_check(engine_cls, orc, pc.batch(name), pc.params(name, lowered))
    except AssertionError as e:
        raise AssertionError("%s%s: %s" % (name, " (max_enum_snps lowered)" if lowered else "", e)) from e


@pytest.mark.parametrize("name", NAMES)
def test_workgroup_scope(engine_cls, orc, name):
    check(engine_cls, orc, name, False)


@pytest.mark.parametrize("name", LOWERED)
def test_workgroup_scope_as_a_chain_region(engine_cls, orc, name):
    check(engine_cls, orc, name, True)


@pytest.mark.parametrize("name", NAMES)
def test_eight_wave_form(engine_cls, orc, monkeypatch, name):
    monkeypatch.setenv("LCR_POST_HALF", "1")
    check(engine_cls, orc, name, False)


@pytest.mark.parametrize("name", NAMES)
def test_grid_scope(engine_cls, orc, monkeypatch, capfd, name):
    monkeypatch.setenv("LCR_GRID_MIN_ENTRIES", "0")
    monkeypatch.setenv("LCR_PHASE_PROF", "1")
    capfd.readouterr()
    check(engine_cls, orc, name, name in LOWERED)
    err = capfd.readouterr().err
    assert [int(g) for g in re.findall(r"k4_gpost region (\d+):", err)] == [0], "the region did not take k4_gpost"
    rounds = [(int(a), int(b)) for a, b in re.findall(r"rescue rounds: RNA-edit list (\d+), low-fraction list (\d+)", err)]
    assert len(rounds) == 1
    print("rescue rounds of %s: RNA-edit list %d, low-fraction list %d" % ((name,) + rounds[0]))
    want = pc.BY_NAME[name]["census"]
    if name == "edit_list_rounds_mps8":
        assert rounds[0][0] >= 2, rounds
    if name == "lowfrac_list":     # the second member holds the rows the first one's success drew for: it cannot share its round
        assert rounds[0][1] >= want["lowfrac_rounds"] == 2, rounds

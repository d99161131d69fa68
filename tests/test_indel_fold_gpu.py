"""The recipes of tests/indel_fold_cases.py in front of the kernels (-m gpu).  K0 folds a 1-base indel behind an M op into that op's record
(REC_F_INS / REC_F_DEL, lcr_dev.h), K1 counts it from there.  Every case, plane buffer poisoned, in the three forms of the tally
(tests/test_pileup_cases_gpu.py: hifi, fused, lean): the 13 planes bit for bit against the C++ oracle, and lcr_pileup_records against the
model of the rule -- the fold happened exactly where the rule says, nowhere else.  Then fold_indels 0: the records of every op on its own,
and planes, candidates and haplotags byte for byte those of the default; the two histogram forms of the candidate stage over flagged
records; all cases one behind the other on one context; one packed batch.  tests/test_indel_fold_cases.py shows on the CPU that the cases
meet the borders they name."""
import functools

import pytest

import indel_fold_cases as fc
import helpers  # noqa: F401  (the recipes' batch builder)
import pileup_cases as pc  # noqa: F401
import test_gpu_parity as par
from test_lean_planes_gpu import check_stages, pass1_bounds, stages, took_lean_form

pytestmark = pytest.mark.gpu

PRIMER = "mid"      # (its het region leaves survivors)


@functools.lru_cache(maxsize=None)
def oracle_of(name, platform, upto):
    from oracle import orc
    orc.build()
    return par.oracle_all(orc, fc.batch(name), fc.params(name, platform), upto=upto)


@functools.lru_cache(maxsize=None)
def has_survivors(name):
    return pass1_bounds(fc.batch(name), fc.params(name, "ont"))[0] > 0


def engine(engine_cls, prm, **switches):
    E = engine_cls(0, prm)
    E.debug_set("poison_planes", 1)
    for k, v in switches.items():
        E.debug_set(k, v)
    return E


def check_records(E, name, platform, fold=True):
    items, records, folded = fc.model(name, platform)
    want = (items, records if fold else records + len(folded))
    assert E.pileup_records() == want, "%s (%s): (items, records) %s, the rule gives %s" % (name, platform, E.pileup_records(), want)


@pytest.mark.parametrize("name", fc.NAMES)
def test_hifi(engine_cls, orc, name):
    b, p = fc.batch(name), fc.params(name, "hifi")
    E = engine(engine_cls, p)
    E.load_batch(b).fill_data_into_freq_vec()
    check_records(E, name, "hifi")
    par.check_pileup(E, oracle_of(name, "hifi", "pileup"), b)
    E.close()


@pytest.mark.parametrize("name", fc.NAMES)
def test_fused(engine_cls, orc, name):
    b, p = fc.batch(name), fc.params(name, "ont")
    regs = oracle_of(name, "ont", "post")
    E = engine(engine_cls, p)
    E.load_batch(b).fill_data_into_freq_vec()
    assert not took_lean_form(E, b, p)
    check_records(E, name, "ont")
    par.check_pileup(E, regs, b)
    check_stages(stages(E), regs)
    E.close()


@pytest.mark.parametrize("name", fc.NAMES)
def test_lean(engine_cls, orc, name):
    assert has_survivors(PRIMER)
    b, p = fc.batch(name), fc.params(name, "ont")
    regs = oracle_of(name, "ont", "post")
    E = engine(engine_cls, p)
    E.load_batch(b).run_all()                       # (a context's first batch leaves the survivor guess the lean form is sized by)
    if not has_survivors(name):
        E.params = fc.params(PRIMER, "ont")
        E.load_batch(fc.batch(PRIMER)).run_all()
        E.params = p
    E.load_batch(b).fill_data_into_freq_vec()
    assert took_lean_form(E, b, p)
    check_records(E, name, "ont")
    check_stages(stages(E), regs)
    par.check_pileup(E, regs, b)                    # the planes only now: the full form replayed over the same records, the insertion plane with it
    assert took_lean_form(E, b, p)
    E.close()


def snapshot(E, platform):
    if platform == "hifi":
        E.fill_data_into_freq_vec()
        return (E.columns().tobytes(),)
    E.run_all()
    c, off = E.candidates()
    return (c.tobytes(), off.tobytes(), E.phase_result()["haplotag"].tobytes(), E.columns().tobytes())


@pytest.mark.parametrize("platform", fc.PLATFORMS)
@pytest.mark.parametrize("name", fc.NAMES)
def test_fold_off_gives_every_op_its_record_and_the_same_results(engine_cls, orc, name, platform):
    b, p = fc.batch(name), fc.params(name, platform)
    got = {}
    for fold in (1, 0):
        E = engine(engine_cls, p, fold_indels=fold)
        E.load_batch(b)
        got[fold] = snapshot(E, platform)
        check_records(E, name, platform, fold=bool(fold))
        if not fold:
            assert E.pileup_records()[1] == fc.unfolded_records(b, p)
            par.check_pileup(E, oracle_of(name, platform, "pileup" if platform == "hifi" else "post"), b)
        E.close()
    assert got[1] == got[0]


@pytest.mark.parametrize("name", [c["name"] for c in fc.CASES if c["hets"]])
def test_tiles(engine_cls, orc, name):
    """the candidate records under hist_tiles 1 (k2_hist_tiles reads K0's records, flags and all) and -1 equal byte for byte, and the oracle's"""
    b, p = fc.batch(name), fc.params(name, "ont")
    regs = oracle_of(name, "ont", "cands")
    got = {}
    for v in (1, -1):
        E = engine(engine_cls, p, hist_tiles=v)
        E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps()
        c, off = par.check_cands(E, regs, phased=False)
        got[v] = (c.tobytes(), off.tobytes())
        g = fc.region_of(name, "hets")
        assert (c["pos"][off[g]:off[g + 1]] - int(b.start0[g])).tolist() == fc.meta(name)["hets"]["het_cols"]
        par.check_pileup(E, regs, b)
        E.close()
    assert got[1] == got[-1]


@pytest.mark.parametrize("platform", fc.PLATFORMS)
def test_all_cases_on_one_context(engine_cls, orc, platform):
    """forwards, then backwards (on ONT a batch behind one with pass-1 survivors takes the lean form): what a fresh context gives for each batch, the
    oracle's planes, the rule's record counts"""
    fresh = {}
    for n in fc.NAMES:
        F = engine(engine_cls, fc.params(n, platform))
        F.load_batch(fc.batch(n))
        fresh[n] = snapshot(F, platform)
        F.close()
    E = engine(engine_cls, fc.params(fc.NAMES[0], platform))
    for n in fc.NAMES + fc.NAMES[::-1]:
        E.params = fc.params(n, platform)
        E.load_batch(fc.batch(n))
        assert snapshot(E, platform) == fresh[n], "%s behind another batch" % n
        check_records(E, n, platform)
        par.check_pileup(E, oracle_of(n, platform, "pileup" if platform == "hifi" else "post"), fc.batch(n))
    E.close()


def test_a_packed_batch(engine_cls, orc):
    """lcr_load_batch_packed: the unpacked bases lie in another buffer, the records' offsets with them"""
    name = "neighbours"
    b, p = fc.batch(name), fc.params(name, "ont")
    E = engine(engine_cls, p)
    E.load_batch(b.pack()).fill_data_into_freq_vec()
    check_records(E, name, "ont")
    par.check_pileup(E, oracle_of(name, "ont", "post"), b)
    check_stages(stages(E), oracle_of(name, "ont", "post"))
    E.close()

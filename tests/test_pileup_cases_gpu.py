"""The recipes of tests/pileup_cases.py in front of the kernels (-m gpu): every case through load_batch -> fill_data_into_freq_vec and
test_gpu_parity.check_pileup, bit for bit on the 13 planes against the C++ oracle, with the plane buffer poisoned in front of every pileup
(lcr_debug_set("poison_planes", 1)), in each form the case is listed for.  tests/test_pileup_cases.py shows on the CPU that each case
meets the limit it names.

  hifi    the HiFi preset: the full tally without a filter pass in its epilogue, K1z behind it (the zone family runs here only, at its (D, L))
  fused   the ONT preset on a fresh context: the full tally with pass 1 of the candidate filters in the epilogue; once more with fuse_filter 0
  lean    the ONT preset on a context primed with the same batch: survivors instead of planes (took_lean_form), candidates, fragments and phase
          against the oracle, the planes through the getter afterwards.  A candidate stage without a pass-1 survivor leaves no guess to size
          the staging by, and the next tally would take the full form: a case without survivors is primed with PRIMER behind itself
  tiles   the ONT cases with het sites on tile edges: the candidate records under hist_tiles 1 (k2_hist_tiles reads K0's records) and -1 equal
          byte for byte, and the oracle's
and every family's batches one behind the other on one context, forwards and backwards, against a fresh context per batch."""
import functools

import pytest

import pileup_cases as pc
import test_gpu_parity as par
from test_lean_planes_gpu import check_stages, pass1_bounds, stages, took_lean_form

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def oracle_of(name, platform, upto):
    from oracle import orc
    orc.build()
    return par.oracle_all(orc, pc.batch(name), pc.params(name, platform), upto=upto)


PRIMER = "seg"      # (its het region leaves two survivors)


@functools.lru_cache(maxsize=None)
def has_survivors(name):
    """pass 1 of the candidate filters keeps at least one column of the case, counted on the CPU"""
    return pass1_bounds(pc.batch(name), pc.params(name, "ont"))[0] > 0


def engine(engine_cls, prm, **switches):
    E = engine_cls(0, prm)
    E.debug_set("poison_planes", 1)
    for k, v in switches.items():
        E.debug_set(k, v)
    return E


@pytest.mark.parametrize("name", pc.names(form="hifi"))
def test_hifi(engine_cls, orc, name):
    b, p = pc.batch(name), pc.params(name, "hifi")
    E = engine(engine_cls, p)
    E.load_batch(b).fill_data_into_freq_vec()
    par.check_pileup(E, oracle_of(name, "hifi", "pileup"), b)
    E.close()


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("name", pc.names(form="fused"))
def test_fused(engine_cls, orc, name, fuse):
    b, p = pc.batch(name), pc.params(name, "ont")
    regs = oracle_of(name, "ont", "post")
    E = engine(engine_cls, p, fuse_filter=fuse)
    E.load_batch(b).fill_data_into_freq_vec()
    assert not took_lean_form(E, b, p)
    par.check_pileup(E, regs, b)
    check_stages(stages(E), regs)                   # the epilogue's flags (fuse 1) / k2_filter's (fuse 0) at the design columns
    E.close()


@pytest.mark.parametrize("name", pc.names(form="lean"))
def test_lean(engine_cls, orc, name):
    assert has_survivors(PRIMER)
    b, p = pc.batch(name), pc.params(name, "ont")
    regs = oracle_of(name, "ont", "post")
    E = engine(engine_cls, p)
    E.load_batch(b).run_all()                       # (a context's first batch leaves the survivor guess the lean form is sized by)
    if not has_survivors(name):
        E.params = pc.params(PRIMER, "ont")
        E.load_batch(pc.batch(PRIMER)).run_all()
        E.params = p
    E.load_batch(b).fill_data_into_freq_vec()
    assert took_lean_form(E, b, p)
    check_stages(stages(E), regs)
    par.check_pileup(E, regs, b)                    # the planes only now: planes_tally runs the full form over the same records
    assert took_lean_form(E, b, p)
    E.close()


@pytest.mark.parametrize("name", pc.names(form="tiles"))
def test_tiles(engine_cls, orc, name):
    b, p = pc.batch(name), pc.params(name, "ont")
    regs = oracle_of(name, "ont", "cands")
    got = {}
    for v in (1, -1):
        E = engine(engine_cls, p, hist_tiles=v)
        E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps()
        c, off = par.check_cands(E, regs, phased=False)
        got[v] = (c.tobytes(), off.tobytes())
        g = pc.region_of(name, "hets")
        assert (c["pos"][off[g]:off[g + 1]] - int(b.start0[g])).tolist() == pc.meta(name)["hets"]["het_cols"]
        par.check_pileup(E, regs, b)
        E.close()
    assert got[1] == got[-1]


def snapshot(E, platform):
    if platform == "hifi":
        E.fill_data_into_freq_vec()
        return (E.columns().tobytes(),)
    E.run_all()
    c, off = E.candidates()
    return (c.tobytes(), off.tobytes(), E.phase_result()["haplotag"].tobytes(), E.columns().tobytes())


@pytest.mark.parametrize("family,platform", [(f, pl) for f in pc.FAMILIES for pl in sorted({x for n in pc.names(family=f) for x in pc.platforms(n)})])
def test_a_family_s_batches_on_one_context(engine_cls, orc, family, platform):
    """forwards, then backwards (on ONT a batch behind one with pass-1 survivors takes the lean form): what a fresh context gives for each batch, and the
    oracle's planes"""
    names = [n for n in pc.names(family=family) if platform in pc.platforms(n)]
    fresh = {}
    for n in names:
        F = engine(engine_cls, pc.params(n, platform))
        F.load_batch(pc.batch(n))
        fresh[n] = snapshot(F, platform)
        F.close()
    E = engine(engine_cls, pc.params(names[0], platform))
    for n in names + names[::-1]:
        E.params = pc.params(n, platform)
        E.load_batch(pc.batch(n))
        assert snapshot(E, platform) == fresh[n], "%s behind another batch" % n
        par.check_pileup(E, oracle_of(n, platform, "pileup" if platform == "hifi" else "post"), pc.batch(n))
    E.close()

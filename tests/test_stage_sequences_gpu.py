"""Stage re-entry on one context: explicit call sequences (pileup, candidate stage, fragments, phase called again on the same upstream
state, debug switches turned between calls, refused calls in between), each result-producing step against the CPU oracle for the
parameters that step was called with.  The candidate-stage parameter sets of a batch differ only in fields lcr_pileup does not read,
so the oracle of set Q is oracle_all(Q) and its planes are the pileup's.  include/lcr.h states which re-entries are allowed."""
import functools
import re

import numpy as np
import pytest

import helpers
import test_gpu_parity as par
import test_import_candidates_gpu as imp
from longcallr_amd import _abi, synth
from longcallr_amd._lib import LcrError

pytestmark = pytest.mark.gpu

# batch key -> (batch factory, preset, preset overrides).  cdna21 / drna22: the ONT presets, pass 1 of the filters fused into the tally
# (test_filter_pass_in_the_tally_epilogue); masseq13: no fused pass, k1_zonefix; lowfrac: rescued low-fraction sites (test_low_fraction_rescue).
BATCHES = {
    "cdna21": (lambda: synth.make_batch("ont-cdna", n_genes=4, gene_len=11000, depth=40, seed=21), "ont-cdna", dict(seed=21)),
    "drna22": (lambda: synth.make_batch("ont-drna", n_genes=4, gene_len=11000, depth=40, seed=22), "ont-drna", dict(seed=22)),
    "masseq13": (lambda: synth.make_batch("masseq", n_genes=5, gene_len=9000, depth=35, seed=13), "hifi-masseq", dict(seed=13)),
    "lowfrac": (lambda: par._low_fraction_batch(seed=1), "ont-cdna", dict(seed=3, min_phase_score=4.0)),
}


def _set_over(p0, name):
    """P1: survivors drop a lot; P2: strand-bias filter flipped, other low-fraction cut; P3: max_depth above the u16 counters of
    k2_hist_tiles (no tile histograms on the same pileup, the read walk and its hit lists instead)"""
    return {"P0": {}, "P1": dict(min_depth=150), "P2": dict(use_strand_bias=1 - int(p0.use_strand_bias), low_frac_cut=0.1),
            "P3": dict(max_depth=70000)}[name]


@functools.lru_cache(maxsize=None)
def batch(key):
    return BATCHES[key][0]()


@functools.lru_cache(maxsize=None)
def params(key, name="P0", **extra):
    _, preset, over = BATCHES[key]
    p0 = _abi.make_params(preset, **over)
    return _abi.make_params(preset, **dict(over, **_set_over(p0, name), **extra))


_ORACLE = {}


def oracle(orc, key, name="P0"):
    if (key, name) not in _ORACLE:
        _ORACLE[key, name] = par.oracle_all(orc, batch(key), params(key, name))
    return _ORACLE[key, name]


def cand_set(regs):
    return [(int(r["region"]), int(r["pos"])) for R in regs for r in R.cands()]


PRE_PHASE_EXACT = ["pos", "region", "ref_base", "allele1", "allele2", "n_alt", "cnt1", "cnt2", "depth"]


def check_called(E, regs):
    """the candidate stage alone: every field lcr_phase leaves as it is (it rewrites haplotype, genotype, variant type, flags,
    phase score and phase set)"""
    c, off = E.candidates()
    for g, R in enumerate(regs):
        rc, gc = R.cands(), c[off[g]:off[g + 1]]
        assert len(gc) == len(rc), "candidate count region %d: %d vs %d" % (g, len(gc), len(rc))
        for f in PRE_PHASE_EXACT:
            assert np.array_equal(gc[f], rc[f]), "cand.%s region %d" % (f, g)
        assert np.array_equal(gc["af1"], rc["af1"]) and np.array_equal(gc["af2"], rc["af2"])
        assert par.close(gc["loglik"], rc["loglik"], 1e-9) and par.close(gc["gt_prob"], rc["gt_prob"], 1e-9)
        assert np.array_equal(par.as_i32(gc["qual"]), par.as_i32(rc["qual"])) and np.array_equal(par.as_i32(gc["gq"]), par.as_i32(rc["gq"]))


def fm_bytes(fm):
    return tuple(fm[k].tobytes() for k in sorted(fm))


def getters(E, cand_first):
    if cand_first:
        c, off = E.candidates()
        pr = E.phase_result()
    else:
        pr = E.phase_result()
        c, off = E.candidates()
    return (c.tobytes(), off.tobytes()) + tuple(pr[k].tobytes() for k in ("haplotag", "assignment", "phase_set", "objective"))


def snapshot(E):
    """the getters read twice, in both orders (same bytes), and the fragment matrix"""
    a, b = getters(E, True), getters(E, False)
    assert a == b, "the getters' order changed their bytes"
    return a + fm_bytes(E.fragmat())


def phase_round(E, regs):
    """lcr_fragments + lcr_phase behind a candidate stage, both against the oracle; returns the round's snapshot"""
    E.get_fragments()
    fm = par.check_fragmat(E, regs)
    E.phase()
    assert fm_bytes(E.fragmat()) == fm_bytes(fm), "fragmat() after lcr_phase differs from the one before"
    par.check_cands(E, regs, phased=True)
    par.check_phase(E, regs, fm)
    return snapshot(E)


def prof_lines(E, capfd, call, pattern):
    """run `call` with the phase_prof switch on and return the numbers of its stderr lines that match `pattern`"""
    capfd.readouterr()
    E.debug_set("phase_prof", 1)
    try:
        call()
    finally:
        E.debug_set("phase_prof", 0)
    return [int(x) for x in re.findall(pattern, capfd.readouterr().err)]


def survivors(E, capfd):
    """lcr_candidates, and the number of survivors of its count filters"""
    n = prof_lines(E, capfd, E.get_candidate_snps, r"\[cand\] (\d+) survivors")
    assert len(n) == 1
    return n[0]


def frag_walked(E, capfd):
    """lcr_fragments, and whether the candidate stage left K3 the hit lists of k2_hist's read walk (hits_valid)"""
    return len(prof_lines(E, capfd, E.get_fragments, r"\[frag\] (\d+) reads with more than")) == 1


@functools.lru_cache(maxsize=None)
def _fresh(engine_cls, key, name, debug=()):
    E = engine_cls(0, params(key, name))
    for k, v in debug:
        E.debug_set(k, v)
    E.load_batch(batch(key)).run_all()
    out = snapshot(E)
    E.close()
    return out


def _engine(engine_cls, key, name="P0"):
    E = engine_cls(0, params(key, name))
    E.load_batch(batch(key))
    return E


# ---- the sequences ----------------------------------------------------------------------------------------------------------------

def seq_cand_p_p2_p(engine_cls, orc, key, capfd):
    """pileup P0; cand P1; frag; phase; cand P0; frag; phase; cand P2; frag; phase.  The ONT presets' pileup leaves pass 1 of P0
    in its epilogue: cand P1 overwrites those flags, so cand P0 has to run the filter pass again."""
    assert cand_set(oracle(orc, key, "P1")) != cand_set(oracle(orc, key, "P0"))
    E = _engine(engine_cls, key)
    E.fill_data_into_freq_vec()
    par.check_pileup(E, oracle(orc, key), batch(key))
    for name in ("P1", "P0", "P2"):
        E.params = params(key, name)
        E.get_candidate_snps()
        assert phase_round(E, oracle(orc, key, name)) == _fresh(engine_cls, key, name), name
    E.close()


def seq_fuse_switch(engine_cls, orc, key, capfd):
    """pileup P0 (fused pass 1); fuse_filter 0; cand P0; fuse_filter 1; cand P1; cand P0"""
    assert cand_set(oracle(orc, key, "P1")) != cand_set(oracle(orc, key, "P0"))
    E = _engine(engine_cls, key)
    E.fill_data_into_freq_vec()
    E.debug_set("fuse_filter", 0)
    E.get_candidate_snps()
    check_called(E, oracle(orc, key, "P0"))
    E.debug_set("fuse_filter", 1)
    for name in ("P1", "P0"):
        E.params = params(key, name)
        E.get_candidate_snps()
        check_called(E, oracle(orc, key, name))
    assert phase_round(E, oracle(orc, key)) == _fresh(engine_cls, key, "P0")
    E.close()


def seq_survivor_guess(engine_cls, orc, key, capfd):
    """cand P1 (few survivors); cand P0 (more than the buffers sized by P1's count: the compaction queued before the count is known
    runs again); cand P1 -- each against the oracle and against a context that waits for the count (spec_compact 0)"""
    got = {}
    for spec in (1, 0):
        E = _engine(engine_cls, key)
        E.debug_set("spec_compact", spec)
        E.fill_data_into_freq_vec()
        rounds, n_sv = [], []
        for name in ("P1", "P0", "P1"):
            E.params = params(key, name)
            n_sv.append(survivors(E, capfd))
            check_called(E, oracle(orc, key, name))
            rounds.append(phase_round(E, oracle(orc, key, name)))
        E.close()
        assert n_sv[1] > n_sv[0] + n_sv[0] // 4 + 64, n_sv   # (lcr_candidates' guess: the last count + a quarter + 64)
        assert rounds[0] == rounds[2]
        got[spec] = rounds
    assert got[1] == got[0]


def seq_hist_path_switch(engine_cls, orc, key, capfd):
    """hist_tiles 1; cand P0 -> frag -> phase (tile histograms, no hit lists); cand P3 -> frag -> phase (u16 counters do not hold
    max_depth: the read walk, whose hit lists K3 takes); hist_tiles 0; cand P0 -> frag -> phase"""
    E = _engine(engine_cls, key)
    E.debug_set("hist_tiles", 1)
    E.fill_data_into_freq_vec()
    walked = []
    for name, tiles in (("P0", 1), ("P3", 1), ("P0", 0)):
        E.debug_set("hist_tiles", tiles)
        E.params = params(key, name)
        E.get_candidate_snps()
        walked.append(frag_walked(E, capfd))
        fm = par.check_fragmat(E, oracle(orc, key, name))
        E.phase()
        assert fm_bytes(E.fragmat()) == fm_bytes(fm)
        par.check_cands(E, oracle(orc, key, name), phased=True)
        par.check_phase(E, oracle(orc, key, name), fm)
        assert snapshot(E) == _fresh(engine_cls, key, name, (("hist_tiles", tiles),)), name
    assert walked[:2] == [False, True], walked
    E.close()


def seq_import_then_call(engine_cls, orc, key, capfd):
    """pileup P0; import S; frag; phase; cand P0; frag; phase; import S; frag; phase.  S: a fresh run's calls, perturbed as in
    test_rephasing_own_calls_on_synthetic_batches.  Import rounds == a fresh context's pileup + import S; call rounds == oracle."""
    b, prm = batch(key), params(key)
    F = engine_cls(0, prm)
    F.load_batch(b).fill_data_into_freq_vec().get_candidate_snps()
    lo, hi = int(b.start0[0]), int(b.start0[-1] + b.len[-1])
    S = imp.perturb(*imp.sites_of(F.candidates()[0]), np.random.default_rng(7), lo, hi)
    F.close()
    F = engine_cls(0, prm)
    F.load_batch(b).fill_data_into_freq_vec().import_external_candidates(*S).get_fragments().phase()
    want = snapshot(F)
    F.close()
    assert S[0].size > 0 and want[0] != _fresh(engine_cls, key, "P0")[0]
    E = _engine(engine_cls, key)
    E.fill_data_into_freq_vec()
    for step in ("import", "call", "import"):
        if step == "import":
            E.import_external_candidates(*S).get_fragments().phase()
            assert snapshot(E) == want
        else:
            E.get_candidate_snps()
            assert phase_round(E, oracle(orc, key)) == _fresh(engine_cls, key, "P0")
    E.close()


def seq_rephase(engine_cls, orc, key, capfd):
    """cand; frag; phase; phase; frag: the second lcr_phase and the lcr_fragments behind it are refused (the first phase rewrote the
    records they read), the getters keep the first phase's bytes; then cand; frag; phase == oracle"""
    E = _engine(engine_cls, key)
    E.fill_data_into_freq_vec().get_candidate_snps()
    pre = E.candidates()[0].copy()
    first = phase_round(E, oracle(orc, key))
    post = E.candidates()[0]
    fp = _abi.F_FOR_PHASING
    assert ((pre["flags"] & fp) != (post["flags"] & fp)).any(), "the first phase changed no FOR_PHASING bit"
    with pytest.raises(LcrError, match=r"lcr_phase failed \(-4\).*candidate stage"):
        E.phase()
    with pytest.raises(LcrError, match=r"lcr_fragments failed \(-4\).*candidate stage"):
        E.get_fragments()
    assert snapshot(E) == first
    E.get_candidate_snps()
    assert phase_round(E, oracle(orc, key)) == first
    E.close()


def seq_async_reentry(engine_cls, orc, key, capfd):
    """async on: pileup; cand P0; frag; phase; cand P1 (the first round never collected); frag; phase; collect == oracle(P1).
    Then the same with the stage synchronous."""
    regs = oracle(orc, key, "P1")
    for on in (True, False):
        E = _engine(engine_cls, key)
        E.set_async_phase(on)
        E.fill_data_into_freq_vec().get_candidate_snps().get_fragments().phase()
        E.params = params(key, "P1")
        E.get_candidate_snps().get_fragments().phase()
        r = E.collect_phase(copy=True)
        fm = par.check_fragmat(E, regs)
        par.check_cands(E, regs, phased=True)
        par.check_phase(E, regs, fm)
        s = snapshot(E)
        assert s == _fresh(engine_cls, key, "P1")
        assert (r["cand"].tobytes(), r["cand_region_off"].tobytes()) + tuple(r[k].tobytes() for k in ("haplotag", "assignment", "phase_set", "objective")) == s[:6]
        assert r["row_region_off"].tobytes() == fm["row_region_off"].tobytes()
        E.close()


def seq_errors_midway(engine_cls, orc, key, capfd):
    """frag with min_linkers = 0 (ARG); frag; phase with ld_weight_threshold = 2 (ARG); cand with another dist_to_end (ARG); phase;
    a batch with an unknown CIGAR op (CIGAR at lcr_pileup); the good batch again.  A refused call changes nothing: the good steps == oracle."""
    regs = oracle(orc, key)
    E = _engine(engine_cls, key)
    E.fill_data_into_freq_vec().get_candidate_snps()
    called = E.candidates()[0].tobytes()
    E.params = params(key, min_linkers=0)
    with pytest.raises(LcrError, match=r"lcr_fragments failed \(-1\).*min_linkers"):
        E.get_fragments()
    assert E.candidates()[0].tobytes() == called
    E.params = params(key)
    E.get_fragments()
    fm = par.check_fragmat(E, regs)
    E.params = params(key, ld_weight_threshold=2)
    with pytest.raises(LcrError, match=r"lcr_phase failed \(-1\).*ld_weight_threshold"):
        E.phase()
    assert E.candidates()[0].tobytes() == called and fm_bytes(E.fragmat()) == fm_bytes(fm)
    E.params = params(key, dist_to_end=int(params(key).dist_to_end) + 1)   # (refused in front of the point where lcr_candidates rewinds)
    with pytest.raises(LcrError, match=r"lcr_candidates failed \(-1\).*dist_to_end"):
        E.get_candidate_snps()
    assert E.candidates()[0].tobytes() == called and fm_bytes(E.fragmat()) == fm_bytes(fm)
    E.params = params(key)
    E.phase()
    par.check_cands(E, regs, phased=True)
    par.check_phase(E, regs, fm)
    assert snapshot(E) == _fresh(engine_cls, key, "P0")
    bad = helpers.mk_batch([dict(pos=10, seq="ACGT" * 5, cigar="10M2P10M")], [(0, "A" * 64)])
    E.load_batch(bad)
    with pytest.raises(LcrError, match=r"lcr_pileup failed \(-2\).*CIGAR"):
        E.fill_data_into_freq_vec()
    E.load_batch(batch(key)).fill_data_into_freq_vec()
    par.check_pileup(E, regs, batch(key))
    E.get_candidate_snps()
    assert phase_round(E, regs) == _fresh(engine_cls, key, "P0")
    E.close()


def seq_pileup_twice(engine_cls, orc, key, capfd):
    """pileup P0; cand P0; pileup P0; cand P1; frag; phase == oracle(P1)"""
    assert cand_set(oracle(orc, key, "P1")) != cand_set(oracle(orc, key, "P0"))
    E = _engine(engine_cls, key)
    E.fill_data_into_freq_vec().get_candidate_snps()
    check_called(E, oracle(orc, key))
    E.fill_data_into_freq_vec()
    par.check_pileup(E, oracle(orc, key), batch(key))
    E.params = params(key, "P1")
    E.get_candidate_snps()
    assert phase_round(E, oracle(orc, key, "P1")) == _fresh(engine_cls, key, "P1")
    E.close()


def seq_platform_mismatch(engine_cls, orc, key, capfd):
    """pileup with the ONT preset; cand with another platform or dist_to_end: LCR_E_ARG, nothing changed; cand P0 == oracle"""
    p0 = params(key)
    E = _engine(engine_cls, key)
    E.fill_data_into_freq_vec().get_candidate_snps()
    first = phase_round(E, oracle(orc, key))
    for bad in (params(key, platform=_abi.LCR_PLATFORM_HIFI), params(key, dist_to_end=int(p0.dist_to_end) + 1)):
        E.params = bad
        with pytest.raises(LcrError, match=r"lcr_candidates failed \(-1\).*dist_to_end"):
            E.get_candidate_snps()
        assert snapshot(E) == first
    E.params = p0
    E.get_candidate_snps()
    assert phase_round(E, oracle(orc, key)) == first
    E.close()


def seq_failed_pileup_rewinds(engine_cls, orc, key, capfd):
    """device-resident batch: pileup; cand; frag; one CIGAR word of the caller's tensor gets an unknown op code; pileup fails (CIGAR)
    part of the way through its rewrite of the tile tables and the record pool: the context is back at the loaded batch, and the
    stage calls and getters behind it are refused -- not answered from the previous pass; the word restored: pileup; cand; frag;
    phase == a fresh context's."""
    import torch
    import bench
    regs = oracle(orc, key)
    reads, regions, t = bench.to_device(batch(key), torch, torch.device("cuda", 0))
    E = engine_cls(0, params(key))
    E.load_batch((reads, regions, t))
    E.fill_data_into_freq_vec()
    par.check_pileup(E, regs, batch(key))
    E.get_candidate_snps()
    check_called(E, regs)
    E.get_fragments()
    par.check_fragmat(E, regs)
    E.sync()
    k = int(t["cigar"].numel()) // 2
    good = int(t["cigar"][k])
    t["cigar"][k] = (good & ~15) | 15
    torch.cuda.synchronize()
    with pytest.raises(LcrError, match=r"lcr_pileup failed \(-2\).*CIGAR"):
        E.fill_data_into_freq_vec()
    for call, text in ((E.get_fragments, "lcr_fragments before lcr_candidates"), (E.candidates, "lcr_get_candidates before lcr_candidates"),
                       (E.fragmat, "lcr_get_fragmat before lcr_fragments"), (E.columns, "lcr_get_columns before lcr_pileup")):
        with pytest.raises(LcrError, match=text):
            call()
    t["cigar"][k] = good
    torch.cuda.synchronize()
    E.fill_data_into_freq_vec()
    par.check_pileup(E, regs, batch(key))
    E.get_candidate_snps()
    assert phase_round(E, regs) == _fresh(engine_cls, key, "P0")
    E.close()


SEQUENCES = [
    ("cand_p_p2_p", "cdna21"), ("cand_p_p2_p", "drna22"), ("cand_p_p2_p", "masseq13"),
    ("fuse_switch", "cdna21"), ("fuse_switch", "drna22"),
    ("survivor_guess", "cdna21"), ("survivor_guess", "drna22"),
    ("hist_path_switch", "cdna21"), ("hist_path_switch", "drna22"),
    ("import_then_call", "cdna21"), ("import_then_call", "masseq13"),
    ("rephase", "lowfrac"),
    ("async_reentry", "cdna21"),
    ("errors_midway", "masseq13"),
    ("pileup_twice", "cdna21"), ("pileup_twice", "masseq13"),
    ("platform_mismatch", "cdna21"),
    ("failed_pileup_rewinds", "cdna21"),
]


@pytest.mark.parametrize("seq,key", SEQUENCES, ids=["%s-%s" % s for s in SEQUENCES])
def test_stage_sequence(engine_cls, orc, capfd, seq, key):
    globals()["seq_" + seq](engine_cls, orc, key, capfd)

"""The tally's lean form (-m gpu): from a context's second batch on, on the presets whose filter pass runs in k1_pileup's epilogue, lcr_pileup
stores no plane and no flag -- the pass-1 survivors go to lcr_candidates as staged records (k2_place orders them), and the planes of the tiles
with records are tallied again when somebody asks (planes_tally, lcr_ctx.h).  Checked here: lean against full (lcr_debug_set("lean_planes", 0))
byte for byte and against the oracle, survivors at every tile edge, the planes whenever they are asked for, the fall-back when the staging
buffer is too small, the readers that need planes behind a lean pileup, and the stage's byte accounting.

A context's first batch has no survivor guess and takes the full form, so every case primes its context with a batch first; that the next
pileup really took the lean form is read off lcr_pileup_stage_bytes (the two forms' formulas differ: took_lean_form)."""
import numpy as np
import pytest

import column_cases as cc
import test_gpu_parity as par
import test_import_candidates_gpu as imp
import test_sparse_planes as sp
from longcallr_amd import _abi
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu

PROFILE = "ont-cdna"
SV_BYTES = 48      # sizeof(Survivor), lcr_dev.h
# rules of pass 1 (k2_eval.h: candidate.rs:90-234 without the base-quality rule) as oracle_np.candidates names them
PASS1_DROPS = ("min_depth", "max_depth", "ref_base", "low_frac", "low_cnt", "deletion", "af_intron", "sor", "binomial", "one_strand")


def base_bytes(b):
    """B + 4 C + 37 R + L: what both forms of the stage move beside the planes / the staged survivors"""
    return int(b.bases.size) + 4 * int(b.cigar.size) + 37 * int(b.n_reads) + int(np.sum(b.len))


def full_bytes(b, p):
    has = sp.tiles_with_records(b, p)
    cols = sum(int(np.minimum(sp.TILE, int(b.len[g]) - np.flatnonzero(h) * sp.TILE).sum()) for g, h in enumerate(has))
    return base_bytes(b) + 4 * _abi.NPLANES * cols


def took_lean_form(E, b, p):
    """the last lcr_pileup stored survivors, not planes: 48 S' <= 48 L'' < 52 L'', so the full form's figure is never a lean one"""
    got = E.pileup_stage_bytes()
    assert (got - base_bytes(b)) % SV_BYTES == 0 or got == full_bytes(b, p)
    return got != full_bytes(b, p)


def pass1_bounds(b, p):
    """(lo, hi) pass-1 survivors of the batch, counted on the CPU from the Python oracle's trace.  The oracle applies the base-quality
    rule in front of the strand rules, pass 1 does not have it: a column it drops for base quality may or may not survive pass 1 -- it
    counts in hi only."""
    lo = hi = 0
    for g in range(b.n_regions):
        trace = {}
        onp.candidates(onp.pileup(b, g, p), int(b.start0[g]), p, trace)
        why = [trace.get(c, "record") for c in range(int(b.len[g]))]
        hi += sum(w not in PASS1_DROPS for w in why)
        lo += sum(w not in PASS1_DROPS and w != "baseq" for w in why)
    return lo, hi


def all_results(E):
    """candidates, offsets, fragment matrix, phase results -- not the planes (the getter would tally them)"""
    c, off = E.candidates()
    pr, fm = E.phase_result(), E.fragmat()
    out = {"cand": c.tobytes(), "cand_off": off.tobytes()}
    out.update({"phase." + k: pr[k].tobytes() for k in ("haplotag", "assignment", "phase_set", "objective")})
    out.update({"fm." + k: fm[k].tobytes() for k in sorted(fm)})
    return out


def check_stages(E, regs):
    """candidates, fragment matrix and phase results of the stages already run, against the oracle"""
    fm = par.check_fragmat(E, regs)
    par.check_cands(E, regs, phased=True)
    par.check_phase(E, regs, fm)


def stages(E):
    E.get_candidate_snps().get_fragments().phase()
    return E


# ---- lean against full ---------------------------------------------------------------------------------------------------------------

def test_lean_and_full_forms_agree(engine_cls, orc):
    """a second batch on one context with lean_planes 1 against 0: every stage's results byte for byte the same and the oracle's; the lean
    side twice -- the order the tiles drew their staging slots in must not show"""
    b, p = sp.batch_of(PROFILE), sp.params_of(PROFILE)
    regs = sp.oracle_of(orc, PROFILE, "post")
    got = {}
    for lean in (1, 0):
        E = engine_cls(0, p)
        E.debug_set("lean_planes", lean)
        E.load_batch(b).run_all()                       # (no guess yet: the full form)
        assert not took_lean_form(E, b, p)
        runs = []
        for _ in range(2 if lean else 1):
            E.load_batch(b).run_all()
            assert took_lean_form(E, b, p) == bool(lean)
            check_stages(E, regs)
            runs.append(all_results(E))
        par.check_pileup(E, regs, b)
        got[lean] = runs
        E.close()
    sp.assert_same(got[1][0], got[1][1], "lean twice")
    sp.assert_same(got[1][0], got[0][0], "lean against full")


# ---- where a survivor sits -----------------------------------------------------------------------------------------------------------

EDGES = (0, 255, 256, 511, 512, 599)     # first / last column of a tile, both sides of both borders, the last column of the partial last tile


def edge_cases():
    """two regions of 600 columns (tiles of 256, 256 and 88) with a het at every EDGES column, between them a region of one tile whose only
    design column falls to low_frac: records, no survivor"""
    hets = [cc._het(x) for x in EDGES]
    quiet = cc.split(100, "C", {"C": 20}, "low_frac")
    return [cc.case("edges_a", hets, length=600), cc.case("records_no_survivor", quiet, length=200), cc.case("edges_b", hets, length=600)]


def test_survivors_at_the_tile_edges(engine_cls, orc):
    cases = edge_cases()
    b, p = cc.build(cases), cc.params(PROFILE, {})
    assert sp.TILE == 256 and pass1_bounds(b, p) == (2 * len(EDGES), 2 * len(EDGES))
    regs = par.oracle_all(orc, b, p)
    assert [len(R.cands()) for R in regs] == [len(EDGES), 0, len(EDGES)]
    for R in (regs[0], regs[2]):
        assert (R.cands()["pos"] - R.cands()["pos"][0]).tolist() == list(EDGES)
    E = engine_cls(0, p)
    E.debug_set("poison_planes", 1)
    E.load_batch(b).run_all()
    for _ in range(2):
        E.load_batch(b).run_all()
        assert took_lean_form(E, b, p)
        check_stages(E, regs)
    par.check_pileup(E, regs, b)
    E.close()


# ---- planes on request ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("poison", [0, 1])
def test_planes_on_request_after_a_lean_pileup(engine_cls, orc, poison):
    """lcr_get_columns == the oracle's planes bit for bit: right after the lean pileup, twice in a row, only after candidates, fragments
    and phase -- whose results are the oracle's with the planes tallied in front of them or behind them"""
    b, p = sp.batch_of(PROFILE), sp.params_of(PROFILE)
    regs = sp.oracle_of(orc, PROFILE, "post")
    E = engine_cls(0, p)
    E.debug_set("poison_planes", poison)
    E.load_batch(b).run_all()
    E.load_batch(b).fill_data_into_freq_vec()
    assert took_lean_form(E, b, p)
    par.check_pileup(E, regs, b)                        # right after the pileup
    par.check_pileup(E, regs, b)                        # twice in a row
    check_stages(stages(E), regs)                       # the staged survivors behind a tally of the planes
    par.check_pileup(E, regs, b)
    E.load_batch(b).fill_data_into_freq_vec()
    assert took_lean_form(E, b, p)
    check_stages(stages(E), regs)
    par.check_pileup(E, regs, b)                        # only after the three stages behind the pileup
    par.check_pileup(E, regs, b)
    E.close()


# ---- overflow of the staging buffer --------------------------------------------------------------------------------------------------

def test_more_survivors_than_the_staging_holds(engine_cls, orc):
    """batch A leaves a guess of a + a / 4 + 64 survivors (lcr_calls.hip); B has more: its lean tally drops what does not fit, and
    lcr_candidates falls back on the full fused form and k2_compact.  B's results are the oracle's, and so are those of a third batch,
    staged with a guess that holds.  A and B are chosen by the oracle's pass-1 count, on the CPU."""
    (over, cases), = cc.groups(cc.all_families(orc)["place"])
    A, B, p = cc.build(cases[:1]), cc.build(cases), cc.params(PROFILE, over)
    (a_lo, a_hi), (b_lo, b_hi) = pass1_bounds(A, p), pass1_bounds(B, p)
    assert a_lo == a_hi and b_lo > a_hi + a_hi // 4 + 64
    regs = par.oracle_all(orc, B, p)
    E = engine_cls(0, p)
    E.debug_set("poison_planes", 1)
    E.load_batch(A).run_all()
    E.load_batch(B).fill_data_into_freq_vec()
    assert took_lean_form(E, B, p)
    assert E.pileup_stage_bytes() == base_bytes(B) + SV_BYTES * (a_hi + a_hi // 4 + 64)    # (the staging was filled to its capacity)
    check_stages(stages(E), regs)                       # guess exceeded
    par.check_pileup(E, regs, B)
    E.load_batch(B).run_all()                           # guess holds
    assert took_lean_form(E, B, p) and E.pileup_stage_bytes() == base_bytes(B) + SV_BYTES * b_hi == base_bytes(B) + SV_BYTES * b_lo
    check_stages(E, regs)
    par.check_pileup(E, regs, B)
    E.close()


# ---- readers that need planes --------------------------------------------------------------------------------------------------------

def test_import_after_a_lean_pileup(engine_cls, orc):
    """lcr_import_candidates behind a lean pileup, at sites inside tiles with records and inside record-free tiles (poisoned planes):
    the oracle's import and its phasing; lcr_candidates then still finds its staged survivors"""
    b, p = sp.batch_of(PROFILE, n_genes=6), sp.params_of(PROFILE, max_enum_snps=6)
    has = sp.tiles_with_records(b, p)
    rng = np.random.default_rng(11)
    pos, n_free, n_cov = [], 0, 0
    for g in range(b.n_regions):
        s0, L = int(b.start0[g]), int(b.len[g])
        depth = orc.Region(b, g, p).pileup().planes()[:4].sum(axis=0)
        free = np.flatnonzero(~has[g])
        for t in rng.choice(free, size=min(8, free.size), replace=False).tolist():
            pos.append(s0 + min(t * sp.TILE + int(rng.integers(0, sp.TILE)), L - 1))
            n_free += 1
        cov = np.flatnonzero(depth >= 8)
        pick = rng.choice(cov, size=min(8, cov.size), replace=False)
        pos += (s0 + pick).tolist()
        n_cov += pick.size
    assert n_free >= 8 and n_cov >= 8
    pos = np.unique(np.array(pos, np.int64))
    gt = np.where(np.arange(pos.size) % 5 == 4, 2, 1).astype(np.uint8)
    qual = np.full(pos.size, 30.0, np.float32)
    regs = par.oracle_all(orc, b, p)
    E = engine_cls(0, p)
    E.debug_set("poison_planes", 1)
    E.load_batch(b).run_all()
    E.load_batch(b).fill_data_into_freq_vec()
    assert took_lean_form(E, b, p)
    E.import_external_candidates(pos, gt, qual)
    cands, off = E.candidates()
    imp.check_records(cands, off, imp.expected_import(orc, b, p, pos, gt, qual), b.n_regions)
    assert (cands["depth"] >= 8).sum() >= n_cov
    E.get_fragments().phase()
    imp.check_downstream(E, b, p, cands, off)
    check_stages(stages(E), regs)                       # the regular candidate stage on the same pileup
    par.check_pileup(E, regs, b)
    E.close()


def test_other_filter_parameters_after_a_lean_pileup(engine_cls, orc):
    """lcr_candidates with another min_depth than the pileup's: the staged survivors do not apply, k2_filter needs the planes; then the
    pileup's own parameters again on the same pileup (k2_filter once more: the staged records are gone), each against the oracle"""
    b, p = sp.batch_of(PROFILE, n_genes=8), sp.params_of(PROFILE)
    p2 = sp.params_of(PROFILE, min_depth=int(p.min_depth) + 6)
    regs, regs2 = par.oracle_all(orc, b, p), par.oracle_all(orc, b, p2)
    assert sum(len(R.cands()) for R in regs2) < sum(len(R.cands()) for R in regs)
    E = engine_cls(0, p)
    E.debug_set("poison_planes", 1)
    E.load_batch(b).run_all()
    E.load_batch(b).fill_data_into_freq_vec()
    assert took_lean_form(E, b, p)
    E.params = p2
    check_stages(stages(E), regs2)
    E.params = p
    check_stages(stages(E), regs)
    par.check_pileup(E, regs, b)
    E.close()


# ---- byte accounting -----------------------------------------------------------------------------------------------------------------

def test_stage_bytes_of_both_forms(engine_cls, orc):
    """lean: lcr_pileup_stage_bytes = B + 4 C + 37 R + L + 48 S' (S' staged survivors: here all of pass 1's, counted by the oracle on
    the CPU); full: ... + 52 L'' as before; tallying the planes for a getter changes neither"""
    cases = edge_cases()
    b, p = cc.build(cases), cc.params(PROFILE, {})
    lo, hi = pass1_bounds(b, p)
    assert lo == hi == 2 * len(EDGES)
    regs = par.oracle_all(orc, b, p, upto="pileup")
    E = engine_cls(0, p)
    E.load_batch(b).fill_data_into_freq_vec()
    assert E.pileup_stage_bytes() == full_bytes(b, p)
    stages(E)
    assert E.pileup_stage_bytes() == full_bytes(b, p)
    for ask_first in (True, False):                     # the count read by the getter itself / left by lcr_candidates
        E.load_batch(b).fill_data_into_freq_vec()
        if not ask_first:
            E.get_candidate_snps()
        assert E.pileup_stage_bytes() == base_bytes(b) + SV_BYTES * hi
        par.check_pileup(E, regs, b)
        assert E.pileup_stage_bytes() == base_bytes(b) + SV_BYTES * hi
    E.debug_set("lean_planes", 0)
    E.load_batch(b).fill_data_into_freq_vec()
    assert E.pileup_stage_bytes() == full_bytes(b, p)
    par.check_pileup(E, regs, b)
    assert E.pileup_stage_bytes() == full_bytes(b, p)
    E.close()

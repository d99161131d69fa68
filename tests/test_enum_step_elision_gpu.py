"""Step elision in the enumeration restarts (lcr_debug_set("enum_elide"), default 1): k4_enum_bits and k4_enum_reg do not execute a sigma
step behind unchanged (delta, eta) or a delta / eta step behind an unchanged sigma.  A skipped step must leave exactly what the executed one
would have left -- results AND tie census (the reference executes those steps and the oracle counts their ties), so every case compares
enum_elide = 1 with enum_elide = 0 byte for byte, and the default with the oracle."""
import functools

import numpy as np
import pytest

import helpers
from longcallr_amd import _abi, synth
from test_gpu_parity import _result_bytes, full_check, oracle_all  # noqa: F401  (oracle_all: full_check's reference)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "ont-cdna":
        return synth.make_batch("ont-cdna", n_genes=10, gene_len=16000, depth=40, seed=7), _abi.make_params("ont-cdna", seed=2025)
    seed = {"masseq-2": 2, "masseq-1": 1}[name]   # masseq-1: the tie-only-steps batch of test_tie_only_steps_take_the_repair_pass
    return synth.make_batch("masseq", n_genes=12, gene_len=16000, depth=40, seed=seed), _abi.make_params("hifi-masseq", seed=2025)


CASES = ["ont-cdna", "masseq-2", "masseq-1"]


def _run(engine_cls, b, p, elide, stream=0):
    E = engine_cls(0, p)
    E.debug_set("enum_elide", elide)
    E.debug_set("enum_force_stream", stream)
    E.load_batch(b).run_all()
    got = (_result_bytes(E), dict(E.tie_census()))
    E.close()
    return got


@pytest.mark.parametrize("name", CASES)
def test_on_off_and_kernel_class(engine_cls, name):
    """enum_elide 0 / 1 x enum_force_stream 0 / 1: one result, one census.  sigma_f64 (all batches) and delta_step_f64 (the tie-only-steps
    batch) are the counters a wrong skip would move."""
    b, p = _case(name)
    runs = {(el, st): _run(engine_cls, b, p, el, st) for el in (0, 1) for st in (0, 1)}
    ref = runs[(0, 0)]
    for k, got in runs.items():
        assert got[0] == ref[0], "results differ: (enum_elide, enum_force_stream) = %s" % (k,)
        assert got[1] == ref[1], (k, got[1], ref[1])
    hc = ref[1]
    assert hc["sigma_f64"] > 0
    if name == "masseq-1":
        assert hc["delta_step_f64"] >= 10 and hc["step_unresolved"] == 0 and hc["delta_unresolved"] == 0, hc


@pytest.mark.parametrize("name", CASES)
def test_default_against_the_oracle(engine_cls, orc, name):
    b, p = _case(name)
    full_check(engine_cls, orc, b, p)


def _one_snp_batch(n_reads):
    """helpers.two_haplotype_batch spaces its sites by (n_snps - 1) and cannot make one site: the same instance with a single het site (error-
    free reads of two haplotypes over one stretch of 2 kb, alt on haplotype A only, every read covers the stretch)."""
    rng = np.random.default_rng(0)
    span = 2000
    ref = "".join(rng.choice(list("ACGT"), size=span))
    alt_of = {"A": "C", "C": "A", "G": "T", "T": "G"}
    x = 100
    reads = []
    for k in range(n_reads):
        s = list(ref)
        if k % 2 == 0:
            s[x] = alt_of[ref[x]]
        reads.append(dict(pos=5000, seq="".join(s), qual=30, cigar="%dM" % span, rev=k // 2 % 2, ts=1 + (k // 2 % 2), region=0))
    return helpers.mk_batch(reads, [(5000, ref)])


@pytest.mark.parametrize("n_snps", [1, 2, 3])
def test_partial_groups(engine_cls, orc, n_snps):
    """2, 4 and 8 restarts: fewer states than a wave's eight, and exactly eight."""
    b = _one_snp_batch(60) if n_snps == 1 else helpers.two_haplotype_batch(n_snps=n_snps, n_reads=60)[0]
    p = _abi.make_params("hifi-masseq", seed=9)
    c = full_check(engine_cls, orc, b, p)
    assert len(c) == n_snps
    for stream in (0, 1):
        assert _run(engine_cls, b, p, 1, stream) == _run(engine_cls, b, p, 0, stream)


@pytest.mark.parametrize("tie_arith", ["1", "2"])
def test_tie_arith_levels(engine_cls, monkeypatch, tie_arith):
    """Below level 3 the delta census is not taken by the repair list, below level 2 the sigma census goes to sigma_unresolved: a skipped step
    counts into the same slots.  (Which slot is not empty follows from the first sigma step, the same at every level.)"""
    monkeypatch.setenv("LCR_TIE_ARITH", tie_arith)
    b, p = _case("ont-cdna")
    for stream in (0, 1):
        on, off = _run(engine_cls, b, p, 1, stream), _run(engine_cls, b, p, 0, stream)
        assert on[0] == off[0]
        assert on[1] == off[1], (on[1], off[1])
        if tie_arith == "1":
            assert on[1]["sigma_unresolved"] > 0 and on[1]["sigma_f64"] == 0
        else:
            assert on[1]["sigma_f64"] > 0 and on[1]["sigma_unresolved"] == 0

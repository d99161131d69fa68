"""The column recipes of tests/column_cases.py on the CPU: both restatements of the candidate filters (C++ oracle, oracle_np) agree
record for record on every case, every design column ends where its case says -- by oracle_np's trace and by the C++ oracle's records
--, and the cases together stand on both sides of every threshold.  The last is a condition on the INPUTS of
test_candidate_boundaries_gpu.py: without it that test could pass while testing nothing."""
import functools

import numpy as np
import pytest

import column_cases as cc
from longcallr_amd import _abi
from oracle import oracle_np
from test_oracle_np import _compare_region

FAMILIES = ["depth", "depth200", "quotient", "deletion", "allele", "strand", "baseq", "classes", "dense", "place"]
KIND_FLAG = dict(edit=_abi.F_RNA_EDIT, somatic=_abi.F_CAND_SOMATIC, hom=_abi.F_HOM, het=_abi.F_HET)


def matches(reason, want):
    if want == "kept":
        return "/" in reason
    return reason == want or reason.startswith(want + "/")


@functools.lru_cache(maxsize=None)
def run_family(orc, family):
    """[(case, {design column: reason}, C++ oracle's records of the region)]"""
    out = []
    for over, cases in cc.groups(cc.all_families(orc)[family]):
        b = cc.build(cases)
        for g, c in enumerate(cases):
            prm = cc.params(c["preset"], over)
            _compare_region(orc, b, g, prm)
            trace = {}
            oracle_np.candidates(oracle_np.pileup(b, g, prm), int(b.start0[g]), prm, trace=trace)
            rec = orc.Region(b, g, prm).pileup().candidates().cands()
            out.append((c, trace, rec, int(b.start0[g])))
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_cases_end_where_they_were_designed_to(orc, family):
    for c, trace, rec, start0 in run_family(orc, family):
        at = {x["at"]: x for x in c["columns"]}
        by_pos = {int(r["pos"]) - start0: r for r in rec}
        assert set(by_pos) <= set(at), "%s: a record beside the design columns" % c["name"]
        assert all("/" not in why for k, why in trace.items() if k not in at), c["name"]
        for k, x in at.items():
            why = trace.get(k)
            assert why is not None and matches(why, x["want"]), "%s column %d: designed for %s, oracle_np says %s" % (c["name"], k, x["want"], why)
            assert ("/" in why) == (k in by_pos), "%s column %d: %s, C++ oracle %s" % (c["name"], k, why, "keeps it" if k in by_pos else "drops it")
            if k in by_pos:
                kind, vt, _ = why.split("/")
                r = by_pos[k]
                assert r["flags"] & KIND_FLAG[kind] and int(r["variant_type"]) == int(vt), "%s column %d" % (c["name"], k)
                assert bool(r["flags"] & _abi.F_DENSE) == x["dense"], "%s column %d: dense" % (c["name"], k)
                if kind in ("het", "hom"):
                    assert bool(r["flags"] & _abi.F_FOR_PHASING) == (not x["dense"])


def test_strand_bias_tuples_qualify(orc):
    """what the issue asks of the census tuples, and that the two restatements give one verdict on each"""
    cases = [c for c in cc.all_families(orc)["strand"] if c["name"].startswith(("sb_near", "sb_above", "sb_below"))]
    tuples = [cc.tuple_of(c) for c in cases]
    assert len(set(tuples)) == len(tuples) and all(cc.ratio_decides(t, c["name"].startswith("sb_near")) for t, c in zip(tuples, cases))
    t, sor, thr, ulp = cc.census(orc)
    assert len(t) == 646249
    near = {tuple(int(v) for v in x) for x in t[np.abs(ulp) <= 3]}
    n_near = [tp for tp, c in zip(tuples, cases) if c["name"].startswith("sb_near")]
    assert len(n_near) >= 24 and set(n_near) <= near
    # the listed tuples all sit on the threshold, and so does every tuple at which this process's NumPy float32 log decides otherwise
    # than the C++ oracle (which tuples those are depends on the NumPy build's log kernel: the list is the one the docstrings quote)
    assert len(cc.NP_LOG_DISAGREED) == 18 and set(cc.NP_LOG_DISAGREED) <= near and set(cc.numpy_log_disagreements(orc)) <= near
    first = [x for x in cc.NP_LOG_DISAGREED if cc.ratio_decides(x)]
    assert n_near[:len(first)] == first and len(first) >= 5
    thr_np = oracle_np.strand_odds_ratio(5, 5, 9, 1)
    for name, want in (("sb_above", False), ("sb_below", True)):
        sel = [tp for tp, c in zip(tuples, cases) if c["name"].startswith(name)]
        assert len(sel) >= 6
        for tp in sel:
            v = oracle_np.strand_odds_ratio(*tp)
            assert (not v > thr_np) == want and abs(float(v) - float(thr_np)) > 0.25, tp     # clearly: 2e6 ulp away
    for tp in tuples:
        assert cc.census_verdict(orc, tp) == (not oracle_np.strand_odds_ratio(*tp) > thr_np), tp


def test_ledger_is_complete(orc):
    """every rule and kind on both sides of its threshold: the probes the cases declare cover cc.LEDGER, a case stands where it
    declares (its design columns ended as designed: the test above), and every reason of cc.REASONS was recorded at a design column"""
    probes, reasons, names = set(), set(), set()
    for family in FAMILIES:
        for c, trace, rec, _ in run_family(orc, family):
            assert c["name"] not in names, c["name"]
            names.add(c["name"])
            probes.update(c["probes"])
            reasons.update(trace[x["at"]] for x in c["columns"])
            for rule, side in c["probes"]:
                if side == "drop" and rule in cc.REASONS:
                    assert any(trace[x["at"]] == rule for x in c["columns"]), c["name"]
                if side == "pass" and rule in cc.REASONS:
                    assert all(trace[x["at"]] != rule for x in c["columns"]), c["name"]
    assert not set(cc.LEDGER) - probes, sorted(set(cc.LEDGER) - probes)
    assert not set(cc.REASONS) - reasons, sorted(set(cc.REASONS) - reasons)
    dense = [x["dense"] for family in ("dense", "place") for c, _, _, _ in run_family(orc, family) for x in c["columns"]]
    assert any(dense) and not all(dense)

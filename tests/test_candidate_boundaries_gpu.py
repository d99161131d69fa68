"""The column recipes of tests/column_cases.py in front of the kernels: every case batch through each way the candidate stage can take,
against the C++ oracle under test_gpu_parity.full_check's bars (planes, candidates, fragments, phasing, VCF text; no tolerance of its
own).  tests/test_candidate_boundaries.py shows on the CPU that the cases stand on both sides of every threshold.

  hifi-isoseq, hifi-masseq   k2_filter's pass over the planes, the read walk's histograms (k2_hist: the tile form is for the ONT presets)
  ont-cdna, ont-drna         the filter in k1_pileup's epilogue (default), fuse_filter = 0 (k2_filter), hist_tiles = 1 against -1
                             (k2_hist_tiles against k2_hist) -- the forms of one preset byte for byte the same
  spec_compact               a context's first batch never speculates (no survivor count to guess from), so the placement batch runs on
                             one context behind a smaller batch (guess exceeded: the compaction drops what does not fit and runs
                             again) and once more (guess holds), against spec_compact = 0 (test_where_a_survivor_sits)"""
import numpy as np
import pytest

import column_cases as cc
import test_gpu_parity as par

pytestmark = pytest.mark.gpu
FORMS = [("fuse_filter", 0), ("hist_tiles", 1), ("hist_tiles", -1)]


def result_bytes(engine_cls, b, p, switch=None):
    E = engine_cls(0, p)
    if switch:
        E.debug_set(*switch)
    E.load_batch(b).run_all()
    out = par._result_bytes(E)
    E.close()
    return out


def every_way(engine_cls, orc, family):
    assert cc.all_families(orc)[family]
    for over, cases in cc.groups(cc.all_families(orc)[family]):
        b = cc.build(cases)
        for preset in ("hifi-isoseq", "hifi-masseq", "ont-cdna", "ont-drna"):
            p = cc.params(preset, over)
            try:
                par.full_check(engine_cls, orc, b, p)
            except AssertionError as e:   # (full_check speaks of region numbers: name the cases)
                raise AssertionError("%s under %s %s: %s -- regions: %s" % (family, preset, over, e, ", ".join(
                    "%d %s" % (g, c["name"]) for g, c in enumerate(cases)))) from e
            if preset.startswith("ont"):
                want = result_bytes(engine_cls, b, p)
                for switch in FORMS:
                    assert result_bytes(engine_cls, b, p, switch) == want, "%s %s: %s = %d against the default form" % ((family, preset) + switch)


@pytest.mark.parametrize("family", ["depth", "depth200", "quotient", "deletion", "allele", "baseq", "classes", "dense"])
def test_family(engine_cls, orc, family):
    every_way(engine_cls, orc, family)


def test_where_a_survivor_sits(engine_cls, orc):
    every_way(engine_cls, orc, "place")
    (over, cases), = cc.groups(cc.all_families(orc)["place"])
    small, b = cc.build(cases[:1]), cc.build(cases)
    for preset in ("hifi-masseq", "ont-cdna"):
        p = cc.params(preset, over)
        want = result_bytes(engine_cls, b, p, ("spec_compact", 0))
        E = engine_cls(0, p)
        E.load_batch(small).run_all()
        # every column beside the design columns has no alt base and falls to low_frac in pass 1: the small batch leaves 5 survivors, so a
        # guess of 5 + 5 / 4 + 64 (lcr_calls.hip), and the whole batch has 523
        assert E.candidates()[0].size == len(cases[0]["columns"]) == 5
        for turn in ("guess exceeded", "guess holds"):
            E.load_batch(b).run_all()
            assert E.candidates()[0].size == sum(len(c["columns"]) for c in cases) > 70
            assert par._result_bytes(E) == want, "%s, %s" % (preset, turn)
        E.close()


def test_strand_bias(engine_cls, orc):
    """... and per census tuple: its region holds a record exactly where the C++ oracle's strand-odds-ratio verdict passes it"""
    every_way(engine_cls, orc, "strand")
    checked = 0
    (over, cases), = cc.groups(cc.all_families(orc)["strand"])
    b = cc.build(cases)
    for preset in ("hifi-isoseq", "ont-cdna"):    # use_strand_bias = 1
        E = engine_cls(0, cc.params(preset, over))
        E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps()
        have = set(int(g) for g in E.candidates()[0]["region"])
        E.close()
        for g, case in enumerate(cases):
            if case["name"].startswith(("sb_near", "sb_above", "sb_below")):
                t = cc.tuple_of(case)
                assert (g in have) == cc.census_verdict(orc, t), "%s: (ref_fw, ref_rv, alt_fw, alt_rv) = %s" % (preset, t)
                checked += 1
    assert checked >= 2 * (24 + 6 + 6)


def test_strand_bias_census_on_the_threshold(engine_cls, orc):
    """every census tuple within 3 ulp of the threshold whose column becomes a record exactly when the ratio passes (cc.ratio_decides
    without the condition on the reference strands: 216 with glibc's logf), a region each: the device's logf gives the C++ oracle's verdict"""
    t, _, _, ulp = cc.census(orc)
    tuples = [x for x in (tuple(int(v) for v in x) for x in t[np.abs(ulp) <= 3]) if cc.ratio_decides(x, skewed_ref=False)]
    assert len(tuples) >= 100
    b = cc.build([cc.tuple_case(x, "on") for x in tuples])
    want = [cc.census_verdict(orc, x) for x in tuples]
    for preset in ("hifi-isoseq", "ont-cdna"):
        E = engine_cls(0, cc.params(preset, {}))
        E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps()
        have = (np.diff(E.candidates()[1]) > 0).tolist()
        E.close()
        differ = [x for x, h, w in zip(tuples, have, want) if h != w]
        assert not differ, "%s: the device decides otherwise at (ref_fw, ref_rv, alt_fw, alt_rv) = %s" % (preset, differ)

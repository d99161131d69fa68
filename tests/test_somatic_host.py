"""The host side of lcr_somatic without a GPU: the record's layout against the header, the rounding of the fixed-point tables, the
fixed-point model against the reference's product form (tests/somatic_ref.py), the depth at which only the log domain still answers, the
contract's worked instance and its LCR_SOM_DEEP / LCR_SOM_ALLELES branches through the restatement, somatic.format_vcf_records on
hand-made records, and the command line's refusals."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import somatic_ref as ref
from longcallr_amd import _abi, _lib, somatic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PURITIES = (0.3, 0.1, 0.5, 1.0)
A, C_, G, T = 0, 1, 2, 3


def test_struct_layout_matches_the_header(tmp_path):
    names = ["phase_set", "n", "n_other", "n_lowq", "cls", "call", "status", "L"]
    pnames = ["purity", "som_rate", "het_rate", "min_baseq", "pad_"]
    src = tmp_path / "som.c"
    src.write_text('#include "lcr.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %d %d %d",sizeof(lcr_somatic_site),'
                   'sizeof(lcr_somatic_params),sizeof(((lcr_somatic_site*)0)->n),sizeof(((lcr_somatic_site*)0)->L),LCR_SOM_OK,LCR_SOM_ALLELES,LCR_SOM_DEEP);'
                   + "".join('printf(" %%zu",offsetof(lcr_somatic_site,%s));' % f for f in names)
                   + "".join('printf(" %%zu",offsetof(lcr_somatic_params,%s));' % f for f in pnames) + 'printf("\\n");return 0;}')
    exe = tmp_path / "som"
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = [int(x) for x in os.popen(str(exe)).read().split()]
    want = ([_abi.SOMATIC_SITE_DTYPE.itemsize, C.sizeof(_abi.LcrSomaticParams), 16, 48, somatic.SOM_OK, somatic.SOM_ALLELES, somatic.SOM_DEEP]
            + [_abi.SOMATIC_SITE_DTYPE.fields[f][1] for f in names] + [getattr(_abi.LcrSomaticParams, f).offset for f in pnames])
    assert got == want and got[0] == 80 and got[1] == 32
    assert _abi.SOMATIC_SITE_DTYPE.fields["n"][0].shape == (2, 2) and _abi.SOMATIC_SITE_DTYPE.fields["L"][0].shape == (2, 3)
    assert {"lcr_somatic", "lcr_get_somatic", "lcr_somatic_ms"} <= set(_lib.SYMBOLS)


@pytest.mark.parametrize("purity", PURITIES)
def test_table_rounding_cannot_depend_on_the_mode(purity):
    """llround(log10(x) * 2^40) of the 124 table entries and the three priors: no product lies within 1e-6 of a half, so every rounding
    to nearest agrees (tests/test_haplotag_host.py's argument, here for the purity-dependent tables and the priors too)"""
    args, pri = somatic.table_arguments(purity)
    assert len(args) == 124 and len(pri) == 3
    fr = []
    for x in args + pri:
        y = abs(math.log10(x) * somatic.FX)
        fr.append(abs(y - math.floor(y) - 0.5))
    print("purity %g: nearest product to a half: %.3g (tables), %.3g (priors)" % (purity, min(fr[:124]), min(fr[124:])))
    assert min(fr) > 1e-6
    t = somatic.tables(purity)
    assert t["fe"][0] == t["fe"][1] and t["f1e"][0] == t["f1e"][1] and t["fs_ref"][0] == t["fs_ref"][1] and t["fs_alt"][0] == t["fs_alt"][1]
    assert (t["fe"][30], t["f1e"][30]) == (-3298534883328, -477750748)          # the phase stage's own entries (HostLut)
    assert all(abs(x) < 1 << 42 for k in ("fe", "f1e", "fs_ref", "fs_alt") for x in t[k])      # the premise of the depth bound
    assert t["prior"] == [somatic._llround(math.log10(x) * somatic.FX) for x in (1.0 - 5e-4 - 5e-6, 5e-4, 5e-6)]


def draws(purity):
    """20 000 shallow haplotypes: 0 - 30 reference and 0 - 12 alternate qualities in 1 .. 30"""
    rng = np.random.default_rng(20261020 + int(round(purity * 10)))
    for _ in range(20000):
        n_ref, n_alt = int(rng.integers(0, 31)), int(rng.integers(0, 13))
        yield [int(q) for q in rng.integers(1, 31, size=n_ref)], [int(q) for q in rng.integers(1, 31, size=n_alt)]


@pytest.mark.parametrize("purity", PURITIES)
def test_fixed_point_model_against_the_product_form(purity):
    """Classes equal wherever the two largest L differ by more than 1e-9 (in log10 units); |SQ_fixed - SQ_product| <= 1e-6 wherever the
    product form's score is finite and <= 60.  The bound: at most 43 table terms, each off by <= 2^-41, give |dl| < 2e-11 and |dSQ| <
    1e-9; the product form's own cancellation at 1 - p >= 1e-6 adds less than 1e-9; the rest of 1e-6 is margin for libm.  Draws whose
    product score is infinite or above 60 are skipped for the score -- at most 30 % of them at purity 0.3, 0.1 and 0.5; at purity 1.0 the
    somatic and the heterozygous model coincide up to the prior, and only the classes are asserted."""
    t = somatic.tables(purity)
    worst, skipped, n, near_ties = 0.0, 0, 0, 0
    for ref_qs, alt_qs in draws(purity):
        n += 1
        L = ref.haplotype_sums(ref_qs, alt_qs, t)
        cls_p, _, p_som = ref.product_form(ref_qs, alt_qs, purity)
        top = sorted(L)
        if (top[2] - top[1]) / somatic.FX > 1e-9:
            assert ref.classes(*L) == cls_p, (ref_qs, alt_qs)
        else:
            near_ties += 1
        if purity == 1.0:
            continue
        sq_p = ref.product_score(p_som)
        if not math.isfinite(sq_p) or sq_p > 60.0:
            skipped += 1
            continue
        worst = max(worst, abs(somatic.score_of(*L) - sq_p))
    print("purity %g: %d draws, %d skipped for the score (%.1f %%), %d near ties, worst |dSQ| %.3g" % (purity, n, skipped, 100.0 * skipped / n, near_ties, worst))
    assert n == 20000 and worst <= 1e-6
    if purity != 1.0:
        assert skipped <= 0.30 * n


def test_depth_is_the_reason_for_the_log_domain():
    """5 000 alternate reads at q30 on one haplotype: the fixed-point sums stay exact and give class 2 or 1 and a finite score.  The
    reference's f64 products underflow there ((10^-3)^n is 0 from n = 108 on): on this haplotype the reference and the somatic product are
    0 exactly and only (1 - eps)^5000 survives, so the product form still answers "het, probability exactly 1" -- it does NOT yield NaN
    on an all-alternate haplotype, as the request for this test assumed.  NaN is what it yields as soon as no product survives: a mosaic
    haplotype of 3 500 reference and 1 500 alternate reads -- the very case the stage is for -- is 0 / 0, class 0 by fall-through."""
    alt = [30] * 5000
    L = ref.haplotype_sums([], alt, somatic.tables(0.3))
    assert ref.classes(*L) in (1, 2) and math.isfinite(somatic.score_of(*L))
    cls_p, prob, p_som = ref.product_form([], alt, 0.3)
    assert (cls_p, prob, p_som) == (1, 1.0, 0.0) and ref.classes(*L) == 1
    assert math.pow(1e-3, 107) > 0.0 and math.pow(1e-3, 108) == 0.0
    cls_p, prob, p_som = ref.product_form([30] * 3500, [30] * 1500, 0.3)
    assert math.isnan(prob) and math.isnan(p_som) and cls_p == 0
    L = ref.haplotype_sums([30] * 3500, [30] * 1500, somatic.tables(0.3))
    assert ref.classes(*L) == 2 and somatic.score_of(*L) > 1000.0 and math.isfinite(somatic.score_of(*L))


# ---- the worked instance of the contract (include/lcr.h), through the restatement ------------------------------------------------------
def cand(pos, ref_base, a1, a2, flags=0, ps=0, vt=1, af1=0.8, af2=0.2, depth=20, qual=33.7):
    c = np.zeros(1, dtype=_abi.CAND_DTYPE)
    c["pos"], c["ref_base"], c["allele1"], c["allele2"] = pos, ord(ref_base), ord(a1), ord(a2)
    c["variant_type"], c["flags"], c["phase_set"], c["af1"], c["af2"], c["depth"], c["qual"] = vt, flags, ps, af1, af2, depth, qual
    return c


FLAGGED = _abi.F_CAND_SOMATIC | _abi.F_NON_SELECTED
# (assignment, phase set, base code, q) of the sixteen rows at the site, reference base A
ROWS = [(1, 100, A, 30)] * 6 + [(2, 100, A, 30)] * 7 + [(2, 100, G, 30)] * 3
WANT_L = [[-3107708873, -23420730163838, -6852080807812], [-9899190109605, -26720698299410, -8745495261838]]


def one_site(rows, c, **kw):
    return ref.somatic_sites(list(range(len(rows) + 1)), [0] * len(rows), [(b << 6) | q for _, _, b, q in rows], [r[0] for r in rows],
                             [r[1] for r in rows], c, **kw)[0]


def test_worked_instance():
    r = one_site(ROWS, cand(99, "A", "A", "G", FLAGGED))
    assert (int(r["phase_set"]), r["n"].tolist(), int(r["n_other"]), int(r["n_lowq"])) == (100, [[6, 0], [7, 3]], 0, 0)
    assert r["L"].tolist() == WANT_L and r["cls"].tolist() == [0, 2] and (int(r["call"]), int(r["status"])) == (2, somatic.SOM_OK)
    assert abs(somatic.score(r) - 10.864161328833896) < 1e-9 and "%.2f" % somatic.score(r) == "10.86"
    # the mirror image calls haplotype 1; without the flag the classes stand and nothing is called
    m = one_site([(3 - a, ps, b, q) for a, ps, b, q in ROWS], cand(99, "A", "A", "G", FLAGGED))
    assert m["L"].tolist() == WANT_L[::-1] and m["cls"].tolist() == [2, 0] and int(m["call"]) == 1 and somatic.score(m) == somatic.score(r)
    u = one_site(ROWS, cand(99, "A", "A", "G", _abi.F_HET))
    assert u["L"].tolist() == WANT_L and u["cls"].tolist() == [0, 2] and int(u["call"]) == 0 and somatic.score(u) is None
    # neither allele is the reference base: counts only
    x = one_site(ROWS, cand(99, "A", "C", "G", FLAGGED))
    assert x["n"].tolist() == [[6, 0], [7, 3]] and int(x["status"]) == somatic.SOM_ALLELES and not x["L"].any() and not x["cls"].any() and int(x["call"]) == 0
    # the depth bound, reached here with a smaller one: counts only
    d = one_site(ROWS, cand(99, "A", "A", "G", FLAGGED), deep=9)
    assert d["n"].tolist() == [[6, 0], [7, 3]] and int(d["status"]) == somatic.SOM_DEEP and not d["L"].any() and not d["cls"].any() and int(d["call"]) == 0
    assert int(one_site(ROWS, cand(99, "A", "A", "G", FLAGGED), deep=10)["status"]) == somatic.SOM_OK and somatic.DEEP == 1 << 20
    # the threshold, q = 0 as q = 1, rows of another set and without one
    rows = ROWS[:15] + [(2, 100, G, 0), (1, 200, G, 30), (0, 0, G, 30), (1, 0, G, 30), (2, 100, G, 12)]
    t = somatic.tables(0.3)
    r0 = one_site(rows, cand(99, "a", "a", "G", FLAGGED))      # (a lower-case reference base: its code is A's)
    assert (r0["n"].tolist(), int(r0["n_other"]), int(r0["n_lowq"])) == ([[6, 0], [7, 4]], 3, 0)
    assert r0["L"][1].tolist() == ref.haplotype_sums([30] * 7, [30, 30, 1, 12], t) and t["fe"][0] == t["fe"][1]
    r13 = one_site(rows, cand(99, "A", "A", "G", FLAGGED), min_baseq=13)
    assert (r13["n"].tolist(), int(r13["n_other"]), int(r13["n_lowq"])) == ([[6, 0], [7, 2]], 3, 2)
    # an empty haplotype has its priors only
    e = one_site(ROWS[6:], cand(99, "A", "A", "G", FLAGGED))
    assert e["L"][0].tolist() == t["prior"] and e["cls"].tolist() == [0, 2] and int(e["call"]) == 2
    none = ref.somatic_sites([0, 0], [], [], [1], [100], np.concatenate([cand(9, "A", "A", "G"), cand(19, "C", "C", "T", ps=7)]))
    assert none["phase_set"].tolist() == [0, 7] and not none["n"].any() and none["L"].tolist() == [[t["prior"]] * 2] * 2


# ---- format_vcf_records on hand-made records ------------------------------------------------------------------------------------------
def rec(call, ps, n, L):
    r = np.zeros(1, dtype=_abi.SOMATIC_SITE_DTYPE)
    r["call"], r["phase_set"], r["n"], r["L"] = call, ps, n, L
    r["cls"] = [[0, 2], [2, 0]][call - 1] if call else [0, 0]
    return r


def test_format_vcf_records():
    cands = np.concatenate([cand(99, "A", "A", "G", FLAGGED, af1=0.8125, af2=0.1875, depth=16),
                            cand(199, "C", "T", "C", FLAGGED, af1=0.2, af2=0.8, depth=30, qual=7.9),
                            cand(299, "A", "A", "G", _abi.F_HET | _abi.F_FOR_PHASING, ps=100),
                            cand(399, "G", "G", "T", FLAGGED, depth=12)])
    recs = np.concatenate([rec(2, 100, [[6, 0], [7, 3]], WANT_L), rec(1, 0, [[9, 5], [8, 0]], WANT_L[::-1]), rec(0, 100, [[9, 0], [0, 9]], WANT_L),
                           rec(2, 4000, [[3, 0], [3, 4]], [WANT_L[0], [-9899190109605, -26720698299410, -5000000000000]])])
    sq3 = somatic.score(recs[3])
    assert sq3 > 20.0
    text = somatic.format_vcf_records(cands, recs, "chr7", 0.0)
    assert text == ("chr7\t100\t.\tA\tG\t33\tPASS\tRDS=somatic;SHP=2;H1=6,0;H2=7,3\tGT:DP:AF:PS:SQ\t0/1:16:0.19:100:10.86\n"
                    "chr7\t200\t.\tC\tT\t7\tPASS\tRDS=somatic;SHP=1;H1=9,5;H2=8,0\tGT:DP:AF:PS:SQ\t0/1:30:0.20:.:10.86\n"
                    "chr7\t400\t.\tG\tT\t33\tPASS\tRDS=somatic;SHP=2;H1=3,0;H2=3,4\tGT:DP:AF:PS:SQ\t0/1:12:0.20:4000:%.2f\n" % sq3)
    low = somatic.format_vcf_records(cands, recs, "chr7", 15.0).split("\n")
    assert [l.split("\t")[6] for l in low[:-1]] == ["LowQual", "LowQual", "PASS"] and [l.split("\t")[1] for l in low[:-1]] == ["100", "200", "400"]
    assert somatic.format_vcf_records(cands, recs, "chr7", 10.864161328833896 - 1e-12).split("\t")[6] == "PASS"      # SQ >= min_score
    assert somatic.format_vcf_records(cands[2:3], recs[2:3], "chr7") == "" and somatic.format_vcf_records(cands[:0], recs[:0], "chr7") == ""
    with pytest.raises(ValueError):
        somatic.format_vcf_records(cands, recs[:2], "chr7")
    assert somatic.INFO_LINES.count("\n") == 3 and all(l.startswith("##INFO=<ID=%s," % k) for l, k in zip(somatic.INFO_LINES.split("\n"), ("SHP", "H1", "H2")))


def test_parameters_are_refused_before_any_gpu_work(tmp_path):
    for bad in (dict(purity=0.0), dict(purity=1.5), dict(purity=float("nan")), dict(som_rate=0.0), dict(het_rate=-1.0),
                dict(het_rate=0.7, som_rate=0.3), dict(min_baseq=31), dict(min_baseq=-1), dict(min_baseq=12.5), dict(min_baseq=True)):
        kw = dict(purity=0.3, som_rate=5e-6, het_rate=5e-4, min_baseq=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            somatic.check_params(**kw)
    somatic.check_params(1.0, 5e-6, 5e-4, 30)
    for extra, word in ((["--somatic-purity", "1.5"], "--somatic-purity"), (["--somatic-min-baseq", "31"], "--somatic-min-baseq")):
        cmd = [sys.executable, os.path.join(ROOT, "tools", "run_pipeline.py"), "-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"),
               "-o", str(tmp_path / "out.vcf"), "--somatic-out", str(tmp_path / "s.vcf")] + extra
        p = subprocess.run(cmd, capture_output=True, text=True)
        assert p.returncode == 2 and word in p.stderr and not (tmp_path / "out.vcf").exists()

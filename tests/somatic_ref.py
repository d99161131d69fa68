"""The contract of lcr_somatic (include/lcr.h) restated loop for loop in plain Python with Python ints: per candidate
the entries of the fragment matrix at it, the site's phase set by lcr_site_counts' rule, the counts per haplotype and allele, the six
fixed-point sums, the classes and the call.  Its inputs are the engine's own outputs -- the fragment matrix, the per-row assignment and
phase set, the candidate records --, nothing is vectorised.  The yardstick of tests/test_somatic_gpu.py.  product_form restates the
reference's calculate_prob_somatic (somatic.rs) as it stands, in f64 products, for one haplotype."""
import math

import numpy as np

from longcallr_amd import _abi, somatic

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def classes(l_ref, l_het, l_som):
    """somatic.rs:38-44: the same strict comparisons"""
    if l_som > l_ref and l_som > l_het:
        return 2
    if l_het > l_ref and l_het > l_som:
        return 1
    return 0


def haplotype_sums(ref_qs, alt_qs, t):
    """the three sums of one haplotype from its counted qualities: [ref, het, som], Python ints"""
    l_ref, l_het, l_som = t["prior"]
    for q in ref_qs:
        l_ref += t["f1e"][q]; l_het += t["fe"][q]; l_som += t["fs_ref"][q]
    for q in alt_qs:
        l_ref += t["fe"][q]; l_het += t["f1e"][q]; l_som += t["fs_alt"][q]
    return [l_ref, l_het, l_som]


def somatic_sites(row_ptr, col, val, assignment, phase_set, cands, purity=0.3, som_rate=5e-6, het_rate=5e-4, min_baseq=0, deep=somatic.DEEP):
    """row_ptr / col / val: the CSR of Engine.fragmat(); assignment / phase_set: per row; cands: the candidate records when the call
    runs -> records as _abi.SOMATIC_SITE_DTYPE, one per candidate.  deep: the bound of LCR_SOM_DEEP (2^20; smaller to reach the branch)"""
    t = somatic.tables(purity, som_rate, het_rate)
    n_cand = len(cands)
    entries = [[] for _ in range(n_cand)]       # per candidate: (row, value byte) of every entry at it
    for r in range(len(row_ptr) - 1):
        for e in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            entries[int(col[e])].append((r, int(val[e])))
    out = np.zeros(n_cand, dtype=_abi.SOMATIC_SITE_DTYPE)
    for c in range(n_cand):
        n_lowq = 0
        counted = []                            # (counting row?, its phase set, its assignment, base code, q)
        for r, v in entries[c]:
            if (v & 31) < min_baseq:
                n_lowq += 1
                continue
            a, ps = int(assignment[r]), int(phase_set[r])
            counted.append((a in (1, 2) and ps != 0, ps, a, v >> 6, v & 31))
        per_set = {}
        for counting, ps, _, _, _ in counted:
            if counting:
                per_set[ps] = per_set.get(ps, 0) + 1
        site_ps = int(cands["phase_set"][c])
        if site_ps == 0:
            for ps in sorted(per_set):          # most entries; a strict > keeps the smallest value
                if site_ps == 0 or per_set[ps] > per_set[site_ps]:
                    site_ps = ps
        ref_code = CODE.get(chr(int(cands["ref_base"][c])).upper(), -1)
        qs = [[[], []], [[], []]]               # [haplotype - 1][0 ref, 1 alt]: the counted qualities
        n_other = 0
        for counting, ps, a, b, q in counted:
            if counting and ps == site_ps:
                qs[a - 1][0 if b == ref_code else 1].append(q)
            else:
                n_other += 1
        rec = out[c]
        rec["phase_set"], rec["n_other"], rec["n_lowq"] = site_ps, n_other, n_lowq
        rec["n"] = [[len(qs[h][0]), len(qs[h][1])] for h in (0, 1)]
        assert sum(len(x) for h in qs for x in h) + n_other + n_lowq == len(entries[c])
        ref_b = int(cands["ref_base"][c])
        if int(cands["allele1"][c]) != ref_b and int(cands["allele2"][c]) != ref_b:
            rec["status"] = somatic.SOM_ALLELES
            continue
        if any(len(qs[h][0]) + len(qs[h][1]) > deep for h in (0, 1)):
            rec["status"] = somatic.SOM_DEEP
            continue
        cls = []
        for h in (0, 1):
            L = haplotype_sums(qs[h][0], qs[h][1], t)
            rec["L"][h] = L
            cls.append(classes(*L))
        rec["cls"] = cls
        if int(cands["flags"][c]) & _abi.F_CAND_SOMATIC:
            rec["call"] = 2 if cls == [0, 2] else 1 if cls == [2, 0] else 0
    return out


def of_engine(fm, pr, cands, **kw):
    """somatic_sites on Engine.fragmat(), Engine.phase_result() and the candidate records behind the phase stage"""
    return somatic_sites(fm["row_ptr"], fm["col"], fm["val"], pr["assignment"], pr["phase_set"], cands, **kw)


def product_form(ref_qs, alt_qs, purity, som_rate=5.0 / 1000000.0, het_rate=1.0 / 2000.0):
    """calculate_prob_somatic for one haplotype, as the reference computes it: f64 products over the reads, times the priors, normalised
    -> (class, prob of that class, prob_som).  NaN where the products underflow to 0 / 0."""
    ref_rate = 1.0 - het_rate - som_rate
    p_ref = p_het = p_som = 1.0
    for q in ref_qs:
        eps = math.pow(10.0, -(float(q) / 10.0))
        p_ref *= 1.0 - eps
        p_het *= eps
        p_som *= purity * eps + (1.0 - purity) * (1.0 - eps)
    for q in alt_qs:
        eps = math.pow(10.0, -(float(q) / 10.0))
        p_ref *= eps
        p_het *= 1.0 - eps
        p_som *= purity * (1.0 - eps) + (1.0 - purity) * eps
    w = [p_ref * ref_rate, p_het * het_rate, p_som * som_rate]
    tot = w[0] + w[1] + w[2]
    pr = [x / tot if tot != 0.0 else float("nan") for x in w]
    if pr[2] > pr[0] and pr[2] > pr[1]:
        return 2, pr[2], pr[2]
    if pr[1] > pr[0] and pr[1] > pr[2]:
        return 1, pr[1], pr[2]
    return 0, pr[0], pr[2]


def product_score(prob_som):
    """snpfrags.rs:754: -10 log10(1 - prob); inf where 1 - prob cancels to 0"""
    d = 1.0 - prob_som
    return float("inf") if d == 0.0 else -10.0 * math.log10(d)

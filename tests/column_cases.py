"""Column recipes for the candidate filters (k2_eval.h, k2_candidates.hip, k1_pileup's epilogue): plain data and helpers, no tests.

A case is ONE region and a list of design columns.  A design column says what the pileup must see there -- A/C/G/T counts per read
strand, reads with a deletion / an intron at the column, base qualities -- and the outcome it was designed for: the rule that drops
it (the names oracle_np.candidates writes into its trace) or "kind/variant_type/genotype class" of its record.  build() turns cases
into reads for helpers.mk_batch: the region's read count is the depth, every read runs straight M over the region (1D / 1N at a
column where asked) and FLANK bases beyond both of its ends, so that no end-zone mask (dist_to_end + polya_len + 8 <= FLANK) touches a
region column wherever it sits; the reference has no two equal neighbours, so no homopolymer of polya_len.

Read r of a region is a forward read for r < n_fwd, a reverse read after that; at a column the forward reads carry A.., C.., G.., T..,
then the deletions, then the introns, and so do the reverse reads.  A case's transcript strands (tsf reads count in ts_fwd, then tsr
in ts_rev, the rest carry no tag) are per read, so they hold for all of its columns; the default alternates."""
import functools

import numpy as np

import helpers
from longcallr_amd import _abi

FLANK = 64          # >= dist_to_end (40) + polya_len (5) + 8
BASES = "ACGT"
HET, HOM, SOMATIC = "het/1/1", "hom/2/2", "somatic"


def _reference(n, seed):
    rng = np.random.default_rng(seed)
    out, prev = [], -1
    for _ in range(n):
        k = int(rng.integers(0, 3))
        prev = k if k < prev or prev < 0 else k + 1
        out.append(prev)
    return [BASES[k] for k in out]


def col(at, ref, fw, rv, want, dfw=0, drv=0, nfw=0, nrv=0, quals=None, dense=False):
    """fw / rv: (A, C, G, T) counts on forward / reverse reads; quals: {base: q or [q of each read with that base, forward reads first]}"""
    return dict(at=at, ref=ref, fw=tuple(fw), rv=tuple(rv), want=want, dfw=dfw, drv=drv, nfw=nfw, nrv=nrv, quals=quals or {}, dense=dense)


def split(at, ref, counts, want, **kw):
    """counts {base: n}: every allele spread evenly over the strands (the odd one forward)"""
    fw = [(counts.get(b, 0) + 1) // 2 for b in BASES]
    rv = [counts.get(b, 0) // 2 for b in BASES]
    return col(at, ref, fw, rv, want, **kw)


def case(name, columns, preset="hifi-masseq", over=None, length=300, ts=None, gap=None, probes=()):
    """probes: (rule, "drop" | "pass") pairs -- which side of which threshold the case stands on (the ledger of
    test_candidate_boundaries.py); gap: (lo, hi) region columns every read skips with one N"""
    columns = columns if isinstance(columns, list) else [columns]
    return dict(name=name, columns=columns, preset=preset, over=dict(over or {}), length=length, ts=ts, gap=gap, probes=tuple(probes))


def case_reads(c, region, start0, seed):
    """(reads for helpers.mk_batch, reference string of the region)"""
    L = c["length"]
    full = _reference(L + 2 * FLANK, seed)
    cols = sorted(c["columns"], key=lambda x: x["at"])
    n_fwd = sum(cols[0]["fw"]) + cols[0]["dfw"] + cols[0]["nfw"]
    n_rev = sum(cols[0]["rv"]) + cols[0]["drv"] + cols[0]["nrv"]
    depth = n_fwd + n_rev
    for x in cols:
        assert 0 <= x["at"] < L and (c["gap"] is None or not c["gap"][0] - 2 <= x["at"] <= c["gap"][1] + 1), c["name"]
        assert sum(x["fw"]) + x["dfw"] + x["nfw"] == n_fwd and sum(x["rv"]) + x["drv"] + x["nrv"] == n_rev, c["name"]
        full[FLANK + x["at"]] = x["ref"]
    if c["ts"] is None:     # the tags alternate over the reads: both planes stay near depth / 2, no A>G / T>C column is an edit
        tag = [1 + r % 2 for r in range(depth)]
    else:
        tag = [1 if r < c["ts"][0] else 2 if r < sum(c["ts"]) else 0 for r in range(depth)]
    seqs = [list(full) for _ in range(depth)]
    quals = [[30] * len(full) for _ in range(depth)]
    cuts = [[] for _ in range(depth)]      # (read offset, op) of 1D / 1N
    for x in cols:
        o = FLANK + x["at"]
        seen = {}
        for strand, cnt, nd, nn, r0 in ((0, x["fw"], x["dfw"], x["nfw"], 0), (1, x["rv"], x["drv"], x["nrv"], n_fwd)):
            what = [b for b, k in zip(BASES, cnt) for _ in range(k)] + ["D"] * nd + ["N"] * nn
            for r, b in enumerate(what, start=r0):
                if b in "DN":
                    cuts[r].append((o, b))
                    continue
                seqs[r][o] = b
                q = x["quals"].get(b, 30)
                if not isinstance(q, int):
                    q = q[seen.get(b, 0)]
                    seen[b] = seen.get(b, 0) + 1
                quals[r][o] = q
    if c["gap"] is not None:
        for r in range(depth):
            cuts[r].append((FLANK + c["gap"][0], c["gap"][1] - c["gap"][0]))
    reads = []
    for r in range(depth):
        seq, q, cigar, last = [], [], "", 0
        for o, op in sorted(cuts[r], key=lambda t: t[0]):
            n = 1 if isinstance(op, str) else op
            assert o > last, c["name"]     # (two cuts never touch)
            cigar += "%dM%d%s" % (o - last, n, op if isinstance(op, str) else "N")
            seq += seqs[r][last:o]; q += quals[r][last:o]
            last = o + n
        cigar += "%dM" % (len(full) - last)
        seq += seqs[r][last:]; q += quals[r][last:]
        strand = 0 if r < n_fwd else 1
        # flags: bit 0 reverse read; ts 1 = '+', 2 = '-': a read counts in ts_fwd when (forward read) == (ts '+')
        t = 0 if tag[r] == 0 else (1 if (strand == 0) == (tag[r] == 1) else 2)
        reads.append(dict(pos=start0 - FLANK, seq="".join(seq), qual=q, cigar=cigar, rev=strand, ts=t, region=region))
    return reads, "".join(full[FLANK:FLANK + L])


def build(cases):
    """one ReadBatch of the cases' regions in list order; region g starts at 100000 * (g + 1)"""
    reads, regions = [], []
    for g, c in enumerate(cases):
        rd, ref = case_reads(c, g, 100000 * (g + 1), seed=1000 + g)
        reads += rd
        regions.append((100000 * (g + 1), ref))
    return helpers.mk_batch(reads, regions)


def params(preset, over, **more):
    return _abi.make_params(preset, **dict(over, **more))


def groups(cases):
    """cases that can share a batch: [(override dict, [cases])] in first-seen order"""
    out = {}
    for c in cases:
        out.setdefault(tuple(sorted(c["over"].items())), []).append(c)
    return [(dict(k), v) for k, v in out.items()]


# ---- strand-bias census ---------------------------------------------------------------------------------------------------------
# The 18 tuples (ref_fw, ref_rv, alt_fw, alt_rv) of total <= 64 at which a strand_odds_ratio built on NumPy's float32 log gave
# another verdict than the C++ oracle's (host logf) -- oracle_np.strand_odds_ratio's docstring.
NP_LOG_DISAGREED = [(0, 6, 0, 34), (1, 6, 1, 34), (1, 13, 0, 34), (2, 20, 0, 34), (3, 6, 3, 34), (3, 13, 1, 34), (3, 27, 0, 34), (5, 20, 1, 34),
                    (6, 0, 34, 0), (6, 1, 34, 1), (6, 3, 34, 3), (7, 13, 3, 34), (13, 1, 34, 0), (13, 3, 34, 1), (13, 7, 34, 3), (20, 2, 34, 0),
                    (20, 5, 34, 1), (27, 3, 34, 0)]


def numpy_log_disagreements(orc):
    """NP_LOG_DISAGREED recomputed: the census tuples at which strand_odds_ratio on NumPy's own float32 log (this process's) gives
    another verdict than the C++ oracle"""
    t, sor, thr, _ = census(orc)
    f = np.float32
    x00, x01, x10, x11 = (t[:, k].astype(f) + f(1) for k in range(4))

    def ratio(x00, x01, x10, x11):
        sym = (x00 * x11) / (x01 * x10) + (x01 * x10) / (x00 * x11)
        return (np.log(sym) + np.log(np.minimum(x00, x01) / np.maximum(x00, x01))) - np.log(np.minimum(x10, x11) / np.maximum(x10, x11))
    mine = ratio(x00, x01, x10, x11)
    thr_np = ratio(*(np.array([v], f) for v in (6, 6, 10, 2)))[0]
    return [tuple(int(v) for v in x) for x in t[(mine > thr_np) != (sor > thr)]]


def _bits(x):
    b = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff), b)


@functools.lru_cache(maxsize=1)
def census(orc):
    """every (ref_fw, ref_rv, alt_fw, alt_rv) in 0..30 x 0..30 x 0..40 x 0..40 with total <= 64 and an alt read (646 249) through the C++ oracle:
    (tuples [n, 4], sor [n] f32, threshold f32, distance to the threshold in ulp [n])"""
    f = orc.lib().orc_strand_odds_ratio
    t = np.array([(a, b, c, d) for a in range(31) for b in range(31) for c in range(41) for d in range(41) if a + b + c + d <= 64 and c + d > 0],
                 dtype=np.int64)
    sor = np.array([f(a, b, c, d) for a, b, c, d in t.tolist()], dtype=np.float32)
    thr = np.float32(f(5, 5, 9, 1))
    return t, sor, thr, _bits(sor) - _bits(thr)


def census_verdict(orc, tup):
    """True: the C++ oracle's strand-odds-ratio test passes the tuple (sor <= threshold)"""
    f = orc.lib().orc_strand_odds_ratio
    return not np.float32(f(*tup)) > np.float32(f(5, 5, 9, 1))


def _binom_rejects(k, n):
    from oracle import oracle_np
    return n <= 30 and oracle_np.binomial_two_tailed(k, n) < 0.05


def ratio_decides(t, skewed_ref=True):
    """the tuple's column is decided by the ratio alone and becomes a record if it passes: both alt strands non-zero, no binomial
    verdict against it, ref_fw != ref_rv; deep enough for every preset; and 3 * alt - 0.301 * total >= 4, which keeps the
    hom-ref genotype's posterior below 0.1 at q30 (log10: -3 per alt base against -0.301 per base, prior 3), so QUAL >= 10"""
    a, b, c, d = (int(v) for v in t)
    return (c > 0 and d > 0 and (a != b or not skewed_ref) and not _binom_rejects(c, c + d) and a + b + c + d >= 10
            and 3.0 * (c + d) - 0.301 * (a + b + c + d) >= 4.0)


def near_threshold_tuples(orc, want=24):
    """`want` census tuples within 3 ulp of the threshold that the ratio alone decides, NP_LOG_DISAGREED's first, then by |ulp| and tuple"""
    t, _, _, ulp = census(orc)
    near = [tuple(int(v) for v in x) for x in t[np.abs(ulp) <= 3]]
    first = [x for x in NP_LOG_DISAGREED if ratio_decides(x)]
    dist = {tuple(int(v) for v in x): abs(int(u)) for x, u in zip(t[np.abs(ulp) <= 3], ulp[np.abs(ulp) <= 3])}
    rest = sorted((x for x in near if ratio_decides(x) and x not in first), key=lambda x: (dist[x], x))
    # spread over the alt totals rather than 24 neighbours of one
    picked, seen = list(first), {}
    for x in rest:
        k = (x[2] + x[3], min(x[2], x[3]))
        if seen.get(k, 0) < 2 and len(picked) < want:
            picked.append(x)
            seen[k] = seen.get(k, 0) + 1
    assert len(picked) >= want, len(picked)
    return picked


CLEARLY_ABOVE = [(10, 10, 3, 30), (12, 9, 2, 31), (9, 12, 33, 2), (15, 5, 1, 32), (5, 15, 34, 1), (8, 11, 2, 35), (11, 8, 36, 3)]
CLEARLY_BELOW = [(10, 9, 15, 16), (9, 10, 20, 12), (3, 12, 8, 25), (12, 3, 25, 8), (6, 7, 10, 10), (2, 9, 6, 12), (0, 6, 16, 16)]


def tuple_case(t, tag):
    a, b, c, d = t
    return case("sb_%s_%d_%d_%d_%d" % (tag, a, b, c, d), col(150, "C", (c, a, 0, 0), (d, b, 0, 0), None), preset="hifi-isoseq")


# ---- the cases ------------------------------------------------------------------------------------------------------------------
Q0 = dict(min_qual=0)     # a column of a few alt reads survives to its class (QUAL >= 0 always holds)


def depth_cases():
    return [
        case("depth_min_minus_1", split(150, "C", {"C": 3, "A": 2}, "min_depth"), probes=[("min_depth", "drop")]),
        case("depth_min", split(150, "C", {"C": 3, "A": 3}, HET), probes=[("min_depth", "pass")]),
        case("depth_max", split(150, "C", {"C": 20, "A": 20}, HET), over=dict(max_depth=40), probes=[("max_depth", "pass")]),
        case("depth_max_plus_1", split(150, "C", {"C": 21, "A": 20}, "max_depth"), over=dict(max_depth=40), probes=[("max_depth", "drop")]),
    ]


def depth200_cases():
    lc = dict(min_qual=0, low_cnt_cut=12)   # (at the default 10 both rules cut at the same count on either side of depth 200)
    return [
        case("d199_alt10", split(150, "C", {"C": 189, "A": 10}, SOMATIC), over=Q0, probes=[("low_frac", "pass")]),
        case("d199_alt9", split(150, "C", {"C": 190, "A": 9}, "low_frac"), over=Q0, probes=[("low_frac", "drop")]),
        case("d200_alt10", split(150, "C", {"C": 190, "A": 10}, SOMATIC), over=Q0, probes=[("low_cnt", "pass")]),
        case("d200_alt9", split(150, "C", {"C": 191, "A": 9}, "low_cnt"), over=Q0, probes=[("low_cnt", "drop")]),
        case("d199_alt11_cut12", split(150, "C", {"C": 188, "A": 11}, SOMATIC), over=lc, probes=[("depth200", "pass")]),
        case("d200_alt11_cut12", split(150, "C", {"C": 189, "A": 11}, "low_cnt"), over=lc, probes=[("depth200", "drop")]),
        case("d200_alt12_cut12", split(150, "C", {"C": 188, "A": 12}, SOMATIC), over=lc, probes=[("low_cnt", "pass")]),
    ]


def quotient_cases():
    out = []
    # (one alt base cannot pass the base-quality filter, which wants two: 1/20 ends there whichever way low_frac compares, and stands in
    # the ledger for that; 2/40 and 5/100 are the cases that see `<` become `<=`)
    for k, n in ((1, 20), (2, 40), (5, 100)):
        out.append(case("low_frac_%d_%d" % (k, n), split(150, "C", {"C": n - k, "A": k}, SOMATIC if k > 1 else "baseq"), over=Q0,
                        probes=[("low_frac", "pass") if k > 1 else ("baseq", "drop")]))
    out.append(case("low_frac_1_21", split(150, "C", {"C": 20, "A": 1}, "low_frac"), over=Q0, probes=[("low_frac", "drop")]))
    for k, n in ((3, 20), (6, 40)):
        out.append(case("min_af_hifi_%d_%d" % (k, n), split(150, "C", {"C": n - k, "A": k}, HET), over=Q0, probes=[("min_af", "pass")]))
    out.append(case("min_af_hifi_3_21", split(150, "C", {"C": 18, "A": 3}, SOMATIC), over=Q0, probes=[("min_af", "drop")]))
    for k, n in ((2, 10), (4, 20), (8, 40)):
        out.append(case("min_af_ont_%d_%d" % (k, n), split(150, "C", {"C": n - k, "A": k}, HET), preset="ont-drna", over=Q0,
                        probes=[("min_af", "pass")]))
    out.append(case("min_af_ont_4_21", split(150, "C", {"C": 17, "A": 4}, SOMATIC), preset="ont-drna", over=Q0, probes=[("min_af", "drop")]))
    ai = dict(min_af_intron=0.5)
    out.append(case("af_intron_10_20", split(150, "C", {"C": 5, "A": 5}, HET, nfw=5, nrv=5), over=ai, probes=[("af_intron", "pass")]))
    out.append(case("af_intron_10_21", split(150, "C", {"C": 5, "A": 5}, "af_intron", nfw=6, nrv=5), over=ai, probes=[("af_intron", "drop")]))
    return out


def deletion_cases():
    return [
        case("del_eq_alt", split(150, "C", {"C": 8, "A": 4}, "deletion", dfw=2, drv=2), probes=[("deletion", "drop")]),
        case("del_alt_minus_1", split(150, "C", {"C": 8, "A": 4}, HET, dfw=2, drv=1), probes=[("deletion", "pass")]),
    ]


def allele_cases():
    v = lambda name, cnt, ref, want, **kw: case(name, split(150, ref, dict(zip(BASES, cnt)), want), probes=[("two_major", want)], **kw)
    return [
        v("tm_5330_G", [5, 3, 3, 0], "G", HET),             # tie for second: the reference allele is preferred
        v("tm_5303_T", [5, 3, 0, 3], "T", HET),             # ... also when it sorts fourth
        v("tm_5330_T", [5, 3, 3, 0], "T", "hom/3/2"),       # tie, reference not among them: stable order
        v("tm_2222_G", [2, 2, 2, 2], "G", HET),
        v("tm_0709_C", [0, 7, 0, 9], "C", HET),
        v("tm_tie_first", [4, 4, 0, 0], "C", HET),          # A and C tie for first place: A sorts first, C is the reference
        v("tm_n_alt_2", [6, 0, 6, 0], "T", "hom/3/2"),      # the reference base in neither top place
        v("tm_ref_lower", [5, 5, 0, 0], "c", "ref_base"),
        v("tm_ref_N", [5, 5, 0, 0], "N", "ref_base"),
    ]


def strand_cases(orc):
    sb = lambda name, column, probes, **kw: case(name, column, preset=kw.pop("preset", "hifi-isoseq"), probes=probes, **kw)
    out = [
        sb("sb_binom_30_9", col(150, "C", (9, 15, 0, 0), (21, 15, 0, 0), "binomial"), [("binomial", "drop")]),
        sb("sb_binom_30_10", col(150, "C", (10, 15, 0, 0), (20, 15, 0, 0), HET), [("binomial", "pass")]),
        sb("sb_binom_31_9", col(150, "C", (9, 15, 0, 0), (22, 15, 0, 0), HET), [("binomial_n30", "pass")]),
        sb("sb_one_strand_31", col(150, "C", (0, 0, 0, 0), (31, 30, 0, 0), "one_strand"), [("one_strand", "drop")]),
        sb("sb_both_strands_31", col(150, "C", (1, 0, 0, 0), (30, 30, 0, 0), HET), [("one_strand", "pass")]),
        # n_alt == 2: A 1 + 8 would fall to the binomial (p = 0.039) if it applied
        sb("sb_n_alt_2_no_binom", col(150, "T", (1, 0, 4, 0), (8, 0, 4, 0), "hom/3/2"), [("binomial_n_alt_2", "pass")]),
        # ... and the second allele's ratio decides: A 5 + 5 passes, G 0 + 9 does not
        sb("sb_n_alt_2_max", col(150, "T", (5, 0, 0, 0), (5, 0, 9, 0), "sor"), [("sor_n_alt_2", "drop")]),
        sb("sb_off", col(150, "C", (9, 15, 0, 0), (21, 15, 0, 0), HET), [("strand_bias_off", "pass")], preset="hifi-masseq"),
    ]
    for t in near_threshold_tuples(orc):
        out.append(tuple_case(t, "near"))
    out += [tuple_case(t, "above") for t in CLEARLY_ABOVE] + [tuple_case(t, "below") for t in CLEARLY_BELOW]
    for c in out:
        if c["columns"][0]["want"] is None:
            x = c["columns"][0]
            ok = census_verdict(orc, (x["fw"][1], x["rv"][1], x["fw"][0], x["rv"][0]))
            x["want"] = "kept" if ok else "sor"
            c["probes"] = (("sor", "pass" if ok else "drop"),)
    return out


def tuple_of(c):
    x = c["columns"][0]
    return (x["fw"][1], x["rv"][1], x["fw"][0], x["rv"][0])


def baseq_cases():
    mq = 10
    return [
        case("bq_two_at_min", split(150, "C", {"C": 2, "A": 12}, HET, quals={"A": [mq, mq] + [mq - 1] * 10}), probes=[("baseq", "pass")]),
        case("bq_one_at_min", split(150, "C", {"C": 2, "A": 12}, "baseq", quals={"A": [mq] + [mq - 1] * 11}), probes=[("baseq", "drop")]),
        case("bq_bin_30", split(150, "C", {"C": 5, "A": 5}, HET, quals={"A": [31, 60, 93, 31, 60], "C": 93}), probes=[("baseq_bin30", "pass")]),
        case("bq_q0_ref", split(150, "C", {"C": 5, "A": 5}, HOM, quals={"C": 0}), probes=[("q0", "ref")]),
        case("bq_q0_alt", split(150, "C", {"C": 5, "A": 5}, HET, quals={"A": [0, 0, 0, 30, 30]}), probes=[("q0", "alt")]),
        case("bq_q0_both", split(150, "C", {"C": 5, "A": 5}, HET, quals={"C": 0, "A": [0, 0, 0, 30, 30]}), probes=[("q0", "both")]),
    ]


def class_cases():
    ag = lambda want, **kw: split(150, "A", {"A": 6, "G": 6}, want, **kw)
    tc = lambda want, **kw: split(150, "T", {"T": 6, "C": 6}, want, **kw)
    return [
        case("ag_ts_2x", ag(HET), ts=(6, 3), probes=[("edit_ts", "drop")]),
        case("ag_ts_2x_plus_1", ag("edit/1/1"), ts=(7, 3), probes=[("edit_ts", "pass")]),
        case("ag_ts_none", ag("edit/1/1"), ts=(0, 0), probes=[("edit_ts0", "pass")]),
        case("tc_ts_2x", tc(HET), ts=(3, 6), probes=[("edit_ts", "drop")]),
        case("tc_ts_2x_plus_1", tc("edit/1/1"), ts=(3, 7), probes=[("edit_ts", "pass")]),
        case("tc_ts_none", tc("edit/1/1"), ts=(0, 0), probes=[("edit_ts0", "pass")]),
        case("ag_hom_var", split(150, "A", {"G": 12}, HOM), ts=(12, 0), probes=[("edit_hom_guard", "drop")]),
        # 18 reference bases at q3 (error 0.5): the het likelihood beats hom-ref by the two alt bases alone, QUAL >= min_qual
        case("somatic_2_20", split(150, "C", {"C": 18, "A": 2}, "somatic/2/2", quals={"C": 3}), probes=[("somatic", "pass")]),
        case("hom_n_alt_2_both", split(150, "T", {"A": 6, "G": 6}, "hom/3/2"), probes=[("hom_n_alt_2", "pass")]),
        case("hom_n_alt_2_one_low", split(150, "T", {"A": 12, "G": 1}, HOM), probes=[("hom_n_alt_2", "drop")]),
        # ... and with the second fraction exactly on min_af (3/20) and just below it (3/21)
        case("hom_n_alt_2_at_min_af", split(150, "T", {"A": 16, "G": 3, "T": 1}, "hom/3/2"), probes=[("hom_n_alt_2", "pass")]),
        case("hom_n_alt_2_below_min_af", split(150, "T", {"A": 17, "G": 3, "T": 1}, HOM), probes=[("hom_n_alt_2", "drop")]),
        case("het_n_alt_2", split(150, "T", {"A": 5, "G": 5, "T": 4}, "hom/3/1"), probes=[("het_n_alt_2", "pass")]),
        # three alt bases at q10 of 20: hom-ref is the best genotype, 3/20 is not below min_af, nothing is left to call it
        case("hom_ref_best", split(150, "C", {"C": 17, "A": 3}, "hom_ref", quals={"A": 10}), over=Q0, probes=[("hom_ref", "drop")]),
        case("min_qual_above", split(150, "C", {"C": 17, "A": 3}, HET), probes=[("min_qual", "pass")]),     # QUAL 2.9
        case("min_qual_below", split(150, "C", {"C": 18, "A": 3}, "min_qual"), probes=[("min_qual", "drop")]),  # QUAL 1.7
    ]


def _het(at, dense=False):
    return split(at, "C", {"C": 10, "A": 10}, HET, dense=dense)


def dense_cases():
    hets = lambda sites, dense: [_het(x, x in dense) for x in sites]
    first5 = [50, 60, 70, 80]
    allts = (20, 0)
    many = [40 + 20 * k for k in range(300)]
    return [
        case("dense_gap_100", hets(first5 + [150, 400], first5 + [150]), length=500, probes=[("dense_win", "pass")]),
        case("dense_gap_101", hets(first5 + [151, 400], []), length=500, probes=[("dense_win", "drop")]),
        case("dense_four", hets(first5 + [400], []), length=500, probes=[("dense_cnt", "drop")]),
        case("dense_five", hets(first5 + [90, 400], first5 + [90]), length=500, probes=[("dense_cnt", "pass")]),
        case("dense_to_the_end", hets(first5 + [90, 100], first5 + [90]), length=500, probes=[("dense_end", "pass")]),
        case("dense_end_exactly_five", hets(first5 + [90], first5), length=500, probes=[("dense_end", "pass")]),
        case("dense_end_four", hets(first5, []), length=500, probes=[("dense_end", "drop")]),
        case("dense_3_in_4bp_at_the_end", hets([50, 52, 54], [50, 52]), length=500, probes=[("dense_5bp_end", "pass")]),
        case("dense_3_in_4bp", hets([50, 52, 54, 300], [50, 52, 54]), length=500, probes=[("dense_5bp", "pass")]),
        case("dense_3_in_5bp", hets([50, 52, 55, 300], []), length=500, probes=[("dense_5bp", "drop")]),
        case("dense_not_counted", hets(first5 + [400], []) + [split(65, "A", {"A": 10, "G": 10}, "edit/1/1"),
                                                                split(75, "C", {"C": 18, "A": 2}, "somatic/2/2", quals={"C": 3})],
             length=500, ts=allts, probes=[("dense_kinds", "drop")]),
        case("dense_300_sites", hets(many, many[:-1]), length=40 + 20 * 300 + 17, probes=[("dense_chunks", "pass")]),
    ]


TILE = 256     # lcr_dev.h: LCR_TILE, columns per pileup tile, counted from the region's first column; k2_candidates.hip: HT_SLOTS is 256 too


def _run(lo, n):
    """n neighbouring het columns from lo on (all dense but the last: `tk in i..j`); reference C / G and alt A / T in turn, so that
    neither the reference nor a read gets a homopolymer"""
    return [split(x, "CG"[x % 2], {"CG"[x % 2]: 10, "AT"[x % 2]: 10}, HET, dense=x != lo + n - 1) for x in range(lo, lo + n)]


def place_cases():
    """k2_filter / k1_pileup's epilogue take a tile of 256 columns per workgroup, k2_compact gives a thread four neighbouring columns,
    k2_hist_tiles keeps HT_SLOTS = 256 survivors per pass over a tile's records.  A tile has LCR_TILE = 256 columns, so it never holds
    more than HT_SLOTS survivors: the second pass of k2_hist_tiles cannot be reached as the constants stand, and the boundary that can
    is a tile whose every column survives (cnt == HT_SLOTS)."""
    L = 1030    # a multiple neither of 4 nor of 256 nor of 1024
    return [
        case("place_a", [_het(x) for x in (0, 4, 256, 1023, L - 1)], length=L, probes=[("place", "0/4/256/1023/last")]),
        case("place_b", [_het(x) for x in (3, 255, 1024)], length=L, probes=[("place", "3/255/1024")]),
        # tiles 4 .. 7 (columns 1024 .. 2047) lie inside every read's intron: no record, survivors on both sides of them
        case("place_empty_tiles", [_het(500), _het(2500)], length=3 * 1024 + 10, gap=(1000, 2100), probes=[("place", "empty tiles")]),
        case("place_full_tile", _run(TILE, TILE), length=3 * TILE + 7, probes=[("place", "every column of a tile")]),
        case("place_257_across_a_border", _run(200, TILE + 1), length=3 * TILE + 7, probes=[("place", "257 neighbours across a border")]),
    ]


@functools.lru_cache(maxsize=1)
def all_families(orc):
    return dict(depth=depth_cases(), depth200=depth200_cases(), quotient=quotient_cases(), deletion=deletion_cases(),
                allele=allele_cases(), strand=strand_cases(orc), baseq=baseq_cases(), classes=class_cases(), dense=dense_cases(),
                place=place_cases())


# every (rule, side) a complete set of cases stands on -- the ledger's other column
LEDGER = [(r, s) for r in ("min_depth", "max_depth", "low_frac", "low_cnt", "depth200", "min_af", "af_intron", "deletion", "binomial",
                           "one_strand", "sor", "baseq", "edit_ts", "min_qual", "hom_n_alt_2", "dense_win", "dense_cnt", "dense_5bp")
          for s in ("drop", "pass")] + [
    ("binomial_n30", "pass"), ("binomial_n_alt_2", "pass"), ("sor_n_alt_2", "drop"), ("strand_bias_off", "pass"), ("baseq_bin30", "pass"),
    ("q0", "ref"), ("q0", "alt"), ("q0", "both"), ("edit_ts0", "pass"), ("edit_hom_guard", "drop"), ("somatic", "pass"),
    ("het_n_alt_2", "pass"), ("hom_ref", "drop"), ("dense_end", "pass"), ("dense_end", "drop"), ("dense_5bp_end", "pass"), ("dense_kinds", "drop"), ("dense_chunks", "pass"),
    ("two_major", HET), ("two_major", "hom/3/2"), ("two_major", "ref_base"),
    ("place", "0/4/256/1023/last"), ("place", "3/255/1024"), ("place", "empty tiles"), ("place", "every column of a tile"),
    ("place", "257 neighbours across a border")]
# the reasons oracle_np.candidates must have recorded at a design column of some case
REASONS = ["min_depth", "max_depth", "ref_base", "low_frac", "low_cnt", "deletion", "af_intron", "baseq", "sor", "binomial", "one_strand",
           "min_qual", "hom_ref", "het/1/1", "hom/2/2", "hom/3/2", "hom/3/1", "edit/1/1", "somatic/2/2"]

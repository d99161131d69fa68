"""K19 lcr_site_pairs on the GPU against the plain-Python restatement of its contract (tests/site_pairs_ref.py): every field of every
record, pair_off and n_eligible, exactly, in pinned host memory and in HBM.  Sites are imported at chosen columns and phased with
Engine.haplotag, as test_site_counts_gpu does: the contract's worked instance, rows on either side of the lane group with partner windows
of 1, 2 and 8, gaps in the eligible ranks, rows without an entry at an intermediate site, the distance limit, region boundaries, empty
cases, the quality threshold, a pair under 3 000 rows, independence from the batch, repeated calls, the call's order and lifetime on one
context, and real data behind lcr_phase and lcr_haplotag with a cross-check against K12's counts."""
import ctypes as C

import numpy as np
import pytest

import helpers
import site_pairs_ref as ref
import test_haplotag_gpu as th
import test_junctions_gpu as tj
import test_site_counts_gpu as ts
import test_site_pairs_host as host
from longcallr_amd import _abi, _lib

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
PARAMS = dict(seed=5, dist_to_end=0)


def from_device(ptr, dtype, n):
    out = np.zeros(n, dtype=dtype)
    if n:
        assert ptr and _lib.load().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


def check(E, fm, mode="all", K=2, D=2, q=13):
    """site_pairs() against the restatement on the engine's own candidates, host and HBM"""
    cands, _ = E.candidates()
    rec, off, n_el = E.site_pairs(mode, K, D, q)
    want, want_off, want_el = ref.of_engine(fm, cands, mode, K, D, q)
    what = (mode, K, D, q)
    assert rec.dtype == _abi.SITE_PAIR_DTYPE and rec.size == want.size, what
    for f in _abi.SITE_PAIR_DTYPE.names:
        assert rec[f].tolist() == want[f].tolist(), (f,) + what
    assert off.tolist() == want_off.tolist() and n_el == want_el, what
    o = E.site_pairs_list()
    assert (o.n_cand, o.n_eligible, o.n_pairs, o.pad_) == (cands.size, n_el, rec.size, 0)
    assert from_device(o.dev_pair, _abi.SITE_PAIR_DTYPE, rec.size).tobytes() == rec.tobytes()        # HBM and host hold the same bytes
    assert from_device(o.dev_pair_off, np.int32, cands.size + 1).tobytes() == off.tobytes()
    assert (rec["n"].reshape(len(rec), 16).sum(axis=1) + rec["n_lowq"]).tolist() == rec["n_rows"].tolist()
    assert (cands["region"][rec["a"]] == cands["region"][rec["b"]]).all() and (rec["a"] < rec["b"]).all()
    return rec, off, n_el, cands


def staged(E, batch, site_gt):
    """the batch up to the fragment stage with the sites {pos0: genotype code} imported"""
    pos = np.array(sorted(site_gt), np.int64)
    return th.staged(E, batch, (pos, np.array([site_gt[int(p)] for p in pos], np.uint8), np.full(pos.size, 30.0, np.float32)))


def third(refseq, c):
    return [x for x in "ACGT" if x not in (refseq[c], tj.ALT[refseq[c]])][0]


# ---- the regions ------------------------------------------------------------------------------------------------------------------------
W_START, L_START, Q_START = 130000, 110000, 120000
W_COLS = (10, 11, 13, 40)
L_COLS = tuple(40 + 3 * k for k in range(17))       # 40 .. 88: seventeen sites three columns apart
Q_COLS = (20, 21)
Q_COMBOS = [(30, 30), (12, 30), (30, 12), (12, 12), (13, 13), (29, 30)]


def worked_region():
    """the header's instance; four more rows hold column 13 alone, so that T stays the third base there"""
    forced = {c: "A" for c in W_COLS}
    reads = [([(0, 60)], {}, {}), ([(0, 60)], {10: "G", 11: "G", 13: "T"}, {}), ([(0, 60)], {10: "G", 11: "G", 13: "G"}, {11: 5})]
    reads += [([(12, 40)], {13: "G"}, {})] * 2 + [([(12, 40)], {}, {})] * 2
    return ts.region(W_START, 100, forced, reads, 61)


def lane_region():
    """rows of 17, 7, 8, 9, 1 and 0 entries (lane group 8); a row with a third base at site 8, one with an intron over sites 7 - 9, two with
    low qualities at the first sites"""
    probe = ts.region(L_START, 200, {}, [], 62)[1]
    end = lambda n: L_COLS[n - 1] + 1
    spec = [([(0, 120)], {}, {})] * 4 + [([(0, end(7))], {}, {})] * 2 + [([(0, end(8))], {}, {})] * 2 + [([(0, end(9))], {}, {})] * 2
    spec += [([(0, end(1))], {}, {}), ([(0, 30)], {}, {})]
    spec += [([(0, 120)], {L_COLS[8]: third(probe, L_COLS[8])}, {}), ([(0, L_COLS[7] - 1), (L_COLS[9] + 2, 120)], {}, {})]
    spec += [([(0, 120)], {}, {L_COLS[0]: 12, L_COLS[1]: 12}), ([(0, 120)], {}, {L_COLS[1]: 5})]
    reads = [(segs, {**ts.hap_bases(probe, [c for c in L_COLS if any(lo <= c < hi for lo, hi in segs)], k % 2), **bases}, quals)
             for k, (segs, bases, quals) in enumerate(spec)]
    return ts.region(L_START, 200, {}, reads, 62)


def qual_region():
    """two adjacent sites under twelve rows: every quality combination on both haplotypes"""
    probe = ts.region(Q_START, 100, {}, [], 63)[1]
    reads = [([(0, 50)], ts.hap_bases(probe, Q_COLS, k % 2), dict(zip(Q_COLS, Q_COMBOS[k // 2]))) for k in range(12)]
    return ts.region(Q_START, 100, {}, reads, 63)


def all_regions():
    return [lane_region(), qual_region(), worked_region()]


COLS = [L_COLS, Q_COLS, W_COLS]
STARTS = [L_START, Q_START, W_START]


def site_codes(which=(0, 1, 2), hom=()):
    """het everywhere; `hom`: [(region, column)] imported as 1/1"""
    return {STARTS[g] + c: (2 if (g, c) in hom else 1) for g in which for c in COLS[g]}


def phased_sites(regs, which=(0, 1, 2), skip=()):
    """haplotype 1 = the reference base; one phase set per region; `skip`: [(region, column)] left out of the phase"""
    d = {}
    for g in which:
        s0, refseq, _ = regs[g]
        for c in COLS[g]:
            if (g, c) not in skip:
                d[s0 + c] = (refseq[c], "G" if g == 2 else tj.ALT[refseq[c]], 500 + g)
    return th.site_arrays(d)


# ---- 1. the worked instance of the contract -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(host.WORKED_WANT))
def test_worked_instance(engine_cls, key):
    mode, K, D, q = key
    regs = all_regions()
    hom = [(2, 11)] if mode == "phased" else []
    E = engine_cls(0, _abi.make_params("hifi-masseq", **PARAMS))
    fm, cands0, _ = staged(E, tj.batch_of([regs[2]]), site_codes((2,), hom))
    assert [int(p) - W_START for p in cands0["pos"]] == list(W_COLS)
    E.haplotag(phased_sites(regs, (2,), hom))
    rec, off, n_el, cands = check(E, fm, mode, K, D, q)
    want_rec, want_off, want_el = host.WORKED_WANT[key]
    assert host.as_tuples(rec) == want_rec and off.tolist() == want_off and n_el == want_el
    E.close()


# ---- 2. rows at the lane group, partner windows, gaps in the ranks, missing entries, the distance limit, the quality threshold ------------
def test_lane_groups_ranks_distance_and_quality(engine_cls):
    regs = all_regions()
    E = engine_cls(0, _abi.make_params("hifi-masseq", **PARAMS))
    hom, skip = [(0, L_COLS[5])], [(0, L_COLS[5]), (0, L_COLS[11])]
    fm, cands0, coff = staged(E, tj.batch_of(regs), site_codes(hom=hom))
    E.haplotag(phased_sites(regs, skip=skip))
    n_ent = np.diff(fm["row_ptr"])[fm["row_region_off"][0]:fm["row_region_off"][1]]
    print("entries per row of the lane region: %r" % (sorted(n_ent.tolist()),))
    for mode in ("all", "phased"):
        for K in (1, 2, 8):
            for D in (0, 6, 5, 3):      # two ranks apart, one column less, one rank apart
                check(E, fm, mode, K, D, 13)
    # the homozygous and the unphased site start no pair and take no partner slot: their neighbours are paired with each other
    rec, off, n_el, cands = check(E, fm, "phased", 1, 0, 13)
    i0 = int(coff[0])
    assert int(cands["variant_type"][i0 + 5]) == 2 and int(cands["haplotype"][i0 + 11]) == 0 and n_el == cands.size - 2
    listed = set(zip(rec["a"].tolist(), rec["b"].tolist()))
    assert (i0 + 4, i0 + 6) in listed and (i0 + 10, i0 + 12) in listed and off[i0 + 6] == off[i0 + 5] and off[i0 + 12] == off[i0 + 11]
    # the row with the intron over sites 7 - 9 and the one with a third base at site 8 still count for the pairs around them
    rec8, off8, _, _ = check(E, fm, "all", 8, 0, 13)
    at = {(int(a) - i0, int(b) - i0): (int(r["n_rows"]), int(r["n_lowq"])) for a, b, r in zip(rec8["a"], rec8["b"], rec8) if b < coff[1]}
    assert (at[(6, 10)], at[(7, 8)], at[(7, 9)], at[(6, 7)]) == ((8, 0), (8, 0), (7, 0), (11, 0))
    assert (at[(0, 8)], at[(0, 1)], at[(1, 2)]) == ((8, 1), (14, 2), (14, 2)) and (0, 9) not in at
    assert off8[i0 + 1] - off8[i0] == 8 and off8[coff[1]] - off8[coff[1] - 1] == 0 and (np.diff(off8) >= 0).all()
    # the quality threshold at the two adjacent sites: below it at the first entry, the second, both
    qa = coff[1]
    for q, lowq in ((0, 0), (13, 6), (30, 10)):
        r, o, _, _ = check(E, fm, "all", 1, 1, q)
        assert o[qa + 1] - o[qa] == 1 and (int(r[o[qa]]["n_rows"]), int(r[o[qa]]["n_lowq"])) == (12, lowq), q
    E.close()


# ---- 3. called candidates: a dense cluster between eligible sites, region boundaries, no candidate, 3 000 rows ----------------------------
def test_called_edges(engine_cls):
    regs = th.edge_regions()
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    fm, cands0, coff = th.staged(E, tj.batch_of(regs))
    E.haplotag(th.site_arrays(th.edge_sites(cands0)))
    for mode in ("all", "phased"):
        for K, D in ((1, 0), (2, 100), (2, 99), (8, 0)):
            rec, off, n_el, cands = check(E, fm, mode, K, D, 13)
    dense = (cands["flags"] & _abi.F_DENSE) != 0
    assert dense.sum() >= 5 and coff[1] == coff[0] and not dense[rec["a"]].any() and not dense[rec["b"]].any()
    rec1, off1, _, _ = check(E, fm, "all", 1, 0, 13)
    plain = [i for i in range(coff[4], coff[5]) if not dense[i]]
    over = [(x, y) for x, y in zip(plain, plain[1:]) if y - x > 1]
    assert over and all(off1[x + 1] - off1[x] == 1 and int(rec1["b"][off1[x]]) == y for x, y in over)     # the dense sites between take no partner slot
    assert all(off1[i + 1] == off1[i] for i in np.flatnonzero(dense))
    for g in range(1, 6):       # the last eligible site of a region starts no pair, whatever follows in the next region
        last = [i for i in range(coff[g], coff[g + 1]) if not dense[i]][-1]
        assert off1[last + 1] == off1[last]
    g5 = rec1[off1[coff[5]]:off1[coff[6]]]
    assert g5["n_rows"].tolist() == [3000] * 4 and all(int(r["n"].max()) == 1500 for r in g5)             # four pairs under 3 000 rows, 1 500 per haplotype
    E.close()


def test_no_candidate_at_all(engine_cls):
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    E.load_batch(tj.batch_of(th.edge_regions()[:1])).run_all()
    rec, off, n_el, cands = check(E, E.fragmat(), "all", 2, 2, 13)
    assert cands.size == 0 and rec.size == 0 and off.tolist() == [0] and n_el == 0
    E.close()


def test_no_and_one_eligible_site(engine_cls):
    regs = all_regions()
    E = engine_cls(0, _abi.make_params("hifi-masseq", **PARAMS))
    fm, _, _ = staged(E, tj.batch_of([regs[1]]), site_codes((1,)))
    E.haplotag(phased_sites(regs, (1,), skip=[(1, Q_COLS[0])]))
    rec, off, n_el, _ = check(E, fm, "phased", 2, 0, 13)
    assert rec.size == 0 and off.tolist() == [0, 0, 0] and n_el == 1
    fm, _, _ = staged(E, tj.batch_of([regs[1]]), site_codes((1,)))
    E.haplotag(None)
    rec, off, n_el, _ = check(E, fm, "phased", 2, 0, 13)
    assert rec.size == 0 and n_el == 0
    assert check(E, fm, "all", 2, 0, 13)[0].size == 1
    E.close()


# ---- 4. independence from the batch; repeated calls ---------------------------------------------------------------------------------------
def test_region_alone_and_in_the_batch(engine_cls):
    regs = all_regions()
    E = engine_cls(0, _abi.make_params("hifi-masseq", **PARAMS))
    fm, _, coff = staged(E, tj.batch_of(regs), site_codes())
    E.haplotag(phased_sites(regs))
    n_ent = np.diff(fm["row_ptr"])[fm["row_region_off"][0]:fm["row_region_off"][1]]
    assert sorted(set(n_ent.tolist())) == [0, 1, 7, 8, 9, 14, 16, 17]        # on either side of the lane group of 8, and past two of them
    rec, off, _, _ = check(E, fm, "all", 8, 0, 13)
    for g in (0, 1, 2):
        fm1, _, _ = staged(E, tj.batch_of([regs[g]]), site_codes((g,)))
        E.haplotag(phased_sites(regs, (g,)))
        rec1, off1, _, _ = check(E, fm1, "all", 8, 0, 13)
        part = rec[off[coff[g]]:off[coff[g + 1]]].copy()
        part["a"] -= coff[g]
        part["b"] -= coff[g]
        assert rec1.tobytes() == part.tobytes() and off1.tolist() == (off[coff[g]:coff[g + 1] + 1] - off[coff[g]]).tolist(), g
    E.close()


def test_repeated_calls(engine_cls):
    regs = all_regions()
    p1, p2 = ("all", 8, 0, 13), ("phased", 1, 3, 30)
    got = []
    for first, second in ((p1, p2), (p2, p1)):
        E = engine_cls(0, _abi.make_params("hifi-masseq", **PARAMS))
        fm, _, _ = staged(E, tj.batch_of(regs), site_codes())
        E.haplotag(phased_sites(regs))
        got.append({p: [x.tobytes() if hasattr(x, "tobytes") else x for x in check(E, fm, *p)[:3]] for p in (first, second)})
        E.close()
    assert got[0] == got[1] and got[0][p1] != got[0][p2]


# ---- 5. order and lifetime on one context -----------------------------------------------------------------------------------------------
def test_order_and_lifetime(engine_cls):
    b1, b2 = tj.batch_of([tj.allele_specific_region()]), tj.batch_of(th.edge_regions()[2:4])
    prm = _abi.make_params("hifi-masseq", seed=7)
    E = engine_cls(0, prm)
    lib = E.lib
    par = lambda *x: _abi.LcrSitePairParams(*x)
    good = par(_abi.PAIRS_ALL, 2, 0, 13)
    o = _abi.LcrSitePairList()
    call = lambda p=good: lib.lcr_site_pairs(E.h, C.byref(p))
    get = lambda: lib.lcr_get_site_pairs(E.h, C.byref(o))
    assert lib.lcr_site_pairs(None, C.byref(good)) == E_ARG and lib.lcr_get_site_pairs(E.h, None) == E_ARG
    E.load_batch(b1).fill_data_into_freq_vec().get_candidate_snps()
    assert call() == E_STATE and get() == E_STATE
    E.get_fragments()
    assert get() == E_STATE and call() == E_STATE and b"before lcr_phase" in lib.lcr_last_error(E.h)     # before the phase stage
    E.phase()
    assert get() == E_STATE                                                                              # phased, not counted yet
    fm = E.fragmat()
    snap = th.snapshot(E)
    first, off, n_el, _ = check(E, fm, "all", 2, 0, 13)
    assert first["n_rows"].tolist() == [40] * 13 and n_el == 8 and th.snapshot(E) == snap                # (the call writes nothing a getter reads)
    # every argument error leaves the last records valid
    for bad, word in ((par(2, 2, 0, 13), b"mode"), (par(0, 0, 0, 13), b"max_partners"), (par(0, 9, 0, 13), b"max_partners"), (par(0, 2, 0, 31), b"min_baseq")):
        assert call(bad) == E_ARG and word in lib.lcr_last_error(E.h)
    assert lib.lcr_site_pairs(E.h, None) == E_ARG
    assert get() == 0 and o.n_pairs == first.size
    assert from_device(o.dev_pair, _abi.SITE_PAIR_DTYPE, first.size).tobytes() == first.tobytes()
    # the next candidate stage ends the records' life; so does the next batch
    E.get_candidate_snps()
    assert get() == E_STATE and call() == E_STATE
    E.get_fragments().phase()
    re, _, _, _ = check(E, E.fragmat(), "all", 2, 0, 13)                                                 # stage re-entry: the same records
    assert re.tobytes() == first.tobytes()
    E.load_batch(b2)
    assert get() == E_STATE and call() == E_STATE
    E.run_all()
    assert get() == E_STATE                                                                              # (nothing stale from the last batch)
    got2, _, _, _ = check(E, E.fragmat(), "phased", 2, 0, 13)
    E.close()
    # behind an asynchronous phase stage: the call settles it
    A = engine_cls(0, prm)
    A.set_async_phase(True)
    A.load_batch(b2).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
    fm2 = A.fragmat()
    A.phase()
    gota, _, _, _ = check(A, fm2, "phased", 2, 0, 13)
    assert gota.tobytes() == got2.tobytes()
    A.close()
    # the timer
    T = engine_cls(0, prm, timing=True)
    with pytest.raises(Exception):
        T.site_pairs_ms()
    T.load_batch(b1).run_all()
    assert T.site_pairs("all", 2, 0, 13)[0].tobytes() == first.tobytes() and T.site_pairs_ms() > 0.0
    T.close()


# ---- 6. real data behind lcr_phase and lcr_haplotag; the cross-check against K12 --------------------------------------------------------------
@pytest.mark.parametrize("stage", ["phase", "haplotag"])
def test_demo(engine_cls, stage):
    b = helpers.demo_batch()
    E = engine_cls(0, _abi.make_params("hifi-masseq"))
    if stage == "phase":
        E.load_batch(b).run_all()
        fm = E.fragmat()
    else:
        fm, cands0, _ = th.staged(E, b)
        E.haplotag(th.site_arrays(th.sites_from_candidates(b, cands0, 11)))
    sc = E.site_counts(13)
    by_base = sc["n"].sum(axis=1)      # counted entries per candidate and base
    # the pipeline's two parameter sets, and ALL without the distance limit (demo.bam holds no two candidates within two columns)
    for mode, K, D in (("phased", 2, 0), ("all", 2, 2), ("all", 2, 0)) if stage == "phase" else (("all", 2, 2), ("all", 2, 0)):
        rec, off, n_el, cands = check(E, fm, mode, K, D, 13)
        print("demo behind %s, %s, max_dist %d: candidates %d, eligible %d, pairs %d, joint rows %d, low-q %d, pairs without a row %d" % (
            stage, mode, D, cands.size, n_el, rec.size, int(rec["n_rows"].sum()), int(rec["n_lowq"].sum()), int((rec["n_rows"] == 0).sum())))
        assert D != 0 or (rec.size > 0 and rec["n_rows"].any())
        assert (rec["n"].sum(axis=2) <= by_base[rec["a"]]).all() and (rec["n"].sum(axis=1) <= by_base[rec["b"]]).all()
    E.close()

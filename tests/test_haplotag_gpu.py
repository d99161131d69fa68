"""K11 lcr_haplotag on the GPU against the plain-Python restatement of its contract (tests/haplotag_ref.py): every field of
phase_result(), the candidate records, the site records and the read records in HBM is compared exactly, phase_score within 1e-4 (the
project's bound for it, tests/test_gpu_parity.py).  A hand-worked instance, the edges of every rule, a round trip through lcr_phase,
synthetic and real data, independence from the batch, device-resident sites, and the call's order and lifetime on one context."""
import ctypes as C

import numpy as np
import pytest

import ase_ref
import asj_ref
import haplotag_ref as ref
import helpers
import test_junctions_gpu as tj
from longcallr_amd import _abi, _lib, synth

pytestmark = pytest.mark.gpu

OTHER = {"A": "CGT", "C": "AGT", "G": "ACT", "T": "ACG"}
E_ARG, E_STATE = -1, -4


def alt_of(s):
    """(REF, ALT) of a candidate as the VCF writer prints them"""
    r, a1, a2 = chr(s["ref_base"]).upper(), chr(s["allele1"]), chr(s["allele2"])
    return r, (a1 if a1 != r else a2 if a2 != r else OTHER[r][0])


def site_arrays(d):
    """{pos0: (h1, h2, ps)} -> the four arrays"""
    pos = np.array(sorted(d), dtype=np.int64)
    return (pos, np.array([ord(d[int(p)][0]) for p in pos], np.uint8), np.array([ord(d[int(p)][1]) for p in pos], np.uint8),
            np.array([d[int(p)][2] for p in pos], np.uint32))


def staged(E, batch, imp=None):
    """the batch up to the fragment stage -> (fragmat, candidate records as the candidate stage wrote them, their offsets)"""
    E.load_batch(batch).fill_data_into_freq_vec()
    if imp is None:
        E.get_candidate_snps()
    else:
        E.import_external_candidates(*imp)
    E.get_fragments()
    fm = E.fragmat()
    cands, coff = E.candidates()
    return fm, cands, coff


def read_records(E):
    ptr, n = E.read_records_device()
    rec = np.zeros(n, dtype=_abi.READ_REC_DTYPE)
    if n:
        assert _lib.load().hipMemcpy(C.c_void_p(rec.ctypes.data), C.c_void_p(ptr), C.c_size_t(rec.nbytes), 2) == 0
    return rec


def compare(E, fm, cands0, sites, want=None):
    """everything the call left against the restatement, field by field"""
    if want is None:
        want = ref.haplotag(fm, cands0, sites, int(E.params.min_linkers), float(E.params.read_assign_cutoff))
    pr = E.phase_result()
    for f in ("haplotag", "assignment", "phase_set"):
        assert pr[f].tolist() == want[f].tolist(), f
    assert pr["objective"].size == len(fm["row_region_off"]) - 1 and not pr["objective"].any()
    assert not any(E.tie_census().values())
    got, _ = E.candidates()
    assert got.size == cands0.size
    for f in _abi.CAND_DTYPE.names:
        if f != "phase_score":
            assert got[f].tobytes() == want["cand"][f].tobytes(), f
    assert np.all(np.abs(got["phase_score"] - want["cand"]["phase_score"]) <= 1e-4)
    # the inputs keep every usable site's computed score away from the constant, so the 1e-4 cannot hide a wrong branch
    both = want["usable"] & (want["site"]["n_h1"] >= 1) & (want["site"]["n_h2"] >= 1)
    assert np.all(np.abs(want["cand"]["phase_score"][both] - ref.PHASE_SCORE_CONST) > 1e-4)
    hs = E.haplotag_sites()
    assert hs.dtype == _abi.HAPSITE_DTYPE and hs.tolist() == want["site"].tolist()
    rec = read_records(E)
    assert rec["row"].tolist() == list(range(len(pr["assignment"])))
    assert rec["haplotag"].tolist() == want["haplotag"].tolist() and rec["assignment"].tolist() == want["assignment"].tolist()
    assert rec["phase_set"].tolist() == want["phase_set"].tolist() and not rec["pad_"].any()
    dptr, dn = E.candidates_device()
    dev = np.zeros(dn, dtype=_abi.CAND_DTYPE)
    if dn:
        assert _lib.load().hipMemcpy(C.c_void_p(dev.ctypes.data), C.c_void_p(dptr), C.c_size_t(dev.nbytes), 2) == 0
    assert dev.tobytes() == got.tobytes()      # HBM and host hold the same records
    return want, pr, got, hs


# ---- 1. the hand-worked instance -----------------------------------------------------------------------------------------------------
HAND_COLS = (150, 300, 450, 600, 2050, 2200, 2350, 2500)


def hand_sites(start0, refseq, swapped=0, ps=4242):
    """haplotype 1 = the reference base at every site (haplotype A of the instance carries the alternate one); the first `swapped` reversed"""
    d = {}
    for k, c in enumerate(HAND_COLS):
        r = refseq[c].upper()
        d[start0 + c] = (tj.ALT[r], r, ps) if k < swapped else (r, tj.ALT[r], ps)
    return d


def test_hand_worked_instance(engine_cls):
    start0, refseq, rs = tj.allele_specific_region()
    b = tj.batch_of([(start0, refseq, rs)])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=7))
    is_a = np.array(["1100N" not in r["cigar"] for r in rs])      # haplotype A: the alternate base everywhere
    for swapped in (0, 3, 4):
        fm, cands0, _ = staged(E, b)
        assert sorted(int(p) - start0 for p in cands0["pos"]) == list(HAND_COLS)
        sites = site_arrays(hand_sites(start0, refseq, swapped))
        E.haplotag(sites)
        want, pr, got, hs = compare(E, fm, cands0, sites)
        rows_a = is_a[fm["row_read"]]
        if swapped < 4:     # 8 : 0 and 5 : 3 -- B's reads show haplotype 1's allele, A's haplotype 2's
            assert pr["assignment"][rows_a].tolist() == [2] * 20 and pr["assignment"][~rows_a].tolist() == [1] * 20
            assert pr["haplotag"][rows_a].tolist() == [-1] * 20 and set(pr["phase_set"].tolist()) == {4242}
            assert hs["n_h1"].tolist() == [20] * 8 and hs["n_h2"].tolist() == [20] * 8
            match = [0] * swapped + [20] * (8 - swapped)
            assert hs["n_h1_match"].tolist() == match and hs["n_h2_match"].tolist() == match
            assert got["haplotype"].tolist() == [-1] * swapped + [1] * (8 - swapped) and set(got["phase_set"].tolist()) == {4242}
        else:               # 4 : 4 at equal qualities: A1 == A2, no evidence even at cutoff 0.0
            assert float(E.params.read_assign_cutoff) == 0.0
            assert not pr["assignment"].any() and not pr["haplotag"].any() and not pr["phase_set"].any() and not hs["n_h1"].any()
            assert got["phase_score"].tolist() == [np.float64(ref.PHASE_SCORE_CONST)] * 8
    E.close()


# ---- 2. edges ------------------------------------------------------------------------------------------------------------------------
S17 = [60 + 40 * k for k in range(17)]
DENSE = tj.ANCHOR + [210, 220, 230, 240, 250, 260]
STARTS = (10000, 20000, 30000, 40000, 50000, 60000)


def edge_regions():
    r = []
    r.append(tj.build_region(10000, 700, [], tj.haps([(0, "600M")] * 8), 41))                                   # G0 no candidate
    lanes = [(0, "760M")] * 20 + [(0, "50M")] * 2 + [(0, "90M")] * 2 + [(0, "350M")] * 2 + [(0, "390M")] * 2     # G1 17, 0, 1, 8 and 9 entries
    r.append(tj.build_region(20000, 800, S17, tj.haps(lanes), 42))
    r.append(tj.build_region(30000, 700, tj.ANCHOR, tj.haps([(0, "600M")] * 20 + [(150, "450M")] * 4), 43))       # G2 two phase sets: 3 : 2 and 2 : 2
    r.append(tj.build_region(40000, 700, tj.ANCHOR, tj.haps([(0, "600M")] * 20), 44))                             # G3 the unusable sites and entries
    r.append(tj.build_region(50000, 700, DENSE, tj.haps([(0, "600M")] * 20), 45))                                 # G4 a dense cluster
    r.append(tj.build_region(60000, 700, tj.ANCHOR, tj.haps([(0, "600M")] * 3000), 46))                           # G5 3 000 rows
    return [(s,) + x for s, x in zip(STARTS, r)]


def edge_sites(cands):
    """A site at every candidate, haplotype 1 = REF except at every third site of a region; G2: columns 100 - 300 in set 9000 (the first
    reversed), 400 / 500 in set 7000; G3: column 100 with REF on neither haplotype, 200 with a third base as haplotype 2, 300 absent."""
    d, k_in = {}, {}
    for s in cands:
        g, p = int(s["region"]), int(s["pos"])
        k = k_in[g] = k_in.get(g, -1) + 1
        r, a = alt_of(s)
        third = [x for x in OTHER[r] if x != a][0]
        col = p - STARTS[g]
        if g == 2:
            d[p] = ((a, r) if col == 100 else (r, a)) + (9000 if col <= 300 else 7000,)
        elif g == 3 and col == 100:
            d[p] = (a, third, 1003)
        elif g == 3 and col == 200:
            d[p] = (r, third, 1003)
        elif g == 3 and col == 300:
            continue
        elif g == 3:
            d[p] = (r, a, 1003)
        else:
            d[p] = ((a, r) if k % 3 == 0 else (r, a)) + (1000 + g,)
    d[5] = ("A", "C", 1)                  # outside every region
    d[45000] = ("A", "C", 2)              # between two regions
    d[40650] = ("G", "T", 1003)           # inside a region, at no candidate
    d[99999999] = ("G", "T", 3)
    return d


def test_edges(engine_cls):
    regs = edge_regions()
    b = tj.batch_of(regs)
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    fm, cands0, coff = staged(E, b)
    rro, n_ent = fm["row_region_off"], np.diff(fm["row_ptr"])
    sites = site_arrays(edge_sites(cands0))
    E.haplotag(sites)
    want, pr, got, hs = compare(E, fm, cands0, sites)
    asg, ps = pr["assignment"], pr["phase_set"]
    col_of = lambda i: int(got["pos"][i]) - STARTS[int(got["region"][i])]
    # G0: no candidate, no row.  G1: the lane-group boundaries, every site usable
    assert coff[1] - coff[0] == 0 and rro[1] - rro[0] == 0
    assert coff[2] - coff[1] == 17 and want["usable"][coff[1]:coff[2]].all()
    e1 = n_ent[rro[1]:rro[2]]
    assert sorted(set(e1.tolist())) == [0, 1, 8, 9, 17] and (e1 == 17).sum() == 20
    a1 = asg[rro[1]:rro[2]]
    assert not a1[e1 == 0].any() and a1[e1 == 1].all() and a1[e1 == 8].all() and a1[e1 == 9].all() and a1[e1 == 17].all()
    assert set(ps[rro[1]:rro[2]][e1 > 0].tolist()) == {1001}
    # G2: 3 entries against 2 -> the larger set although its value is larger; 2 against 2 -> the smaller value, and only its entries count
    r2 = np.arange(rro[2], rro[3])
    full, part = r2[n_ent[r2] == 5], r2[n_ent[r2] == 4]
    assert full.size == 20 and part.size == 4 and set(ps[full].tolist()) == {9000} and set(ps[part].tolist()) == {7000} and asg[r2].all()
    c2 = {col_of(i): i for i in range(coff[2], coff[3])}
    assert [int(hs["n_h1"][c2[c]] + hs["n_h2"][c2[c]]) for c in (100, 200, 300, 400, 500)] == [20, 20, 20, 4, 4]
    # G3: REF on neither haplotype / absent from pos0 -> not usable, NON_SELECTED; a third base as haplotype 2 -> only REF reads have an entry
    c3 = {col_of(i): i for i in range(coff[3], coff[4])}
    assert [bool(want["usable"][c3[c]]) for c in (100, 200, 300, 400, 500)] == [False, True, False, True, True]
    for c in (100, 300):
        i = c3[c]
        assert got["flags"][i] == cands0["flags"][i] | _abi.F_NON_SELECTED and got["haplotype"][i] == 0 and got["phase_set"][i] == 0 and got["phase_score"][i] == 0
        assert hs[i].tolist() == (0, 0, 0, 0, 0, 0)
    assert (int(hs["n_h1"][c3[200]]), int(hs["n_h2"][c3[200]])) in ((10, 0), (0, 10)) and int(hs["n_h1"][c3[400]] + hs["n_h2"][c3[400]]) == 20
    assert got["phase_score"][c3[200]] == ref.PHASE_SCORE_CONST and asg[rro[3]:rro[4]].all()
    # G4: the dense candidates are left as they were, with NON_SELECTED
    dense = (cands0["flags"][coff[4]:coff[5]] & _abi.F_DENSE) != 0
    assert dense.sum() >= 5 and not dense.all() and not want["usable"][coff[4]:coff[5]][dense].any() and want["usable"][coff[4]:coff[5]][~dense].all()
    assert ((got["flags"][coff[4]:coff[5]][dense] & _abi.F_NON_SELECTED) != 0).all()
    # G5: 3 000 rows, all assigned, 1 500 on each haplotype
    a5 = asg[rro[5]:rro[6]]
    assert a5.size == 3000 and (a5 == 1).sum() == 1500 and (a5 == 2).sum() == 1500
    assert hs["n_h1"][coff[5]:coff[6]].tolist() == [1500] * 5 and hs["n_h2"][coff[5]:coff[6]].tolist() == [1500] * 5

    # min_linkers 2: the rows with one counted entry drop out, nothing else moves
    E2 = engine_cls(0, _abi.make_params("hifi-masseq", seed=5, min_linkers=2))
    fm2, c02, _ = staged(E2, b)
    assert fm2["col"].tobytes() == fm["col"].tobytes()
    E2.haplotag(sites)
    w2, pr2, _, _ = compare(E2, fm2, c02, sites)
    one = np.flatnonzero(n_ent == 1)
    assert one.size == 2 and asg[one].all() and not pr2["assignment"][one].any()
    rest = np.delete(np.arange(asg.size), one)
    assert pr2["assignment"][rest].tolist() == asg[rest].tolist()
    E2.close()

    # read_assign_cutoff on either side of a G2 row's margin: one entry of haplotype 1 against two of haplotype 2, all q = 30
    fe, f1e = ref.FE[30], ref.F1E[30]
    a1, a2 = f1e + 2 * fe, fe + 2 * f1e
    ratio = abs(a1 - a2) / abs(a1 + a2)
    assert 0.33 < ratio < 0.3334
    for cut, assigned in ((ratio * (1 - 1e-9), True), (ratio * (1 + 1e-9), False)):
        Ec = engine_cls(0, _abi.make_params("hifi-masseq", seed=5, read_assign_cutoff=cut))
        fmc, c0c, _ = staged(Ec, b)
        Ec.haplotag(sites)
        wc, prc, _, _ = compare(Ec, fmc, c0c, sites)
        assert bool(wc["assignment"][full].all()) == assigned and bool(wc["assignment"][full].any()) == assigned
        assert prc["assignment"][part].all()      # (two entries of one haplotype: margin 0.9997)
        Ec.close()

    # imported candidates with genotype codes 2 and 3 beside 1: left as the import wrote them, with NON_SELECTED
    ipos = cands0["pos"].astype(np.int64)
    igt = np.array([(1, 1, 2, 3)[k % 4] for k in range(ipos.size)], np.uint8)
    fmi, c0i, _ = staged(E, b, (ipos, igt, np.full(ipos.size, 30.0, np.float32)))
    assert sorted(set(c0i["variant_type"].tolist())) == [1, 2, 3]
    E.haplotag(sites)
    wi, pri, goti, _ = compare(E, fmi, c0i, sites)
    other = c0i["variant_type"] != 1
    assert not wi["usable"][other].any() and wi["usable"][~other].any() and pri["assignment"].any()
    assert (goti["flags"][other] == (c0i["flags"][other] | _abi.F_NON_SELECTED)).all() and not goti["haplotype"][other].any()

    # no site at all: every row unassigned, every candidate NON_SELECTED
    fm0, c00, _ = staged(E, b)
    E.haplotag(None)
    w0, pr0, got0, hs0 = compare(E, fm0, c00, None)
    assert not pr0["assignment"].any() and ((got0["flags"] & _abi.F_NON_SELECTED) != 0).all() and not hs0["n_h1"].any()
    empty = tuple(a[:0] for a in sites)
    fm0, c00, _ = staged(E, b)
    E.haplotag(empty)
    compare(E, fm0, c00, None)

    # an RNA-editing candidate (A > G on '+' transcripts) is left as it was
    br, _ = helpers.two_haplotype_batch(n_snps=5, n_reads=60, edit_sites=(777,), edit_frac=0.95, seed=2)
    br.flags[:] = 0 | (1 << 1)
    fmr, c0r, _ = staged(E, br)
    edit = (c0r["flags"] & _abi.F_RNA_EDIT) != 0
    assert edit.sum() == 1
    sr = site_arrays({int(s["pos"]): alt_of(s) + (77,) for s in c0r})
    E.haplotag(sr)
    wr, prr, gotr, _ = compare(E, fmr, c0r, sr)
    assert not wr["usable"][edit].any() and wr["usable"][~edit].all() and prr["assignment"].all()
    E.close()


# ---- 3. round trip through lcr_phase -------------------------------------------------------------------------------------------------
def test_round_trip_through_phase(engine_cls):
    b = tj.batch_of([tj.allele_specific_region()])
    prm = _abi.make_params("hifi-masseq", seed=7)
    A = engine_cls(0, prm)
    A.load_batch(b).run_all()
    pa = A.phase_result()
    ca, _ = A.candidates()
    A.close()
    assert pa["assignment"].all()
    d = {}
    for s in ca:
        if int(s["haplotype"]) != 0 and int(s["genotype"]) == 0 and int(s["flags"]) & _abi.F_FOR_PHASING:
            r, a = alt_of(s)
            d[int(s["pos"])] = ((r, a) if int(s["haplotype"]) == 1 else (a, r)) + (int(s["phase_set"]) or 1,)
    assert len(d) == 8
    B = engine_cls(0, prm)
    fm, cands0, _ = staged(B, b)
    sites = site_arrays(d)
    B.haplotag(sites)
    want, pb, cb, _ = compare(B, fm, cands0, sites)
    B.close()
    assert pb["assignment"].tolist() == pa["assignment"].tolist() and pb["haplotag"].tolist() == pa["haplotag"].tolist()
    assert cb["haplotype"].tolist() == ca["haplotype"].tolist() and pb["phase_set"].tolist() == pa["phase_set"].tolist()


# ---- 4. synthetic and real data ------------------------------------------------------------------------------------------------------
def sites_from_candidates(batch, cands, seed):
    """a site at every candidate, REF / ALT in a seeded order, one of two seeded phase-set values; beside them positions that are no
    candidate and positions outside every region"""
    rng = np.random.default_rng(seed)
    sets = [int(x) for x in rng.integers(1, 1 << 32, size=2)]
    d = {}
    for s in cands:
        r, a = alt_of(s)
        d[int(s["pos"])] = ((r, a) if rng.random() < 0.5 else (a, r)) + (sets[int(rng.random() < 0.3)],)
    for g in range(batch.n_regions):
        for p in rng.integers(int(batch.start0[g]), int(batch.start0[g]) + int(batch.len[g]), size=20).tolist():
            d.setdefault(p, ("A", "C", sets[0]))
    for p in (0, int(batch.start0[0]) - 1, int(batch.start0[-1]) + int(batch.len[-1]) + 12345):
        if p >= 0:
            d.setdefault(p, ("G", "T", sets[1]))
    return d


@pytest.mark.parametrize("which", ["ont-cdna", "masseq", "demo"])
def test_synth_and_demo(engine_cls, which):
    if which == "demo":
        b, prm = helpers.demo_batch(), _abi.make_params("hifi-masseq")
    else:
        b, prm = synth.make_batch(which, n_genes=4), _abi.make_params(synth.preset_for(which))
    E = engine_cls(0, prm)
    fm, cands0, _ = staged(E, b)
    sites = site_arrays(sites_from_candidates(b, cands0, 11))
    E.haplotag(sites)
    want, pr, got, hs = compare(E, fm, cands0, sites)
    sets = sorted(set(pr["phase_set"].tolist()) - {0})
    print("%s: rows %d, assigned %d, candidates %d, usable %d, phase sets %r" % (which, pr["assignment"].size, int((pr["assignment"] != 0).sum()),
                                                                                 cands0.size, int(want["usable"].sum()), sets))
    assert want["usable"].any() and pr["assignment"].any() and (which == "demo" or len(sets) == 2)
    E.close()


# ---- 5. independence from the batch's composition ------------------------------------------------------------------------------------
def test_region_alone_and_in_the_batch(engine_cls):
    regs = edge_regions()[:4]
    b = tj.batch_of(regs)
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    fm, cands0, coff = staged(E, b)
    sites = site_arrays(edge_sites(cands0))
    E.haplotag(sites)
    _, pr, got, hs = compare(E, fm, cands0, sites)
    rro = fm["row_region_off"]
    for g in (1, 2):
        fm1, c01, _ = staged(E, tj.batch_of([regs[g]]))
        E.haplotag(sites)      # (the other regions' sites lie outside this batch's one region)
        _, pr1, got1, hs1 = compare(E, fm1, c01, sites)
        for f in ("haplotag", "assignment", "phase_set"):
            assert pr1[f].tobytes() == pr[f][rro[g]:rro[g + 1]].tobytes(), (g, f)
        assert hs1.tobytes() == hs[coff[g]:coff[g + 1]].tobytes()
        for f in _abi.CAND_DTYPE.names:
            if f != "region":
                assert got1[f].tobytes() == got[f][coff[g]:coff[g + 1]].tobytes(), (g, f)
    E.close()


# ---- 6. device-resident sites ---------------------------------------------------------------------------------------------------------
def test_device_resident_sites(engine_cls):
    import torch
    b = tj.batch_of(edge_regions()[1:4])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    fm, cands0, _ = staged(E, b)
    sites = site_arrays(edge_sites_shifted(cands0))
    E.haplotag(sites)
    _, pr, got, hs = compare(E, fm, cands0, sites)
    fm, cands0, _ = staged(E, b)
    dev = (torch.from_numpy(sites[0]).cuda(), torch.from_numpy(sites[1]).cuda(), torch.from_numpy(sites[2]).cuda(),
           torch.from_numpy(sites[3].view(np.int32)).cuda())
    E.haplotag(dev)
    _, prd, gotd, hsd = compare(E, fm, cands0, sites)
    assert prd["assignment"].tobytes() == pr["assignment"].tobytes() and gotd.tobytes() == got.tobytes() and hsd.tobytes() == hs.tobytes()
    # bad device sites are found by the check kernel; the stage behind the call still runs with good ones
    fm, cands0, _ = staged(E, b)
    bad = (dev[0].flip(0).contiguous(),) + dev[1:]
    with pytest.raises(Exception, match="sorted by position"):
        E.haplotag(bad)
    E.haplotag(dev)
    compare(E, fm, cands0, sites)
    E.sync()
    E.close()


def edge_sites_shifted(cands):
    """edge_sites for a batch that starts at edge region 1: the region index of a candidate is one lower"""
    c = cands.copy()
    c["region"] += 1
    return edge_sites(c)


# ---- 7. order and lifetime on one context ---------------------------------------------------------------------------------------------
def snapshot(E):
    pr, (c, off), fm = E.phase_result(), E.candidates(), E.fragmat()
    return [pr[k].tobytes() for k in sorted(pr)] + [c.tobytes(), off.tobytes()] + [fm[k].tobytes() for k in sorted(fm)]


def test_order_and_lifetime(engine_cls):
    start0, refseq, rs = tj.allele_specific_region()
    b1, b2 = tj.batch_of([(start0, refseq, rs)]), tj.batch_of(edge_regions()[2:4])
    prm = _abi.make_params("hifi-masseq", seed=7)
    E = engine_cls(0, prm)
    lib = E.lib
    good = site_arrays(hand_sites(start0, refseq, 3))

    def call(pos, h1, h2, ps, mem=_abi.LCR_MEM_HOST):
        pos, ps = np.array(pos, np.int64), np.array(ps, np.uint32)
        h1, h2 = np.frombuffer(h1, np.uint8), np.frombuffer(h2, np.uint8)
        return lib.lcr_haplotag(E.h, C.byref(E.params), mem, pos.size, pos.ctypes.data, h1.ctypes.data, h2.ctypes.data, ps.ctypes.data)
    n, p1, p2 = C.c_int32(), C.c_void_p(), C.c_void_p()
    get_sites = lambda: lib.lcr_get_haplotag_sites(E.h, C.byref(n), C.byref(p1), C.byref(p2))
    E.load_batch(b1).fill_data_into_freq_vec().get_candidate_snps()
    assert call([4, 5], b"AA", b"CC", [1, 1]) == E_STATE and get_sites() == E_STATE          # before lcr_fragments
    E.get_fragments()
    fm, (cands0, coff) = E.fragmat(), E.candidates()
    before = [cands0.tobytes(), coff.tobytes()] + [fm[k].tobytes() for k in sorted(fm)]
    # refused arguments: LCR_E_ARG, nothing changed
    assert lib.lcr_haplotag(E.h, None, 0, 0, None, None, None, None) == E_ARG
    assert lib.lcr_haplotag(E.h, C.byref(E.params), 2, 0, None, None, None, None) == E_ARG
    assert lib.lcr_haplotag(E.h, C.byref(E.params), 0, -1, None, None, None, None) == E_ARG
    assert lib.lcr_haplotag(E.h, C.byref(E.params), 0, 2, None, None, None, None) == E_ARG
    assert call([5, 4], b"AA", b"CC", [1, 1]) == E_ARG and call([5, 5], b"AA", b"CC", [1, 1]) == E_ARG      # unsorted, duplicate
    assert call([4, 5], b"AC", b"CC", [1, 1]) == E_ARG and call([4, 5], b"AN", b"CC", [1, 1]) == E_ARG      # h1 == h2, outside ACGT
    assert call([4, 5], b"Aa", b"CC", [1, 1]) == E_ARG and call([4, 5], b"AA", b"CC", [1, 0]) == E_ARG      # lower case, phase set 0
    assert b"sorted by position" in lib.lcr_last_error(E.h)
    fm_, (c_, off_) = E.fragmat(), E.candidates()
    assert before == [c_.tobytes(), off_.tobytes()] + [fm_[k].tobytes() for k in sorted(fm_)]
    assert lib.lcr_get_phase_result(E.h, C.byref(_abi.LcrPhaseResult())) == E_STATE and get_sites() == E_STATE
    # the call; a second one, lcr_phase and lcr_fragments behind it are refused and change nothing
    E.haplotag(good)
    want, pr, got, hs = compare(E, fm, cands0, good)
    snap = snapshot(E)
    assert call(*[x.tolist() if x.dtype != np.uint8 else x.tobytes() for x in (good[0], good[1], good[2], good[3])]) == E_STATE
    assert lib.lcr_phase(E.h, C.byref(E.params)) == E_STATE and lib.lcr_fragments(E.h, C.byref(E.params)) == E_STATE
    assert snapshot(E) == snap and get_sites() == 0 and n.value == 8
    # the consumers of the phase results: the junction and expression tables of the restatements fed with these results
    j, joff = E.junctions(10, 0)
    wj, wjoff = asj_ref.junctions(b1, fm["row_region_off"], fm["row_read"], pr["assignment"], pr["phase_set"], 10, 0)
    assert tj.tuples(j) == tj.tuples(wj) and joff.tolist() == wjoff.tolist() and j.size == 3
    par = {int(p): (chr(a), chr(c)) for p, a, c in zip(good[0], good[1], good[2])}
    a = E.ase((good[0], good[1], good[2]), 13, 0.0)
    wa = ase_ref.regions(fm, pr["assignment"], pr["phase_set"], got, coff, par, 13, 0.0)
    assert a.tolist() == wa.tolist() and a["h1"][0] == 20 and a["h2"][0] == 20 and a["n_sites"][0] == 8
    assert (a["h1_pat"][0], a["h1_mat"][0], a["h2_pat"][0], a["h2_mat"][0]) == (20, 0, 0, 20)      # haplotype 1 IS the sites' first allele
    assert snapshot(E) == snap
    # lcr_collect_phase delivers them, also behind the next batch's binding; load_batch rewinds the rest
    E.load_batch(b2)
    res = E.collect_phase(copy=True)
    assert res["assignment"].tobytes() == pr["assignment"].tobytes() and res["phase_set"].tobytes() == pr["phase_set"].tobytes()
    assert res["haplotag"].tobytes() == pr["haplotag"].tobytes() and res["cand"].tobytes() == got.tobytes() and not res["objective"].any()
    assert get_sites() == E_STATE and lib.lcr_get_phase_result(E.h, C.byref(_abi.LcrPhaseResult())) == E_STATE
    assert call([4, 5], b"AA", b"CC", [1, 1]) == E_STATE
    # a later candidate stage and lcr_phase on this context: what a context that never haplotagged gives, byte for byte
    E.fill_data_into_freq_vec().get_candidate_snps().get_fragments().phase()
    F = engine_cls(0, prm)
    F.load_batch(b2).run_all()
    assert snapshot(E) == snapshot(F) and E.tie_census() == F.tie_census()
    assert get_sites() == E_STATE
    F.close()
    # ... and a haplotag behind a phase on one context, timed
    T = engine_cls(0, prm, timing=True)
    with pytest.raises(Exception):
        T.haplotag_ms()
    fm, cands0, _ = staged(T, b1)
    T.haplotag(good)
    compare(T, fm, cands0, good)
    assert T.haplotag_ms() > 0.0
    T.close()
    E.close()

"""K12 lcr_site_counts on the GPU against the plain-Python restatement of its contract (tests/site_counts_ref.py): every field of every
record, exactly, in pinned host memory and in HBM.  Rows are put on chosen haplotypes and phase sets with Engine.haplotag and hand-picked
sites; the contract's worked instance, the lane-group boundaries of columns and rows, the phase-set rules at unphased and phased sites,
the quality threshold, dense / RNA-edit / triallelic candidates, synthetic and real data behind lcr_phase, independence from the batch,
and the call's order and lifetime on one context."""
import ctypes as C

import numpy as np
import pytest

import helpers
import site_counts_ref as ref
import test_haplotag_gpu as th
import test_junctions_gpu as tj
from longcallr_amd import _abi, _lib, synth

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def region(start0, length, forced, reads, seed):
    """A region's random reference with `forced` = {column: base} written into it, and its reads.  reads: [(segments, bases, quals)] --
    segments [(lo, hi)] of region columns joined by N, bases {column: base} in place of the reference's, quals {column: q} in place of 30.
    -> (start0, reference, read dicts sorted by position; "k" is the read's index in `reads`)"""
    rng = np.random.default_rng(seed)
    refseq = list(rng.choice(list("ACGT"), size=length))
    for c, x in forced.items():
        refseq[c] = x
    out = []
    for k, (segs, bases, quals) in enumerate(reads):
        seq, q, cig, prev = [], [], "", None
        for lo, hi in segs:
            assert 0 <= lo < hi <= length and (prev is None or lo > prev)
            if prev is not None:
                cig += "%dN" % (lo - prev)
            cig += "%dM" % (hi - lo)
            seq += [bases.get(c, refseq[c]) for c in range(lo, hi)]
            q += [quals.get(c, 30) for c in range(lo, hi)]
            prev = hi
        out.append(dict(pos=start0 + segs[0][0], seq="".join(seq), qual=q, cigar=cig, rev=k // 2 % 2, ts=1 + (k // 2 % 2), k=k))
    out.sort(key=lambda r: r["pos"])
    return start0, "".join(refseq), out


def hap_bases(refseq, cols, h2):
    """the reference base (haplotype 1) or its tj.ALT (haplotype 2) at every column of `cols` a read covers"""
    return {c: tj.ALT[refseq[c]] for c in cols} if h2 else {}


def dev_records(E):
    n, rec, dev = C.c_int32(), C.c_void_p(), C.c_void_p()
    assert E.lib.lcr_get_site_counts(E.h, C.byref(n), C.byref(rec), C.byref(dev)) == 0
    out = np.zeros(n.value, dtype=_abi.SITE_COUNT_DTYPE)
    if n.value:
        assert _lib.load().hipMemcpy(C.c_void_p(out.ctypes.data), dev, C.c_size_t(out.nbytes), 2) == 0
    return out


def check(E, fm, min_baseq=13, assignment=None, phase_set=None):
    """site_counts() against the restatement on the engine's own phase results (or the given per-row arrays), host and HBM"""
    pr = E.phase_result()
    cands, _ = E.candidates()
    got = E.site_counts(min_baseq)
    want = ref.site_counts(fm["row_ptr"], fm["col"], fm["val"], pr["assignment"] if assignment is None else assignment,
                           pr["phase_set"] if phase_set is None else phase_set, cands["phase_set"], min_baseq)
    assert got.dtype == _abi.SITE_COUNT_DTYPE and got.size == cands.size
    for f in _abi.SITE_COUNT_DTYPE.names:
        assert got[f].tolist() == want[f].tolist(), f
    assert dev_records(E).tobytes() == got.tobytes()       # HBM and host hold the same records
    assert (got["n"].reshape(len(got), 12).sum(axis=1) + got["n_lowq"]).tolist() == got["n_entries"].tolist()
    assert got["n_entries"].tolist() == np.bincount(fm["col"], minlength=cands.size).tolist()
    return got, cands, pr


def imported(E, batch, cols_by_region, starts):
    """the batch staged with a het site imported at every listed column"""
    pos = np.array(sorted(s + c for s, cols in zip(starts, cols_by_region) for c in cols), np.int64)
    return th.staged(E, batch, (pos, np.ones(pos.size, np.uint8), np.full(pos.size, 30.0, np.float32)))


def cells(rec):
    return [[int(x) for x in row] for row in rec["n"]]


# ---- 1. the worked instance of the contract -------------------------------------------------------------------------------------------
W_SET100, W_SET200, W_X = (100, 200, 300), (400, 500, 600), 350


def worked_region(start0=5000):
    """the seven rows of the instance at column 350 (reference A), and twelve rows that anchor the two phase sets without covering it"""
    forced = {W_X: "A"}
    probe = region(start0, 700, forced, [], 21)[1]
    left, right = [(40, 360)], [(340, 660)]
    spec = [(left, False, "A", 30), (left, False, "G", 30), (left, True, "G", 12), (right, True, "G", 30), (right, True, "A", 30),
            ([(330, 370)], False, "A", 20), ([(330, 370)], False, "G", 30)]
    reads = [(segs, {**hap_bases(probe, W_SET100 + W_SET200, h2), W_X: x}, {W_X: q}) for segs, h2, x, q in spec]
    for k in range(6):
        reads.append(([(40, 340)], hap_bases(probe, W_SET100, k % 2), {}))
        reads.append(([(360, 660)], hap_bases(probe, W_SET200, k % 2), {}))
    return region(start0, 700, forced, reads, 21)


def test_worked_instance(engine_cls):
    start0, refseq, rs = worked_region()
    b = tj.batch_of([(start0, refseq, rs)])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=7, min_linkers=2, dist_to_end=0))
    anchors = {start0 + c: (refseq[c], tj.ALT[refseq[c]], 100 if c in W_SET100 else 200) for c in W_SET100 + W_SET200}
    want_meta = {(0, 13): (100, 2, 7, 1), (0, 0): (100, 2, 7, 0), (200, 13): (200, 2, 7, 1)}
    want_cells = {(0, 13): [[2, 0, 2, 0], [1, 0, 1, 0], [0, 0, 0, 0]], (0, 0): [[2, 0, 2, 0], [1, 0, 1, 0], [0, 0, 1, 0]],
                  (200, 13): [[2, 0, 2, 0], [0, 0, 0, 0], [1, 0, 1, 0]]}
    for own in (0, 200):
        fm, cands0, _ = imported(E, b, [W_SET100 + W_SET200 + (W_X,)], [start0])
        sites = dict(anchors)
        if own:
            sites[start0 + W_X] = ("A", "G", own)
        E.haplotag(th.site_arrays(sites))
        pr = E.phase_result()
        row_of = {rs[int(r)]["k"]: row for row, r in enumerate(fm["row_read"])}
        asg, ps = pr["assignment"].copy(), pr["phase_set"].copy()
        assert [(int(asg[row_of[k]]), int(ps[row_of[k]])) for k in range(7)] == [(1, 100), (1, 100), (2, 100), (2, 200), (2, 200), (0, 0), (0, 0)]
        # row 6 of the instance is assigned without a phase set: no stage of this library's leaves such a row behind lcr_haplotag, so its
        # read record is written in HBM here, as a caller of the C ABI who holds the records could
        ptr, n = E.read_records_device()
        one = np.zeros(1, dtype=_abi.READ_REC_DTYPE)
        one["row"], one["haplotag"], one["assignment"], one["phase_set"] = row_of[6], 1, 1, 0
        assert _lib.load().hipMemcpy(C.c_void_p(ptr + 12 * row_of[6]), C.c_void_p(one.ctypes.data), C.c_size_t(12), 1) == 0
        asg[row_of[6]] = 1
        x = int(np.flatnonzero(E.candidates()[0]["pos"] == start0 + W_X)[0])
        assert int(E.candidates()[0]["phase_set"][x]) == own
        for q in (13, 0) if own == 0 else (13,):
            got, _, _ = check(E, fm, q, asg, ps)
            r = got[x]
            assert (int(r["phase_set"]), int(r["n_phase_sets"]), int(r["n_entries"]), int(r["n_lowq"])) == want_meta[(own, q)], (own, q)
            assert cells(r) == want_cells[(own, q)], (own, q)
    E.close()


# ---- 2. the edges of test_haplotag_gpu's batch: rows of 0 / 1 / 8 / 9 / 17 entries, two sets in a region, a dense cluster, 3 000 rows ----
def test_called_edges(engine_cls):
    regs = th.edge_regions()
    b = tj.batch_of(regs)
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    fm, cands0, coff = th.staged(E, b)
    E.haplotag(th.site_arrays(th.edge_sites(cands0)))
    got, cands, pr = check(E, fm, 13)
    rro, n_ent = fm["row_region_off"], np.diff(fm["row_ptr"])
    assert sorted(set(n_ent[rro[1]:rro[2]].tolist())) == [0, 1, 8, 9, 17]
    # the dense candidates: no entry, a zero record with the candidate's own set (0: lcr_haplotag leaves them unphased)
    dense = (cands["flags"] & _abi.F_DENSE) != 0
    assert dense.sum() >= 5 and not got["n_entries"][dense].any() and not got["n"][dense].any()
    assert got["phase_set"][dense].tolist() == cands["phase_set"][dense].tolist() and not got["n_phase_sets"][dense].any()
    # G2's sites: the rows of both sets meet at columns 200 - 500; the phased ones keep their own set
    c2 = {int(cands["pos"][i]) - th.STARTS[2]: i for i in range(coff[2], coff[3])}
    assert [int(got["n_phase_sets"][c2[c]]) for c in (100, 200, 300, 400, 500)] == [1, 2, 2, 2, 2]
    assert [int(got["phase_set"][c2[c]]) for c in (100, 300, 400)] == [9000, 9000, 7000]
    assert int(got["n"][c2[400]][1:].sum()) == 4 and int(got["n"][c2[400]][0].sum()) == 20       # the 20 rows of set 9000 are "other" at a site of 7000
    # G5: one column of 3 000 rows, 1 500 per haplotype
    g5 = got[coff[5]:coff[6]]
    assert g5["n_entries"].tolist() == [3000] * 5 and [int(r["n"][1].sum()) for r in g5] == [1500] * 5 and [int(r["n"][2].sum()) for r in g5] == [1500] * 5
    for q in (0, 30):
        check(E, fm, q)
    E.close()


# ---- 3. imported sites: column depths, the phase-set rules, the quality threshold, a triallelic column --------------------------------
DEPTH_COLS = (100, 200, 300, 400, 500, 600)       # 129, 65, 64, 63, 1 and 0 entries
SET_P, SET_Q, SET_R = 2000, 1000, 3000
ANCH_P, ANCH_Q, ANCH_R = (100, 150, 200), (320, 360, 400), (500, 550, 600)
TARGETS = (250, 260, 270, 280, 290)
TRI_COLS = (100, 200, 300)
STARTS3 = (70000, 80000, 90000)


def depth_region():
    """129 reads from column 0: one of 550 columns, 62 of 450, one of 350, one of 250, 64 of 150; at column 100 the qualities 12, 13, 29, 30"""
    probe = region(STARTS3[0], 700, {}, [], 31)[1]
    lens = [550] + [450] * 62 + [350, 250] + [150] * 64
    reads = [([(0, n)], hap_bases(probe, DEPTH_COLS, k % 2), {100: (12, 13, 29, 30)[k % 4]}) for k, n in enumerate(lens)]
    return region(STARTS3[0], 700, {}, reads, 31)


def sets_region():
    """three phase sets P (2000), Q (1000), R (3000) with three anchor sites each, and five target sites that their rows cover unevenly:
    column 250: P 3, Q 2    260: P 2, Q 2    270: P 1, Q 2, R 3    280: P 1, Q 3    290: P 1, Q 3"""
    probe = region(STARTS3[1], 700, {}, [], 32)[1]
    segs = [[(60, 300)], [(60, 265)], [(60, 255)], [(245, 440)], [(245, 440)], [(275, 440)]] + [[(265, 275), (460, 640)]] * 3
    reads = [(s, hap_bases(probe, ANCH_P + ANCH_Q + ANCH_R + TARGETS, k % 2), {}) for k, s in enumerate(segs)]
    return region(STARTS3[1], 700, {}, reads, 32)


def tri_region():
    """column 300, reference A: six reads with C, six with G, three with A -- the two major alleles and the reference"""
    forced = {300: "A"}
    probe = region(STARTS3[2], 700, forced, [], 33)[1]
    reads = [([(0, 400)], {**hap_bases(probe, TRI_COLS[:2], k % 2), 300: "CGCGCGCGCGCGAAA"[k]}, {}) for k in range(15)]
    return region(STARTS3[2], 700, forced, reads, 33)


def imported_regions():
    return [depth_region(), sets_region(), tri_region()]


def imported_sites(regs, which=(0, 1, 2)):
    """haplotype 1 = the reference base everywhere.  Depth region: one set; sets region: the anchors in their sets, target 280 in P and
    290 in R, the other targets absent (unphased); triallelic region: the two anchors"""
    d = {}
    for g in which:
        s0, refseq, _ = regs[g]
        site = lambda c, ps: d.__setitem__(s0 + c, (refseq[c], tj.ALT[refseq[c]], ps))
        if g == 0:
            for c in DEPTH_COLS:
                site(c, 500)
        elif g == 1:
            for cols, ps in ((ANCH_P, SET_P), (ANCH_Q, SET_Q), (ANCH_R, SET_R), ((280,), SET_P), ((290,), SET_R)):
                for c in cols:
                    site(c, ps)
        else:
            for c in TRI_COLS[:2]:
                site(c, 600)
    return th.site_arrays(d)


IMPORT_COLS = [DEPTH_COLS, ANCH_P + ANCH_Q + ANCH_R + TARGETS, TRI_COLS]


def test_imported_edges(engine_cls):
    regs = imported_regions()
    b = tj.batch_of(regs)
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5, dist_to_end=0))
    fm, cands0, coff = imported(E, b, IMPORT_COLS, STARTS3)
    E.haplotag(imported_sites(regs))
    got, cands, pr = check(E, fm, 13)
    at = lambda g, c: int(np.flatnonzero(cands["pos"] == STARTS3[g] + c)[0])
    # column depths on either side of the 64 lanes of a site's wave, twice that plus one, one and none
    assert [int(got["n_entries"][at(0, c)]) for c in DEPTH_COLS] == [129, 65, 64, 63, 1, 0]
    z = got[at(0, 600)]       # no read reaches it: a zero record with the candidate's own set
    assert (int(z["phase_set"]), int(z["n_phase_sets"]), int(z["n_lowq"])) == (500, 0, 0) and not z["n"].any()
    # the threshold at column 100: q = 12 / 13 / 29 / 30 on every fourth read
    n12 = sum(1 for k in range(129) if k % 4 == 0)
    n_lt30 = sum(1 for k in range(129) if k % 4 != 3)
    a = at(0, 100)
    assert int(got["n_lowq"][a]) == n12 and not got["n_lowq"][at(0, 200)]
    got0, _, _ = check(E, fm, 0)
    got30, _, _ = check(E, fm, 30)
    got12, _, _ = check(E, fm, 12)
    assert int(got0["n_lowq"][a]) == 0 and int(got12["n_lowq"][a]) == 0 and int(got30["n_lowq"][a]) == n_lt30
    assert int(got0["n"][a].sum()) == 129 and int(got30["n"][a].sum()) == 129 - n_lt30
    # 31 is refused and leaves the previous records valid
    p31 = _abi.LcrSiteCountParams(31)
    assert E.lib.lcr_site_counts(E.h, C.byref(p31)) == E_ARG and b"min_baseq" in E.lib.lcr_last_error(E.h)
    assert E.lib.lcr_site_counts(E.h, None) == E_ARG
    assert dev_records(E).tobytes() == got12.tobytes()
    got, _, _ = check(E, fm, 13)
    # the phase-set rules
    t = {c: got[at(1, c)] for c in TARGETS}
    assert [int(t[c]["n_entries"]) for c in TARGETS] == [5, 4, 6, 4, 4]
    assert [(int(t[c]["phase_set"]), int(t[c]["n_phase_sets"])) for c in TARGETS] == [(SET_P, 2), (SET_Q, 2), (SET_R, 3), (SET_P, 2), (SET_R, 2)]
    assert [int(t[c]["n"][1:].sum()) for c in TARGETS] == [3, 2, 3, 1, 0]         # the rows of the site's set; at 280 the minority, at 290 none
    assert [int(t[c]["n"][0].sum()) for c in TARGETS] == [2, 2, 3, 3, 4]
    assert [int(cands["phase_set"][at(1, c)]) for c in TARGETS] == [0, 0, 0, SET_P, SET_R]
    # the triallelic column: three bases in the cells
    r = got[at(2, 300)]
    by_base = r["n"].sum(axis=0).tolist()
    assert by_base == [3, 6, 6, 0] and int(r["n_entries"]) == 15
    E.close()


def test_region_alone_and_in_the_batch(engine_cls):
    regs = imported_regions()
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5, dist_to_end=0))
    fm, _, coff = imported(E, tj.batch_of(regs), IMPORT_COLS, STARTS3)
    E.haplotag(imported_sites(regs))
    got, _, _ = check(E, fm, 13)
    for g in (0, 1, 2):
        fm1, _, _ = imported(E, tj.batch_of([regs[g]]), [IMPORT_COLS[g]], [STARTS3[g]])
        E.haplotag(imported_sites(regs, (g,)))
        got1, _, _ = check(E, fm1, 13)
        assert got1.tobytes() == got[coff[g]:coff[g + 1]].tobytes(), g
    E.close()


# ---- 4. behind lcr_phase: RNA-edit candidates, synthetic and real data ----------------------------------------------------------------
def test_rna_edit_candidates(engine_cls):
    b, _ = helpers.two_haplotype_batch(n_snps=5, n_reads=60, edit_sites=(777,), edit_frac=0.95, seed=2)
    b.flags[:] = 0 | (1 << 1)
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=3))
    fm, cands0, _ = th.staged(E, b)
    edit = (cands0["flags"] & _abi.F_RNA_EDIT) != 0       # (as the candidate stage classified it)
    E.phase()
    got, cands, pr = check(E, fm, 13)
    assert edit.sum() == 1 and pr["assignment"].any()
    r = got[np.flatnonzero(edit)[0]]
    print("RNA-edit candidate: %r" % (r.tolist(),))
    # the edited base sits on haplotype A's reads only: whatever the matrix holds of the site, G is on one haplotype
    assert int(r["n_entries"]) == int(np.count_nonzero(fm["col"] == np.flatnonzero(edit)[0]))
    assert min(int(r["n"][1][CODE["G"]]), int(r["n"][2][CODE["G"]])) == 0
    E.close()


@pytest.mark.parametrize("which", ["ont-cdna", "masseq", "demo"])
def test_synth_and_demo(engine_cls, which):
    if which == "demo":
        b, prm = helpers.demo_batch(), _abi.make_params("hifi-masseq")
    else:
        b, prm = synth.make_batch(which, n_genes=4), _abi.make_params(synth.preset_for(which))
    E = engine_cls(0, prm)
    E.load_batch(b).run_all()
    fm = E.fragmat()
    got, cands, pr = check(E, fm, 13)
    print("%s: candidates %d, entries %d, low-q %d, on haplotype 1 / 2 / other %d / %d / %d, sites with two or more sets %d, unphased sites with a set %d" % (
        which, cands.size, int(got["n_entries"].sum()), int(got["n_lowq"].sum()), int(got["n"][:, 1].sum()), int(got["n"][:, 2].sum()),
        int(got["n"][:, 0].sum()), int((got["n_phase_sets"] >= 2).sum()), int(((cands["phase_set"] == 0) & (got["phase_set"] != 0)).sum())))
    assert got["n_entries"].any() and got["n"][:, 1:].any()
    check(E, fm, 0)
    E.close()


# ---- 5. order and lifetime on one context ---------------------------------------------------------------------------------------------
def test_order_and_lifetime(engine_cls):
    b1, b2 = tj.batch_of([tj.allele_specific_region()]), tj.batch_of(th.edge_regions()[2:4])
    prm = _abi.make_params("hifi-masseq", seed=7)
    E = engine_cls(0, prm)
    lib = E.lib
    p13 = _abi.LcrSiteCountParams(13)
    n, p1, p2 = C.c_int32(), C.c_void_p(), C.c_void_p()
    call = lambda: lib.lcr_site_counts(E.h, C.byref(p13))
    get = lambda: lib.lcr_get_site_counts(E.h, C.byref(n), C.byref(p1), C.byref(p2))
    assert lib.lcr_site_counts(None, C.byref(p13)) == E_ARG and lib.lcr_get_site_counts(E.h, None, C.byref(p1), C.byref(p2)) == E_ARG
    E.load_batch(b1).fill_data_into_freq_vec().get_candidate_snps()
    assert call() == E_STATE and get() == E_STATE
    E.get_fragments()
    assert get() == E_STATE and call() == E_STATE and b"before lcr_phase" in lib.lcr_last_error(E.h)     # before the phase stage
    E.phase()
    assert get() == E_STATE                                                                              # phased, not counted yet
    fm = E.fragmat()
    snap = th.snapshot(E)
    first, _, _ = check(E, fm, 13)
    assert first["n_entries"].tolist() == [40] * 8 and th.snapshot(E) == snap                            # (the call writes nothing a getter reads)
    again, _, _ = check(E, fm, 0)                                                                        # repeated with another threshold
    assert again.tobytes() == first.tobytes()                                                            # (every quality is 30)
    # the next candidate stage ends the records' life; so does the next batch
    E.get_candidate_snps()
    assert get() == E_STATE and call() == E_STATE
    E.get_fragments().phase()
    re, _, _ = check(E, E.fragmat(), 13)                                                                 # stage re-entry: the same records
    assert re.tobytes() == first.tobytes()
    E.load_batch(b2)
    assert get() == E_STATE and call() == E_STATE
    E.run_all()
    assert get() == E_STATE                                                                              # (nothing stale from the last batch)
    got2, _, _ = check(E, E.fragmat(), 13)
    E.close()
    # behind an asynchronous phase stage: the call settles it
    A = engine_cls(0, prm)
    A.set_async_phase(True)
    A.load_batch(b2).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
    fm2 = A.fragmat()
    A.phase()
    assert A.lib.lcr_site_counts(A.h, C.byref(p13)) == 0
    assert A.lib.lcr_get_site_counts(A.h, C.byref(n), C.byref(p1), C.byref(p2)) == 0 and n.value == got2.size
    gota, _, _ = check(A, fm2, 13)
    assert gota.tobytes() == got2.tobytes()
    A.close()
    # the timer
    T = engine_cls(0, prm, timing=True)
    with pytest.raises(Exception):
        T.site_counts_ms()
    T.load_batch(b1).run_all()
    assert T.site_counts(13).tobytes() == first.tobytes() and T.site_counts_ms() > 0.0
    T.close()

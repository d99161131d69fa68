"""K14 lcr_somatic on the GPU against the plain-Python restatement of its contract (tests/somatic_ref.py): every field of every record,
exactly, in pinned host memory and in HBM.  Rows are put on chosen haplotypes and phase sets with Engine.haplotag and hand-picked sites, as
tests/test_site_counts_gpu.py does (its regions are reused); a site is made a low-fraction one by writing LCR_F_CAND_SOMATIC into its
candidate record in HBM, as a caller of the C ABI who holds the records could -- the candidate stage's own flag is exercised behind
lcr_phase.  The contract's worked instance, wave boundaries, an empty haplotype, the quality threshold and q = 0, the phase-set rules and
their equality with lcr_site_counts, LCR_SOM_ALLELES / dense / RNA-edit candidates, no call without the flag, both outcomes of the rescue,
purity, independence from the batch, the call's order and lifetime on one context, and the segment scratch it shares with
lcr_site_counts.  LCR_SOM_DEEP needs 2^20 + 1 entries on one
haplotype: not a shape for this suite; the restatement's branch is covered in tests/test_somatic_host.py."""
import ctypes as C

import numpy as np
import pytest

import helpers
import somatic_ref as ref
import test_gpu_parity as tp
import test_haplotag_gpu as th
import test_junctions_gpu as tj
import test_site_counts_gpu as sc
from longcallr_amd import _abi, _lib, somatic, synth

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
FLAGGED = _abi.F_CAND_SOMATIC | _abi.F_NON_SELECTED
CAND_SIZE, FLAGS_AT = _abi.CAND_DTYPE.itemsize, _abi.CAND_DTYPE.fields["flags"][1]


def dev_candidates(E):
    """the candidate records in HBM: what the call reads"""
    ptr, n = E.candidates_device()
    out = np.zeros(n, dtype=_abi.CAND_DTYPE)
    if n:
        assert _lib.load().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


def set_flags(E, idx, flags):
    """write one candidate's flags in HBM"""
    ptr, n = E.candidates_device()
    assert 0 <= idx < n
    w = np.array([flags], np.uint32)
    assert _lib.load().hipMemcpy(C.c_void_p(ptr + idx * CAND_SIZE + FLAGS_AT), C.c_void_p(w.ctypes.data), C.c_size_t(4), 1) == 0


def dev_records(E):
    n, rec, dev = C.c_int32(), C.c_void_p(), C.c_void_p()
    assert E.lib.lcr_get_somatic(E.h, C.byref(n), C.byref(rec), C.byref(dev)) == 0
    out = np.zeros(n.value, dtype=_abi.SOMATIC_SITE_DTYPE)
    if n.value:
        assert _lib.load().hipMemcpy(C.c_void_p(out.ctypes.data), dev, C.c_size_t(out.nbytes), 2) == 0
    return out


def check(E, fm, **kw):
    """somatic() against the restatement on the engine's own phase results and the candidate records in HBM, host and HBM; the
    invariant; the site's phase set against site_counts() at the same threshold"""
    pr = E.phase_result()
    cands = dev_candidates(E)
    got = E.somatic(**kw)
    want = ref.of_engine(fm, pr, cands, **kw)
    assert got.dtype == _abi.SOMATIC_SITE_DTYPE and got.size == cands.size
    for f in _abi.SOMATIC_SITE_DTYPE.names:
        assert got[f].tolist() == want[f].tolist(), f
    assert dev_records(E).tobytes() == got.tobytes()       # HBM and host hold the same records
    n_entries = np.bincount(fm["col"], minlength=cands.size)
    assert (got["n"].reshape(len(got), 4).sum(axis=1) + got["n_other"] + got["n_lowq"]).tolist() == n_entries.tolist()
    assert got["phase_set"].tolist() == E.site_counts(kw.get("min_baseq", 0))["phase_set"].tolist()
    bad = got["status"] != somatic.SOM_OK
    assert not got["L"][bad].any() and not got["cls"][bad].any() and not got["call"][bad].any()
    assert not got["call"][(cands["flags"] & _abi.F_CAND_SOMATIC) == 0].any()
    return got, cands, pr


# ---- 1. the worked instance of the contract, and its neighbours ---------------------------------------------------------------------
W_START, W_ANCH, W_PS = 5000, (100, 200, 300), 100
W_X, W_X2, W_Y, W_Z = 350, 380, 410, 500       # the instance; the same column unflagged; q = 0 and q = 12 entries; haplotype 2 only
W_COLS = W_ANCH + (W_X, W_X2, W_Y, W_Z)


def worked_region():
    """sixteen reads, 6 on haplotype 1 (they end at column 440) and 10 on haplotype 2; at 350 and 380 (reference A) three reads of
    haplotype 2 carry C; at 410 those three carry C with q = 0, 12 and 30; column 500 is covered by haplotype 2 only, one read with C"""
    forced = {W_X: "A", W_X2: "A", W_Y: "A", W_Z: "A"}
    probe = sc.region(W_START, 700, forced, [], 41)[1]
    reads = []
    for k in range(16):
        h2 = k >= 6
        bases, quals = sc.hap_bases(probe, W_ANCH, h2), {}
        if k >= 13:
            bases.update({W_X: "C", W_X2: "C", W_Y: "C"})
            quals[W_Y] = (0, 12, 30)[k - 13]
        if k == 15:
            bases[W_Z] = "C"
        reads.append(([(40, 660 if h2 else 440)], bases, quals))
    return sc.region(W_START, 700, forced, reads, 41)


WANT_L = [[-3107708873, -23420730163838, -6852080807812], [-9899190109605, -26720698299410, -8745495261838]]


def worked_engine(engine_cls):
    start0, refseq, rs = worked_region()
    b = tj.batch_of([(start0, refseq, rs)])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=7, min_linkers=2, dist_to_end=0))
    fm, cands0, _ = sc.imported(E, b, [W_COLS], [start0])
    E.haplotag(th.site_arrays({start0 + c: (refseq[c], tj.ALT[refseq[c]], W_PS) for c in W_ANCH}))
    at = {c: int(np.flatnonzero(cands0["pos"] == start0 + c)[0]) for c in W_COLS}
    for c in (W_X, W_Y, W_Z):
        set_flags(E, at[c], FLAGGED)
    return E, fm, at


def test_worked_instance(engine_cls):
    E, fm, at = worked_engine(engine_cls)
    pr = E.phase_result()
    assert sorted(pr["assignment"].tolist()) == [1] * 6 + [2] * 10 and set(pr["phase_set"].tolist()) == {W_PS}
    got, cands, _ = check(E, fm)
    x = got[at[W_X]]
    assert (int(x["phase_set"]), x["n"].tolist(), int(x["n_other"]), int(x["n_lowq"])) == (W_PS, [[6, 0], [7, 3]], 0, 0)
    assert x["L"].tolist() == WANT_L and x["cls"].tolist() == [0, 2] and (int(x["call"]), int(x["status"])) == (2, somatic.SOM_OK)
    assert "%.4f" % somatic.score(x) == "10.8642"
    assert int(cands["phase_set"][at[W_X]]) == 0                          # (the set is the rows')
    # no call without the flag: the same column, the same classes
    x2 = got[at[W_X2]]
    assert x2["L"].tolist() == WANT_L and x2["cls"].tolist() == [0, 2] and int(x2["call"]) == 0 and not int(cands["flags"][at[W_X2]]) & _abi.F_CAND_SOMATIC
    # an empty haplotype: its priors only, class 0
    z = got[at[W_Z]]
    t = somatic.tables(0.3)
    assert z["n"].tolist() == [[0, 0], [9, 1]] and z["L"][0].tolist() == t["prior"] and int(z["cls"][0]) == 0
    # the anchors of an ordinary phase read "ref on one haplotype, het on the other"
    assert [got["cls"][at[c]].tolist() for c in W_ANCH] == [[0, 1]] * 3 and not got["call"][[at[c] for c in W_ANCH]].any()
    # q = 0 takes the q = 1 row; the thresholds move entries to n_lowq
    y = got[at[W_Y]]
    assert y["n"].tolist() == [[6, 0], [7, 3]] and y["L"][1].tolist() == ref.haplotype_sums([30] * 7, [1, 12, 30], t)
    for q, n_alt, lowq in ((13, 1, 2), (12, 2, 1), (1, 2, 1), (30, 1, 2)):
        g, _, _ = check(E, fm, min_baseq=q)
        assert (g["n"][at[W_Y]].tolist(), int(g["n_lowq"][at[W_Y]])) == ([[6, 0], [7, n_alt]], lowq), q
    E.close()


def test_purity(engine_cls):
    E, fm, at = worked_engine(engine_cls)
    first, _, _ = check(E, fm, purity=0.3)
    mid, _, _ = check(E, fm, purity=0.1)
    third, _, _ = check(E, fm, purity=0.3)
    assert first.tobytes() == third.tobytes() and mid.tobytes() != first.tobytes()
    assert mid["n"].tolist() == first["n"].tolist() and mid["L"][:, :, :2].tolist() == first["L"][:, :, :2].tolist()      # (purity moves the somatic sums only)
    check(E, fm, purity=1.0)
    check(E, fm, purity=0.5, som_rate=1e-3, het_rate=0.25, min_baseq=13)
    E.close()


# ---- 2. test_site_counts_gpu's regions: column depths, phase-set rules, thresholds, a two-alternate column -----------------------------
def imported_engine(engine_cls, regs, which=(0, 1, 2)):
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5, dist_to_end=0))
    fm, cands0, coff = sc.imported(E, tj.batch_of([regs[g] for g in which]), [sc.IMPORT_COLS[g] for g in which], [sc.STARTS3[g] for g in which])
    E.haplotag(sc.imported_sites(regs, which))
    cands = dev_candidates(E)
    for i in range(cands.size):       # every site that lcr_haplotag left unphased becomes a low-fraction one
        if int(cands["flags"][i]) & _abi.F_NON_SELECTED:
            set_flags(E, i, FLAGGED)
    return E, fm, coff


def test_imported_edges(engine_cls):
    regs = sc.imported_regions()
    E, fm, coff = imported_engine(engine_cls, regs)
    got, cands, pr = check(E, fm)
    at = lambda g, c: int(np.flatnonzero(cands["pos"] == sc.STARTS3[g] + c)[0])
    # column depths on either side of the 64 lanes of a site's wave, twice that plus one, one and none
    depth = [int(got["n"][at(0, c)].sum() + got["n_other"][at(0, c)] + got["n_lowq"][at(0, c)]) for c in sc.DEPTH_COLS]
    assert depth == [129, 65, 64, 63, 1, 0]
    z = got[at(0, 600)]       # no read reaches it: zero counts with the candidate's own set
    assert int(z["phase_set"]) == 500 and not z["n"].any() and int(z["n_other"]) == 0 and z["cls"].tolist() == [0, 0]
    # the threshold at column 100: q = 12 / 13 / 29 / 30 on every fourth read
    a = at(0, 100)
    for q, lowq in ((0, 0), (12, 0), (13, 33), (30, 97)):
        g, _, _ = check(E, fm, min_baseq=q)
        assert int(g["n_lowq"][a]) == lowq, q
    # the phase-set rules: majority, tie to the smaller value, three sets, the candidate's own set in the minority and with no row
    got, _, _ = check(E, fm, min_baseq=13)
    t = {c: got[at(1, c)] for c in sc.TARGETS}
    assert [int(t[c]["phase_set"]) for c in sc.TARGETS] == [sc.SET_P, sc.SET_Q, sc.SET_R, sc.SET_P, sc.SET_R]
    assert [int(t[c]["n"].sum()) for c in sc.TARGETS] == [3, 2, 3, 1, 0] and [int(t[c]["n_other"]) for c in sc.TARGETS] == [2, 2, 3, 3, 4]
    assert [bool(int(cands["flags"][at(1, c)]) & _abi.F_CAND_SOMATIC) for c in sc.TARGETS] == [True, True, True, False, False]
    # the two-alternate column: neither allele is the reference base
    r = got[at(2, 300)]
    assert int(r["status"]) == somatic.SOM_ALLELES and int(r["n"].sum() + r["n_other"]) == 15 and int(r["n"][:, 0].sum()) <= 3
    assert int(got["status"][a]) == somatic.SOM_OK and all(int(t[c]["status"]) == somatic.SOM_OK for c in sc.TARGETS)
    E.close()


def test_region_alone_and_in_the_batch(engine_cls):
    regs = sc.imported_regions()
    E, fm, coff = imported_engine(engine_cls, regs)
    got, _, _ = check(E, fm, min_baseq=13)
    E.close()
    for g in (0, 1, 2):
        E1, fm1, _ = imported_engine(engine_cls, regs, (g,))
        got1, _, _ = check(E1, fm1, min_baseq=13)
        assert got1.tobytes() == got[coff[g]:coff[g + 1]].tobytes(), g
        E1.close()


def test_called_edges(engine_cls):
    """test_haplotag_gpu's batch through the candidate stage: rows of 0 / 1 / 8 / 9 / 17 entries, two sets in a region, a dense cluster
    (no entries: zero counts, the priors), a column of 3 000 rows"""
    b = tj.batch_of(th.edge_regions())
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    fm, cands0, coff = th.staged(E, b)
    E.haplotag(th.site_arrays(th.edge_sites(cands0)))
    got, cands, pr = check(E, fm)
    dense = (cands["flags"] & _abi.F_DENSE) != 0
    assert dense.sum() >= 5 and not got["n"][dense].any() and not got["n_other"][dense].any() and not got["n_lowq"][dense].any()
    ok = dense & (got["status"] == somatic.SOM_OK)
    assert not got["cls"][dense].any() and not got["call"][dense].any() and got["L"][ok].tolist() == [[somatic.tables(0.3)["prior"]] * 2] * int(ok.sum())
    print("dense candidates: %d, of them status OK: %d" % (int(dense.sum()), int(ok.sum())))
    g5 = got[coff[5]:coff[6]]
    assert [int(r["n"][0].sum()) for r in g5] == [1500] * 5 and [int(r["n"][1].sum()) for r in g5] == [1500] * 5
    check(E, fm, min_baseq=13)
    E.close()


# ---- 3. behind lcr_phase: both outcomes of the rescue, RNA-edit candidates, a synthetic preset batch ---------------------------------
@pytest.mark.parametrize("min_phase_score,rescued", [(13.0, False), (4.0, True)])
def test_low_fraction_sites_behind_phase(engine_cls, min_phase_score, rescued):
    b = tp._low_fraction_batch(seed=1)
    E = engine_cls(0, _abi.make_params("ont-cdna", seed=3, min_phase_score=min_phase_score))
    E.load_batch(b).run_all()
    fm = E.fragmat()
    got, cands, pr = check(E, fm)
    low = (cands["pos"] == 1000 + 900) | (cands["pos"] == 1000 + 2000)
    flagged = (cands["flags"] & _abi.F_CAND_SOMATIC) != 0
    assert low.sum() >= 1 and pr["assignment"].any()
    print("min_phase_score %g: %r" % (min_phase_score, [(int(c["pos"]), int(c["flags"]), r["n"].tolist(), r["cls"].tolist(), int(r["call"]), somatic.score(r))
                                                        for c, r in zip(cands[low], got[low])]))
    if rescued:       # promoted: no site is flagged any more, nothing is called
        assert not flagged.any() and not got["call"].any()
    else:             # not rescued: flagged and evaluated, alternate entries counted on a haplotype
        assert flagged[low].all() and (got["status"][low] == somatic.SOM_OK).all()
        assert all(int(r["n"][:, 1].sum()) > 0 for r in got[low])
    check(E, fm, purity=0.1, min_baseq=13)
    E.close()


def test_rna_edit_candidates(engine_cls):
    b, _ = helpers.two_haplotype_batch(n_snps=5, n_reads=60, edit_sites=(777,), edit_frac=0.95, seed=2)
    b.flags[:] = 0 | (1 << 1)
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=3))
    fm, cands0, _ = th.staged(E, b)
    edit = (cands0["flags"] & _abi.F_RNA_EDIT) != 0
    E.phase()
    got, cands, pr = check(E, fm)
    assert edit.sum() == 1 and pr["assignment"].any()
    r = got[np.flatnonzero(edit)[0]]
    assert int(r["status"]) == somatic.SOM_OK and int(r["call"]) == 0 and int(r["n"].sum() + r["n_other"]) == int(np.count_nonzero(fm["col"] == np.flatnonzero(edit)[0]))
    E.close()


def test_synth_preset_batch(engine_cls):
    b, prm = synth.make_batch("masseq", n_genes=4), _abi.make_params(synth.preset_for("masseq"))
    E = engine_cls(0, prm)
    E.load_batch(b).run_all()
    fm = E.fragmat()
    got, cands, pr = check(E, fm)
    print("masseq: candidates %d, flagged %d, calls %d, classes per haplotype %r, low-q at 13: %d" % (
        cands.size, int(((cands["flags"] & _abi.F_CAND_SOMATIC) != 0).sum()), int(np.count_nonzero(got["call"])),
        np.bincount(got["cls"].reshape(-1), minlength=3).tolist(), int(check(E, fm, min_baseq=13)[0]["n_lowq"].sum())))
    assert got["n"].any() and (got["cls"] == 1).any()
    E.close()


# ---- 4. order and lifetime on one context ---------------------------------------------------------------------------------------------
def test_order_and_lifetime(engine_cls):
    b1, b2 = tj.batch_of([tj.allele_specific_region()]), tj.batch_of(th.edge_regions()[2:4])
    prm = _abi.make_params("hifi-masseq", seed=7)
    E = engine_cls(0, prm)
    lib = E.lib
    P = lambda purity=0.3, som=5e-6, het=5e-4, q=0: _abi.LcrSomaticParams(purity, som, het, q, 0)
    p0 = P()
    n, p1, p2 = C.c_int32(), C.c_void_p(), C.c_void_p()
    call = lambda p=p0: lib.lcr_somatic(E.h, C.byref(p))
    get = lambda: lib.lcr_get_somatic(E.h, C.byref(n), C.byref(p1), C.byref(p2))
    assert lib.lcr_somatic(None, C.byref(p0)) == E_ARG and lib.lcr_get_somatic(E.h, None, C.byref(p1), C.byref(p2)) == E_ARG
    E.load_batch(b1).fill_data_into_freq_vec().get_candidate_snps()
    assert call() == E_STATE and get() == E_STATE
    E.get_fragments()
    assert get() == E_STATE and call() == E_STATE and b"before lcr_phase" in lib.lcr_last_error(E.h)     # before the phase stage
    E.phase()
    assert get() == E_STATE                                                                              # phased, not evaluated yet
    fm = E.fragmat()
    snap = th.snapshot(E)
    first, _, _ = check(E, fm)
    assert th.snapshot(E) == snap and first["cls"].any()                                                 # (the call writes nothing a getter reads)
    # refused parameters leave the last records readable
    for bad, word in ((P(0.0), b"purity"), (P(1.5), b"purity"), (P(float("nan")), b"purity"), (P(som=0.0), b"rate"), (P(het=0.0), b"rate"),
                      (P(het=0.6, som=0.4), b"rate"), (P(q=31), b"min_baseq")):
        assert call(bad) == E_ARG and word in lib.lcr_last_error(E.h)
        assert dev_records(E).tobytes() == first.tobytes()
    assert lib.lcr_somatic(E.h, None) == E_ARG and dev_records(E).tobytes() == first.tobytes()
    again, _, _ = check(E, fm, min_baseq=13)                                                             # repeated with other parameters
    assert again.tobytes() == first.tobytes()                                                            # (every quality is 30)
    # the next candidate stage ends the records' life; so does the next batch
    E.get_candidate_snps()
    assert get() == E_STATE and call() == E_STATE
    E.get_fragments().phase()
    re, _, _ = check(E, E.fragmat())                                                                     # stage re-entry: the same records
    assert re.tobytes() == first.tobytes()
    E.load_batch(b2)
    assert get() == E_STATE and call() == E_STATE
    E.run_all()
    assert get() == E_STATE                                                                              # (nothing stale from the last batch)
    got2, _, _ = check(E, E.fragmat())
    slot_batch = b2
    E.load_batch_async(slot_batch, 0)
    E.bind_batch(0)
    assert get() == E_STATE and call() == E_STATE                                                        # lcr_bind_batch
    E.close()
    # behind an asynchronous phase stage: the call settles it
    A = engine_cls(0, prm)
    A.set_async_phase(True)
    A.load_batch(b2).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
    fm2 = A.fragmat()
    A.phase()
    assert A.lib.lcr_somatic(A.h, C.byref(p0)) == 0
    assert A.lib.lcr_get_somatic(A.h, C.byref(n), C.byref(p1), C.byref(p2)) == 0 and n.value == got2.size
    gota, _, _ = check(A, fm2)
    assert gota.tobytes() == got2.tobytes()
    A.close()
    # the timer
    T = engine_cls(0, prm, timing=True)
    with pytest.raises(Exception):
        T.somatic_ms()
    T.load_batch(b1).run_all()
    assert T.somatic().tobytes() == first.tobytes() and T.somatic_ms() > 0.0
    T.close()


# ---- 5. lcr_site_counts and lcr_somatic fill the same per-candidate segments on one context ---------------------------------------------
def shared_engine(engine_cls):
    """test_site_counts_gpu's seven-row worked instance and its depth region (129 / 65 / 64 / 63 / 1 / 0 entries: a segment on either side
    of the 64 lanes of its wave) in one batch, behind lcr_haplotag"""
    (w0, wref, wrs), (d0, dref, drs) = sc.worked_region(), sc.depth_region()
    sites = {w0 + c: (wref[c], tj.ALT[wref[c]], 100 if c in sc.W_SET100 else 200) for c in sc.W_SET100 + sc.W_SET200}
    sites.update({d0 + c: (dref[c], tj.ALT[dref[c]], 500) for c in sc.DEPTH_COLS})
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5, dist_to_end=0))
    sc.imported(E, tj.batch_of([(w0, wref, wrs), (d0, dref, drs)]), [sc.W_SET100 + sc.W_SET200 + (sc.W_X,), sc.DEPTH_COLS], [w0, d0])
    E.haplotag(th.site_arrays(sites))
    return E


def queue_site_counts(E, q):
    p = _abi.LcrSiteCountParams(q)
    assert E.lib.lcr_site_counts(E.h, C.byref(p)) == 0


def queue_somatic(E, q):
    p = _abi.LcrSomaticParams(0.3, 5e-6, 5e-4, q, 0)
    assert E.lib.lcr_somatic(E.h, C.byref(p)) == 0


def fetched(E, which):
    """the records of the calls named in `which` as their getters hand them out, pinned host memory and HBM, as bytes"""
    out = {}
    for name, getter, dtype, dev in (("site_counts", E.lib.lcr_get_site_counts, _abi.SITE_COUNT_DTYPE, sc.dev_records),
                                     ("somatic", E.lib.lcr_get_somatic, _abi.SOMATIC_SITE_DTYPE, dev_records)):
        if name in which:
            n, rec, d = C.c_int32(), C.c_void_p(), C.c_void_p()
            assert getter(E.h, C.byref(n), C.byref(rec), C.byref(d)) == 0 and n.value > 0
            out[name] = (C.string_at(rec.value, n.value * dtype.itemsize), dev(E).tobytes())
    return out


def test_shared_segments_with_site_counts(engine_cls):
    # every call alone on a fresh context
    alone = {}
    for key, queue, q in (("sc13", queue_site_counts, 13), ("sc0", queue_site_counts, 0), ("som13", queue_somatic, 13)):
        A = shared_engine(engine_cls)
        queue(A, q)
        (alone[key],) = fetched(A, ("somatic",) if key == "som13" else ("site_counts",)).values()
        assert alone[key][0] == alone[key][1]
        A.close()
    assert alone["sc13"] != alone["sc0"]                       # (column 100 of the depth region holds q = 12 entries)
    n_entries = np.frombuffer(alone["sc13"][0], dtype=_abi.SITE_COUNT_DTYPE)["n_entries"].tolist()
    assert len(n_entries) == 13 and n_entries[3] == 7 and n_entries[7:] == [129, 65, 64, 63, 1, 0]       # (column 350 of the instance; the depth columns)
    E = shared_engine(engine_cls)
    both = ("site_counts", "somatic")
    queue_site_counts(E, 13); queue_somatic(E, 13)             # one behind the other, both fetched afterwards
    assert fetched(E, both) == {"site_counts": alone["sc13"], "somatic": alone["som13"]}
    queue_somatic(E, 13); queue_site_counts(E, 13)             # the other order
    assert fetched(E, both) == {"site_counts": alone["sc13"], "somatic": alone["som13"]}
    queue_site_counts(E, 13); queue_somatic(E, 13); queue_site_counts(E, 0)       # ... and again with another threshold
    assert fetched(E, both) == {"site_counts": alone["sc0"], "somatic": alone["som13"]}
    E.close()

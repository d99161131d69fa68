"""K7 lcr_ase on the GPU against the plain-Python restatement of its contract (tests/ase_ref.py), fed with the GPU's own phasing
results: a hand-checkable instance, the edges of every rule of the contract, more rows than a workgroup has threads, parental sites
built from the engine's candidates on synthetic ONT cDNA / MAS-Seq and demo.bam, and the call's order and lifetime on one context."""
import ctypes as C

import numpy as np
import pytest

import ase_ref
import helpers
import test_junctions_gpu as tj
from longcallr_amd import _abi, synth

pytestmark = pytest.mark.gpu

OTHER = {"A": "CGT", "C": "AGT", "G": "ACT", "T": "ACG"}


def site_arrays(parental):
    pos = np.array(sorted(parental), dtype=np.int64)
    return (pos, np.array([ord(parental[int(p)][0]) for p in pos], np.uint8), np.array([ord(parental[int(p)][1]) for p in pos], np.uint8))


def results(E):
    fm, pr = E.fragmat(), E.phase_result()
    cands, coff = E.candidates()
    return fm, pr, cands, coff


def check(E, res, parental=None, min_baseq=13, mps=None):
    """the engine's records and the restatement's on the engine's own phasing results: every field of every record"""
    fm, pr, cands, coff = res
    mps = float(E.params.min_phase_score) if mps is None else float(np.float32(mps))
    got = E.ase(site_arrays(parental) if parental else None, min_baseq, mps)
    want = ase_ref.regions(fm, pr["assignment"], pr["phase_set"], cands, coff, parental, min_baseq, mps)
    assert got.dtype == _abi.ASE_DTYPE and got.tolist() == want.tolist()
    return got


def alt_of(s):
    """(REF, ALT) of a candidate as the VCF writer prints them (one_alt)"""
    ref, a1, a2 = chr(s["ref_base"]).upper(), chr(s["allele1"]), chr(s["allele2"])
    return ref, (a1 if a1 != ref else a2 if a2 != ref else OTHER[ref][0])


# ---- 1. the hand-worked instance -----------------------------------------------------------------------------------------------------
def test_hand_worked_instance(engine_cls):
    """tj.allele_specific_region: 40 error-free reads over eight het sites, 20 of haplotype A (the alternate base everywhere) and 20 of B,
    one phase set.  Parental sites at all eight, the alternate base paternal: every A read sees 8 pat / 0 mat, every B read 0 / 8."""
    start0, ref, rs = tj.allele_specific_region()
    b = tj.batch_of([(start0, ref, rs)])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=7))
    E.load_batch(b).run_all()
    res = results(E)
    fm, pr, cands, coff = res
    sites = [start0 + c for c in (150, 300, 450, 600, 2050, 2200, 2350, 2500)]
    assert sorted(int(p) for p in cands["pos"] if int(p) in sites) == sites
    par = {p: (tj.ALT[ref[p - start0]], ref[p - start0]) for p in sites}
    got = check(E, res, par)
    ps = int(pr["phase_set"][0])
    a_is_h1 = int(pr["assignment"][[i for i, r in enumerate(rs) if "1100N" not in r["cigar"]][0]]) == 1
    assert ps != 0 and got.tolist() == [(0, ps, 1, 20, 20, 8, 20, 0, 0, 20) if a_is_h1 else (0, ps, 1, 20, 20, 8, 0, 20, 20, 0)]
    # three sites the other way round: 5 against 3, the same votes; four: 4 against 4, no vote at all
    for n_swapped, voting in ((3, True), (4, False)):
        p2 = dict(par)
        for p in sites[:n_swapped]:
            p2[p] = par[p][::-1]
        g = check(E, res, p2)
        assert g.tolist()[0][5:] == (got.tolist()[0][5:] if voting else (8, 0, 0, 0, 0))
    # a third allele as the maternal one at every site: B's reads carry neither, A's still vote paternal
    p3 = {p: (par[p][0], [x for x in OTHER[par[p][0]] if x != par[p][1]][0]) for p in sites}
    g = check(E, res, p3)
    assert g.tolist()[0][5:] == ((8, 20, 0, 0, 0) if a_is_h1 else (8, 0, 0, 20, 0))
    E.close()


# ---- 2. edges ------------------------------------------------------------------------------------------------------------------------
SITES12 = [60 + 40 * k for k in range(12)]


def edge_regions():
    """hifi-masseq.  Every region but E0 has an exon [0, 600) with het sites its reads phase on."""
    r = []
    r.append(tj.build_region(10000, 700, [], tj.haps([(0, "600M")] * 8), 31))                         # E0 no candidate: no rows
    r.append(tj.build_region(20000, 700, tj.ANCHOR, [(0, "600M", True)] * 12, 32))                    # E1 homozygous sites only: rows, none assigned
    r.append(tj.build_region(30000, 2800, tj.ANCHOR + [1100, 1200, 1300, 1400, 1500],
                             tj.haps([(0, "600M2000N50M10N50M")] * 8 + [(1000, "600M10N50M10N50M")] * 8), 33))   # E2 two phase sets, 8 rows each
    r.append(tj.build_region(40000, 700, tj.ANCHOR, tj.haps([(0, "600M")] * 3000), 34))               # E3 more rows than a workgroup has threads
    r.append(tj.build_region(50000, 700, SITES12, tj.haps([(0, "600M")] * 20 + [(0, "30M20N550M")] * 2 + [(20, "10M")] * 2), 35))   # E4 12 entries; none
    r.append(tj.build_region(60000, 700, tj.ANCHOR + [210, 220, 230, 240, 250, 260], tj.haps([(0, "600M")] * 20), 36))   # E5 a dense cluster
    return [(s,) + x for s, x in zip((10000, 20000, 30000, 40000, 50000, 60000), r)]


@pytest.fixture(scope="module")
def edge_run(engine_cls):
    regs = edge_regions()
    b = tj.batch_of(regs)
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    E.load_batch(b).run_all()
    yield E, b, regs, results(E)
    E.close()


def everything_parental(cands, seed):
    """a parental site at every candidate, REF / ALT in a seeded random order"""
    rng = np.random.default_rng(seed)
    par = {}
    for s in cands:
        ref, alt = alt_of(s)
        par[int(s["pos"])] = (ref, alt) if rng.random() < 0.5 else (alt, ref)
    return par


def test_edges(edge_run):
    E, b, regs, res = edge_run
    fm, pr, cands, coff = res
    rro, asg, ps = fm["row_region_off"], pr["assignment"], pr["phase_set"]
    plain = check(E, res)
    par = everything_parental(cands, 1)
    got = check(E, res, par)
    for g in range(len(regs)):
        print("E%d rows %d assigned %d phase sets %r record %r" % (g, rro[g + 1] - rro[g], int((asg[rro[g]:rro[g + 1]] != 0).sum()),
                                                                     sorted(set(ps[rro[g]:rro[g + 1]].tolist())), got.tolist()[g]))
    # E0: no rows.  E1: rows, none assigned
    assert rro[1] - rro[0] == 0 and plain.tolist()[0] == (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert rro[2] - rro[1] == 12 and not asg[rro[1]:rro[2]].any() and plain.tolist()[1] == (1, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    # E2: two phase sets of eight rows each: the smaller value, 2 sets
    s2 = sorted(set(ps[rro[2]:rro[3]].tolist()))
    assert len(s2) == 2 and s2[0] != 0 and all(int((ps[rro[2]:rro[3]] == v).sum()) == 8 for v in s2) and asg[rro[2]:rro[3]].all()
    assert plain.tolist()[2][:5] == (2, s2[0], 2, 4, 4)
    # E3: 3 000 rows, all counted
    assert rro[4] - rro[3] == 3000 and plain["h1"][3] + plain["h2"][3] == 3000 and plain["n_phase_sets"][3] == 1
    assert got["n_sites"][3] == 5 and got["h1_pat"][3] + got["h1_mat"][3] + got["h2_pat"][3] + got["h2_mat"][3] == 3000    # (5 sites: never a tie)
    # E4: rows of 12 entries (more than the vote kernel's eight lanes), and rows without an entry
    n_ent = np.diff(fm["row_ptr"])[rro[4]:rro[5]]
    assert n_ent.max() == 12 and (n_ent == 0).sum() == 2 and got["n_sites"][4] == 12
    votes4 = int(got["h1_pat"][4] + got["h1_mat"][4] + got["h2_pat"][4] + got["h2_mat"][4])
    n_pat_ref = sum(par[int(s["pos"])][0] == alt_of(s)[0] for s in cands[coff[4]:coff[5]])
    assert (votes4 >= 20) == (n_pat_ref != 6)       # (the 20 reads over all 12 sites vote unless the seeded order splits the sites 6 : 6)
    # E1's homozygous candidates, E2's other phase set and E5's dense cluster all carry a parental site: none is eligible
    assert got["n_sites"][1] == 0 and coff[2] - coff[1] == 5 and (cands["variant_type"][coff[1]:coff[2]] == 2).all()
    assert got["n_sites"][2] == 5 and coff[3] - coff[2] == 10 and len(set(cands["phase_set"][coff[2]:coff[3]].tolist())) == 2
    dense = (cands["flags"][coff[5]:coff[6]] & _abi.F_DENSE) != 0
    assert dense.sum() >= 5 and not dense.all() and got["n_sites"][5] == int((~dense).sum()) > 0
    # every region alone: the same records
    for g in (2, 4):
        A = type(E)(0, E.params)
        A.load_batch(tj.batch_of([regs[g]])).run_all()
        r1 = results(A)
        one = check(A, r1, par)          # (the other regions' sites lie outside this batch's one region)
        assert one.tolist()[0][1:] == got.tolist()[g][1:]
        A.close()


def test_all_rows_without_a_phase_set(edge_run):
    """Rows that are assigned but carry no phase set: with min_phase_score above every score no site is a node of the phase-set graph, so
    every read's phase set is 0 while the assignment stands -- no counting row, whatever the sites."""
    E, b, regs, res = edge_run
    H = type(E)(0, _abi.make_params("hifi-masseq", seed=5, min_phase_score=1.0e6))
    H.load_batch(tj.batch_of(regs[2:3])).run_all()
    r = results(H)
    assert r[1]["assignment"].any() and not r[1]["phase_set"].any()
    got = check(H, r, everything_parental(r[2], 2))
    assert got.tolist() == [(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)]
    H.close()


# ---- 3. parental sites built from the engine's candidates ----------------------------------------------------------------------------
def parental_from_candidates(batch, res, mps, seed):
    """For every candidate that is eligible apart from the join a parental site REF / ALT in a seeded random order; beside them sites
    at every other candidate (dense, non-selected, homozygous, another phase set, ...), one with a third allele, positions that are no
    candidate and positions outside every region.  -> (sites, what was added per kind)"""
    fm, pr, cands, coff = res
    rng = np.random.default_rng(seed)
    plain = ase_ref.regions(fm, pr["assignment"], pr["phase_set"], cands, coff, None)
    par, kinds = {}, dict(eligible=0, dense=0, non_selected=0, homozygous=0, other_phase_set=0, other=0, third=0, no_candidate=0, outside=0)
    for i, s in enumerate(cands):
        ref, alt = alt_of(s)
        par[int(s["pos"])] = (ref, alt) if rng.random() < 0.5 else (alt, ref)
        if ase_ref.pass_phased_het(cands[i:i + 1], mps) and int(s["phase_set"]) != 0:
            kinds["eligible" if int(s["phase_set"]) == int(plain["phase_set"][int(s["region"])]) else "other_phase_set"] += 1
        elif int(s["flags"]) & _abi.F_DENSE:
            kinds["dense"] += 1
        elif int(s["flags"]) & _abi.F_NON_SELECTED:
            kinds["non_selected"] += 1
        elif int(s["variant_type"]) == 2:
            kinds["homozygous"] += 1
        else:
            kinds["other"] += 1
    elig = [i for i in range(len(cands)) if ase_ref.pass_phased_het(cands[i:i + 1], mps)
            and int(cands["phase_set"][i]) != 0 and int(cands["phase_set"][i]) == int(plain["phase_set"][int(cands["region"][i])])]
    for i in elig[1::7]:                                  # a third allele in place of REF
        ref, alt = alt_of(cands[i])
        par[int(cands["pos"][i])] = (alt, [x for x in OTHER[ref] if x != alt][0])
        kinds["third"] += 1
    have = set(par)
    for g in range(batch.n_regions):                      # positions of the region that are no candidate; the first and last candidate have one above
        for p in rng.integers(int(batch.start0[g]), int(batch.start0[g]) + int(batch.len[g]), size=20).tolist():
            if p not in have:
                par[p] = ("A", "C")
                kinds["no_candidate"] += 1
    for p in (0, 1, int(batch.start0[0]) - 1, int(batch.start0[-1]) + int(batch.len[-1]), int(batch.start0[-1]) + int(batch.len[-1]) + 12345):
        if p >= 0 and p not in have:
            par[p] = ("G", "T")
            kinds["outside"] += 1
    for g in range(batch.n_regions):
        if coff[g + 1] > coff[g]:
            assert int(cands["pos"][coff[g]]) in par and int(cands["pos"][coff[g + 1] - 1]) in par
    return par, kinds, elig


@pytest.mark.parametrize("profile", ["ont-cdna", "masseq"])
def test_parental_sites_from_candidates(engine_cls, profile):
    b = synth.make_batch(profile, n_genes=4)
    E = engine_cls(0, _abi.make_params(synth.preset_for(profile)))
    E.load_batch(b).run_all()
    res = results(E)
    fm, pr, cands, coff = res
    mps = float(E.params.min_phase_score)
    par, kinds, elig = parental_from_candidates(b, res, mps, 11)
    print("%s: rows %d, assigned %d, candidates %d, sites %r" % (profile, pr["assignment"].size, int((pr["assignment"] != 0).sum()), len(cands), kinds))
    assert kinds["eligible"] > 0 and kinds["no_candidate"] > 0 and kinds["outside"] > 0 and kinds["third"] > 0
    want = ase_ref.regions(fm, pr["assignment"], pr["phase_set"], cands, coff, par, 13, mps)
    with_site = [r for r in want.tolist() if r[5] > 0]
    voting = [r for r in with_site if any(r[6:])]
    assert with_site and 2 * len(voting) >= len(with_site)          # not vacuous, by the restatement alone
    got = check(E, res, par)
    print(got.tolist())
    # plain mode: the same haplotype counts, nothing else
    plain = check(E, res)
    for f in ("region", "phase_set", "n_phase_sets", "h1", "h2"):
        assert plain[f].tolist() == got[f].tolist()
    for f in ("n_sites", "h1_pat", "h1_mat", "h2_pat", "h2_mat"):
        assert not plain[f].any()
    # min_phase_score just below and just above a real site's score
    sc = np.float32(sorted(cands["phase_score"][elig].tolist())[len(elig) // 2])
    below, above = np.nextafter(sc, np.float32(-np.inf)), np.nextafter(sc, np.float32(np.inf))
    n_lo, n_hi = int(check(E, res, par, mps=max(below, np.float32(mps)))["n_sites"].sum()), int(check(E, res, par, mps=above)["n_sites"].sum())
    assert n_hi < n_lo <= int(got["n_sites"].sum())
    # min_baseq at a quality value that is present at an eligible site, and one above it
    rro = fm["row_region_off"]
    es = set(elig)
    qs = sorted({int(v) & 31 for e, v in zip(fm["col"].tolist(), fm["val"].tolist()) if e in es})
    q = ([x for x in qs if x < 30] or [29])[len([x for x in qs if x < 30]) // 2]       # (all at the clamp: 29 and 30)
    print("qualities at eligible sites %r, min_baseq %d and %d" % (qs, q, q + 1))
    at_q, above_q = check(E, res, par, min_baseq=q), check(E, res, par, min_baseq=q + 1)
    assert at_q["n_sites"].tolist() == above_q["n_sites"].tolist() == got["n_sites"].tolist()
    assert rro[-1] == pr["assignment"].size
    check(E, res, par, min_baseq=0)
    check(E, res, par, min_baseq=30)
    E.close()


@pytest.mark.parametrize("mode", ["plain", "parental"])
def test_demo_bam(engine_cls, mode):
    """demo.bam under hifi-masseq; the record is printed and recorded in DESIGN.md section 1c"""
    b = helpers.demo_batch()
    E = engine_cls(0, _abi.make_params("hifi-masseq"))
    E.load_batch(b).run_all()
    res = results(E)
    par = None
    if mode == "parental":
        par, kinds, _ = parental_from_candidates(b, res, float(E.params.min_phase_score), 3)
        print("demo.bam sites %r" % (kinds,))
    got = check(E, res, par)
    print("demo.bam %s: rows %d, assigned %d, record %r" % (mode, res[1]["assignment"].size, int((res[1]["assignment"] != 0).sum()), got.tolist()))
    assert got.size == 1 and got["h1"][0] + got["h2"][0] > 0
    E.close()


# ---- 4. call order and lifetime --------------------------------------------------------------------------------------------------------
def test_call_order_and_lifetime(engine_cls):
    import torch
    regs = edge_regions()
    b1, b2 = tj.batch_of([tj.allele_specific_region()]), tj.batch_of([regs[2], regs[4]])
    prm = _abi.make_params("hifi-masseq", seed=7)
    E = engine_cls(0, prm)
    lib, ap, al = E.lib, _abi.LcrAseParams(13, prm.min_phase_score), _abi.LcrAseList()

    def call(pos, pat, mat, p=ap):
        pos, pat, mat = np.array(pos, np.int64), np.frombuffer(pat, np.uint8), np.frombuffer(mat, np.uint8)
        return lib.lcr_ase(E.h, C.byref(p), _abi.LCR_MEM_HOST, pos.size, pos.ctypes.data, pat.ctypes.data, mat.ctypes.data)
    E.load_batch(b1).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
    assert lib.lcr_ase(E.h, C.byref(ap), 0, 0, None, None, None) == -4 and lib.lcr_get_ase(E.h, C.byref(al)) == -4      # LCR_E_STATE
    E.phase()
    assert lib.lcr_get_ase(E.h, C.byref(al)) == -4                                                                       # no records yet
    res = results(E)
    par = everything_parental(res[2], 5)
    first = check(E, res, par)
    before = (E.phase_result(), E.candidates(), E.fragmat())
    # bad arguments: LCR_E_ARG, and the last call's records stand
    assert lib.lcr_ase(E.h, None, 0, 0, None, None, None) == -1
    assert call([5, 4], b"AA", b"CC") == -1 and call([5, 5], b"AA", b"CC") == -1            # unsorted, duplicate
    assert call([4, 5], b"AC", b"CC") == -1 and call([4, 5], b"AN", b"CC") == -1            # pat == mat, a byte outside ACGT
    assert call([4, 5], b"Aa", b"CC") == -1 and call([4, 5], b"AA", b"C\0") == -1
    assert call([4, 5], b"AA", b"CC", _abi.LcrAseParams(31, prm.min_phase_score)) == -1     # min_baseq above the clamp
    assert lib.lcr_ase(E.h, C.byref(ap), 2, 0, None, None, None) == -1 and lib.lcr_ase(E.h, C.byref(ap), 0, -1, None, None, None) == -1
    assert lib.lcr_ase(E.h, C.byref(ap), 0, 2, None, None, None) == -1                      # sites without arrays
    assert lib.lcr_get_ase(E.h, C.byref(al)) == 0 and al.n_regions == 1
    assert np.frombuffer((C.c_char * 40).from_address(al.rec), dtype=_abi.ASE_DTYPE).tolist() == first.tolist()
    assert call([4, 5], b"AA", b"CC") == 0                                                  # good sites outside the region: plain counts
    assert E.ase(None).tolist() == check(E, res).tolist()
    # repeated with other sites; device-memory sites equal host-memory sites
    p2 = {p: v[::-1] for p, v in par.items()}
    second = check(E, res, p2)
    assert second.tolist()[0][6:] == tuple(first.tolist()[0][k] for k in (7, 6, 9, 8)) and second.tolist() != first.tolist()
    dev = [torch.from_numpy(a).cuda() for a in site_arrays(par)]
    assert E.ase(tuple(dev)).tolist() == first.tolist()
    # lcr_junctions before or after changes nothing in either table
    j1 = E.junctions(10, 0)[0]
    assert check(E, res, par).tolist() == first.tolist()
    assert E.junctions(10, 0)[0].tobytes() == j1.tobytes() and j1.size == 3
    after = (E.phase_result(), E.candidates(), E.fragmat())
    for x, y in zip(before, after):
        for k in (x if isinstance(x, dict) else range(len(x))):
            assert x[k].tobytes() == y[k].tobytes(), k
    # the asynchronous phase stage: the same records, and lcr_collect_phase still delivers afterwards
    A = engine_cls(0, prm)
    A.set_async_phase(True)
    A.load_batch(b1).run_all()
    assert A.ase(site_arrays(par)).tolist() == first.tolist()
    got = A.collect_phase(copy=True)
    assert got["assignment"].tobytes() == after[0]["assignment"].tobytes() and got["cand"].tobytes() == after[1][0].tobytes()
    A.close()
    # batch independence: two regions together and each alone
    E.load_batch(b2)
    assert lib.lcr_get_ase(E.h, C.byref(al)) == -4                                          # the records died with the binding
    E.run_all()
    assert lib.lcr_get_ase(E.h, C.byref(al)) == -4
    r2 = results(E)
    par2 = everything_parental(r2[2], 6)
    both = check(E, r2, par2)
    assert both.size == 2 and both["n_sites"].tolist() == [5, 12]
    E.get_candidate_snps()                                   # a new candidate stage drops the phase stage's results, and the records with them
    assert lib.lcr_get_ase(E.h, C.byref(al)) == -4 and lib.lcr_ase(E.h, C.byref(ap), 0, 0, None, None, None) == -4
    for g, reg in enumerate((regs[2], regs[4])):
        E.load_batch(tj.batch_of([reg])).run_all()
        one = check(E, results(E), par2)
        assert one.tolist()[0][1:] == both.tolist()[g][1:]
    E.close()

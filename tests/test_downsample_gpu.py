"""Down-sampled phasing on the GPU (lcr_set_downsample / lcr_set_downsample_rows / lcr_get_downsample) against the CPU reference
tests/downsample_ref.py: the sampler's bytes, the enumeration and the chain branch in their kernel classes, the rescue lists, the
explicit sample, and the entry points' contract."""
import functools

import numpy as np
import pytest

import downsample_ref as dsr
import helpers
import test_downsample_ref as ref_t
from longcallr_amd import _abi
from longcallr_amd._lib import LcrError

pytestmark = pytest.mark.gpu
F = _abi
CUT = 1e-6   # read_assign_cutoff > 0 (the presets' 0.0 is refused while down-sampling is on)


def noisy(b, sites, seed, frac=0.25):
    """base qualities from a few classes and, at the het sites, a fraction of swapped alleles: the sample and the full set of reads then
    disagree about a haplotype, an assignment or a phase score (asserted on the reference, compare())"""
    rng = np.random.default_rng(seed)
    b.quals[:] = rng.choice(np.array([7, 12, 18, 25, 35], dtype=np.uint8), size=b.quals.size)
    alt_of = {ord("A"): ord("C"), ord("C"): ord("A"), ord("G"): ord("T"), ord("T"): ord("G")}
    for r in range(b.n_reads):
        for x in sites:
            k = x - int(b.pos[r])
            if 0 <= k < int(b.seq_len[r]) and rng.random() < frac:
                rb = int(b.ref[x - int(b.start0[0])])
                i = int(b.seq_off[r]) + k
                b.bases[i] = alt_of[rb] if int(b.bases[i]) == rb else rb
    return b


def decisions(sf):
    """what down-sampling has to change somewhere: a haplotype, an assignment or a phase score"""
    return ([s.haplotype for s in sf.candidate_snps], [f.assignment for f in sf.fragments], [s.phase_score for s in sf.candidate_snps])


def compare(E, batch, prm, cands0, off0, depth=0, seed=2025, rows=None, need_effect=True):
    """every field the parity tests compare, region by region, against the CPU reference; returns the regions that were down-sampled.
    need_effect: for one of them the reference WITH the sample differs from the reference without it (a kernel that ignores the
    sample cannot pass)"""
    fm, pr = E.fragmat(), E.phase_result()
    c1, _ = E.candidates()
    info = E.downsample_info()
    applied, effect = [], False
    compare.refs, compare.cands0 = {}, cands0       # region -> the reference's SNPFrag, for what a case asserts on the reference side
    for g in range(batch.n_regions):
        a, b = int(off0[g]), int(off0[g + 1])
        r0, r1 = int(fm["row_region_off"][g]), int(fm["row_region_off"][g + 1])
        sf, read_ps, app = dsr.run_region(batch, g, prm, cands0[a:b], depth=depth, seed=seed, rows=None if rows is None else rows[r0:r1])
        assert len(sf.fragments) == r1 - r0 and bool(info["applied"][g]) == app
        compare.refs[g] = sf
        if app:
            applied.append(g)
            assert np.array_equal(info["sampled"][r0:r1], sf.sampled)
            off, ops, _ = dsr.run_region(batch, g, prm, cands0[a:b])
            effect = effect or decisions(off) != decisions(sf)
        if b == a:
            continue
        assert sf.objective == pytest.approx(pr["objective"][g], abs=1e-4)
        assert [f.haplotag for f in sf.fragments] == pr["haplotag"][r0:r1].tolist()
        assert [f.assignment for f in sf.fragments] == pr["assignment"][r0:r1].tolist()
        assert [read_ps.get(k, 0) for k in range(len(sf.fragments))] == pr["phase_set"][r0:r1].tolist()
        for s, c in zip(sf.candidate_snps, c1[a:b]):
            assert (s.haplotype, s.genotype, s.variant_type, s.phase_set) == (c["haplotype"], c["genotype"], c["variant_type"], c["phase_set"])
            fl = int(c["flags"])
            assert (s.rna_editing, s.dense, s.for_phasing, s.hom_var, s.single, s.non_selected, s.cand_somatic) == (
                bool(fl & F.F_RNA_EDIT), bool(fl & F.F_DENSE), bool(fl & F.F_FOR_PHASING), bool(fl & F.F_HOM), bool(fl & F.F_SINGLE),
                bool(fl & F.F_NON_SELECTED), bool(fl & F.F_CAND_SOMATIC))
            assert s.phase_score == pytest.approx(float(c["phase_score"]), rel=1e-9, abs=1e-12)
    if not applied:
        assert info["sampled"] is None and info["dev_sampled"] == 0
    tc = E.tie_census()
    assert tc["delta_unresolved"] == tc["step_unresolved"] == tc["best_unresolved"] == tc["sigma_unresolved"] == 0, tc
    if need_effect:
        assert applied and effect
    return applied


def run(engine_cls, batch, prm, depth=0, rows=None, debug=(), **kw):
    E = engine_cls(0, prm)
    for k, v in debug:
        E.debug_set(k, v)
    E.load_batch(batch).fill_data_into_freq_vec().get_candidate_snps()
    cands, off = E.candidates()
    cands = cands.copy()
    E.get_fragments()
    if rows is not None:
        E.set_downsample_rows(rows)
    else:
        E.set_downsample(depth, 2025)
    E.phase()
    out = compare(E, batch, prm, cands, off, depth=depth, rows=rows, **kw)
    res = (E.phase_result()["haplotag"].copy(), E.phase_result()["assignment"].copy(), E.candidates()[0].copy(), E.phase_result()["phase_set"].copy())
    E.close()
    return out, res


# ---- case 1: the sampler ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sampler_batch(sizes):
    """regions of sizes[i] identical short reads over one site each (the row count is what matters)"""
    ref = "ACGT" * 10
    reads, regions = [], []
    for g, n in enumerate(sizes):
        regions.append((1000 * (g + 1), ref))
        for k in range(n):
            s = list(ref[4:36])
            if k % 2:
                s[16] = "G"
            reads.append(dict(pos=1000 * (g + 1) + 4, seq="".join(s), qual=30, cigar="32M", rev=k // 2 % 2, ts=1 + k // 2 % 2, region=g))
    return helpers.mk_batch(reads, regions)


def sampler_masks(engine_cls, sizes, depth):
    b = sampler_batch(sizes)
    prm = _abi.make_params("hifi-masseq", seed=3, read_assign_cutoff=CUT)
    E = engine_cls(0, prm)
    E.load_batch(b).fill_data_into_freq_vec()
    pos0 = np.array([1000 * (g + 1) + 20 for g in range(len(sizes))], np.int64)
    E.import_external_candidates(pos0, np.ones(len(sizes), np.uint8), np.full(len(sizes), 30.0, np.float32))
    E.get_fragments()
    off = E.fragmat()["row_region_off"].copy()
    assert np.diff(off).tolist() == list(sizes)
    E.set_downsample(depth, 2025).phase()
    info = E.downsample_info()
    want, applied = dsr.batch_mask(2025, b.start0, off, depth)
    assert info["applied"].tolist() == [int(x) for x in applied]
    if any(applied):
        assert np.array_equal(info["sampled"], want)
        for g, n in enumerate(sizes):
            assert int(info["sampled"][off[g]:off[g + 1]].sum()) == (depth if applied[g] else n)
    else:
        assert info["sampled"] is None
    E.close()


def test_sampler_matches_the_reference_rule(engine_cls):
    sampler_masks(engine_cls, (63, 64, 65, 257), 64)          # depth - 1: not applied; depth: all ones; depth + 1; several passes' worth
    sampler_masks(engine_cls, (63, 64, 65, 257), 1)
    sampler_masks(engine_cls, (63,), 64)                       # nothing applies: the null path
    for n in (64, 65, 257):                                    # each region alone: the same bytes
        sampler_masks(engine_cls, (n,), 64)


def test_sampler_large_regions(engine_cls):
    sampler_masks(engine_cls, (9999, 10000, 10001, 70000), 10000)
    sampler_masks(engine_cls, (70000,), 10000)
    sampler_masks(engine_cls, (9999, 10000, 10001, 70000), 64)   # the small depths on the large regions
    sampler_masks(engine_cls, (9999, 10000, 10001, 70000), 1)
    sampler_masks(engine_cls, (70000,), 64)


# ---- case 2: enumeration branch ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def enum_batch():
    """S = 5: a region of 300 reads, one of 63 (below the depth) and one of exactly 64"""
    parts = [helpers.two_haplotype_batch(n_snps=5, n_reads=n, seed=s) for n, s in ((300, 1), (63, 2), (64, 3))]
    reads, regions = [], []
    for g, (p, sites) in enumerate(parts):
        noisy(p, sites[0], 10 + g)
        ref = bytes(p.ref).decode()
        regions.append((100000 * (g + 1), ref))
        for r in range(p.n_reads):
            so, n = int(p.seq_off[r]), int(p.seq_len[r])
            reads.append(dict(pos=int(p.pos[r]) - 5000 + 100000 * (g + 1), seq=bytes(p.bases[so:so + n]).decode(), qual=p.quals[so:so + n].tolist(),
                              cigar="%dM" % n, rev=int(p.flags[r]) & 1, ts=int(p.flags[r]) >> 1, region=g))
    return helpers.mk_batch(reads, regions)


@pytest.mark.parametrize("debug", [(), (("enum_force_stream", 1),), (("enum_force_big", 1),)], ids=["bits", "stream", "big"])
def test_enumeration_branch(engine_cls, debug):
    b = enum_batch()
    prm = _abi.make_params("hifi-masseq", seed=7, read_assign_cutoff=CUT)
    applied, res = run(engine_cls, b, prm, depth=64, debug=debug)
    assert applied == [0, 2]
    _, res_off = run(engine_cls, b, prm, depth=0, debug=debug, need_effect=False)
    fm_off = np.cumsum([0, 300, 63, 64])
    # the region exactly at the depth (all rows sampled) and the one below it: as with the feature off -- haplotags, assignments, read
    # phase sets and the candidate records, byte for byte
    for x, y in zip((res[0], res[1], res[3]), (res_off[0], res_off[1], res_off[3])):
        assert x.size == fm_off[3] and np.array_equal(x[fm_off[1]:], y[fm_off[1]:])
    c_on, c_off = res[2][res[2]["region"] >= 1], res_off[2][res_off[2]["region"] >= 1]
    assert c_on.size >= 10 and c_on.tobytes() == c_off.tobytes()
    assert res[2][res[2]["region"] == 0].tobytes() != res_off[2][res_off[2]["region"] == 0].tobytes()


# ---- case 3: chain branch ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_batch():
    b, sites = helpers.two_haplotype_batch(n_snps=8, groups=2, n_reads=200, seed=5)
    return noisy(b, sites[0] + sites[1], 21)


@pytest.mark.parametrize("debug", [(), (("grid_min_entries", 0), ("grid_spec_batch", 1)), (("grid_min_entries", 0), ("grid_spec_batch", 0))],
                         ids=["wg", "grid_batch", "grid_lanes"])
def test_chain_branch(engine_cls, debug):
    b = chain_batch()
    prm = _abi.make_params("hifi-masseq", seed=9, max_enum_snps=3, read_assign_cutoff=CUT)
    applied, _ = run(engine_cls, b, prm, depth=100, debug=debug)
    assert applied == [0]


def test_chain_staged_by_all_cus_phased_by_a_workgroup(engine_cls):
    """the combination only a sample produces: the island's full entry count is at the all-CU threshold (k4_stage_grid stages it), its
    sampled entry count below it (k4_chain_wg phases it, its LD pair table over four times the rows the optimiser sees)"""
    b = chain_batch()
    prm = _abi.make_params("hifi-masseq", seed=9, max_enum_snps=3, read_assign_cutoff=CUT)
    E = engine_cls(0, prm)
    E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps()
    cands, off = E.candidates()
    cands = cands.copy()
    E.get_fragments()
    rp = E.fragmat()["row_ptr"]
    rows = dsr.sample_rows(2025, int(b.start0[0]), 400, 100)
    e_all, e_smp = int(rp[-1]), int((np.diff(rp) * rows).sum())        # (e_smp: an upper bound of the sampled phase matrix)
    assert rp.size == 401 and 0 < e_smp < e_all
    E.debug_set("grid_min_entries", e_all)                              # sampled entries < grid_min <= all entries
    E.set_downsample(100, 2025).phase()
    assert compare(E, b, prm, cands, off, depth=100) == [0]
    E.close()


# ---- case 4: rescue ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mps", [8.0, 60.0], ids=["rescued", "not_rescued"])
def test_rescue_lists(engine_cls, mps):
    b, sites = helpers.two_haplotype_batch(n_snps=5, n_reads=120, edit_sites=(777,), edit_frac=0.95, seed=2)
    b.flags[:] = 0 | (1 << 1)
    noisy(b, sites[0], 34, frac=0.3)   # (noise seed, fraction and depth chosen on the CPU reference: both outcomes, and the sample changes decisions)
    prm = _abi.make_params("hifi-masseq", seed=4, min_phase_score=mps, read_assign_cutoff=CUT)
    run(engine_cls, b, prm, depth=40)      # 80 of the edit site's 120 cover rows are unsampled
    # on the reference side: the outcome is the one the id names, and the commit loop (snpfrags.rs:257-262) drew once for every unsampled
    # cover row (their assignment is 0 there) -- the draws of a rescued site, none otherwise
    sf = compare.refs[0]
    edit = [s for s in sf.candidate_snps if s.pos == 5777]
    assert len(edit) == 1 and len(edit[0].snp_cover_fragments) == 120
    assert sum(not sf.fragments[k].downsampled for k in edit[0].snp_cover_fragments) == 80
    rescued = mps == 8.0
    assert (edit[0].rna_editing, edit[0].for_phasing) == ((False, True) if rescued else (True, False))
    other, _, _ = dsr.run_region(b, 0, _abi.make_params("hifi-masseq", seed=4, min_phase_score=68.0 - mps, read_assign_cutoff=CUT), compare.cands0, depth=40)
    assert (sf.ctr - other.ctr) * (1 if rescued else -1) == 80


# ---- case 5: the known answer through the explicit sample; an explicit sample equal to sample_rows ---------------------------------
def test_known_answer_and_explicit_rows(engine_cls):
    b, sites = ref_t.kat_batch()
    prm = _abi.make_params("hifi-masseq", seed=11, read_assign_cutoff=CUT)
    E = engine_cls(0, prm)
    E.load_batch(b).fill_data_into_freq_vec()
    E.import_external_candidates(np.array(sites, np.int64), np.ones(2, np.uint8), np.full(2, 30.0, np.float32))
    cands, off = E.candidates()
    cands = cands.copy()
    rows = np.zeros(32, np.uint8); rows[24:] = 7             # (non-zero = sampled)
    E.get_fragments().set_downsample_rows(rows).phase()
    compare(E, b, prm, cands, off, rows=(rows != 0).astype(np.uint8))
    pr, c1 = E.phase_result(), E.candidates()[0]
    assert int(c1["haplotype"][0]) * int(c1["haplotype"][1]) == -1
    assert pr["assignment"][:24].tolist() == [0] * 24 and pr["haplotag"][:24].tolist() == [0] * 24
    assert sorted(pr["assignment"][24:].tolist()) == [1] * 4 + [2] * 4
    E.close()
    cb = chain_batch()
    prm = _abi.make_params("hifi-masseq", seed=9, max_enum_snps=3, read_assign_cutoff=CUT)
    _, res_a = run(engine_cls, cb, prm, depth=100)
    _, res_b = run(engine_cls, cb, prm, rows=dsr.sample_rows(2025, int(cb.start0[0]), 400, 100))
    for x, y in zip(res_a, res_b):
        assert x.tobytes() == y.tobytes()


# ---- case 6: the contract of the entry points -------------------------------------------------------------------------------------
def test_contract_and_reentry(engine_cls):
    b = enum_batch()
    prm = _abi.make_params("hifi-masseq", seed=7, read_assign_cutoff=CUT)
    prm0 = _abi.make_params("hifi-masseq", seed=7)             # the preset's cutoff of 0.0

    def stage(E):
        E.get_candidate_snps()
        c, off = E.candidates()
        return c.copy(), off.copy()

    def snap(E):
        pr = E.phase_result()
        return (pr["haplotag"].tobytes(), pr["assignment"].tobytes(), pr["phase_set"].tobytes(), E.candidates()[0].tobytes())

    never = engine_cls(0, prm)
    never.load_batch(b).fill_data_into_freq_vec()
    stage(never); never.get_fragments().phase()
    base = snap(never)
    assert never.downsample_info()["sampled"] is None
    never.close()

    E = engine_cls(0, prm)
    E.load_batch(b).fill_data_into_freq_vec()
    with pytest.raises(LcrError, match=r"\(-4\)"):              # no fragment stage yet
        E.set_downsample_rows(np.ones(427, np.uint8))
    c0, off = stage(E)
    E.get_fragments()
    with pytest.raises(LcrError, match=r"\(-1\)"):              # wrong row count
        E.set_downsample_rows(np.ones(426, np.uint8))
    E.set_downsample(64)
    E.phase()
    on = snap(E)
    assert on != base and E.downsample_info()["applied"].tolist() == [1, 0, 1]   # (enum_batch: the sample changes the first region's results)
    with pytest.raises(LcrError, match=r"\(-4\)"):              # after lcr_phase: the rows of a consumed fragment stage
        E.set_downsample_rows(np.ones(427, np.uint8))
    E.set_downsample(0)                                         # on -> off: as a context that never had it on
    stage(E); E.get_fragments().phase()
    assert snap(E) == base and E.downsample_info()["sampled"] is None
    E.set_downsample(64)                                        # off -> on
    stage(E); E.get_fragments().phase()
    assert snap(E) == on
    E.set_downsample(0)                                         # the explicit sample is one-shot
    rows, _ = dsr.batch_mask(2025, b.start0, [0, 300, 363, 427], 64)
    stage(E); E.get_fragments().set_downsample_rows(rows).phase()
    assert snap(E) == on
    stage(E); E.get_fragments().phase()
    assert snap(E) == base
    # read_assign_cutoff <= 0 is refused while down-sampling is on, and nothing has changed; the keys of the host epilogue are unknown
    E.set_downsample(64)
    stage(E); E.get_fragments()
    E.params = prm0
    with pytest.raises(LcrError, match=r"\(-1\)"):
        E.phase()
    E.params = prm
    with pytest.raises(LcrError, match=r"\(-1\)"):
        E.debug_set("post_host", 1)
    with pytest.raises(LcrError, match=r"\(-1\)"):
        E.debug_set("host_threads", 4)
    E.phase()
    assert snap(E) == on
    E.close()
    # asynchronous stage + lcr_collect_phase in the pipelined order = the synchronous result
    A = engine_cls(0, prm)
    A.set_async_phase(True)
    A.set_downsample(64)
    A.load_batch(b).fill_data_into_freq_vec()
    stage(A); A.get_fragments().phase()
    A.load_batch(chain_batch()).fill_data_into_freq_vec()       # (another batch: the getters below speak of the phase stage in flight)
    col = A.collect_phase(copy=True)
    info = A.downsample_info()
    assert info["applied"].tolist() == [1, 0, 1] and np.array_equal(info["sampled"], rows)
    A.get_candidate_snps()
    with pytest.raises(LcrError, match=r"\(-4\)"):              # as lcr_collect_phase: not past the next candidate stage
        A.downsample_info()
    assert (col["haplotag"].tobytes(), col["assignment"].tobytes(), col["phase_set"].tobytes(), col["cand"].tobytes()) == on
    A.close()

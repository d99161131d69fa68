"""The three forms of phase staging side by side on ONE small batch: k4_stage from its LDS image, k4_stage from global memory, and
k4_stage_grid (grid_min_entries = 0: every region with an entry; the chain region then also takes k4_chain_grid / k4_gpost).  Each region
of the batch is there for one form or one early return, and says so by a precondition asserted on the GPU's own fragment matrix and
candidate list before anything is compared.  Every run equals the oracle (down-sampled runs: tests/downsample_ref.py), and the
enumeration regions come out byte for byte the same whichever kernel staged them.

The deep region is two_haplotype_batch(n_snps=4, n_reads=2100), 8 400 entries, where (n_snps=9, n_reads=1000) would do for the form: the
down-sampled runs compare with a pure-Python reference that walks every fragment row in each of its 2^S restarts (31 s at S = 9, 1.4 s at
S = 4), and what selects the form is the entry count alone (entries > STG_E with rows <= STG_R)."""
import functools

import numpy as np
import pytest

import downsample_ref as dsr
import helpers
import test_gpu_parity as par
from longcallr_amd import _abi, vcf
from test_downsample_gpu import CUT, noisy

pytestmark = pytest.mark.gpu
F = _abi
STG_E, STG_R, STG_S = 8192, 4096, 512    # k4_kernels.h: the LDS image of k4_stage
NONE, LONE, ENUM, DEEP, CHAIN = range(5)
DEPTH = 100                               # below the deep region's and the chain region's row counts, above the others'


@functools.lru_cache(maxsize=1)
def forms_batch():
    reads, regions = [], []

    def add(p):
        g = len(regions)
        regions.append((100000 * (g + 1), bytes(p.ref).decode()))
        for r in range(p.n_reads):
            so, n = int(p.seq_off[r]), int(p.seq_len[r])
            reads.append(dict(pos=int(p.pos[r]) - int(p.start0[0]) + 100000 * (g + 1), seq=bytes(p.bases[so:so + n]).decode(),
                              qual=p.quals[so:so + n].tolist(), cigar="%dM" % n, rev=int(p.flags[r]) & 1, ts=int(p.flags[r]) >> 1, region=g))

    p, _ = helpers.two_haplotype_batch(n_snps=3, n_reads=20, seed=1)          # NONE: every read is the reference
    for r in range(p.n_reads):
        so, n = int(p.seq_off[r]), int(p.seq_len[r])
        p.bases[so:so + n] = p.ref[:n]
    add(p)
    p, sites = helpers.two_haplotype_batch(n_snps=4, n_reads=2, seed=2)       # LONE: 24 reads of 60 bases over each site, none over two
    ref = bytes(p.ref).decode()
    alt_of = {"A": "C", "C": "A", "G": "T", "T": "G"}
    short = []
    for x in (s - 5000 for s in sites[0]):
        for k in range(24):
            s = list(ref[x - 30:x + 30])
            if k % 2 == 0:
                s[30] = alt_of[ref[x]]
            short.append(dict(pos=5000 + x - 30, seq="".join(s), qual=30, cigar="60M", rev=k // 2 % 2, ts=1 + k // 2 % 2, region=0))
    add(helpers.mk_batch(short, [(5000, ref)]))
    for n_snps, n_reads, seed in ((5, 40, 3), (4, 2100, 4), (12, 300, 5)):    # ENUM, DEEP, CHAIN
        p, sites = helpers.two_haplotype_batch(n_snps=n_snps, n_reads=n_reads, seed=seed)
        add(noisy(p, sites[0], 40 + seed, frac=0.08))
    return helpers.mk_batch(reads, regions)


def check_preconditions(E, prm):
    """what makes each region exercise its form, from the GPU's fragment matrix and candidates"""
    _, off = E.candidates()
    fm = E.fragmat()
    S = np.diff(off)
    ro = fm["row_region_off"]
    rows = np.diff(ro)
    ent = np.diff(fm["row_ptr"][ro])
    links = [fm["row_links"][ro[g]:ro[g + 1]] for g in range(5)]
    assert S[NONE] == 0
    assert S[LONE] > 0 and rows[LONE] > 0 and np.all(links[LONE] == 1)           # min_linkers = 2: candidates and no phasing row
    assert 0 < S[ENUM] <= prm.max_enum_snps and rows[ENUM] <= STG_R and ent[ENUM] <= STG_E and np.all(links[ENUM] >= 2)
    assert 0 < S[DEEP] <= min(prm.max_enum_snps, STG_S) and ent[DEEP] > STG_E and rows[DEEP] <= STG_R and DEPTH < rows[DEEP]
    assert S[CHAIN] > prm.max_enum_snps and 200 <= rows[CHAIN] <= 500 and DEPTH < rows[CHAIN]
    assert rows[LONE] < DEPTH and rows[ENUM] < DEPTH


def staged(engine_cls, prm, grid_min, depth=0):
    """the batch up to the fragment stage (preconditions asserted), the sample set, phased; returns the engine and the candidates before phasing"""
    E = engine_cls(0, prm)
    if grid_min is not None:
        E.debug_set("grid_min_entries", grid_min)
    E.load_batch(forms_batch()).fill_data_into_freq_vec().get_candidate_snps()
    c0, off = E.candidates()
    c0, off = c0.copy(), off.copy()
    E.get_fragments()
    check_preconditions(E, prm)
    if depth:
        E.set_downsample(depth, 2025)
    E.phase()
    return E, c0, off


def region_bytes(E, g):
    """par._result_bytes of one region"""
    c, off = E.candidates()
    ro = E.fragmat()["row_region_off"]
    pr = E.phase_result()
    return (c[off[g]:off[g + 1]].tobytes(),) + tuple(pr[f][ro[g]:ro[g + 1]].tobytes() for f in ("haplotag", "assignment", "phase_set")) + (
        pr["objective"][g:g + 1].tobytes(),)


@pytest.mark.parametrize("min_linkers", [1, 2])
def test_forms_agree_with_the_oracle_and_each_other(engine_cls, orc, monkeypatch, min_linkers):
    b = forms_batch()
    prm = _abi.make_params("hifi-masseq", seed=7, min_linkers=min_linkers)
    got = {}
    for grid_min in (None, 0):
        # all CUs on a chain region: sigma ties only (orc.TIE_MASK_LIBLCR_GRID differs from the default mask in the chain branch alone)
        monkeypatch.setitem(par.ORACLE_TIE_MASK, 0, None if grid_min is None else orc.TIE_MASK_LIBLCR_GRID)
        regs = par.oracle_all(orc, b, prm)
        par.check_f64_mode(orc, b, prm, regs, "chrS")
        E, _, _ = staged(engine_cls, prm, grid_min)
        par.check_pileup(E, regs, b)
        fm = par.check_fragmat(E, regs)
        c, off = par.check_cands(E, regs, phased=True)
        par.check_phase(E, regs, fm)
        for g, R in enumerate(regs):
            assert vcf.format_records(c[off[g]:off[g + 1]], "chrS", prm.min_phase_score) == R.vcf_text("chrS")
        assert E.ld_blocks(CHAIN) == regs[CHAIN].ld_blocks()
        if min_linkers == 2:
            assert not fm["row_for_phasing"][fm["row_region_off"][LONE]:fm["row_region_off"][LONE + 1]].any()
        got[grid_min] = [region_bytes(E, g) for g in range(5)]
        assert par._result_bytes(E) == tuple(b"".join(x[k] for x in got[grid_min]) for k in range(5))   # (the regions partition the results)
        E.close()
    for g in (NONE, LONE, ENUM, DEEP):
        assert got[None][g] == got[0][g], "region %d: k4_stage against k4_stage_grid" % g


@functools.lru_cache(maxsize=1)
def downsampled_reference(cands0, off0):
    """tests/downsample_ref.py on every region, once for both grid_min_entries settings (the candidates before phasing are the same bytes)"""
    b = forms_batch()
    prm = _abi.make_params("hifi-masseq", seed=7, read_assign_cutoff=CUT)
    c0 = np.frombuffer(cands0, dtype=_abi.CAND_DTYPE)
    return [dsr.run_region(b, g, prm, c0[off0[g]:off0[g + 1]], depth=DEPTH, seed=2025) for g in range(5)]


@pytest.mark.parametrize("grid_min", [None, 0], ids=["default", "all_cus"])
def test_forms_down_sampled(engine_cls, grid_min):
    """the draw ordinals of both staging kernels: the fields tests/test_downsample_gpu.py compares, against the same reference"""
    prm = _abi.make_params("hifi-masseq", seed=7, read_assign_cutoff=CUT)
    E, c0, off = staged(engine_cls, prm, grid_min, depth=DEPTH)
    ref = downsampled_reference(c0.tobytes(), tuple(int(x) for x in off))
    fm, pr, info = E.fragmat(), E.phase_result(), E.downsample_info()
    c1, _ = E.candidates()
    assert info["applied"].tolist() == [0, 0, 0, 1, 1]
    for g, (sf, read_ps, app) in enumerate(ref):
        a, z = int(off[g]), int(off[g + 1])
        r0, r1 = int(fm["row_region_off"][g]), int(fm["row_region_off"][g + 1])
        assert len(sf.fragments) == r1 - r0 and bool(info["applied"][g]) == app
        if app:
            assert np.array_equal(info["sampled"][r0:r1], sf.sampled) and int(sf.sampled.sum()) == DEPTH
        if z == a:
            continue
        assert sf.objective == pytest.approx(pr["objective"][g], abs=1e-4)
        assert [f.haplotag for f in sf.fragments] == pr["haplotag"][r0:r1].tolist()
        assert [f.assignment for f in sf.fragments] == pr["assignment"][r0:r1].tolist()
        assert [read_ps.get(k, 0) for k in range(len(sf.fragments))] == pr["phase_set"][r0:r1].tolist()
        for s, c in zip(sf.candidate_snps, c1[a:z]):
            assert (s.haplotype, s.genotype, s.variant_type, s.phase_set) == (c["haplotype"], c["genotype"], c["variant_type"], c["phase_set"])
            fl = int(c["flags"])
            assert (s.rna_editing, s.dense, s.for_phasing, s.hom_var, s.single, s.non_selected, s.cand_somatic) == (
                bool(fl & F.F_RNA_EDIT), bool(fl & F.F_DENSE), bool(fl & F.F_FOR_PHASING), bool(fl & F.F_HOM), bool(fl & F.F_SINGLE),
                bool(fl & F.F_NON_SELECTED), bool(fl & F.F_CAND_SOMATIC))
            assert s.phase_score == pytest.approx(float(c["phase_score"]), rel=1e-9, abs=1e-12)
    tc = E.tie_census()
    assert tc["delta_unresolved"] == tc["step_unresolved"] == tc["best_unresolved"] == tc["sigma_unresolved"] == 0, tc
    E.close()

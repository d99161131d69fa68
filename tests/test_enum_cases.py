"""The recipes of tests/enum_cases.py on the CPU: for every case the two oracles -- oracle/lcr_oracle.cpp (ORC_MODE_TIE with the tie classes
liblcr resolves, what the GPU tests compare with) and oracle_np_phase.run_region, its restarts run by enum_cases.Census -- leave the same sites
and reads; the region is phased by enumeration with the case's number of sites; its phase matrix is the one the recipe implies and lands in
the kernel class the case names (enum_cases.predicted_class; tests/test_enum_cases_gpu.py holds that restatement against the library's own
report); and the case's census holds: the restarts met the limit the case was built for."""
import functools

import numpy as np
import pytest

import enum_cases as ec
from longcallr_amd import _abi
from oracle import oracle_np_phase as onp2

F = _abi


@functools.lru_cache(maxsize=None)
def _visit(name):
    """per region of the case: both oracles' runs, once for all tests (what they left, not the oracle's region object: the cache outlives it)"""
    from oracle import orc
    orc.build()
    b, prm = ec.batch(name), ec.params(name)
    out = []
    for g in range(b.n_regions):
        R = orc.Region(b, g, prm).pileup().candidates().fragments()
        c0, fm = R.cands(), R.fragmat()
        sf, read_ps = onp2.run_region(b, g, prm, c0, frag_cls=ec.Census)
        R.set_tie_mask(orc.TIE_MASK_LIBLCR).phase(orc.MODE_TIE)
        phased = R.cands()                 # delta / eta as the restarts leave them
        R.post_phase()
        out.append(dict(c0=c0, fm=fm, sf=sf, read_ps=read_ps, phased=phased, report=sf.report(), cands=R.cands(), phase=R.phase_result(),
                        violations=R.stats()["assert_violations"], tie_census=R.tie_census()))
    return out


@pytest.mark.parametrize("name", ec.NAMES)
def test_oracles_agree_and_the_census_holds(orc, name):
    b, prm, case = ec.batch(name), ec.params(name), ec.BY_NAME[name]
    assert b.bases.size <= 550000 and all(int(n) <= 1500 for n in np.diff(b.read_begin)) and len(case["cls"]) == b.n_regions
    for g, v in enumerate(_visit(name)):
        sf, rep = v["sf"], v["report"]
        assert v["violations"] == 0
        c, pr = v["cands"], v["phase"]
        assert len(c) == len(sf.candidate_snps) == case["S"] <= prm.max_enum_snps             # phased by enumeration, S as the case says
        for s, x in zip(sf.candidate_snps, c):
            fl = int(x["flags"])
            assert (s.pos, s.haplotype, s.genotype, s.variant_type, s.phase_set) == tuple(int(x[f]) for f in ("pos", "haplotype", "genotype", "variant_type", "phase_set")), s.pos
            assert (s.rna_editing, s.dense, s.for_phasing, s.single, s.non_selected, s.cand_somatic) == tuple(
                bool(fl & m) for m in (F.F_RNA_EDIT, F.F_DENSE, F.F_FOR_PHASING, F.F_SINGLE, F.F_NON_SELECTED, F.F_CAND_SOMATIC)), s.pos
            assert s.phase_score == pytest.approx(x["phase_score"], abs=1e-9)
        assert [f.assignment for f in sf.fragments] == pr["assignment"].tolist()
        assert [f.haplotag for f in sf.fragments] == pr["haplotag"].tolist()
        assert [v["read_ps"].get(k, 0) for k in range(len(sf.fragments))] == pr["phase_set"].tolist()
        # the phase matrix and its class
        nR, nE, rp = ec.phase_matrix(v["fm"], v["c0"])
        assert (nR, nE, len(c), ec.max_rows(rp)) == ec.shape(name)[g] and (nR, nE) == (rep["R"], rep["E"])
        assert ec.predicted_class(nR, nE, len(c), ec.max_rows(rp)) == case["cls"][g] == ec.classes(name)[g]
        # the census of the restatement is the C++ oracle's, count for count: sigma ties, delta / eta ties at the maximum, tie-only steps,
        # compares at equal objective
        tc = v["tie_census"]
        assert rep["n_restarts"] == 1 << len(c)
        assert [rep["sigma_ties"], rep["class2_ties"], rep["class4_steps"], rep["equal_objective_compares"]] == tc[:4].tolist()
        print("%s region %d: R %d E %d S %d %s %s" % (name, g, nR, nE, len(c), case["cls"][g], {
            k: rep[k] for k in ("max_tied_rows", "tied_rows_final", "maxima", "term_sequences", "redo_restarts", "class4_steps", "max_iters")}))
        want = case["census"]
        bad = ec.census_holds(want, rep)
        assert not bad, "census of %s: (wanted, got) %s" % (name, bad)
        lanes = ec.lane_rows(rp)
        if "one_lane" in want:
            a, z = want["one_lane"]
            assert z == a + 1 and a % 64 == 63 and lanes[a] == lanes[z]          # the last row of a sigma word and the next one in one lane's run
        if name == "single_entry_rows":      # base qualities 31, 60 and 93 went in; the one-entry rows hold them clamped, and q <= 3 as it is
            fm = v["fm"]
            one = np.flatnonzero(np.diff(fm["row_ptr"]) == 1)
            assert {31, 60, 93} <= set(b.quals.tolist())
            assert set((fm["val"][fm["row_ptr"][one]] & 31).tolist()) == {min(q, 30) for q in ec.SINGLE_Q} >= {1, 2, 3, 30}
        if "max_rows" in want:
            assert ec.max_rows(rp) >= want["max_rows"][1] > 64
            assert ec.predicted_class(nR, nE, len(c)) == "stream"                 # (its image fits: the lane's rows alone send it away)


@pytest.mark.parametrize("name", [n for n in ec.NAMES if n.startswith("tq_")])
def test_tied_rows_of_the_last_sigma_step(orc, name):
    """the tq_* cases from the C++ oracle's side alone: under its final delta / eta the rows of more than two phase entries whose signed
    fixed-point weights cancel are exactly the case's number (at least 300 for tq_300*); the restatement's winning restart meets exactly
    these rows in its last sigma step, no step of any restart meets more, and the oracle counted sigma ties."""
    (v,) = _visit(name)
    fm, c = v["fm"], v["phased"]
    fp = (v["c0"]["flags"] & F.F_FOR_PHASING) != 0
    het = c["genotype"] == 0
    w = np.array(ec.FX_1E) - np.array(ec.FX_E)
    tied, k = [], 0
    for r in np.flatnonzero(fm["row_for_phasing"]):
        e = np.arange(fm["row_ptr"][r], fm["row_ptr"][r + 1])
        e = e[fp[fm["col"][e]]]
        col, val = fm["col"][e], fm["val"][e]
        x = np.where((val & 32) != 0, 1, -1) * c["haplotype"][col]                 # p * delta: +1 = a match under sigma = +1
        if len(e) > 2 and int((x * w[val & 31] * het[col]).sum()) == 0:
            tied.append(k)
        k += 1
    n = int(name.split("_")[1])
    assert len(tied) == n if n < 300 else len(tied) >= 300
    assert (n > ec.ENUM_TQ) == (name != "tq_126")
    rep = v["report"]
    assert tied == rep["zero_weight_rows"] == rep["winner_last_step_tied"]
    assert rep["max_tied_rows"] == n
    assert v["tie_census"][0] > 0 and v["tie_census"][8] > 0


def test_the_cases_meet_every_limit_they_name():
    """the ledger: each limit of enum_cases' docstring has a case whose census or class demands it"""
    want = {c["name"]: c["census"] for c in ec.CASES}
    cls = {c["name"]: c["cls"] for c in ec.CASES}
    # ENUM_TQ: the last count that fits, the first that does not, far beyond; with hom sites under the tied rows
    assert [want[n]["max_tied_rows"] for n in ("tq_126", "tq_127", "tq_300", "tq_300_hom")] == [ec.ENUM_TQ, ec.ENUM_TQ + 1, 300, 300]
    assert want["tq_300_hom"]["hom_sites"] == 2
    # ENUM_TCAP: more maxima than one batch, of more than one term sequence, at two sizes of resolve_tlcap, in both LDS classes
    for n in ("tcap_1024", "tcap_512"):
        assert want[n]["maxima"][1] > ec.ENUM_TCAP and want[n]["term_sequences"][1] >= 2
    assert ec.resolve_tlcap(ec.BY_NAME["tcap_1024"]["S"]) == 1024 and ec.resolve_tlcap(ec.BY_NAME["tcap_512"]["S"]) == 512
    assert {cls["tcap_1024"], cls["tcap_512"]} == {("stream",), ("bits",)}
    # REDO_GRID < repair list < REDO_CAP (a region of 2^10 restarts cannot pass the cap)
    assert want["redo_over_grid"]["redo_restarts"][1] > ec.REDO_GRID and 1 << ec.BY_NAME["redo_over_grid"]["S"] < ec.REDO_CAP
    # ENUM_LDS_MAX: both edges from either side, by size alone; all three classes in one batch; the rows-per-lane rule
    assert [cls[n] for n in ("class_bits_last", "class_stream_first", "class_stream_last", "class_big_first")] == [("bits",), ("stream",), ("stream",), ("big",)]
    R = {n: ec.shape(n)[0][0] for n in cls if n.startswith("class_") and n != "class_mixed"}
    assert R["class_stream_first"] == R["class_bits_last"] + 1 and R["class_big_first"] == R["class_stream_last"] + 1
    assert cls["class_mixed"] == ("bits", "stream", "big", "bits") and ec.shape("class_mixed")[3][0] < ec.shape("class_mixed")[0][0]
    assert cls["max_rows_65"] == ("big",) and want["max_rows_65"]["max_rows"][1] == 65
    # sigma words, lane shares, one-entry rows, negative weights, tiles
    assert [ec.shape("rows_%d" % n)[0][0] for n in (63, 64, 65, 128, 129)] == [63, 64, 65, 128, 129]
    assert want["rows_65"]["one_lane"] == (63, 64) and want["rows_129"]["one_lane"] == (127, 128)
    assert [want["entries_%d" % n]["E"] for n in (60, 64, 65)] == [60, 64, 65]
    assert want["single_entry_rows"]["one_entry_rows"] > ec.shape("single_entry_rows")[0][0] // 2 and want["single_entry_rows"]["q_le_3"][1] >= 1
    n_restarts = [1 << ec.BY_NAME["tile_s%d" % S]["S"] for S in (5, 6, 7, 8, 9)]
    assert n_restarts == [ec.ENUM_BITS_PER // 2, ec.ENUM_BITS_PER, 2 * ec.ENUM_BITS_PER, 256, 512]
    assert ec.enum_bits_sp(8) == 8 and ec.enum_bits_sp(9) == 16


def test_class_edges_move_with_the_row_length():
    """predicted_class over uniform rows: one edge pair per (S, entries per row), bit-state below streaming below global memory"""
    for S, per in ((3, 3), (4, 4), (2, 2), (4, 1)):
        a, z = ec.class_edges(S, per)
        assert 0 < a < z
        assert [ec.predicted_class(R, R * per, S) for R in (a, a + 1, z, z + 1)] == ["bits", "stream", "stream", "big"]

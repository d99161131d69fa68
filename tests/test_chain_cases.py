"""The recipes of tests/chain_cases.py on the CPU: for every case the two oracles -- oracle/lcr_oracle.cpp and oracle_np_phase.run_region, its
chain run by chain_cases.ChainCensus -- leave the same fragment rows, LD blocks, sigma / delta / eta, objective and phase sets; the tie census
of the restatement is the C++ oracle's count for count; every region is a chain region of the shape the recipe implies and lands in the form
the case names (chain_cases.predicted_form; tests/test_chain_cases_gpu.py holds that restatement against the library's own report); and the
case's census holds: the run met the limit the case was built for.  The four cases of chain_cases.BLOCKS_ONLY stop behind the LD blocks
(oracle_np_phase would take minutes on them)."""
import functools

import numpy as np
import pytest

import chain_cases as cc
from longcallr_amd import _abi
from oracle import oracle_np_phase as onp2

F = _abi


@functools.lru_cache(maxsize=None)
def _visit(name):
    """per region of the case: both oracles' runs, once for all tests"""
    from oracle import orc
    orc.build()
    b, prm = cc.batch(name), cc.params(name)
    out = []
    for g in range(b.n_regions):
        R = orc.Region(b, g, prm).set_fast(1).pileup().candidates().fragments()
        c0, fm = R.cands(), R.fragmat()
        v = dict(c0=c0, fm=fm, shape=cc.region_shape(fm, c0))
        if name in cc.BLOCKS_ONLY:
            sf = onp2.fragment_rows(b, g, prm, c0, frag_cls=cc.ChainCensus)
            sf.divide_snps_into_blocks(1)
            R.phase(orc.MODE_F64)
            v.update(sf=sf, report=sf.report(), ld_blocks=R.ld_blocks())
        else:
            sf, read_ps = onp2.run_region(b, g, prm, c0, frag_cls=cc.ChainCensus)
            R.phase(orc.MODE_F64)
            v.update(sf=sf, read_ps=read_ps, report=sf.report(), ld_blocks=R.ld_blocks())
            R.post_phase()
            v.update(cands=R.cands(), phase=R.phase_result(), stats=R.stats())
            T = orc.Region(b, g, prm).set_fast(1).pileup().candidates().fragments().set_tie_mask(orc.TIE_MASK_LIBLCR).phase(orc.MODE_TIE).post_phase()
            v.update(tie_census=T.tie_census(), tie_phase=T.phase_result())
        out.append(v)
    return out


def _forms(name, grid_min=cc.GRID_MIN):
    return cc.forms([v["shape"] for v in _visit(name)], grid_min)


@pytest.mark.parametrize("name", cc.NAMES)
def test_oracles_agree_and_the_census_holds(orc, name):
    prm, case = cc.params(name), cc.BY_NAME[name]
    assert len(case["shape"]) == cc.batch(name).n_regions
    for g, v in enumerate(_visit(name)):
        sf, rep, fm = v["sf"], v["report"], v["fm"]
        # fragment rows
        assert len(sf.fragmat_snapshot) == len(fm["row_read"])
        for k, (read, ents, links, fp) in enumerate(sf.fragmat_snapshot):
            e0, e1 = fm["row_ptr"][k], fm["row_ptr"][k + 1]
            assert read == fm["row_read"][k] and [e[0] for e in ents] == fm["col"][e0:e1].tolist()
            assert [(e[2] & 31) | (32 if e[3] == 1 else 0) for e in ents] == [int(x) & 63 for x in fm["val"][e0:e1]]
            assert links == fm["row_links"][k] and int(fp) == fm["row_for_phasing"][k]
        # a chain region of the shape the recipe implies
        R_, S, E, n_ent, W = v["shape"]
        assert S > prm.max_enum_snps
        if case["shape"][g] is not None:
            assert v["shape"] == case["shape"][g]
        # LD blocks in the reference's block / node order
        assert sf.ld_blocks == v["ld_blocks"]
        print("%s region %d: R %d S %d E %d n_ent %d W %d %s %s" % (name, g, R_, S, E, n_ent, W, _forms(name)[g], {
            k: rep.get(k) for k in ("max_degree", "dfs_depth", "block_sizes", "block_order", "flipped_blocks", "flip_run_kinds", "block_column_lengths",
                                    "sigma_ties", "class2_ties", "class4_steps", "equal_objective_compares", "f64_sum_compares", "max_tied_rows",
                                    "trans_edges", "eligible_without_edge", "phasing_not_eligible", "not_phasing")}))
        assert rep["block_order"] == sorted(rep["block_order"], reverse=True)       # device block 0 = the block the reference visits last
        if name not in cc.BLOCKS_ONLY:
            assert v["stats"]["assert_violations"] == 0
            c, pr = v["cands"], v["phase"]
            assert sf.n_cross == v["stats"]["cross_optimize_calls"] == 1 + 2 * (S // 4 + 1)
            assert sf.objective == pytest.approx(pr["objective"], abs=1e-9)
            for s, x in zip(sf.candidate_snps, c):
                fl = int(x["flags"])
                assert (s.pos, s.haplotype, s.genotype, s.variant_type, s.phase_set) == tuple(int(x[f]) for f in ("pos", "haplotype", "genotype", "variant_type", "phase_set")), s.pos
                assert (s.rna_editing, s.for_phasing, s.single, s.non_selected, s.cand_somatic) == tuple(
                    bool(fl & m) for m in (F.F_RNA_EDIT, F.F_FOR_PHASING, F.F_SINGLE, F.F_NON_SELECTED, F.F_CAND_SOMATIC)), s.pos
                assert s.phase_score == pytest.approx(x["phase_score"], abs=1e-9)
            assert [f.assignment for f in sf.fragments] == pr["assignment"].tolist()
            assert [f.haplotag for f in sf.fragments] == pr["haplotag"].tolist()
            assert [v["read_ps"].get(k, 0) for k in range(len(sf.fragments))] == pr["phase_set"].tolist()
            # the tie census of the restatement is the C++ oracle's (every class resolved by the f64 arithmetic: the same run)
            tc = v["tie_census"]
            assert [rep["sigma_ties"], rep["class2_ties"], rep["class4_steps"], rep["equal_objective_compares"]] == tc[:4].tolist()
            assert np.array_equal(v["tie_phase"]["haplotag"], pr["haplotag"]) and abs(v["tie_phase"]["objective"] - pr["objective"]) < 1e-6
        if g == len(case["shape"]) - 1 or len(case["shape"]) == 1:
            bad = cc.census_holds(case["census"], rep)
            assert not bad, "census of %s: (wanted, got) %s" % (name, bad)


def test_the_block_recipe_meets_every_kind_of_row_and_site(orc):
    """blocks_flip / blocks_stay: one batch, two seeds of the start draws -- block 0 flips under one and stays under the other; four blocks,
    one of two nodes; trans-only pairs; eligible sites without an edge; for_phasing sites that are not eligible; every kind of row of
    cross_optimize_by_block's flip_read"""
    S = cc.BLOCK_SITES
    for name, flips in (("blocks_flip", True), ("blocks_stay", False)):
        (v,) = _visit(name)
        rep = v["report"]
        assert rep["block0_flips"] is flips
        assert [sorted(b) for b in rep["blocks"]] == [list(S["D"]), list(S["C"]), list(S["B"]), list(S["A"])]
        assert rep["trans_edges"] >= len(S["C"]) - 1 and rep["cis_edges"] >= 1
        assert rep["eligible_without_edge"] == list(S["X"]) + [S["N1"]]
        assert S["two_alt"] in rep["phasing_not_eligible"]
        assert S["hom"] in rep["not_phasing"] + rep["phasing_not_eligible"]
        assert all(n >= 1 for n in rep["flip_run_kinds"].values()), rep["flip_run_kinds"]


def test_the_cases_meet_every_limit_they_name():
    """the ledger: (limit, side) -> the case that stands there, with the form or census that proves it"""
    form = {n: _forms(n) for n in cc.NAMES}
    shape = {n: [v["shape"] for v in _visit(n)] for n in cc.NAMES}
    rep = {n: _visit(n)[-1]["report"] for n in cc.NAMES}
    ledger = {}

    def stand(limit, side, name, ok):
        assert ok, (limit, side, name, form[name], shape[name])
        ledger[(limit, side)] = name
    # windows of 64: adjacency lists (degree), blocks (nodes, DFS depth), columns (entries)
    for S in (63, 64, 65, 66, 130):
        n = "complete_%d" % S
        stand("degree / block nodes / DFS depth", S - 1, n, rep[n]["max_degree"] == S - 1 == rep[n]["dfs_depth"] and rep[n]["block_sizes"] == [S])
    stand("pair table: S W alone beyond the scratch", "beyond", "complete_130", 8 * 130 * 129 > cc.STAGE_BYTES and form["complete_130"][0]["pair_table"] == "global")
    stand("path graph", "W = 1", "path_70", shape["path_70"][0][4] == 1 and rep["path_70"]["dfs_depth"] == 69)
    w = shape["path_70_wide_row"][0]
    stand("band set by the single widest row", "W = 9", "path_70_wide_row", w[4] == 9 and form["path_70_wide_row"][0]["pair_table"] == "LDS")
    for n_ in (63, 64, 65, 128, 129):
        stand("column entries", n_, "columns_%d" % n_, rep["columns_%d" % n_]["block_column_lengths"] == [n_])
    stand("block flip", "flips", "blocks_flip", rep["blocks_flip"]["block0_flips"] is True)
    stand("block flip", "stays", "blocks_stay", rep["blocks_stay"]["block0_flips"] is False)
    # the pair table's byte rule
    a, z = shape["pair_table_lds_last"][0], shape["pair_table_global_first"][0]
    stand("pair table bytes", "last in LDS", "pair_table_lds_last", cc.pair_table_bytes(a[1], a[4], a[3]) == cc.STAGE_BYTES and form["pair_table_lds_last"][0]["pair_table"] == "LDS")
    stand("pair table bytes", "first in global memory", "pair_table_global_first", z[3] == a[3] + 1 and z[1] == a[1] and z[4] == a[4]
          and form["pair_table_global_first"][0]["pair_table"] == "global")
    # workgroup forms
    stand("racc_cap", "R = 4160", "rows_4160", shape["rows_4160"][0][0] == cc.RACC_CAP == 4160 and form["rows_4160"][0]["cross"] == "rows_balanced")
    stand("racc_cap", "R = 4161", "rows_4161", shape["rows_4161"][0][0] == 4161 and form["rows_4161"][0]["cross"] == "cols_balanced")
    stand("SCN", "S = 256", "sites_256", shape["sites_256"][0][1] == 256 and form["sites_256"][0]["scn"] == "LDS")
    stand("SCN", "S = 257", "sites_257", shape["sites_257"][0][1] == 257 and form["sites_257"][0]["scn"] == "global")
    stand("CROSS_MACC", "S = 2048", "sites_2048", shape["sites_2048"][0][1] == 2048 and form["sites_2048"][0]["cross"] == "rows_balanced")
    stand("CROSS_MACC", "S = 2049", "sites_2049", shape["sites_2049"][0][1] == 2049 and form["sites_2049"][0]["cross"] == "plain")
    a, z = shape["matrix_lds_last"][0], shape["matrix_global_first"][0]
    stand("matrix bytes", "last in LDS", "matrix_lds_last", form["matrix_lds_last"][0]["matrix"] == "LDS" and z[0] == a[0] + 1)
    stand("matrix bytes", "first in global memory", "matrix_global_first", form["matrix_global_first"][0]["matrix"] == "global" and form["matrix_global_first"][0]["state"] == "LDS")
    a, z = shape["state_lds_last"][0], shape["state_global_first"][0]
    stand("state stride", "last in LDS", "state_lds_last", a[0] + 2 * a[1] == cc.WG_LDS * 3 // 4 and form["state_lds_last"][0]["state"] == "LDS" and a[2] < cc.GRID_MIN)
    stand("state stride", "first in global memory", "state_global_first", z[0] == a[0] + 1 and form["state_global_first"][0]["state"] == "global" and z[2] < cc.GRID_MIN)
    stand("one deep region moves the launch's state", "small region beside it", "mixed_state",
          [f["state"] for f in form["mixed_state"]] == ["global", "global"] and form["scope"][0]["state"] == "LDS" and shape["mixed_state"][0] == shape["scope"][0])
    stand("matrix in LDS and not, one launch", "both", "mixed_matrix", [f["matrix"] for f in form["mixed_matrix"]] == ["LDS", "global"])
    # ties
    t = "ties_2_4_matrix_global"
    stand("COMPLETE pass, matrix in global memory", "in_lds = false", t, form[t][0]["matrix"] == "global" and form[t][0]["scope"] == "workgroup"
          and rep[t]["class2_ties"] + rep[t]["class4_steps"] >= 1)
    for n, m in (("class8_e448", 0), ("class8_e449", 1), ("class8_e447", 63)):
        stand("f64 sums of equal objectives", "E %% 64 = %d" % m, n, shape[n][0][2] % 64 == m and rep[n]["f64_sum_compares"] >= 1)
    stand("TIE_CAP", "beyond", "tie_queue_64", 4 * rep["tie_queue_64"]["max_tied_rows"] >= cc.TIE_CAP)
    stand("TIE_CAP", "within", "tie_queue_24", 0 < 8 * rep["tie_queue_24"]["max_tied_rows"] <= cc.TIE_CAP)
    # scope: grid_min = E and E + 1
    E = shape["scope"][0][2]
    stand("grid_min", "E >= grid_min", "scope", _forms("scope", E)[0]["scope"] == "all-CU")
    stand("grid_min", "E < grid_min", "scope", _forms("scope", E + 1)[0]["scope"] == "workgroup")
    sides = {}
    for (limit, side) in ledger:
        sides.setdefault(limit, []).append(side)
    two_sided = ("block flip", "pair table bytes", "racc_cap", "SCN", "CROSS_MACC", "matrix bytes", "state stride", "TIE_CAP", "grid_min")
    assert all(len(sides[k]) == 2 for k in two_sided), sides
    assert len(sides["degree / block nodes / DFS depth"]) == 5 and len(sides["column entries"]) == 5 and len(sides["f64 sums of equal objectives"]) == 3


def test_edges_move_with_the_restated_constants():
    """the edge values of the recipes come from predicted_form, and lie where the rules put them"""
    f = lambda R, S: cc.predicted_form(R, S, 2 * R, 2 * R, 1, R + 2 * S)
    assert f(cc.MATRIX_LAST, cc.MATRIX_S)["matrix"] == "LDS" and f(cc.MATRIX_LAST + 1, cc.MATRIX_S)["matrix"] == "global"
    assert cc.state_stride(cc.MATRIX_LAST + 2 * cc.MATRIX_S) + cc.matview_bytes(cc.MATRIX_LAST, cc.MATRIX_S, 2 * cc.MATRIX_LAST) + 64 <= cc.WG_LDS
    assert cc.STATE_LAST + 2 * cc.STATE_S == 49152 and 2 * (cc.STATE_LAST + 1) < cc.GRID_MIN
    assert cc.RACC_CAP == 4160 and cc.STAGE_BYTES == 33280
    assert cc.pair_table_bytes(12, 11, 8052) == cc.STAGE_BYTES

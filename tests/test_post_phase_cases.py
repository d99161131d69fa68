"""The recipes of tests/post_phase_cases.py on the CPU: for every case the two oracles -- oracle/lcr_oracle.cpp (ORC_MODE_TIE with the
tie classes liblcr resolves, what the GPU tests compare with) and oracle_np_phase.run_region -- leave the same sites and reads, and the
case's census holds: the run met the branch of the post-phase steps the case was built for.  A case that is phased by enumeration
is run a second time as a chain region (post_phase_cases.params(lowered=True)), the form tests/test_post_phase_gpu.py needs for k4_gpost."""
import numpy as np
import pytest

import post_phase_cases as pc
from longcallr_amd import _abi
from oracle import oracle_np_phase as onp2

F = _abi


def outputs(R):
    pr = R.phase_result()
    return R.cands().tobytes(), pr["haplotag"].tobytes(), pr["assignment"].tobytes(), pr["phase_set"].tobytes()


@pytest.mark.parametrize("name,lowered", pc.VARIANTS, ids=pc.VARIANT_IDS)
def test_oracles_agree_and_the_census_holds(orc, name, lowered):
    b, prm = pc.batch(name), pc.params(name, lowered)
    assert b.n_regions == 1 and int(b.len[0]) <= 3000 and b.n_reads <= 130
    R = orc.Region(b, 0, prm).pileup().candidates().fragments()
    sf, read_ps = onp2.run_region(b, 0, prm, R.cands(), frag_cls=pc.Census)
    R.set_tie_mask(orc.TIE_MASK_LIBLCR).phase(orc.MODE_TIE).post_phase()
    assert R.stats()["assert_violations"] == 0
    c, pr = R.cands(), R.phase_result()
    assert len(c) == len(sf.candidate_snps)
    assert (len(c) > prm.max_enum_snps) == (lowered or not pc.is_enumerated(name))
    for s, x in zip(sf.candidate_snps, c):
        fl = int(x["flags"])
        assert (s.pos, s.haplotype, s.genotype, s.variant_type, s.phase_set) == tuple(int(x[f]) for f in ("pos", "haplotype", "genotype", "variant_type", "phase_set")), s.pos
        assert (s.rna_editing, s.dense, s.for_phasing, s.single, s.non_selected, s.cand_somatic) == tuple(
            bool(fl & m) for m in (F.F_RNA_EDIT, F.F_DENSE, F.F_FOR_PHASING, F.F_SINGLE, F.F_NON_SELECTED, F.F_CAND_SOMATIC)), s.pos
        assert s.phase_score == pytest.approx(x["phase_score"], abs=1e-9)
    assert [f.assignment for f in sf.fragments] == pr["assignment"].tolist()
    assert [f.haplotag for f in sf.fragments] == pr["haplotag"].tolist()
    assert [read_ps.get(k, 0) for k in range(len(sf.fragments))] == pr["phase_set"].tolist()
    got = sf.report()
    print("%s%s: %s" % (name, " (chain)" if lowered else "", {k: got[k] for k in sorted(got) if got[k] not in (0, [], ())}))
    bad = pc.census_holds(pc.BY_NAME[name]["census"], got)
    assert not bad, "census of %s: (wanted, got) %s" % (name, bad)
    if len(c) > prm.max_enum_snps:
        # a chain region that gets all CUs resolves sigma ties only (orc.TIE_MASK_LIBLCR_GRID); no case depends on the other classes,
        # so the GPU tests hold every scope to the default mask and keep test_gpu_parity.check_f64_mode
        G = orc.Region(b, 0, prm).set_tie_mask(orc.TIE_MASK_LIBLCR_GRID).run_all(orc.MODE_TIE)
        assert outputs(G) == outputs(R)


def test_the_cases_meet_every_branch_they_name():
    """the ledger: each branch of the module docstring's list has a case whose census demands it"""
    want = {c["name"]: c["census"] for c in pc.CASES}
    codes = set()
    for w in want.values():
        codes |= set(w.get("edit_codes", [])) | set(w.get("lowfrac_codes", []))
    assert codes == {2, 3, 4, 5}                                       # (code 1 cannot occur: post_phase_cases' docstring)
    assert [want[n]["max_node_entries"] for n in ("ps_64", "ps_65", "ps_70", "ps_tail")] == [64, 65, 70, 70]
    assert want["ps_tail"]["rows_on_tail_only"] > 0
    assert want["ps_self_loop"]["one_node_components"] == 1 and want["ps_self_loop"]["single_node_rows"] > 0
    assert want["ps_no_edge"]["no_edge_rows"] > 0 and want["ps_no_edge_mps20"]["node_sites"] < want["ps_no_edge_mps10"]["node_sites"]
    assert {g for n in want for _, g, _ in want[n].get("genotype_calls", [])} == {1, -1}
    assert want["edit_list_rounds_mps8"]["edit_rounds"][1] >= 2 and want["lowfrac_list"]["lowfrac_rounds"] >= 2
    assert set(want["lowfrac_list"]["lowfrac_codes"]) >= {4, 5} and want["lowfrac_list"]["edit_codes"] == [4]


def test_no_edge_score_stands_between_the_two_thresholds(orc):
    """ps_no_edge's second site: its phase score is the one number the node test !(score < min_phase_score) is probed with"""
    b = pc.batch("ps_no_edge")
    c = orc.Region(b, 0, pc.params("ps_no_edge")).set_tie_mask(orc.TIE_MASK_LIBLCR).run_all(orc.MODE_TIE).cands()
    assert 10.0 < float(c["phase_score"][1]) < 20.0 and np.all(c["phase_score"][:1] > 20.0)

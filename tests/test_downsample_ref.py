"""CPU reference of down-sampled phasing (tests/downsample_ref.py): equal to oracle_np_phase with every row sampled, the sample's
properties, and a hand-derived known answer."""
import numpy as np

import downsample_ref as dsr
import helpers
from longcallr_amd import _abi
from oracle import oracle_np_phase as onp2

F = _abi


def cands_of(orc, batch, g, prm):
    """candidate records of region g as of get_candidate_snps (the candidate half is pinned separately)"""
    return orc.Region(batch, g, prm).pileup().candidates().fragments().cands()


def kat_batch():
    """one region, two het sites 100 bp apart, uniform quality: rows 0-11 alt/alt, 12-23 ref/ref (cis), 24-27 alt/ref, 28-31 ref/alt (trans)"""
    ref = "ACGT" * 60
    s1, s2 = 60, 160
    a1, a2 = "G", "C"
    assert ref[s1] == "A" and ref[s2] == "A"
    reads = []
    for k in range(32):
        x1 = k < 12 or 24 <= k < 28
        x2 = k < 12 or k >= 28
        s = list(ref[20:220])
        if x1:
            s[s1 - 20] = a1
        if x2:
            s[s2 - 20] = a2
        reads.append(dict(pos=1020, seq="".join(s), qual=30, cigar="200M", rev=k % 2, ts=1 + k % 2))
    return helpers.mk_batch(reads, [(1000, ref)]), [1000 + s1, 1000 + s2]


def kat_cands(sites):
    c = np.zeros(2, _abi.CAND_DTYPE)
    for i, (p, alt) in enumerate(zip(sites, "GC")):
        c[i]["pos"] = p; c[i]["ref_base"] = ord("A"); c[i]["allele1"] = ord("A"); c[i]["allele2"] = ord(alt)
        c[i]["af1"] = c[i]["af2"] = 0.5; c[i]["variant_type"] = 1; c[i]["genotype"] = 0
        c[i]["flags"] = F.F_HET | F.F_FOR_PHASING
    return c


def test_all_rows_sampled_equals_the_oracle(orc):
    cases = [(helpers.demo_batch(), _abi.make_params("hifi-masseq", seed=2025)),
             (helpers.two_haplotype_batch(n_snps=5, n_reads=30, seed=1)[0], _abi.make_params("hifi-masseq", seed=3)),
             (helpers.two_haplotype_batch(n_snps=6, groups=2, n_reads=24, seed=2)[0], _abi.make_params("hifi-masseq", seed=4, max_enum_snps=3))]
    for b, prm in cases:
        c0 = cands_of(orc, b, 0, prm)
        sf, ps = onp2.run_region(b, 0, prm, c0)
        for kw in (dict(depth=0), dict(rows=np.ones(len(sf.fragments), np.uint8)), dict(depth=len(sf.fragments) + 1)):
            ds, dps, app = dsr.run_region(b, 0, prm, c0, **kw)
            assert not app and dsr.summary(ds, dps) == dsr.summary(sf, ps) and ds.ctr == sf.ctr


def test_sample_rows_properties():
    for n, depth in ((64, 64), (65, 64), (257, 1), (257, 100), (5000, 1234)):
        m = dsr.sample_rows(2025, 777, n, depth)
        assert m.dtype == np.uint8 and int(m.sum()) == depth and set(m.tolist()) <= {0, 1}
        assert np.array_equal(m, dsr.sample_rows(2025, 777, n, depth))
    assert not np.array_equal(dsr.sample_rows(2025, 777, 257, 100), dsr.sample_rows(2025, 778, 257, 100))
    assert not np.array_equal(dsr.sample_rows(2025, 777, 257, 100), dsr.sample_rows(2026, 777, 257, 100))
    # a region's bytes do not depend on the batch's other regions, and regions below the depth are left alone
    one, a1 = dsr.batch_mask(2025, [500], [0, 300], 64)
    many, a3 = dsr.batch_mask(2025, [100, 500, 900], [0, 63, 363, 427], 64)
    assert a1 == [True] and a3 == [False, True, True]
    assert np.array_equal(many[63:363], one) and many[:63].all() and int(many[363:].sum()) == 64
    # nested in the depth: the rows with the smallest keys
    assert not (dsr.sample_rows(1, 0, 300, 10) & ~dsr.sample_rows(1, 0, 300, 20)).any()


def test_known_answer_trans_sample():
    """32 reads over two het sites.  On the 8 trans reads alone the two sites sit on opposite haplotypes, the trans reads are assigned 4 / 4
    and every cis read has one match and one mismatch under either haplotag: q == qn, unassigned with haplotag 0 (the last round sees
    every read).  Without the sample the 24 cis reads decide: same haplotype, cis reads 12 / 12, trans reads unassigned."""
    b, sites = kat_batch()
    prm = _abi.make_params("hifi-masseq", seed=11, read_assign_cutoff=1e-6)   # (> 0: a read with q == qn stays unassigned)
    c0 = kat_cands(sites)
    rows = np.zeros(32, np.uint8); rows[24:] = 1
    sf, ps, app = dsr.run_region(b, 0, prm, c0, rows=rows)
    assert app and len(sf.fragments) == 32
    d = [s.haplotype for s in sf.candidate_snps]
    assert d[0] * d[1] == -1
    asg = [f.assignment for f in sf.fragments]
    assert asg[:24] == [0] * 24 and [f.haplotag for f in sf.fragments[:24]] == [0] * 24
    assert sorted(asg[24:]) == [1] * 4 + [2] * 4 and len(set(asg[24:28])) == 1 and len(set(asg[28:])) == 1
    off, ps0, app0 = dsr.run_region(b, 0, prm, c0)
    assert not app0
    d = [s.haplotype for s in off.candidate_snps]
    asg = [f.assignment for f in off.fragments]
    assert d[0] * d[1] == 1 and asg[24:] == [0] * 8 and sorted(asg[:24]) == [1] * 12 + [2] * 12

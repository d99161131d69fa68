"""User-provided candidates on the GPU: lcr_import_candidates (SNPFrag::import_external_candidates, candidate.rs:530-613)
against the import restated here over the oracle's pileup planes, the phasing stages behind it against the Python
phasing oracle (oracle/oracle_np_phase.run_region), its call-order / argument contract, and pipeline.run(input_vcf=...)."""
import gzip
import os
import struct

import numpy as np
import pytest

import helpers
from longcallr_amd import _abi, synth, vcf
from longcallr_amd._lib import LcrError
from oracle import oracle_np as onp
from oracle import oracle_np_phase as onp2

pytestmark = pytest.mark.gpu
F = _abi


def expected_import(orc, batch, prm, pos0, gt, qual):
    """candidate.rs:530-613 with min_variant_qual = 0.0 over the oracle's planes: the records, region by region"""
    recs = []
    for g in range(batch.n_regions):
        s0, L, o = int(batch.start0[g]), int(batch.len[g]), int(batch.col_off[g])
        pl = orc.Region(batch, g, prm).pileup().planes()
        for p, c, q in zip(pos0.tolist(), gt.tolist(), np.asarray(qual, np.float32)):
            if not (s0 <= p < s0 + L) or q < np.float32(0.0) or c not in (1, 2, 3):
                continue
            col = p - s0
            c4 = [int(pl[k, col]) for k in range(4)]
            ref = int(batch.ref[o + col])
            (a1, c1), (a2, c2) = onp.two_major(c4, chr(ref))
            depth = sum(c4)
            with np.errstate(invalid="ignore", divide="ignore"):
                af1, af2 = np.float32(c1) / np.float32(depth), np.float32(c2) / np.float32(depth)
            vt, gtp, fl = {1: (1, 0, F.F_HET | F.F_FOR_PHASING), 2: (2, -1, F.F_HOM | F.F_FOR_PHASING), 3: (3, -1, F.F_HOM)}[c]
            recs.append(dict(pos=p, region=g, ref_base=ref, allele1=ord(a1), allele2=ord(a2), n_alt=0, cnt1=c1, cnt2=c2, depth=depth,
                             af1=af1, af2=af2, variant_type=vt, genotype=gtp, haplotype=0, flags=fl, phase_set=0, qual=float(q), gq=float(q),
                             phase_score=0.0))
    return recs


def check_records(cands, off, recs, n_regions):
    assert cands.size == len(recs)
    assert off.tolist() == np.searchsorted([r["region"] for r in recs], np.arange(n_regions + 1), side="left").tolist()
    for c, r in zip(cands, recs):
        for f, v in r.items():
            if f in ("af1", "af2"):
                a, b = np.float32(c[f]), np.float32(v)
                assert (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes(), (r["pos"], f)
            elif f in ("qual", "gq", "phase_score"):
                assert (np.isnan(c[f]) and np.isnan(v)) or float(c[f]) == v, (r["pos"], f)
            else:
                assert int(c[f]) == v, (r["pos"], f, int(c[f]), v)
        assert not c["loglik"].any() and not c["gt_prob"].any()


def check_downstream(E, batch, prm, cands0, off0):
    """fragments + phase + post-phase of the imported candidates against oracle_np_phase.run_region, region by region"""
    fm, pr = E.fragmat(), E.phase_result()
    c1, _ = E.candidates()
    for g in range(batch.n_regions):
        a, b = int(off0[g]), int(off0[g + 1])
        sf, read_ps = onp2.run_region(batch, g, prm, cands0[a:b])
        r0, r1 = int(fm["row_region_off"][g]), int(fm["row_region_off"][g + 1])
        assert len(sf.fragmat_snapshot) == r1 - r0
        for k, (read, ents, links, fp) in enumerate(sf.fragmat_snapshot):
            r = r0 + k
            assert read == fm["row_read"][r]
            e0, e1 = int(fm["row_ptr"][r]), int(fm["row_ptr"][r + 1])
            assert [e[0] for e in ents] == (fm["col"][e0:e1] - a).tolist()
            assert [(e[2] & 31) | (32 if e[3] == 1 else 0) for e in ents] == [int(v) & 63 for v in fm["val"][e0:e1]]
            assert links == fm["row_links"][r] and int(fp) == fm["row_for_phasing"][r]
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
            assert s.phase_score == pytest.approx(float(c["phase_score"]), abs=1e-4)
    tc = E.tie_census()
    assert tc["delta_unresolved"] == tc["step_unresolved"] == tc["best_unresolved"] == tc["sigma_unresolved"] == 0


def run_import(engine_cls, orc, batch, prm, pos0, gt, qual):
    E = engine_cls(0, prm)
    E.load_batch(batch).fill_data_into_freq_vec().import_external_candidates(pos0, gt, qual)
    cands, off = E.candidates()
    check_records(cands, off, expected_import(orc, batch, prm, pos0, gt, qual), batch.n_regions)
    E.get_fragments().phase()
    check_downstream(E, batch, prm, cands, off)
    E.close()
    return cands


def sites_of(recs):
    """(pos0, genotype code, qual) of candidate records: re-phasing one's own calls"""
    code = np.array([{0: 0, 1: 1, 2: 2, 3: 3}[int(v)] for v in recs["variant_type"]], np.uint8)
    return recs["pos"].astype(np.int64), code, recs["qual"].astype(np.float32)


def perturb(pos0, gt, qual, rng, lo, hi):
    """drop a few sites, add a few het sites at random columns, a code 4, a NaN and a negative quality"""
    keep = rng.random(pos0.size) > 0.2
    p, g, q = pos0[keep], gt[keep].copy(), qual[keep].copy()
    extra = rng.choice(np.arange(lo, hi), size=4, replace=False).astype(np.int64)
    extra = extra[~np.isin(extra, p)]
    p = np.concatenate([p, extra]); g = np.concatenate([g, np.ones(extra.size, np.uint8)])
    q = np.concatenate([q, np.full(extra.size, 20.0, np.float32)])
    o = np.argsort(p, kind="stable")
    p, g, q = p[o], g[o], q[o]
    if p.size >= 3:
        g[0], q[1], q[2] = 4, np.float32(np.nan), np.float32(-1.0)
    return p, g, q


def two_haplotype_sites():
    b, truth = helpers.two_haplotype_batch(n_snps=5, groups=2, n_reads=40, seed=3)
    s0, L = int(b.start0[0]), int(b.len[0])
    t = [x for grp in truth for x in grp]
    sites = {x: (1, 30.0) for x in t}
    sites[t[2]] = (1, float("nan"))               # NaN QUAL: kept
    sites[s0 + 150] = (2, 25.0)                   # 1/1 at a reference column
    sites[s0 + 250] = (3, 25.0)                   # 1/2: variant_type 3, not for phasing
    sites[s0 + 300] = (0, 25.0)                   # 0/0: no record
    sites[s0 + 310] = (4, 25.0)                   # other genotype: no record
    sites[s0 + 320] = (1, -1.0)                   # QUAL < 0: no record
    sites[s0 + 3500] = (1, 30.0)                  # between the two stretches: depth 0, af NaN
    for x in (s0 - 1, s0 + L, 10, s0 + L + 1000):  # outside every region
        sites[x] = (1, 30.0)
    ks = sorted(sites)
    return b, (np.array(ks, np.int64), np.array([sites[k][0] for k in ks], np.uint8), np.array([sites[k][1] for k in ks], np.float32))


def test_records_and_phasing_of_a_constructed_site_list(engine_cls, orc):
    b, (p, g, q) = two_haplotype_sites()
    prm = _abi.make_params("ont-cdna", max_enum_snps=6)
    c = run_import(engine_cls, orc, b, prm, p, g, q)
    assert c.size == 10 + 2 + 1 and np.isnan(c["af1"][c["depth"] == 0]).all() and (c["depth"] == 0).sum() == 1
    assert ((c["variant_type"] == 3) & ((c["flags"] & F.F_FOR_PHASING) == 0)).sum() == 1


def test_rephasing_own_calls_on_demo_bam(engine_cls, orc):
    b = helpers.demo_batch()
    prm = _abi.make_params("hifi-masseq")
    E = engine_cls(0, prm)
    E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps()
    calls, _ = E.candidates()
    E.close()
    p, g, q = sites_of(calls)
    run_import(engine_cls, orc, b, prm, p, g, q)
    rng = np.random.default_rng(5)
    run_import(engine_cls, orc, b, prm, *perturb(p, g, q, rng, int(b.start0[0]), int(b.start0[0] + b.len[0])))


@pytest.mark.parametrize("profile,seed", [("ont-cdna", 31), ("masseq", 32)])
def test_rephasing_own_calls_on_synthetic_batches(engine_cls, orc, profile, seed):
    b = synth.make_batch(profile, n_genes=3, gene_len=7000, depth=25, seed=seed)
    prm = _abi.make_params(synth.preset_for(profile), seed=seed, max_enum_snps=6)
    E = engine_cls(0, prm)
    E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps()
    calls, _ = E.candidates()
    E.close()
    p, g, q = sites_of(calls)
    rng = np.random.default_rng(seed)
    lo, hi = int(b.start0[0]), int(b.start0[-1] + b.len[-1])
    run_import(engine_cls, orc, b, prm, *perturb(p, g, q, rng, lo, hi))


def test_call_order_and_argument_contract(engine_cls):
    import torch
    b, (p, g, q) = two_haplotype_sites()
    prm = _abi.make_params("ont-cdna")
    E = engine_cls(0, prm)
    E.load_batch(b)
    with pytest.raises(LcrError, match=r"failed \(-4\)"):
        E.import_external_candidates(p, g, q)
    E.fill_data_into_freq_vec().get_candidate_snps()
    ref_c, ref_off = E.candidates()
    for bad in ((p[::-1].copy(), g[::-1].copy(), q[::-1].copy()), (np.repeat(p, 2), np.repeat(g, 2), np.repeat(q, 2)),
                (p, np.where(np.arange(g.size) == 3, 5, g).astype(np.uint8), q)):
        with pytest.raises(LcrError, match=r"failed \(-1\)"):
            E.import_external_candidates(*bad)
    # pileup -> import -> candidates gives the records of pileup -> candidates, byte for byte
    E.fill_data_into_freq_vec().import_external_candidates(p, g, q).get_candidate_snps()
    c2, off2 = E.candidates()
    assert c2.tobytes() == ref_c.tobytes() and np.array_equal(off2, ref_off)
    # import twice = import once; device-resident sites = host sites
    E.import_external_candidates(p, g, q)
    a, aoff = E.candidates()
    E.import_external_candidates(p, g, q)
    a2, aoff2 = E.candidates()
    assert a.tobytes() == a2.tobytes() and np.array_equal(aoff, aoff2) and a.size > 0
    dp, dg, dq = (torch.from_numpy(x).cuda() for x in (p, g, q))
    torch.cuda.synchronize()
    E.import_external_candidates(dp, dg, dq)
    a3, aoff3 = E.candidates()
    assert a.tobytes() == a3.tobytes() and np.array_equal(aoff, aoff3)
    with pytest.raises(LcrError, match=r"failed \(-1\)"):
        E.import_external_candidates(*(torch.from_numpy(x).cuda() for x in (p[::-1].copy(), g, q)))
    # device tensors of another dtype than int64 / uint8 / float32, or mixed with host arrays, are refused before any kernel reads them
    for bad in ((dp, dg.to(torch.int64), dq), (dp.to(torch.int32), dg, dq), (dp, dg, dq.to(torch.float64)), (dp, g, dq), (dp[:-1], dg, dq)):
        with pytest.raises(ValueError):
            E.import_external_candidates(*bad)
    # temporaries: the engine holds them until the stage has read them, while torch's allocator hands out blocks again
    E.import_external_candidates(*(torch.as_tensor(x, device="cuda") for x in (p, g, q)))
    junk = [torch.full((p.size * 4,), -7, dtype=torch.int64, device="cuda") for _ in range(4)]
    a4, aoff4 = E.candidates()
    assert a.tobytes() == a4.tobytes() and np.array_equal(aoff, aoff4) and len(junk) == 4
    E.import_external_candidates(*(torch.as_tensor(x, device="cuda") for x in (p, g, q))).get_fragments()
    assert E.candidates()[0].tobytes() == a.tobytes()
    # the stages behind it run as after get_candidate_snps
    E.import_external_candidates(p, g, q).get_fragments().phase()
    assert E.phase_result()["haplotag"].size == E.fragmat()["row_read"].size
    # no sites: no candidates
    E.import_external_candidates(p[:0], g[:0], q[:0])
    assert E.candidates()[0].size == 0
    E.close()


def _demo_fasta(tmp_path):
    from longcallr_amd import bamio
    refs, _ = bamio.read_bam(os.path.join(helpers.GOLDEN, "demo.bam"))
    b = helpers.demo_batch()
    start0, length = int(b.start0[0]), int(b.len[0])
    fa = str(tmp_path / "pseudo.fa")
    with open(fa, "wb") as f, open(fa + ".fai", "w") as fi:   # as test_gpu_parity's driver test: N everywhere but the demo window
        for name, ln in refs:
            if name not in ("chr19", "chr20"):
                continue
            seq = np.full(ln, ord("N"), np.uint8)
            if name == "chr20":
                seq[start0:start0 + length] = helpers.load_pseudo_ref()
            f.write(b">" + name.encode() + b" pseudo\n" + seq.tobytes() + b"\n")
            fi.write("%s\t%d\t0\t%d\t%d\n" % (name, ln, ln, ln + 1))
    return fa


def test_pipeline_with_input_vcf(engine_cls, tmp_path):
    from longcallr_amd import bamio, pipeline
    src = os.path.join(helpers.GOLDEN, "demo.bam")
    fa = _demo_fasta(tmp_path)
    b = helpers.demo_batch()
    prm = _abi.make_params("hifi-masseq", seed=2025)
    E = engine_cls(0, prm)
    E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps()
    p, g, q = perturb(*sites_of(E.candidates()[0]), np.random.default_rng(9), int(b.start0[0]), int(b.start0[0] + b.len[0]))
    # expected: the region's results through the engine, formatted by the writer
    E.fill_data_into_freq_vec().import_external_candidates(p, g, q).get_fragments().phase()
    want = vcf.format_records(E.candidates()[0], "chr20", prm.min_phase_score)
    fm, pr = E.fragmat(), E.phase_result()
    E.close()
    assert want.count("\n") > 5
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"]
    lines += ["chr19\t1000\t.\tA\tG\t30\tPASS\t.\tGT\t0/1", "chrUn\t5\t.\tA\tG\t30\tPASS\t.\tGT\t0/1"]
    lines += ["chr20\t%d\t.\tA\tG\t%s\tPASS\t.\tGT\t%s" % (x + 1, "." if qq != qq else repr(float(qq)), {0: "0/0", 1: "0|1", 2: "1/1", 3: "1/2", 4: "./."}[int(c)])
              for x, c, qq in zip(p, g, q)]
    text = "\n".join(lines) + "\n"
    path = str(tmp_path / "sites.vcf.gz")
    with open(path, "wb") as f:
        f.write(gzip.compress(text[:len(text) // 2].encode()) + gzip.compress(text[len(text) // 2:].encode()) + gzip.compress(b""))
    assert vcf.read_sites(path)["chr20"][0].tolist() == p.tolist()
    outs = []
    for k, (asy, devs) in enumerate([(True, [0]), (False, [0]), (True, [0, 0]), (False, [0, 0])]):
        out_vcf, out_bam = str(tmp_path / ("o%d.vcf" % k)), str(tmp_path / ("o%d.bam" % k))
        st = pipeline.run(src, fa, out_vcf, out_bam if k == 0 else None, preset="hifi-masseq", threads=4, async_phase=asy, devices=devs,
                          input_vcf=path)
        assert st["input_sites"] == p.size + 2 and st["imported_sites"] == p.size
        body = open(out_vcf).read().split("#CHROM")[1].split("\n", 1)[1]
        assert body == want
        outs.append(body)
    assert len(set(outs)) == 1
    # phased BAM: HP / PS of every fragment row as the assignment says (thread.rs:204-214, 307-361)
    refs, recs = bamio.read_bam(src)
    keep = [r for r in recs if bamio.passes_filter(r, **_abi.READ_FILTER)]
    _, out_recs = bamio.read_bam(str(tmp_path / "o0.bam"), keep_raw=True)
    by_name = {}
    for r in out_recs:
        by_name.setdefault(r["name"], r)
    n_tagged = 0
    for row, rd in enumerate(fm["row_read"]):
        r = by_name[keep[int(rd)]["name"]]
        aux = r["raw"][r["aux_off"]:]
        a, ps = int(pr["assignment"][row]), int(pr["phase_set"][row])
        assert (b"HPi" + struct.pack("<i", a) in aux) == (a in (1, 2))
        assert (b"PSI" + struct.pack("<I", ps) in aux) == (ps != 0)
        n_tagged += a in (1, 2)
    assert n_tagged > 0

"""K8 on the GPU: lcr_assign_genes against the hand-derived answers of tests/genes_cases.py and the loop-for-loop restatement of the
script (tests/genes_ref.py), refused annotations and call order, and lcr_ase_genes against the restatement's per-gene counting on the
engine's own phasing results -- synthetic ONT cDNA with interleaved, split and decoy genes, the edge regions of test_ase_gpu.py, a
one-gene-per-region annotation against lcr_ase, and demo.bam."""
import ctypes as C

import numpy as np
import pytest

import genes_cases
import genes_ref
import helpers
import test_ase_gpu as ta
import test_gpu_parity as tp
import test_junctions_gpu as tj
from longcallr_amd import _abi, annotation, synth

pytestmark = pytest.mark.gpu


def ann_struct(genes, **over):
    """LcrGeneAnnotation over a ContigGenes' arrays, fields replaced by `over` -> (struct, the arrays it points to)"""
    arr = dict(span_start0=genes.span_start0.astype(np.int64), span_end0=genes.span_end0.astype(np.int64), exon_off=genes.exon_off.astype(np.int32),
               exon_start0=genes.exon_start0.astype(np.int64), exon_end0=genes.exon_end0.astype(np.int64))
    arr.update({k: np.ascontiguousarray(v, dtype=arr[k].dtype) for k, v in over.items()})
    a = _abi.LcrGeneAnnotation()
    a.n_genes, a.n_exons = arr["span_start0"].size, arr["exon_start0"].size
    for k, v in arr.items():
        setattr(a, k, v.ctypes.data)
    return a, arr


# ---- 1. read -> gene ----------------------------------------------------------------------------------------------------------------------
def test_hand_built_instance(engine_cls):
    genes = genes_cases.contig_genes()
    b, names = genes_cases.batch()
    want_gene, want_ov = genes_cases.expected(names, genes)
    E = engine_cls(0, _abi.make_params("hifi-masseq"))
    E.load_batch(b).assign_genes(genes)          # a bound batch is enough: no pileup
    gene, ov = E.read_genes()
    for n, g, o, wg, wo in zip(names, gene.tolist(), ov.tolist(), want_gene, want_ov):
        assert (g, o) == (wg, wo), n
    ref_gene, ref_ov = genes_ref.assign(b, genes)
    assert gene.tolist() == ref_gene.tolist() and ov.tolist() == ref_ov.tolist()
    assert gene.dtype == np.int32 and ov.dtype == np.uint32
    # no gene at all is valid: every read gets -1
    none, zero = E.assign_genes(None).read_genes()
    assert (none == -1).all() and not zero.any() and none.size == b.n_reads
    # one gene; the same genes once more
    one = annotation.ContigGenes.from_exons(genes_cases.GENES[:1])
    g1, o1 = E.assign_genes(one).read_genes()
    r1 = genes_ref.assign(b, one)
    assert g1.tolist() == r1[0].tolist() and o1.tolist() == r1[1].tolist() and (g1 == 0).sum() > 10
    assert E.assign_genes(genes).read_genes()[0].tolist() == gene.tolist()
    E.close()


def random_genes(rng, lo, hi, n):
    out = []
    for k in range(n):
        x = int(rng.integers(lo - 200, hi))
        ex = []
        for _ in range(int(rng.integers(1, 8))):
            l = int(rng.choice([1, 2, 3, 30, 150, 600]))
            ex.append((x, x + l))
            x += l + int(rng.choice([0, 1, 2, 40, 300, 1500]))      # 0: abutting exons stay apart
        out.append(("R%02d" % k, ex))
    return annotation.ContigGenes.from_exons(out)


def test_random_cigars_against_the_restatement(engine_cls):
    """batches of the parity tests' random-CIGAR generator (M = X I D N S H in any order, blocks of 1 and 2 bases) until 300 reads are
    through, each against 40 random genes over its span: gene and overlap equal the restatement's exactly"""
    E = engine_cls(0, _abi.make_params("hifi-masseq"))
    rng = np.random.default_rng(8)
    n_reads, n_assigned, n_multi, seed = 0, 0, 0, 200
    while n_reads < 300:
        b = tp._random_batch(seed)
        seed += 1
        genes = random_genes(rng, int(b.start0[0]), int(b.start0[-1]) + int(b.len[-1]), 40)
        assert genes.n_genes == 40
        gene, ov = E.load_batch(b).assign_genes(genes).read_genes()
        want_gene, want_ov = genes_ref.assign(b, genes)
        assert gene.tolist() == want_gene.tolist() and ov.tolist() == want_ov.tolist()
        n_reads += b.n_reads
        n_assigned += int((gene >= 0).sum())
        n_multi += len(set(gene.tolist()))
    print("random: %d reads, %d assigned, %d distinct (batch, gene)" % (n_reads, n_assigned, n_multi))
    assert n_assigned > n_reads // 2 and n_multi > 20          # not vacuous
    E.close()


def test_refused_annotations_and_call_order(engine_cls):
    genes = genes_cases.contig_genes()
    b, names = genes_cases.batch()
    E = engine_cls(0, _abi.make_params("hifi-masseq"))
    lib = E.lib
    n, g, o, d = C.c_int32(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    get = lambda: lib.lcr_get_read_genes(E.h, C.byref(n), C.byref(g), C.byref(o), C.byref(d))
    good, keep = ann_struct(genes)
    assert lib.lcr_assign_genes(E.h, 0, C.byref(good)) == -4 and get() == -4           # LCR_E_STATE: no batch bound
    E.load_batch(b)
    assert get() == -4                                                                  # no assignment yet
    first = E.assign_genes(genes).read_genes()

    def refused(**over):
        a, keep2 = ann_struct(genes, **over)
        rc = lib.lcr_assign_genes(E.h, 0, C.byref(a))
        now = E.read_genes()                                                            # the earlier result still answers
        assert now[0].tolist() == first[0].tolist() and now[1].tolist() == first[1].tolist()
        return rc
    s, e, off, xs, xe = genes.span_start0, genes.span_end0, genes.exon_off, genes.exon_start0, genes.exon_end0
    swap = lambda a, i, j: np.concatenate([a[:i], a[[j]], a[i + 1:j], a[[i]], a[j + 1:]])
    assert refused() == 0
    assert refused(span_start0=swap(s, 3, 4), span_end0=swap(e, 3, 4)) == -1            # unsorted spans (the exons no longer match them either)
    k = genes.gene_id.index("GD1")                                                      # equal starts, the larger end first
    assert genes.gene_id[k + 1] == "GD2"
    bad = s.copy(); bad[k + 1] = s[k]
    bad2 = xs.copy(); bad2[int(off[k + 1])] = s[k]
    assert refused(span_start0=bad, exon_start0=bad2) == 0                              # (start, end) ascending: fine
    bad3, bad4 = e.copy(), xe.copy()
    bad3[k], bad4[int(off[k])] = e[k + 1] + 5, e[k + 1] + 5
    assert refused(span_start0=bad, exon_start0=bad2, span_end0=bad3, exon_end0=bad4) == -1
    ga = genes.gene_id.index("GA")
    x0 = int(off[ga])
    bad = xe.copy(); bad[x0] = xs[x0 + 1] + 1                                           # GA's first exon runs one base into the second
    assert refused(exon_end0=bad) == -1
    bad = xs.copy(); bad[x0 + 1] = xe[x0] - 1
    assert refused(exon_start0=bad) == -1
    bad = e.copy(); bad[ga] = xe[x0 + 2] - 1                                            # GA's last exon ends behind the span
    assert refused(span_end0=bad) == -1
    bad = s.copy(); bad[ga] = xs[x0] + 1                                                # ... its first one begins in front of it
    assert refused(span_start0=bad) == -1
    bad = xs.copy(); bad[x0 + 1] = xe[x0 + 1]                                           # an empty exon
    assert refused(exon_start0=bad) == -1
    bad = xs.copy(); bad[x0 + 1], bad[x0 + 2] = xs[x0 + 2], xs[x0 + 1]                  # exons out of order
    bad2 = xe.copy(); bad2[x0 + 1], bad2[x0 + 2] = xe[x0 + 2], xe[x0 + 1]
    assert refused(exon_start0=bad, exon_end0=bad2) == -1
    bad = off.copy(); bad[ga + 1] = bad[ga]                                             # a gene without an exon
    assert refused(exon_off=bad) == -1
    bad = off.copy(); bad[-1] += 1
    assert refused(exon_off=bad) == -1
    bad = off.copy(); bad[0] = 1
    assert refused(exon_off=bad) == -1
    bad = off.copy(); bad[ga + 1] = 1 << 30                                             # an offset far outside: refused, nothing read through it
    assert refused(exon_off=bad) == -1
    # equal spans are sorted (the gene_id breaks the tie on the host)
    twin = annotation.ContigGenes.from_exons([("a", [(1000, 1100)]), ("b", [(1000, 1100)])])
    assert E.assign_genes(twin).read_genes()[0].max() == 0
    first = E.assign_genes(genes).read_genes()
    # argument errors in front of any work
    assert lib.lcr_assign_genes(E.h, 0, None) == -1 and lib.lcr_assign_genes(E.h, 2, C.byref(good)) == -1
    a, _ = ann_struct(genes); a.n_genes = -1
    assert lib.lcr_assign_genes(E.h, 0, C.byref(a)) == -1
    a, _ = ann_struct(genes); a.exon_end0 = None
    assert lib.lcr_assign_genes(E.h, 0, C.byref(a)) == -1
    assert refused() == 0
    # device-resident arrays give the same result
    import torch
    dev = {k: torch.from_numpy(v).cuda() for k, v in keep.items()}
    a = _abi.LcrGeneAnnotation()
    a.n_genes, a.n_exons = good.n_genes, good.n_exons
    for kk, t in dev.items():
        setattr(a, kk, t.data_ptr())
    torch.cuda.synchronize()
    assert lib.lcr_assign_genes(E.h, _abi.LCR_MEM_DEVICE, C.byref(a)) == 0
    assert E.read_genes()[0].tolist() == first[0].tolist()
    # the stage does not move and the result outlives the stages; it dies with the binding
    ap, al = _abi.LcrAseParams(13, 11.0), _abi.LcrAseGeneList()
    assert lib.lcr_ase_genes(E.h, C.byref(ap), 0, 0, None, None, None) == -4 and lib.lcr_get_ase_genes(E.h, C.byref(al)) == -4    # before lcr_phase
    assert get() == 0 and n.value == b.n_reads and d.value
    E.load_batch(b)
    assert get() == -4
    E.close()


# ---- 2. per-gene counts -------------------------------------------------------------------------------------------------------------------
def results(E):
    fm, pr = E.fragmat(), E.phase_result()
    cands, coff = E.candidates()
    return fm, pr, cands, coff


def check_pairs(E, b, res, genes, parental=None, min_baseq=13, mps=None, assign=True):
    """read -> gene and the pair records against the restatement on the engine's own phasing results: every field of every record"""
    fm, pr, cands, coff = res
    mps = float(E.params.min_phase_score) if mps is None else float(np.float32(mps))
    if assign:
        E.assign_genes(genes)
    gene, ov = E.read_genes()
    want_gene, want_ov = genes_ref.assign(b, genes)
    assert gene.tolist() == want_gene.tolist() and ov.tolist() == want_ov.tolist()
    got, off = E.ase_genes(ta.site_arrays(parental) if parental else None, min_baseq, mps)
    want, woff = genes_ref.pairs(fm, pr["assignment"], pr["phase_set"], cands, coff, gene, parental, min_baseq, mps)
    assert got.dtype == _abi.AGENE_DTYPE and off.tolist() == woff.tolist()
    assert got.tolist() == want.tolist()
    return got, off, gene


def region_exons(b, g):
    """the union of the aligned blocks of region g's reads, 0-based half-open"""
    ex = []
    for r in range(int(b.read_begin[g]), int(b.read_begin[g + 1])):
        ex += [(s - 1, e) for s, e in genes_ref.splice_regions(int(b.pos[r]), genes_ref.cigartuples(b, r))]
    return annotation.merge_exons(ex)


def test_pairs_on_synthetic_cdna(engine_cls):
    """ont-cdna, four regions.  Region 0: two genes that take its exons in turn; regions 1 and 2: ONE gene over both; region 3: one gene,
    and in front of it a decoy whose one exon is the span of a read whose row stayed unassigned (it wins that read, and every read
    nested in it, on the tie); a gene over the last region's first exon only that nothing prefers."""
    b = synth.make_batch("ont-cdna", n_genes=4)
    E = engine_cls(0, _abi.make_params(synth.preset_for("ont-cdna")))
    E.load_batch(b).run_all()
    res = results(E)
    fm, pr, cands, coff = res
    ex = [region_exons(b, g) for g in range(4)]
    assert all(len(x) >= 2 for x in ex)
    gl = [("I0", ex[0][0::2]), ("I1", ex[0][1::2]), ("SPLIT", ex[1] + ex[2]), ("MAIN3", ex[3]), ("WEAK3", [(ex[3][0][0], ex[3][0][0] + 3)])]
    rro = fm["row_region_off"]
    una = [int(fm["row_read"][r]) for r in range(int(rro[3]), int(rro[4])) if pr["assignment"][r] == 0]
    print("rows %r, unassigned rows per region %r" % (np.diff(rro).tolist(), [int((pr["assignment"][rro[g]:rro[g + 1]] == 0).sum()) for g in range(4)]))
    if una:
        u = min(una, key=lambda r: sum(l for op, l in genes_ref.cigartuples(b, r) if op in (0, 2, 3, 7, 8)))
        pos = int(b.pos[u])
        rend = pos + sum(l for op, l in genes_ref.cigartuples(b, u) if op in (0, 2, 3, 7, 8))
        gl.append(("DECOY", [(ex[3][0][0] - 20, ex[3][0][0] - 10), (pos, rend)]))
    genes = annotation.ContigGenes.from_exons(gl)
    got, off, gene = check_pairs(E, b, res, genes)
    ids = [genes.gene_id[k] for k in got["gene"]]
    print("pairs %r" % list(zip(got["region"].tolist(), ids, got["h1"].tolist(), got["h2"].tolist(), got["n_phase_sets"].tolist())))
    assert {"I0", "I1"} <= {i for i, g in zip(ids, got["region"]) if g == 0}              # two interleaved genes in one region
    assert sorted(int(g) for i, g in zip(ids, got["region"]) if i == "SPLIT") == [1, 2]   # one gene in two regions
    assert una and got[ids.index("DECOY")].tolist()[1:10] == (0,) * 9                     # the decoy's rows are all unassigned: a pair of zeros
    assert (got["h1"] + got["h2"]).sum() > 0 and not got["n_sites"].any() and not got["pad_"].any()
    # parental sites at the candidates, as test_ase_gpu builds them
    mps = float(E.params.min_phase_score)
    par, kinds, elig = ta.parental_from_candidates(b, res, mps, 11)
    withp, _, _ = check_pairs(E, b, res, genes, par, assign=False)
    assert withp["n_sites"].sum() > 0 and sum(int(withp[f].sum()) for f in ("h1_pat", "h1_mat", "h2_pat", "h2_mat")) > 0
    for f in ("region", "gene", "phase_set", "n_phase_sets", "h1", "h2"):
        assert withp[f].tolist() == got[f].tolist()
    check_pairs(E, b, res, genes, par, min_baseq=0, assign=False)
    check_pairs(E, b, res, genes, par, min_baseq=30, mps=mps + 5, assign=False)
    # device-memory sites equal host-memory sites
    import torch
    dev = tuple(torch.from_numpy(a).cuda() for a in ta.site_arrays(par))
    assert E.ase_genes(dev)[0].tolist() == withp.tolist()
    # batch independence: region 1 alone gives SPLIT's record of region 1
    A = engine_cls(0, E.params)
    sub = synth_subbatch(b, 1)
    A.load_batch(sub).run_all()
    one, _, _ = check_pairs(A, sub, results(A), genes, par)
    k = [n for n, (i, g) in enumerate(zip(ids, withp["region"])) if i == "SPLIT" and g == 1][0]
    assert [r[1:] for r in one.tolist()] == [withp.tolist()[k][1:]]
    A.close()
    E.close()


def synth_subbatch(b, g):
    """region g of a host batch as a batch of its own"""
    r0, r1 = int(b.read_begin[g]), int(b.read_begin[g + 1])
    s0, s1 = int(b.seq_off[r0]), (int(b.seq_off[r1]) if r1 < b.n_reads else int(b.bases.size))
    c0, c1 = int(b.cig_off[r0]), (int(b.cig_off[r1]) if r1 < b.n_reads else int(b.cigar.size))
    kw = {f: getattr(b, f)[r0:r1] for f in ("pos", "seq_len", "lead_clip", "trail_clip", "flags", "n_cig")}
    return _abi.ReadBatch(seq_off=b.seq_off[r0:r1] - np.uint64(s0), cig_off=b.cig_off[r0:r1] - np.uint64(c0), bases=b.bases[s0:s1], quals=b.quals[s0:s1],
                          cigar=b.cigar[c0:c1], start0=b.start0[g:g + 1], len=b.len[g:g + 1], read_begin=[0, r1 - r0],
                          ref=b.ref[int(b.col_off[g]):int(b.col_off[g + 1])], **kw)


@pytest.fixture(scope="module")
def edge_run(engine_cls):
    regs = ta.edge_regions()
    b = tj.batch_of(regs)
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    E.load_batch(b).run_all()
    yield E, b, regs, results(E)
    E.close()


def test_pairs_on_the_edge_regions(edge_run):
    """test_ase_gpu's edge regions (no rows; rows, none assigned; two phase sets; 3 000 rows; rows of twelve entries; a dense cluster)
    under an annotation with one gene per region, two in the regions of two phase sets and of twelve entries"""
    E, b, regs, res = edge_run
    fm, pr, cands, coff = res
    s = [r[0] for r in regs]
    genes = annotation.ContigGenes.from_exons([
        ("E0", [(s[0], s[0] + 600)]), ("E1", [(s[1], s[1] + 600)]),
        ("E2a", [(s[2], s[2] + 600)]), ("E2b", [(s[2] + 1000, s[2] + 1600), (s[2] + 2600, s[2] + 2800)]),   # the reads from 0 / from 1000
        ("E3", [(s[3], s[3] + 600)]),
        ("E4a", [(s[4], s[4] + 25), (s[4] + 50, s[4] + 600)]), ("E4b", [(s[4] + 20, s[4] + 30)]),           # E4b: the two 10M reads [20, 30): 10 against E4a's 5
        ("E5", [(s[5], s[5] + 600)])])
    par = ta.everything_parental(cands, 1)
    plain, off, gene = check_pairs(E, b, res, genes)
    got, off2, _ = check_pairs(E, b, res, genes, par, assign=False)
    ids = [genes.gene_id[k] for k in got["gene"]]
    print(list(zip(ids, got.tolist())))
    assert off.tolist() == off2.tolist() and "E0" not in ids                               # no rows: no pair
    e1 = got[ids.index("E1")]
    assert e1.tolist()[1:10] == (0,) * 9                                                   # rows, none assigned: a pair of zeros
    assert {"E2a", "E2b", "E4a", "E4b"} <= set(ids) and got[ids.index("E4b")].tolist()[1:10] == (0,) * 9       # E4b: rows without an entry
    # the region's two phase sets of eight rows each go to the two genes: each pair has ITS phase set, and its sites follow it
    a2, b2 = got[ids.index("E2a")], got[ids.index("E2b")]
    assert a2["phase_set"] != b2["phase_set"] and a2["h1"] + a2["h2"] == 8 == b2["h1"] + b2["h2"] and a2["n_sites"] == 5 == b2["n_sites"]
    reg = E.ase(ta.site_arrays(par))
    assert reg["n_sites"][2] == 5 and reg["phase_set"][2] == min(a2["phase_set"], b2["phase_set"])     # lcr_ase sees one of them only
    e3, e4 = got[ids.index("E3")], got[ids.index("E4a")]
    assert e3["h1"] + e3["h2"] == 3000 and e3.tolist()[1:10] == reg.tolist()[3][1:]
    assert np.diff(fm["row_ptr"])[fm["row_region_off"][4]:fm["row_region_off"][5]].max() == 12 and e4["n_sites"] == 12
    assert e4.tolist()[1:10] == reg.tolist()[4][1:]


def test_one_gene_per_region_equals_lcr_ase(engine_cls):
    """an annotation with one single-exon gene over every region: every read goes to its region's gene, and the pair records are
    lcr_ase's records of the regions that have rows"""
    for profile in ("ont-cdna", "masseq"):
        b = synth.make_batch(profile, n_genes=4)
        E = engine_cls(0, _abi.make_params(synth.preset_for(profile)))
        E.load_batch(b).run_all()
        res = results(E)
        genes = annotation.ContigGenes.from_exons([("R%d" % g, [(int(b.start0[g]), int(b.start0[g]) + int(b.len[g]))]) for g in range(b.n_regions)])
        gene, _ = E.assign_genes(genes).read_genes()
        assert gene.tolist() == np.repeat(np.arange(b.n_regions), np.diff(b.read_begin)).tolist()
        par, _, _ = ta.parental_from_candidates(b, res, float(E.params.min_phase_score), 11)
        for sites in (None, ta.site_arrays(par)):
            pairs, off = E.ase_genes(sites)
            reg = E.ase(sites)
            rows = np.diff(res[0]["row_region_off"])
            assert off.tolist() == np.concatenate([[0], np.cumsum(rows > 0)]).tolist()
            assert pairs["gene"].tolist() == pairs["region"].tolist() == np.flatnonzero(rows > 0).tolist()
            assert [r[:10] for r in pairs.tolist()] == [r for r, n in zip(reg.tolist(), rows) if n > 0]
        assert pairs["n_sites"].sum() > 0
        E.close()


def test_demo_bam_one_gene(engine_cls):
    """demo.bam under hifi-masseq with one gene over its island: the counts DESIGN.md section 1c records for lcr_ase"""
    b = helpers.demo_batch()
    E = engine_cls(0, _abi.make_params("hifi-masseq"))
    E.load_batch(b).run_all()
    genes = annotation.ContigGenes.from_exons([("demo", [(int(b.start0[0]), int(b.start0[0]) + int(b.len[0]))])])
    got, off, gene = check_pairs(E, b, results(E), genes)
    assert (gene == 0).all() and off.tolist() == [0, 1]
    assert (int(got["h1"][0]), int(got["h2"][0])) == (514, 553)
    assert got.tolist()[0][:10] == E.ase().tolist()[0]
    E.close()


def test_timing_slots(engine_cls):
    """LCR_K_GENES / LCR_K_ASE_GENES: HIP-event time of the two calls through lcr_kernel_ms; no time before the call"""
    b = tj.batch_of([tj.allele_specific_region()])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=7), timing=True)
    ms = C.c_float()
    E.load_batch(b)
    assert E.lib.lcr_kernel_ms(E.h, _abi.K_GENES, C.byref(ms)) == -4 and E.lib.lcr_kernel_ms(E.h, _abi.NTIMERS, C.byref(ms)) == -1
    E.assign_genes(annotation.ContigGenes.from_exons([("a", [(5000, 5800)])])).run_all()
    assert E.lib.lcr_kernel_ms(E.h, _abi.K_ASE_GENES, C.byref(ms)) == -4
    E.ase_genes()
    t = [E.kernel_ms(_abi.K_GENES), E.kernel_ms(_abi.K_ASE_GENES), E.kernel_ms(_abi.K_PHASE)]
    print("ms: assign_genes %.4f, ase_genes %.4f, phase %.4f" % tuple(t))
    assert all(0.0 < x < 1000.0 for x in t)
    E.close()


def test_ase_genes_call_order(engine_cls):
    b1 = tj.batch_of([tj.allele_specific_region()])
    prm = _abi.make_params("hifi-masseq", seed=7)
    E = engine_cls(0, prm)
    lib, ap, al = E.lib, _abi.LcrAseParams(13, prm.min_phase_score), _abi.LcrAseGeneList()
    genes = annotation.ContigGenes.from_exons([("a", [(5000, 5800)]), ("b", [(6100, 6400), (6900, 7700)])])   # the reads with the middle exon: b 1100 > a 800; the others tie at 800: a
    plain = lambda p=ap: lib.lcr_ase_genes(E.h, C.byref(p), 0, 0, None, None, None)
    E.load_batch(b1).run_all()
    assert plain() == -4 and lib.lcr_get_ase_genes(E.h, C.byref(al)) == -4                 # LCR_E_STATE: no gene assignment
    E.assign_genes(genes)
    assert lib.lcr_get_ase_genes(E.h, C.byref(al)) == -4                                   # no records yet
    res = results(E)
    par = ta.everything_parental(res[2], 5)
    first, off, _ = check_pairs(E, b1, res, genes, par, assign=False)
    assert first.size == 2 and first["n_sites"].tolist() == [8, 8]                         # no restriction to the gene's coordinates
    before = (E.phase_result(), E.candidates(), E.fragmat(), E.ase(ta.site_arrays(par)))
    # bad arguments: LCR_E_ARG, and the last call's records stand
    pos, pat, mat = np.array([5, 4], np.int64), np.frombuffer(b"AA", np.uint8), np.frombuffer(b"CC", np.uint8)
    assert lib.lcr_ase_genes(E.h, None, 0, 0, None, None, None) == -1
    assert lib.lcr_ase_genes(E.h, C.byref(ap), 0, 2, pos.ctypes.data, pat.ctypes.data, mat.ctypes.data) == -1      # unsorted
    assert lib.lcr_ase_genes(E.h, C.byref(ap), 0, 2, None, None, None) == -1 and lib.lcr_ase_genes(E.h, C.byref(ap), 2, 0, None, None, None) == -1
    assert plain(_abi.LcrAseParams(31, prm.min_phase_score)) == -1
    assert lib.lcr_get_ase_genes(E.h, C.byref(al)) == 0 and (al.n_regions, al.n_pairs) == (1, 2)
    assert np.frombuffer((C.c_char * 96).from_address(al.rec), dtype=_abi.AGENE_DTYPE).tolist() == first.tolist()
    # no other table changes, before or after
    j1 = E.junctions(10, 0)[0]
    assert check_pairs(E, b1, res, genes, par, assign=False)[0].tolist() == first.tolist()
    after = (E.phase_result(), E.candidates(), E.fragmat(), E.ase(ta.site_arrays(par)))
    assert E.junctions(10, 0)[0].tobytes() == j1.tobytes()
    for x, y in zip(before, after):
        for k in (x if isinstance(x, dict) else range(len(x)) if isinstance(x, tuple) else [None]):
            assert (x if k is None else x[k]).tobytes() == (y if k is None else y[k]).tobytes(), k
    # a new gene assignment drops the pair records of the one it replaces; a refused one does not
    bad, _ = ann_struct(genes, span_start0=genes.span_start0[::-1])
    assert lib.lcr_assign_genes(E.h, 0, C.byref(bad)) == -1 and lib.lcr_get_ase_genes(E.h, C.byref(al)) == 0
    E.assign_genes(genes)
    assert lib.lcr_get_ase_genes(E.h, C.byref(al)) == -4
    assert E.ase_genes(ta.site_arrays(par))[0].tolist() == first.tolist()
    # no gene: no pair
    E.assign_genes(None)
    assert lib.lcr_get_ase_genes(E.h, C.byref(al)) == -4
    none, noff = E.ase_genes()
    assert none.size == 0 and noff.tolist() == [0, 0]
    # the asynchronous phase stage: the same records
    A = engine_cls(0, prm)
    A.set_async_phase(True)
    A.load_batch(b1).assign_genes(genes).run_all()
    assert A.ase_genes(ta.site_arrays(par))[0].tolist() == first.tolist()
    A.close()
    # the records die with the phase stage's results and with the binding
    E.assign_genes(genes)
    assert plain() == 0
    E.get_candidate_snps()
    assert lib.lcr_get_ase_genes(E.h, C.byref(al)) == -4 and plain() == -4
    E.get_fragments().phase()
    assert plain() == 0 and lib.lcr_get_ase_genes(E.h, C.byref(al)) == 0                   # the gene assignment outlived the stages
    E.load_batch(b1)
    assert lib.lcr_get_ase_genes(E.h, C.byref(al)) == -4
    E.run_all()
    assert plain() == -4                                                                   # ... and died with the binding
    E.close()

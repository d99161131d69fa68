"""K9 lcr_junctions_genes on the GPU against the plain-Python restatement of its contract (tests/asj_genes_ref.py), fed with the GPU's
own phasing results and gene map: the edges of every rule of the contract in hand-built regions (an anchor exon with five het sites
each, so that the reads phase), more than one workgroup per kernel on synthetic ONT cDNA, demo.bam under a two-gene annotation, the
call's order and re-entry on one context, its timing, and the one-gene-per-region case that equals lcr_junctions."""
import ctypes as C

import numpy as np
import pytest

import asj_genes_ref
import genes_ref
import helpers
import test_junctions_gpu as tj
from longcallr_amd import _abi, annotation, synth

pytestmark = pytest.mark.gpu

FIELDS = ("region", "gene", "motif", "start0", "len", "n_reads", "phase_set", "n_phase_sets", "h1_absent", "h1_present", "h2_absent", "h2_present")


def tuples(rec):
    return [tuple(int(rec[f][i]) for f in FIELDS) for i in range(len(rec))]


def check(E, batch, genes, min_count, min_junctions, rerun=True):
    """the engine's table against the restatement's on the engine's own phasing results and gene map: record for record, offset for offset"""
    if rerun:
        E.load_batch(batch).assign_genes(genes).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    gene, _ = E.read_genes()
    got, off = E.junctions_genes(genes, min_count, min_junctions)
    want, woff = asj_genes_ref.junctions_genes(batch, fm["row_region_off"], fm["row_read"], pr["assignment"], pr["phase_set"], gene, genes,
                                               min_count, min_junctions)
    assert got.dtype == _abi.JUNC_GENE_DTYPE and off.tolist() == woff.tolist()
    assert tuples(got) == tuples(want)
    assert not got["pad_"].any() and not got["pad2_"].any()
    return got, off, fm, pr, gene


# ---- 1. edges ------------------------------------------------------------------------------------------------------------------------------
# Params (min_count 4, min_junctions 1).  Columns are relative to the region; a gene's exons are listed the same way and moved to the
# region's start.  Every region has tj.ANCHOR's five het sites in [0, 600).
S = [10000, 20000, 30000, 40000, 50000, 60000, 62000, 64000]      # region starts


def edge_case():
    regs, genes = [], []

    def gene(name, g, exons):
        genes.append((name, [(S[g] + x, S[g] + y) for x, y in exons]))
    # R0 (a, e): two overlapping genes that share the anchor.  P goes to GA (700 against 650 bases), Q and Q2 to GB (750 against 650 / 670).
    #   (600, 100): GA 5 rows, GB 4 + 3 = 7 rows -- two records; (750, 100): GA 5, GB 3 < min_count -- a record in GA only
    r0 = ([(0, "600M100N50M100N50M")] * 5               # P: (600, 100) (750, 100)
          + [(0, "600M100N50M450N100M")] * 4            # Q: (600, 100) (750, 450)
          + [(0, "600M100N50M100N20M330N100M")] * 3     # Q2: (600, 100) (750, 100) (870, 330)
          + [(0, "600M100N50M")] * 2                    # exactly min_junctions junctions: no part
          + [(50, "10M2650N10M2N10M")])                 # a row without an entry: assignment 0
    regs.append((S[0],) + tj.build_region(S[0], 2800, tj.ANCHOR, tj.haps(r0), 31))
    gene("GA", 0, [(0, 600), (700, 750), (850, 900), (1000, 1050)])
    gene("GB", 0, [(0, 600), (700, 750), (1200, 1300)])
    # R1 (b, c, e): GC's exons [720, 740) [900, 950) leave the anchor out.
    #   N x 3: (600, 100) (750, 150), 20 + 50 bases of GC.
    #   B: blocks [700, 710) [750, 760): GC's only candidate with overlap 0 and NO shared base: raises n_reads(600, 100) to 4, in no cell.
    #   C1: blocks [739, 740) [750, 760): a one-base block inside exon [720, 740): overlap 0, a shared base: counted (absent).
    #   C2: blocks [701, 721) [750, 760): the exon met by the block's last base only: overlap 0, base 720 shared: counted (absent).
    #   X x 4: [0, 670): end in front of GC: gene -1, no part although (300, 5) and (600, 50) have four rows.
    r1 = ([(0, "600M100N50M150N50M")] * 3 + [(0, "600M100N10M40N10M")] + [(0, "600M139N1M10N10M")] + [(0, "600M101N20M29N10M")]
          + [(0, "300M5N295M50N20M")] * 4)
    regs.append((S[1],) + tj.build_region(S[1], 1000, tj.ANCHOR, tj.haps(r1), 32))
    gene("GC", 1, [(720, 740), (900, 950)])
    # R2 (d): GD's exons lie in the reads' first intron and far behind them: four rows, two kept junctions, no counted row (six more
    # reads over the anchor alone, gene -1, give the region the depth its het sites need)
    regs.append((S[2],) + tj.build_region(S[2], 2100, tj.ANCHOR, tj.haps([(0, "600M100N10M40N10M")] * 4 + [(0, "600M")] * 6), 33))
    gene("GD", 2, [(650, 660), (2000, 2010)])
    # R3 (f): GF's exons [757, 759) [790, 791) are met by one op of every read only, in its last round of sixteen:
    #   f33: 33 ops, M ops [605 + 10 i, 610 + 10 i): op 32 = [755, 760)          f65: 65 ops, M ops [603 + 6 i, 606 + 6 i): op 64 = [789, 792),
    #                                                                                 [757, 759) lies in its gap [756, 759)
    #   n15: 17 ops, op 15 an N [670, 677), op 16 the M [677, 777)                 d_n: a D directly behind an N: the D [750, 760) alone meets
    #   f16: 16 ops, op 14 the M [665, 765)                                         f32: 32 ops, op 30 the M [687, 787)
    f = ["600M" + "5N5M" * 16, "600M" + "3N3M" * 32, "600M" + "5N5M" * 7 + "7N100M", "600M150N10D5M5N5M",
         "600M" + "5N5M" * 6 + "5N100M3S", "600M" + "3N3M" * 14 + "3N100M3S"]
    regs.append((S[3],) + tj.build_region(S[3], 1000, tj.ANCHOR, tj.haps([(0, c) for c in f for _ in range(4)]), 34))
    gene("GF", 3, [(757, 759), (790, 791)])
    # R4 (h): two phase sets of eight rows no read links, in one gene: the long intron of the first group spans the second group's reads
    two = [(0, "600M2000N50M10N50M")] * 8 + [(1000, "600M10N50M10N50M")] * 8
    regs.append((S[4],) + tj.build_region(S[4], 2800, tj.ANCHOR + [1100, 1200, 1300, 1400, 1500], tj.haps(two), 35))
    gene("GH", 4, [(0, 600), (1000, 1600), (2600, 2650)])
    # R5, R6, R7 (g): one gene over three regions, the middle one without a participating row
    for g, seed in ((5, 36), (7, 37)):
        regs.append((S[g],) + tj.build_region(S[g], 1000, tj.ANCHOR, tj.haps([(0, "600M100N50M50N50M")] * 4 + [(0, "600M")] * 6), seed))
    regs.insert(6, (S[6],) + tj.build_region(S[6], 700, tj.ANCHOR, tj.haps([(0, "600M")] * 8), 38))
    genes.append(("GG", [(S[5] + 700, S[5] + 750), (S[7] + 700, S[7] + 750)]))
    return regs, annotation.ContigGenes.from_exons(genes), f


def test_edges(engine_cls):
    import re
    regs, genes, f = edge_case()
    assert [len(re.findall(r"\d+[MIDNSHP=X]", c)) for c in f] == [33, 65, 17, 6, 16, 32]
    assert re.findall(r"\d+[MIDNSHP=X]", f[2])[15] == "7N" and genes.gene_id == ["GA", "GB", "GC", "GD", "GF", "GH", "GG"]
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    b = tj.batch_of(regs)
    got, off, fm, pr, gene = check(E, b, genes, 4, 1)
    all_t = tuples(got)
    rb, rro, asg, ps = b.read_begin, fm["row_region_off"], pr["assignment"], pr["phase_set"]
    want_gene, want_ov = genes_ref.assign(b, genes)
    assert gene.tolist() == want_gene.tolist()
    rec = {}
    for t in all_t:
        rec[(t[0], genes.gene_id[t[1]], t[3] - S[t[0]], t[4])] = t
    cells = lambda t: t[8:]
    # a: the shared junction has a record in both genes with its own count; (750, 100) reaches min_count in GA only
    assert rec[(0, "GA", 600, 100)][5] == 5 and rec[(0, "GB", 600, 100)][5] == 7
    assert rec[(0, "GA", 750, 100)][5] == 5 and (0, "GB", 750, 100) not in rec and (0, "GB", 870, 330) not in rec
    assert sum(cells(rec[(0, "GA", 600, 100)])) == 5 and sum(cells(rec[(0, "GB", 600, 100)])) == 7      # not the region's twelve
    assert sorted(k[1:] for k in rec if k[0] == 0) == [("GA", 600, 100), ("GA", 750, 100), ("GB", 600, 100), ("GB", 750, 450)]
    # b, c, e: n_reads 4 = min_count with B; cells: the three N rows present, C1 and C2 absent, B nowhere; the gene -1 reads nowhere
    t = rec[(1, "GC", 600, 100)]
    assert t[5] == 4 and t[9] + t[11] == 3 and t[8] + t[10] == 2 and [k for k in rec if k[0] == 1] == [(1, "GC", 600, 100)]
    r1 = list(range(int(rb[1]), int(rb[2])))
    assert [int(want_ov[r]) for r in r1 if gene[r] == 2].count(0) == 3 and [int(gene[r]) for r in r1].count(-1) == 4
    # d: kept junctions nobody counted overlaps: the zero records
    assert [rec[(2, "GD", s, l)][5:] for s, l in ((600, 100), (710, 40))] == [(4, 0, 0, 0, 0, 0, 0)] * 2
    # f: every one of the 24 rows is counted -- through op 32 / 64 / 16 / the D / 14 / 30 of its read
    t = rec[(3, "GF", 600, 3)]
    assert t[5] == 8 and t[9] + t[11] == 8 and t[8] + t[10] == 16
    assert rec[(3, "GF", 786, 3)][5] == 4 and rec[(3, "GF", 750, 5)][5] == 4 and rec[(3, "GF", 670, 7)][5] == 4 and rec[(3, "GF", 600, 150)][5] == 4
    assert len([k for k in rec if k[0] == 3]) == 16 + 32 + 1 + 2                         # f33's, f65's, n15's (670, 7), d_n's two; f16 and f32 add none
    # g: the middle region has no record and shares its offset; GG has records in both outer regions
    assert off[7] - off[6] == 0 and {k[1] for k in rec if k[0] in (5, 7)} == {"GG"} and off[6] - off[5] == 2 == off[8] - off[7]
    # h: the long intron is overlapped by eight rows of either phase set: the smaller value wins
    r0 = int(rro[4])
    rows4 = list(range(r0, int(rro[5])))
    p1 = {int(ps[r]) for r in rows4 if int(b.pos[fm["row_read"][r]]) == S[4]}
    p2 = {int(ps[r]) for r in rows4 if int(b.pos[fm["row_read"][r]]) == S[4] + 1000}
    assert len(p1) == 1 and len(p2) == 1 and p1 != p2 and 0 not in p1 | p2
    t = rec[(4, "GH", 600, 2000)]
    assert t[7] == 2 and t[6] == min(p1 | p2) and sum(cells(t)) == 8
    # every region alone: the same records (batch independence)
    for g in (0, 3, 6):
        one, off1, _, _, _ = check(E, tj.batch_of([regs[g]]), genes, 4, 1)
        assert [(0,) + x[1:] for x in all_t[off[g]:off[g + 1]]] == tuples(one), g
    # i: no genes at all
    E.load_batch(b).assign_genes(None).run_all()
    none, off0 = E.junctions_genes(None, 4, 1)
    assert none.size == 0 and off0.tolist() == [0] * (len(regs) + 1)
    E.close()


# ---- 2. more than one workgroup per kernel; demo.bam -----------------------------------------------------------------------------------------
def region_exons(b, g):
    """the union of the aligned blocks of region g's reads, 0-based half-open"""
    ex = []
    for r in range(int(b.read_begin[g]), int(b.read_begin[g + 1])):
        ex += [(s - 1, e) for s, e in genes_ref.splice_regions(int(b.pos[r]), genes_ref.cigartuples(b, r))]
    return annotation.merge_exons(ex)


def test_synthetic_cdna(engine_cls):
    """ont-cdna, four regions of a few thousand reads: per synthetic gene its reads' block union, plus a decoy over the second half of
    region 0's exons that overlaps the gene there and takes the reads that lie in that half"""
    b = synth.make_batch("ont-cdna", n_genes=4)
    assert b.n_reads * 16 > 4 * 256
    ex = [region_exons(b, g) for g in range(4)]
    decoy = [(ex[0][0][0] - 20, ex[0][0][0] - 10)] + [(x - 5, y + 5) for x, y in ex[0][len(ex[0]) // 2:]]     # in front of S0: it wins the ties
    genes = annotation.ContigGenes.from_exons([("S%d" % g, ex[g]) for g in range(4)] + [("DECOY", decoy)])
    E = engine_cls(0, _abi.make_params("ont-cdna"))
    n = {}
    for k, (mc, mj) in enumerate(((10, 2), (2, 0))):
        got, off, fm, pr, gene = check(E, b, genes, mc, mj, rerun=k == 0)
        n[(mc, mj)] = (got.size, sorted(set(genes.gene_id[i] for i in got["gene"])))
    print("rows %d, assigned %d, reads per gene %r, kept junctions %r" % (pr["assignment"].size, int((pr["assignment"] != 0).sum()),
                                                                          np.bincount(gene + 1).tolist(), n))
    E.close()
    assert n[(2, 0)][0] >= 1 and len(n[(2, 0)][1]) >= 2


def test_demo_bam_two_genes(engine_cls):
    """demo.bam with two overlapping genes over its island: D0 over its first 60 % with an intron, D1 over its last 60 %"""
    b = helpers.demo_batch()
    s0, n = int(b.start0[0]), int(b.len[0])
    genes = annotation.ContigGenes.from_exons([("D0", [(s0, s0 + 3 * n // 10), (s0 + 4 * n // 10, s0 + 6 * n // 10)]), ("D1", [(s0 + 4 * n // 10, s0 + n)])])
    E = engine_cls(0, _abi.make_params("hifi-masseq"))
    got, off, fm, pr, gene = check(E, b, genes, 10, 2)
    low = check(E, b, genes, 2, 0, rerun=False)[0]
    print("demo.bam: reads per gene %r, kept junctions (10, 2) %d, (2, 0) %d" % (np.bincount(gene + 1).tolist(), got.size, low.size))
    E.close()
    assert low.size >= 1 and set(gene.tolist()) == {0, 1} and {0, 1} <= set(low["gene"].tolist())


# ---- 3. one gene per region equals lcr_junctions -----------------------------------------------------------------------------------------------
def test_one_gene_per_region_equals_lcr_junctions(engine_cls):
    """one single-exon gene over every region: every read goes to it and shares a base with it, and the records are lcr_junctions'"""
    regs = tj.edge_regions()
    b = tj.batch_of(regs)
    genes = annotation.ContigGenes.from_exons([("R%d" % g, [(int(b.start0[g]), int(b.start0[g]) + int(b.len[g]))]) for g in range(b.n_regions)])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    got, off, fm, pr, gene = check(E, b, genes, 4, 1)
    assert gene.tolist() == np.repeat(np.arange(b.n_regions), np.diff(b.read_begin)).tolist()
    plain, poff = E.junctions(4, 1)
    assert off.tolist() == poff.tolist() and got["gene"].tolist() == got["region"].tolist()
    for f in _abi.JUNC_DTYPE.names:
        assert got[f].tolist() == plain[f].tolist(), f
    E.close()


# ---- 4. call order, re-entry, timing -----------------------------------------------------------------------------------------------------------
def ann_struct(genes, **over):
    """lcr_gene_annotation over host arrays (kept alive by the caller through the returned list)"""
    a, keep = _abi.LcrGeneAnnotation(), []
    arr = dict(span_start0=(genes.span_start0, np.int64), span_end0=(genes.span_end0, np.int64), exon_off=(genes.exon_off, np.int32),
               exon_start0=(genes.exon_start0, np.int64), exon_end0=(genes.exon_end0, np.int64))
    for f, (v, dt) in arr.items():
        keep.append(np.ascontiguousarray(over.get(f, v), dtype=dt))
        setattr(a, f, keep[-1].ctypes.data)
    a.n_genes, a.n_exons = int(keep[0].size), int(keep[3].size)
    return a, keep


def test_call_order_and_reentry(engine_cls):
    regs, genes, _ = edge_case()
    b1, b2 = tj.batch_of(regs[:2]), tj.batch_of([tj.allele_specific_region()])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    lib, jp, jl = E.lib, _abi.LcrJunctionParams(4, 1), _abi.LcrJunctionGeneList()
    a, keep = ann_struct(genes)
    call = lambda ann=a, p=jp: lib.lcr_junctions_genes(E.h, C.byref(p), _abi.LCR_MEM_HOST, C.byref(ann))
    E.load_batch(b1).assign_genes(genes).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
    assert call() == -4 and lib.lcr_get_junctions_genes(E.h, C.byref(jl)) == -4               # before lcr_phase: LCR_E_STATE
    E.load_batch(b1).run_all()
    assert call() == -4                                                                        # the binding dropped the assignment
    E.assign_genes(genes)
    assert lib.lcr_get_junctions_genes(E.h, C.byref(jl)) == -4                                 # no table yet
    assert lib.lcr_junctions_genes(E.h, None, _abi.LCR_MEM_HOST, C.byref(a)) == -1             # LCR_E_ARG
    assert lib.lcr_junctions_genes(E.h, C.byref(jp), _abi.LCR_MEM_HOST, None) == -1 and lib.lcr_junctions_genes(E.h, C.byref(jp), 7, C.byref(a)) == -1
    j_before = E.junctions(4, 1)
    before = (E.phase_result(), E.candidates(), E.read_genes())
    t1 = check(E, b1, genes, 4, 1, rerun=False)[0]
    assert t1.size > 0
    # refused calls leave the table as it is: another number of genes; unsorted spans
    fewer = annotation.ContigGenes.from_exons([(i, [(int(genes.exon_start0[x]), int(genes.exon_end0[x])) for x in range(genes.exon_off[k], genes.exon_off[k + 1])])
                                               for k, i in enumerate(genes.gene_id[:-1])])
    a2, keep2 = ann_struct(fewer)
    assert call(a2) == -1 and "number of genes" in lib.lcr_last_error(E.h).decode()
    swapped = genes.span_start0.copy()
    swapped[[0, 2]] = swapped[[2, 0]]
    a3, keep3 = ann_struct(genes, span_start0=swapped)
    assert call(a3) == -1 and "sorted" in lib.lcr_last_error(E.h).decode()
    assert lib.lcr_get_junctions_genes(E.h, C.byref(jl)) == 0 and jl.n_junctions == t1.size
    assert helpers_view(jl).tobytes() == t1.tobytes()
    # other parameters; lcr_junctions before and after gives its unchanged table
    t2 = check(E, b1, genes, 5, 1, rerun=False)[0]
    t3 = check(E, b1, genes, 3, 2, rerun=False)[0]
    assert (t1.size, t2.size, t3.size) == (5, 3, 3)        # (750, 450) and R1's (600, 100) have four rows; only Q2's rows have three junctions
    j_after = E.junctions(4, 1)
    assert j_before[0].tobytes() == j_after[0].tobytes() and j_before[1].tolist() == j_after[1].tolist() and j_before[0].size > 0
    assert check(E, b1, genes, 4, 1, rerun=False)[0].tobytes() == t1.tobytes()
    after = (E.phase_result(), E.candidates(), E.read_genes())
    for k in before[0]:
        assert before[0][k].tobytes() == after[0][k].tobytes(), k
    assert before[1][0].tobytes() == after[1][0].tobytes() and before[2][0].tolist() == after[2][0].tolist()
    # the asynchronous phase stage: the same table
    A = engine_cls(0, E.params)
    A.set_async_phase(True)
    A.load_batch(b1).assign_genes(genes).run_all()
    assert A.junctions_genes(genes, 4, 1)[0].tobytes() == t1.tobytes()
    A.close()
    # a new lcr_assign_genes kills the records; so does rebinding; so does a new candidate stage
    E.assign_genes(genes)
    assert lib.lcr_get_junctions_genes(E.h, C.byref(jl)) == -4
    assert call() == 0 and lib.lcr_get_junctions_genes(E.h, C.byref(jl)) == 0
    E.load_batch(b2)
    assert lib.lcr_get_junctions_genes(E.h, C.byref(jl)) == -4
    one = annotation.ContigGenes.from_exons([("a", [(5000, 5800), (6100, 6400), (6900, 7700)])])
    t4 = check(E, b2, one, 10, 0)[0]
    assert [(int(r["start0"]), int(r["len"]), int(r["n_reads"])) for r in t4] == [(5800, 300, 20), (5800, 1100, 20), (6400, 500, 20)]
    E.get_candidate_snps()
    assert lib.lcr_get_junctions_genes(E.h, C.byref(jl)) == -4
    E.close()


def helpers_view(jl):
    buf = (C.c_char * (_abi.JUNC_GENE_DTYPE.itemsize * jl.n_junctions)).from_address(jl.junc)
    return np.frombuffer(buf, dtype=_abi.JUNC_GENE_DTYPE, count=jl.n_junctions).copy()


def test_kernel_ms(engine_cls):
    regs, genes, _ = edge_case()
    b = tj.batch_of(regs[:1])
    for timing in (False, True):
        E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5), timing=timing)
        E.load_batch(b).assign_genes(genes).run_all()
        got, _ = E.junctions_genes(genes, 4, 1)
        assert got.size > 0
        ms = E.last_junctions_genes_ms
        print("timing %r: lcr_junctions_genes %.4f ms" % (timing, ms))
        assert (0.0 < ms < 1000.0) if timing else ms == -1.0
        ms_k = C.c_float()
        assert E.lib.lcr_kernel_ms(E.h, _abi.NTIMERS, C.byref(ms_k)) == -1          # no new slot
        E.close()

"""K10 lcr_asj_genes on the GPU against the plain-Python restatement of its contract (tests/asj_modes_ref.py), fed with the GPU's own
phasing results, candidates and gene map: flags 0 against lcr_junctions_genes byte for byte, the rules of a read's blocks, the carry
across rounds of sixteen ops, a retained intron, the DNA filter on two unlinked phase sets, the coverage count, all three flags on
synthetic ONT cDNA and demo.bam, the call's order and re-entry on one context, and both calls' empty exits between full calls.  Hand-built regions as in test_asj_genes_gpu (an
anchor exon [0, 600) with five het sites, parameters (4, 1))."""
import ctypes as C
import re

import numpy as np
import pytest

import asj_modes_ref
import asj_ref
import helpers
import test_asj_genes_gpu as tg
import test_junctions_gpu as tj
from longcallr_amd import _abi, annotation, synth

pytestmark = pytest.mark.gpu

XFIELDS = ("region", "gene", "start0", "len", "n_reads")


def xtuples(rec):
    return [tuple(int(rec[f][i]) for f in XFIELDS) for i in range(len(rec))]


def check(E, batch, genes, min_count, min_junctions, exons=False, dna=None, coverage=False, mps=None, rerun=True):
    """the engine's tables against the restatement's on the engine's own results: record for record, offset for offset"""
    if rerun:
        E.load_batch(batch).assign_genes(genes).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    gene, _ = E.read_genes()
    cands, coff = E.candidates()
    got = E.asj_genes(genes, min_count, min_junctions, exons=exons, dna_pos0=dna, coverage=coverage, min_phase_score=mps)
    want = asj_modes_ref.asj_genes(batch, fm["row_region_off"], fm["row_read"], pr["assignment"], pr["phase_set"], gene, genes, cands, coff,
                                   min_count, min_junctions, exons, dna, coverage, float(E.params.min_phase_score) if mps is None else mps)
    assert got["junc"].dtype == _abi.JUNC_GENE_DTYPE and got["exon"].dtype == _abi.EXON_GENE_DTYPE
    assert got["junc_region_off"].tolist() == want["junc_region_off"].tolist()
    assert tg.tuples(got["junc"]) == tg.tuples(want["junc"])
    assert not got["junc"]["pad_"].any() and not got["junc"]["pad2_"].any()
    assert got["exon_region_off"].tolist() == want["exon_region_off"].tolist()
    assert xtuples(got["exon"]) == xtuples(want["exon"])
    if coverage:
        assert got["gene_reads"].dtype == np.int32 and got["gene_reads"].tolist() == want["gene_reads"].tolist()
    else:
        assert got["gene_reads"] is None
    return got, dict(fm=fm, pr=pr, gene=gene, cands=cands, coff=coff)


def hifi(engine_cls, **kw):
    return engine_cls(0, _abi.make_params("hifi-masseq", seed=5), **kw)


def n_ops(cigar):
    return len(re.findall(r"\d+[MIDNSHP=X]", cigar))


# ---- 1. flags 0 ----------------------------------------------------------------------------------------------------------------------------
def test_flags_zero_equals_junctions_genes(engine_cls):
    regs, genes, _ = tg.edge_case()
    b = tj.batch_of(regs)
    E = hifi(engine_cls)
    got, _ = check(E, b, genes, 4, 1)
    junc, off = E.junctions_genes(genes, 4, 1)
    assert junc.size > 0 and got["junc"].tobytes() == junc.tobytes() and got["junc_region_off"].tobytes() == off.tobytes()
    assert got["exon"].size == 0 and got["exon_region_off"].tolist() == [0] * (len(regs) + 1) and got["gene_reads"] is None
    E.close()


# ---- 2. blocks -----------------------------------------------------------------------------------------------------------------------------
S0 = 70000
BLOCK_READS = [
    ("ins_del", "600M100N20M5I20M10D10M100N50M", 4),      # interior [700, 760) with an I and a D inside
    ("d_behind_n", "600M110N10D40M100N50M", 4),           # interior [710, 760) begins with a D
    ("zero_n", "600M120N20M0N20M100N50M", 4),             # a zero-length N ends nothing: interior [720, 760)
    ("two_n", "600M5N5N50M10N50M", 4),                    # the block the second N closes is empty: interior [610, 660) alone
    ("n_first", "5N595M125N30M100N50M", 4),               # blocks [5, 600) [725, 755) [855, 905): the first one is never counted
    ("two_blocks", "600M100N50N50M", 4),                  # two blocks: no interior one
    ("last_same", "600M50N20M55N30M", 3),                 # interior [650, 670) with min_count - 1 rows; its LAST block is n_first's interior [725, 755)
]


def block_region():
    reads = [(0, c) for _, c, n in BLOCK_READS for _ in range(n)]
    reg = (S0,) + tj.build_region(S0, 1200, tj.ANCHOR, tj.haps(reads), 41)
    genes = annotation.ContigGenes.from_exons([("GX", [(S0, S0 + 600), (S0 + 700, S0 + 1000)])])
    return reg, genes


def test_blocks(engine_cls):
    reg, genes = block_region()
    E = hifi(engine_cls)
    got, res = check(E, tj.batch_of([reg]), genes, 4, 1, exons=True)
    assert (res["pr"]["assignment"] != 0).all() and (res["gene"] == 0).all()
    ex = {(s - S0, l): n for _, _, s, l, n in xtuples(got["exon"])}
    assert ex == {(700, 60): 4, (710, 50): 4, (720, 40): 4, (610, 50): 4, (725, 30): 4}     # (650, 20) has three rows; (725, 30) is not 7
    low, _ = check(E, tj.batch_of([reg]), genes, 3, 1, exons=True, rerun=False)
    assert {(s - S0, l): n for _, _, s, l, n in xtuples(low["exon"])}[(650, 20)] == 3
    # one block kept in two genes of a region with different counts: edge_case R0, P's / Q's / Q2's [700, 750)
    regs, genes2, _ = tg.edge_case()
    got2, _ = check(E, tj.batch_of(regs[:1]), genes2, 4, 1, exons=True)
    both = [(genes2.gene_id[k], n) for _, k, s, l, n in xtuples(got2["exon"]) if (s - tg.S[0], l) == (700, 50)]
    assert both == [("GA", 5), ("GB", 7)]
    E.close()


# ---- 3. rounds of sixteen --------------------------------------------------------------------------------------------------------------------
ROUND_READS = [
    "600M" + "5N5M" * 7 + "2I10M5N5M",              # 19 ops: the block of ops 14 | 15 | 16 spans the rounds, closed in lane 1
    "600M" + "5N5M" * 7 + "2D5N5M5N5M",             # 20 ops: op 16, lane 0 of the second round, closes the block of ops 14 - 15
    "600M" + "5N5M" * 7 + "7N50M5N5M",              # 19 ops: op 15 an N in lane 15: the next block's start is the carry
    "600M5N" + "2M1I" * 24 + "5N5M",                # 52 ops: the block of ops 2 .. 49 spans the second and third round whole
    "600M" + "5N5M" * 8,                            # 17 ops
    "600M" + "5N5M" * 16,                           # 33 ops
    "600M" + "3N3M" * 32,                           # 65 ops
]


def test_rounds_of_sixteen(engine_cls):
    assert [n_ops(c) for c in ROUND_READS] == [19, 20, 19, 52, 17, 33, 65]
    assert re.findall(r"\d+[MIDNSHP=X]", ROUND_READS[1])[16] == "5N" and re.findall(r"\d+[MIDNSHP=X]", ROUND_READS[2])[15] == "7N"
    reg = (S0,) + tj.build_region(S0, 1000, tj.ANCHOR, tj.haps([(0, c) for c in ROUND_READS for _ in range(4)]), 42)
    genes = annotation.ContigGenes.from_exons([("GX", [(S0, S0 + 1000)])])
    E = hifi(engine_cls)
    got, res = check(E, tj.batch_of([reg]), genes, 4, 1, exons=True)
    ex = {(s - S0, l): n for _, _, s, l, n in xtuples(got["exon"])}
    assert ex[(665, 15)] == 4 and ex[(665, 7)] == 4 and ex[(677, 50)] == 4 and ex[(605, 48)] == 4
    assert ex[(605, 5)] == 4 * 5 and ex[(603, 3)] == 4 and (789, 3) not in ex      # the 65-op read's last block is never closed
    E.close()


# ---- 4. retained intron ------------------------------------------------------------------------------------------------------------------------
def test_retained_intron(engine_cls):
    reads = [(0, "600M50N50M50N50M")] * 4 + [(0, "600M100N50M100N50M")] * 4      # junction (700, 50) | interior block [700, 750)
    reg = (S0,) + tj.build_region(S0, 1000, tj.ANCHOR, tj.haps(reads), 43)
    genes = annotation.ContigGenes.from_exons([("GX", [(S0, S0 + 1000)])])
    E = hifi(engine_cls)
    got, _ = check(E, tj.batch_of([reg]), genes, 4, 1, exons=True)
    assert [(int(r["n_reads"])) for r in got["junc"] if (int(r["start0"]), int(r["len"])) == (S0 + 700, 50)] == [4]
    assert [n for _, _, s, l, n in xtuples(got["exon"]) if (s, l) == (S0 + 700, 50)] == [4]
    E.close()


# ---- 5. DNA filter -----------------------------------------------------------------------------------------------------------------------------
def test_dna_filter(engine_cls):
    regs, genes, _ = tg.edge_case()
    b = tj.batch_of(regs[4:5])
    s4 = tg.S[4]
    E = hifi(engine_cls)
    plain, res = check(E, b, genes, 4, 1)
    key = lambda rec: [(int(r["start0"]) - s4, int(r["len"])) for r in rec]
    i_long = key(plain["junc"]).index((600, 2000))
    assert int(plain["junc"]["n_phase_sets"][i_long]) == 2
    ps1 = {int(p) for p, r in zip(res["pr"]["phase_set"], res["fm"]["row_read"]) if int(b.pos[r]) == s4}
    assert len(ps1) == 1 and 0 not in ps1
    # a het site of the first group only: its eight rows alone
    one, _ = check(E, b, genes, 4, 1, dna=[s4 + 100], rerun=False)
    r = one["junc"][i_long]
    assert key(one["junc"]) == key(plain["junc"]) and one["junc"]["n_reads"].tolist() == plain["junc"]["n_reads"].tolist()
    assert int(r["n_phase_sets"]) == 1 and int(r["phase_set"]) in ps1 and int(r["n_reads"]) == 8
    assert int(r["h1_absent"]) + int(r["h1_present"]) + int(r["h2_absent"]) + int(r["h2_present"]) == 8
    # both groups: flags 0's records
    both, _ = check(E, b, genes, 4, 1, dna=[s4 + 100, s4 + 1100], rerun=False)
    assert both["junc"].tobytes() == plain["junc"].tobytes()
    # no site, a column that is no candidate, a score above every candidate's: zero records with their n_reads
    for kw in (dict(dna=[]), dict(dna=[s4 + 150]), dict(dna=[s4 + 100, s4 + 1100], mps=1e30)):
        zero, _ = check(E, b, genes, 4, 1, rerun=False, **kw)
        assert key(zero["junc"]) == key(plain["junc"]) and zero["junc"]["n_reads"].tolist() == plain["junc"]["n_reads"].tolist()
        for f in ("phase_set", "n_phase_sets", "h1_absent", "h1_present", "h2_absent", "h2_present"):
            assert not zero["junc"][f].any(), (kw, f)
    # refused lists: the last result stays readable and unchanged
    last, _ = check(E, b, genes, 4, 1, exons=True, dna=[s4 + 100], coverage=True, rerun=False)
    a, keep = tg.ann_struct(genes)
    for bad in ([s4 + 1100, s4 + 100], [s4 + 100, s4 + 100]):
        arr = np.array(bad, dtype=np.int64)
        p = _abi.LcrAsjParams(4, 1, _abi.LCR_ASJ_DNA_FILTER, 0.0, 2, 0, arr.ctypes.data)
        assert E.lib.lcr_asj_genes(E.h, C.byref(p), _abi.LCR_MEM_HOST, C.byref(a)) == -1 and b"dna_pos0" in E.lib.lcr_last_error(E.h)
        o = _abi.LcrAsjGeneList()
        assert E.lib.lcr_get_asj_genes(E.h, C.byref(o)) == 0 and o.n_junctions == last["junc"].size and o.n_exons == last["exon"].size
        buf = (C.c_char * (56 * o.n_junctions)).from_address(o.junc)
        assert bytes(buf) == last["junc"].tobytes()
    for p in (_abi.LcrAsjParams(4, 1, 8, 0.0, 0, 0, None), _abi.LcrAsjParams(4, 1, _abi.LCR_ASJ_DNA_FILTER, 0.0, -1, 0, None)):
        assert E.lib.lcr_asj_genes(E.h, C.byref(p), _abi.LCR_MEM_HOST, C.byref(a)) == -1
    E.close()


# ---- 6. coverage -------------------------------------------------------------------------------------------------------------------------------
def numpy_coverage(b, gene, n_genes, min_junctions):
    nj = np.array([len(asj_ref.read_junctions(b, i)[0]) for i in range(b.n_reads)])
    return np.bincount(gene[(gene >= 0) & (nj > min_junctions)], minlength=n_genes).tolist()


def test_coverage(engine_cls):
    reads = ([(0, "600M100N50M100N50M")] * 6           # rows with two junctions
             + [(0, "600M100N50M")] * 2                # exactly min_junctions junctions: not counted
             + [(50, "10M1000N10M2N10M")]              # a row without an entry: assignment 0, counted
             + [(700, "50M5N50M5N50M")]                # behind the last candidate: no row, counted
             + [(2000, "50M5N50M5N50M")])              # no row and no gene
    reg = (S0,) + tj.build_region(S0, 2800, tj.ANCHOR, tj.haps(reads), 44)
    genes = annotation.ContigGenes.from_exons([("GX", [(S0, S0 + 600), (S0 + 700, S0 + 1500)]), ("GZ", [(S0 + 2500, S0 + 2600)])])
    b = tj.batch_of([reg])
    E = hifi(engine_cls)
    got, res = check(E, b, genes, 4, 1, coverage=True)
    assert res["fm"]["row_read"].size == 9 and (res["pr"]["assignment"] == 0).sum() == 1 and res["gene"].tolist().count(-1) == 1
    assert got["gene_reads"].tolist() == [8, 0] == numpy_coverage(b, res["gene"], 2, 1)
    assert check(E, b, genes, 4, 2, coverage=True, rerun=False)[0]["gene_reads"].tolist() == [0, 0]
    regs, genes2, _ = tg.edge_case()
    b2 = tj.batch_of(regs)
    got2, res2 = check(E, b2, genes2, 4, 1, coverage=True)
    assert got2["gene_reads"].tolist() == numpy_coverage(b2, res2["gene"], len(genes2.gene_id), 1) and sum(got2["gene_reads"]) > 0
    E.close()


# ---- 7. all three flags; more than one workgroup per kernel; demo.bam ---------------------------------------------------------------------------
def het_sites(res, mps):
    import ase_ref
    c = res["cands"]
    return sorted({int(c["pos"][i]) for i in range(len(c)) if int(c["phase_set"][i]) and ase_ref.pass_phased_het(c[i:i + 1], mps)})


def test_all_flags_synthetic_cdna(engine_cls):
    b = synth.make_batch("ont-cdna", n_genes=4)
    ex = [tg.region_exons(b, g) for g in range(4)]
    decoy = [(ex[0][0][0] - 20, ex[0][0][0] - 10)] + [(x - 5, y + 5) for x, y in ex[0][len(ex[0]) // 2:]]
    genes = annotation.ContigGenes.from_exons([("S%d" % g, ex[g]) for g in range(4)] + [("DECOY", decoy)])
    E = engine_cls(0, _abi.make_params("ont-cdna"))
    _, res = check(E, b, genes, 10, 2)
    sites = het_sites(res, float(E.params.min_phase_score))
    got, _ = check(E, b, genes, 10, 2, exons=True, dna=sites[::2], coverage=True, rerun=False)
    low, _ = check(E, b, genes, 2, 0, exons=True, dna=sites[::2], coverage=True, rerun=False)
    print("ont-cdna: reads %d, DNA sites %d of %d, exons (10, 2) %d, (2, 0) %d, coverage %r" % (
        b.n_reads, len(sites[::2]), len(sites), got["exon"].size, low["exon"].size, got["gene_reads"].tolist()))
    assert b.n_reads * 16 > 4 * 256 and low["exon"].size >= 1 and sum(low["gene_reads"]) > 0
    E.close()


def test_all_flags_demo_bam(engine_cls):
    b = helpers.demo_batch()
    s0, n = int(b.start0[0]), int(b.len[0])
    genes = annotation.ContigGenes.from_exons([("D0", [(s0, s0 + 3 * n // 10), (s0 + 4 * n // 10, s0 + 6 * n // 10)]), ("D1", [(s0 + 4 * n // 10, s0 + n)])])
    E = engine_cls(0, _abi.make_params("hifi-masseq"))
    _, res = check(E, b, genes, 2, 0)
    sites = het_sites(res, float(E.params.min_phase_score))
    got, _ = check(E, b, genes, 2, 0, exons=True, dna=sites[::2], coverage=True, rerun=False)
    print("demo.bam: reads %d, DNA sites %d of %d, junctions %d, exons %d, coverage %r" % (
        b.n_reads, len(sites[::2]), len(sites), got["junc"].size, got["exon"].size, got["gene_reads"].tolist()))
    assert sum(got["gene_reads"]) > 0
    E.close()


# ---- 8. order and re-entry ------------------------------------------------------------------------------------------------------------------------
def test_call_order_and_reentry(engine_cls):
    regs, genes, _ = tg.edge_case()
    b1 = tj.batch_of(regs[:2])
    E = hifi(engine_cls)
    lib, ol = E.lib, _abi.LcrAsjGeneList()
    a, keep = tg.ann_struct(genes)
    p = _abi.LcrAsjParams(4, 1, _abi.LCR_ASJ_EXONS | _abi.LCR_ASJ_COVERAGE, 0.0, 0, 0, None)
    call = lambda: lib.lcr_asj_genes(E.h, C.byref(p), _abi.LCR_MEM_HOST, C.byref(a))
    E.load_batch(b1).assign_genes(genes).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
    assert call() == -4 and lib.lcr_get_asj_genes(E.h, C.byref(ol)) == -4                      # before lcr_phase: LCR_E_STATE
    E.load_batch(b1).run_all()
    assert call() == -4                                                                       # before lcr_assign_genes
    E.assign_genes(genes)
    assert lib.lcr_get_asj_genes(E.h, C.byref(ol)) == -4                                      # no table yet
    j_before, jg_before = E.junctions(4, 1), E.junctions_genes(genes, 4, 1)
    full, _ = check(E, b1, genes, 4, 1, exons=True, dna=[tg.S[0] + 100], coverage=True, rerun=False)
    assert full["exon"].size > 0
    # repeated calls with other flags; two runs give identical bytes
    for kw in (dict(), dict(exons=True), dict(coverage=True), dict(dna=[tg.S[0] + 100]), dict(exons=True, dna=[tg.S[0] + 100], coverage=True)):
        x, _ = check(E, b1, genes, 4, 1, rerun=False, **kw)
    assert x["junc"].tobytes() == full["junc"].tobytes() and x["exon"].tobytes() == full["exon"].tobytes()
    assert x["gene_reads"].tobytes() == full["gene_reads"].tobytes()
    # lcr_junctions_genes' getter still answers with ITS table; both calls and lcr_junctions give what they gave before
    jl = _abi.LcrJunctionGeneList()
    assert lib.lcr_get_junctions_genes(E.h, C.byref(jl)) == 0 and tg.helpers_view(jl).tobytes() == jg_before[0].tobytes()
    j_after, jg_after = E.junctions(4, 1), E.junctions_genes(genes, 4, 1)
    assert j_before[0].tobytes() == j_after[0].tobytes() and jg_before[0].tobytes() == jg_after[0].tobytes() and jg_before[0].size > 0
    assert lib.lcr_get_asj_genes(E.h, C.byref(ol)) == 0 and ol.n_exons == full["exon"].size   # ... and K10's table outlives K9's call
    # batch independence: a region alone gives the same records
    for g in (0, 1):
        one, _ = check(E, tj.batch_of([regs[g]]), genes, 4, 1, exons=True, coverage=True)
        lo, hi = full["exon_region_off"][g], full["exon_region_off"][g + 1]
        assert [(0,) + t[1:] for t in xtuples(full["exon"])[lo:hi]] == xtuples(one["exon"]), g
    # dropped at the next lcr_assign_genes and at the next bind
    E.load_batch(b1).assign_genes(genes).run_all()
    assert call() == 0 and lib.lcr_get_asj_genes(E.h, C.byref(ol)) == 0
    E.assign_genes(genes)
    assert lib.lcr_get_asj_genes(E.h, C.byref(ol)) == -4
    assert call() == 0 and lib.lcr_get_asj_genes(E.h, C.byref(ol)) == 0
    E.load_batch(b1)
    assert lib.lcr_get_asj_genes(E.h, C.byref(ol)) == -4
    E.close()


def test_empty_exits_between_full_calls(engine_cls):
    """both calls leave through their empty exits -- no participating row (min_junctions 1000: in front of the row records), no kept slot
    (min_count 1000: behind the second wait) -- between two full calls on one context, every call against the restatements"""
    regs, genes, _ = tg.edge_case()
    b = tj.batch_of(regs[:2])
    E = hifi(engine_cls)
    zeros = [0] * (len(regs[:2]) + 1)
    # lcr_junctions_genes
    k1 = tg.check(E, b, genes, 4, 1)
    assert k1[0].size > 0
    for mc, mj in ((4, 1000), (1000, 1)):
        got, off = tg.check(E, b, genes, mc, mj, rerun=False)[:2]
        jl = _abi.LcrJunctionGeneList()
        assert E.lib.lcr_get_junctions_genes(E.h, C.byref(jl)) == 0 and jl.n_junctions == 0 and jl.n_regions == 2
        assert got.size == 0 and off.tolist() == zeros
    k4 = tg.check(E, b, genes, 4, 1, rerun=False)
    assert k4[0].tobytes() == k1[0].tobytes() and k4[1].tobytes() == k1[1].tobytes()
    # lcr_asj_genes with the exon table and the coverage
    kw = dict(exons=True, coverage=True, rerun=False)
    a1, res = check(E, b, genes, 4, 1, **kw)
    assert a1["junc"].size > 0 and a1["exon"].size > 0
    want_cov = numpy_coverage(b, res["gene"], len(genes.gene_id), 1)
    for mc, mj, cov in ((4, 1000, [0] * len(genes.gene_id)), (1000, 1, want_cov)):
        got, _ = check(E, b, genes, mc, mj, **kw)
        ol = _abi.LcrAsjGeneList()
        assert E.lib.lcr_get_asj_genes(E.h, C.byref(ol)) == 0 and ol.n_junctions == 0 and ol.n_exons == 0 and ol.n_regions == 2
        assert got["junc"].size == 0 and got["exon"].size == 0
        assert got["junc_region_off"].tolist() == zeros and got["exon_region_off"].tolist() == zeros
        assert got["gene_reads"].tolist() == cov
    assert sum(want_cov) > 0
    a4, _ = check(E, b, genes, 4, 1, **kw)
    for f in ("junc", "junc_region_off", "exon", "exon_region_off", "gene_reads"):
        assert a4[f].tobytes() == a1[f].tobytes(), f
    # lcr_junctions_genes' table from before the four lcr_asj_genes calls
    jl = _abi.LcrJunctionGeneList()
    assert E.lib.lcr_get_junctions_genes(E.h, C.byref(jl)) == 0 and tg.helpers_view(jl).tobytes() == k1[0].tobytes()
    assert bytes((C.c_int32 * (jl.n_regions + 1)).from_address(jl.junc_region_off)) == k1[1].tobytes()
    E.close()


def test_kernel_ms(engine_cls):
    regs, genes, _ = tg.edge_case()
    b = tj.batch_of(regs[:1])
    for timing in (False, True):
        E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5), timing=timing)
        E.load_batch(b).assign_genes(genes).run_all()
        ms = E.asj_genes(genes, 4, 1, exons=True, coverage=True)["kernel_ms"]
        assert (0.0 < ms < 1000.0) if timing else ms == -1.0
        E.close()

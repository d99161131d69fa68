"""lcr_asj_genes without a GPU: the layout of its three ABI structs (gcc against ctypes, and the Rust binding of INTEGRATION.md), the
symbols, the driver's argument checks as a stand-alone program under the host sanitizers, asj.cluster with exon records, the coverage
text and annotation.gene_features, the restatement's block rules by hand, and pipeline.run's argument checks."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import asj_genes_ref
import asj_modes_ref
import test_asj_genes_host as th
from longcallr_amd import _abi, _lib, annotation, asj, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. layouts, bindings, the argument checks -----------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(tmp_path):
    fields = {"lcr_asj_params": [n for n, _ in _abi.LcrAsjParams._fields_], "lcr_exon_gene": list(_abi.EXON_GENE_DTYPE.names),
              "lcr_asj_gene_list": [n for n, _ in _abi.LcrAsjGeneList._fields_]}
    lines = ['#include "lcr.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(){"]
    for name, fs in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in fs]
    lines.append('printf("flags %d\\n", LCR_ASJ_EXONS | LCR_ASJ_DNA_FILTER << 4 | LCR_ASJ_COVERAGE << 8);')
    lines.append("return 0;}")
    src, exe = tmp_path / "j.c", tmp_path / "j"
    src.write_text("\n".join(lines))
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = {k: int(v) for k, v in (l.split() for l in os.popen(str(exe)).read().strip().split("\n"))}
    assert got["flags"] == _abi.LCR_ASJ_EXONS | _abi.LCR_ASJ_DNA_FILTER << 4 | _abi.LCR_ASJ_COVERAGE << 8 == 0x421
    assert got["lcr_exon_gene"] == 24 == _abi.EXON_GENE_DTYPE.itemsize and got["lcr_asj_params"] == 32 == C.sizeof(_abi.LcrAsjParams)
    assert got["lcr_asj_gene_list"] == C.sizeof(_abi.LcrAsjGeneList)
    for f in fields["lcr_exon_gene"]:
        assert got["lcr_exon_gene." + f] == _abi.EXON_GENE_DTYPE.fields[f][1], f
    for name, cls in (("lcr_asj_params", _abi.LcrAsjParams), ("lcr_asj_gene_list", _abi.LcrAsjGeneList)):
        for f in fields[name]:
            assert got["%s.%s" % (name, f)] == getattr(cls, f).offset, (name, f)
    # lcr_junction_gene_list's fields first, in the same places (kernel_ms moves to the end)
    for f, _ in _abi.LcrJunctionGeneList._fields_[:-1]:
        assert getattr(_abi.LcrAsjGeneList, f).offset == getattr(_abi.LcrJunctionGeneList, f).offset, f
    for name in fields:
        rust, size = th._rust_layout(name)
        assert size == got[name] and list(rust) == fields[name], name
        for f in fields[name]:
            assert rust[f] == got["%s.%s" % (name, f)], (name, f)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"pub fn lcr_asj_genes\(ctx: \*mut lcr_ctx, p: \*const lcr_asj_params, mem: i32,\s*a: \*const lcr_gene_annotation\) -> i32", doc)
    assert re.search(r"pub fn lcr_get_asj_genes\(ctx: \*mut lcr_ctx, out: \*mut lcr_asj_gene_list\) -> i32", doc)
    assert _abi.NTIMERS == _abi.NKERNELS + 2        # no new slot of lcr_kernel_ms


def test_symbols_in_the_library():
    assert {"lcr_asj_genes", "lcr_get_asj_genes"} <= set(_lib.SYMBOLS)
    lib = _lib.load()                    # (no GPU is touched by loading it)
    assert lib.lcr_asj_genes and lib.lcr_get_asj_genes
    p = _abi.LcrAsjParams(4, 1, 8, 0.0, 0, 0, None)
    assert lib.lcr_asj_genes(None, C.byref(p), _abi.LCR_MEM_HOST, None) == -1          # a NULL context: LCR_E_ARG before anything else
    assert lib.lcr_get_asj_genes(None, None) == -1


def test_argument_checks_stand_alone_under_sanitizers(tmp_path):
    """the driver's argument checks (csrc/lcr_asj_args.h) compiled into a program of their own with the host sanitizers"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "asj_args")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "asj_args_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and not r.stderr, r.stdout + r.stderr


# ---- 2. asj.cluster with exons -------------------------------------------------------------------------------------------------------------------
def _exons(rows):
    a = np.zeros(len(rows), dtype=_abi.EXON_GENE_DTYPE)
    for i, r in enumerate(rows):
        for k, v in r.items():
            a[k][i] = v
    return a


def test_cluster_with_exons():
    # two junctions of one read chain, joined only through the exon [700, 750) between them
    rec = th._recs([dict(gene=0, start0=600, len=100), dict(gene=0, start0=750, len=100)])
    ex = _exons([dict(gene=0, start0=700, len=50, n_reads=4)])
    assert asj.cluster(rec).tolist() == [0, 1] and asj.cluster(rec, None).tolist() == [0, 1]
    assert asj.cluster(rec, ex).tolist() == [0, 0] == asj_modes_ref.cluster(rec, ex).tolist()
    assert asj.cluster(rec, ex[:0]).tolist() == [0, 1]
    # the exon of another gene or region joins nothing; neither does one that touches nothing (one base off on either side)
    for other in (_exons([dict(gene=1, start0=700, len=50)]), _exons([dict(region=1, gene=0, start0=700, len=50)]),
                  _exons([dict(gene=0, start0=701, len=48)]), _exons([dict(gene=0, start0=699, len=52)]),
                  _exons([dict(gene=0, start0=600, len=100)])):         # the retained intron of the first junction: s == a, not s == b
        assert asj.cluster(rec, other).tolist() == [0, 1] == asj_modes_ref.cluster(rec, other).tolist()
    # exon - exon edges: [700, 750) reaches (600, 100); [700, 800) shares its start and reaches (800, 50)
    rec2 = th._recs([dict(gene=0, start0=600, len=100), dict(gene=0, start0=800, len=50), dict(gene=0, start0=900, len=10)])
    ex2 = _exons([dict(gene=0, start0=700, len=50), dict(gene=0, start0=700, len=100)])
    assert asj.cluster(rec2, ex2).tolist() == [0, 0, 2] == asj_modes_ref.cluster(rec2, ex2).tolist()
    assert asj.cluster(rec2, ex2[:1]).tolist() == [0, 1, 2] and asj.cluster(rec2, ex2[1:]).tolist() == [0, 0, 2]
    # ... and on a shared end: [850, 900) reaches (900, 10), [820, 900) shares its end and [750, 820)... is not there: (600, 100) stays apart
    ex3 = _exons([dict(gene=0, start0=850, len=50), dict(gene=0, start0=820, len=80)])
    assert asj.cluster(rec2, ex3).tolist() == [0, 1, 1] == asj_modes_ref.cluster(rec2, ex3).tolist()       # (800, 50) ends at 850
    # the first junction of a component stays its name although an exon joined it first
    rec4 = th._recs([dict(gene=0, start0=100, len=10), dict(gene=0, start0=600, len=100), dict(gene=0, start0=750, len=100)])
    assert asj.cluster(rec4, ex).tolist() == [0, 1, 1]
    with pytest.raises(ValueError):
        asj.cluster(np.zeros(1, dtype=_abi.JUNC_DTYPE), ex)
    # the tables of gene_events / format_tsv_genes may carry the exons: Junction_set of the second row changes, nothing else
    genes = annotation.ContigGenes.from_exons([("g0", [(0, 1000)], "ALPHA", "+", True)])
    full = th._recs([dict(gene=0, start0=600, len=100, motif=1, phase_set=5, n_phase_sets=1, cells=(10, 0, 0, 10)),
                     dict(gene=0, start0=750, len=100, motif=1, phase_set=5, n_phase_sets=1, cells=(0, 10, 10, 0))])
    a = asj.format_tsv_genes([("c", full, genes)], 10).split("\n")
    b = asj.format_tsv_genes([("c", full, genes, ex)], 10).split("\n")
    assert a[1] == b[1] and a[2].split("\t")[2] == "c:751-850" and b[2].split("\t")[2] == "c:601-700"
    assert [x for i, x in enumerate(a[2].split("\t")) if i != 2] == [x for i, x in enumerate(b[2].split("\t")) if i != 2]
    assert asj.format_gene_tsv([("c", full, genes, ex)], 10) == asj.format_gene_tsv([("c", full, genes)], 10)


# ---- 3. the coverage text; gene features -----------------------------------------------------------------------------------------------------------
GTF = [("chr1", "gene", 101, 900, 'gene_id "gA"; gene_type "protein_coding"; gene_name "ALPHA";'),
       ("chr1", "exon", 101, 300, 'gene_id "gA"; gene_type "protein_coding"; transcript_id "t1";'),
       ("chr1", "gene", 50, 80, 'gene_id "gNoExon"; gene_type "lncRNA";'),                                       # no exons: listed, never assigned
       ("chr1", "exon", 400, 500, 'gene_id "gExonOnly"; gene_type "protein_coding"; transcript_id "t2";'),      # takes reads, not listed
       ("chr1", "gene", 1, 2000, 'gene_id "gRT"; gene_type "protein_coding"; gene_name "RT"; tag "readthrough_gene";'),
       ("chr2", "gene", 10, 20, 'gene_id "gB"; gene_type "protein_coding"; gene_name "BETA";')]


def test_gene_features_and_coverage_text(tmp_path):
    path = str(tmp_path / "six.gtf")
    with open(path, "w") as f:
        f.write("# six lines\n" + "".join("\t".join([c, "src", feat, str(a), str(b), ".", "+", ".", at]) + "\n" for c, feat, a, b, at in GTF))
    feats = annotation.gene_features(path)
    assert feats == [("chr1", "gA", "ALPHA", 101, 900), ("chr1", "gNoExon", ".", 50, 80), ("chr2", "gB", "BETA", 10, 20)]
    assert annotation.gene_features(path, ("lncRNA",)) == [("chr1", "gNoExon", ".", 50, 80)]
    with pytest.raises(ValueError):
        annotation.gene_features(str(tmp_path / "six.txt"))
    g = annotation.load(path)                                        # load and ContigGenes keep their results
    assert list(g) == ["chr1"] and g["chr1"].gene_id == ["gA", "gExonOnly"] and g["chr1"].reported.tolist() == [True, False]
    reads = {("chr1", "gA"): 12, ("chr1", "gExonOnly"): 5}
    text = asj.format_gene_coverage([(name, c, s, e, reads.get((c, gid), 0)) for c, gid, name, s, e in feats])
    assert text == "#Gene_name\tChr\tStart\tEnd\tNum_reads\nALPHA\tchr1\t101\t900\t12\n.\tchr1\t50\t80\t0\nBETA\tchr2\t10\t20\t0\n"
    assert asj.format_gene_coverage([]) == "#Gene_name\tChr\tStart\tEnd\tNum_reads\n"


# ---- 4. the restatement by hand ----------------------------------------------------------------------------------------------------------------------
def test_restatement_blocks_by_hand():
    f = lambda pos, cig: asj_genes_ref.read_exon_regions(pos, [(op, n) for op, n in cig if not (op in (0, 7, 8, 2) and n == 0)])
    M, I, D, N = 0, 1, 2, 3
    # the issue's example 600M5N5N50M10N50M: one interior block [610, 660) = 1-based (611, 660)
    ex = f(0, [(M, 600), (N, 5), (N, 5), (M, 50), (N, 10), (M, 50)])
    assert ex == [(1, 600), (611, 660), (671, 720)]
    assert asj_modes_ref.interior_exons({0: ex, 1: ex, 2: ex[:2]}, 2) == {(611, 660): 2}
    assert asj_modes_ref.interior_exons({0: ex, 1: ex}, 3) == {}
    assert f(0, [(N, 5), (M, 10), (N, 5), (D, 3), (M, 2), (I, 4), (M, 1), (N, 0), (M, 4), (N, 9), (M, 1)]) == [(6, 15), (21, 30), (40, 40)]
    assert f(0, [(M, 5), (M, 0), (N, 5), (D, 0), (M, 5)]) == [(1, 5), (11, 15)]                 # zero-length M / D open nothing
    # the hand instance of test_asj_genes_host with the modes: exons of gene 0 at min_count 2 -- a1 / a2's [1200, 1300), z1 / z2's [1720, 1730)
    batch, rro, rread, asg, ps, gene, genes = th.hand_instance()
    cands, coff = np.zeros(0, dtype=_abi.CAND_DTYPE), np.array([0, 0])
    out = asj_modes_ref.asj_genes(batch, rro, rread, asg, ps, gene, genes, cands, coff, 2, 1, exons=True, coverage=True)
    assert th.tuples(out["junc"]) == th.WANT
    assert [tuple(int(x) for x in r) for r in out["exon"].tolist()] == [(0, 0, 1200, 100, 2), (0, 0, 1720, 10, 2), (0, 1, 1170, 10, 2), (0, 1, 1200, 50, 2)]
    assert out["exon_region_off"].tolist() == [0, 4] and out["gene_reads"].tolist() == [6, 4]   # gene 0: a1 a2 unasg one z1 z2; `few` has one junction
    # no DNA site at all: every row is removed in front of the cells; n_reads stay
    zero = asj_modes_ref.asj_genes(batch, rro, rread, asg, ps, gene, genes, cands, coff, 2, 1, dna_pos0=[])
    assert [t[:5] for t in th.tuples(zero["junc"])] == [t[:5] for t in th.WANT] and all(t[5:] == (0,) * 6 for t in th.tuples(zero["junc"]))


# ---- 5. pipeline.run's argument checks ------------------------------------------------------------------------------------------------------------------
def test_pipeline_argument_errors(tmp_path):
    o = str(tmp_path / "o.vcf")
    for kw in (dict(asj_cluster_with_exons=True), dict(asj_dna_vcf=str(tmp_path / "d.vcf")), dict(asj_gene_coverage=True)):
        with pytest.raises(ValueError, match="need asj_annotation"):
            pipeline.run("x.bam", "x.fa", o, asj_out=str(tmp_path / "o.asj.tsv"), **kw)
        with pytest.raises(ValueError, match="need asj_annotation"):
            pipeline.run("x.bam", "x.fa", o, **kw)

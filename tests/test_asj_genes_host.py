"""Per-gene allele-specific junctions without a GPU: the restatement of the script's analyze_gene (tests/asj_genes_ref.py) on a
hand-derived table, the annotation's introns on GTF / GFF3 text, the per-gene TSV texts and the merge, the layout of the new ABI
structs, and pipeline.run's argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import asj_genes_ref
import genes_ref
import helpers
from longcallr_amd import _abi, _lib, annotation, asj, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("region", "gene", "start0", "len", "n_reads", "phase_set", "n_phase_sets", "h1_absent", "h1_present", "h2_absent", "h2_present")


def tuples(rec):
    return [tuple(int(rec[f][i]) for f in FIELDS) for i in range(len(rec))]


# ---- 1. the restatement by hand -------------------------------------------------------------------------------------------------------------
# Two overlapping genes (0-based half-open): G0 exons [1000, 1100) [1200, 1300) [1500, 1600); G1 exons [1050, 1150) [1200, 1250).
# One region; row r is read r; assignment, phase set and gene of every read are fabricated.  min_count 2, min_junctions 1.
#   name  pos   CIGAR               blocks                                     junctions (s, l)        gene hap ps
READS = [
    ("a1", 1010, "90M100N100M200N50M", 0, 1, 7),   # [1010,1100) [1200,1300) [1500,1550)    (1100,100) (1300,200)
    ("a2", 1010, "90M100N100M200N50M", 0, 2, 7),
    ("few", 1010, "90M100N50M", 0, 1, 7),          # one junction = min_junctions: takes no part
    ("nogene", 1010, "90M100N100M200N50M", -1, 1, 7),   # gene -1: no part anywhere
    ("unasg", 1010, "90M100N100M200N50M", 0, 0, 7),     # assignment 0: no part
    ("b1", 1060, "40M100N50M250N20M", 1, 1, 7),    # [1060,1100) [1200,1250) [1500,1520)    (1100,100) (1250,250)
    ("b2", 1060, "40M100N50M250N20M", 1, 2, 9),
    ("one", 1099, "1M100N1M299N1M", 0, 2, 7),      # [1099,1100) [1200,1201) [1500,1501): one-base blocks; (1100,100) (1201,299)
    ("i1", 1150, "10M10N10M10N5M", 1, 1, 7),       # [1150,1160) [1170,1180) [1190,1195): in G1's intron; (1160,10) (1180,10)
    ("i2", 1150, "10M10N10M10N5M", 1, 2, 7),
    ("z1", 1700, "10M10N10M10N10M", 0, 1, 7),      # [1700,1710) [1720,1730) [1740,1750): behind G0; (1710,10) (1730,10)
    ("z2", 1700, "10M10N10M10N10M", 0, 2, 7),
]
# Gene 0.  Participating: a1 a2 one z1 z2.  n_reads: (1100,100) 3, (1201,299) 1 (dropped), (1300,200) 2, (1710,10) 2, (1730,10) 2.
#   Counted: a1, a2 (exon bases), one (base 1099 lies in [1000,1100): its K8 overlap is 0, a one-base block); z1, z2 share nothing.
#   (1100,100): a1 present h1, a2 present h2, one present h2                         -> ps 7, 1 set, (0, 1, 0, 2)
#   (1300,200): a1, a2 present; one [1099,1501) overlaps (1099 < 1500, 1501 > 1300): absent h2 -> ps 7, 1 set, (0, 1, 1, 1)
#   (1710,10), (1730,10): only z1, z2 overlap, neither is counted                    -> the zero record
# Gene 1.  Participating: b1 b2 i1 i2.  n_reads: (1100,100) 2, (1160,10) 2, (1180,10) 2, (1250,250) 2.  Counted: b1, b2 only.
#   every junction lies inside [1060, 1520): b1 (h1, ps 7) and b2 (h2, ps 9) overlap each: two sets of one row, the smaller value 7 wins
#   (1100,100), (1250,250): b1 present -> (0, 1, 0, 0);   (1160,10), (1180,10): b1 absent -> (1, 0, 0, 0)
WANT = [(0, 0, 1100, 100, 3, 7, 1, 0, 1, 0, 2), (0, 0, 1300, 200, 2, 7, 1, 0, 1, 1, 1),
        (0, 0, 1710, 10, 2, 0, 0, 0, 0, 0, 0), (0, 0, 1730, 10, 2, 0, 0, 0, 0, 0, 0),
        (0, 1, 1100, 100, 2, 7, 2, 0, 1, 0, 0), (0, 1, 1160, 10, 2, 7, 2, 1, 0, 0, 0),
        (0, 1, 1180, 10, 2, 7, 2, 1, 0, 0, 0), (0, 1, 1250, 250, 2, 7, 2, 0, 1, 0, 0)]


def hand_instance():
    genes = annotation.ContigGenes.from_exons([("G0", [(1000, 1100), (1200, 1300), (1500, 1600)]), ("G1", [(1050, 1150), (1200, 1250)])])
    reads = []
    for name, pos, cigar, _, _, _ in READS:
        n = sum(int(l) for l, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MIS=X")
        reads.append(dict(pos=pos, seq="A" * n, qual=30, cigar=cigar, region=0))
    ref = list("A" * 2000)
    ref[1100:1102], ref[1198:1200] = "gt", "AG"          # (1100, 100): GT..AG = 1
    batch = helpers.mk_batch(reads, [(0, "".join(ref))])
    n = len(READS)
    return (batch, np.array([0, n]), np.arange(n), np.array([r[4] for r in READS]), np.array([r[5] for r in READS]),
            np.array([r[3] for r in READS]), genes)


def test_restatement_by_hand():
    batch, rro, rread, asg, ps, gene, genes = hand_instance()
    assert genes.gene_id == ["G0", "G1"]
    rec, off = asj_genes_ref.junctions_genes(batch, rro, rread, asg, ps, gene, genes, 2, 1)
    assert off.tolist() == [0, 8] and tuples(rec) == WANT
    assert rec["motif"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0] and not rec["pad_"].any() and not rec["pad2_"].any()
    # the read of one-base blocks has overlap 0 by lcr_assign_genes' rule and still shares a base
    tree, gi = genes_ref.script_trees(genes)
    assert genes_ref.assign_read(1099, genes_ref.cigartuples(batch, 7), tree, gi) == (0, 0)
    # the threshold comes before the filter: at min_count 3 only gene 0's (1100, 100) is left, with the same cells
    rec3, _ = asj_genes_ref.junctions_genes(batch, rro, rread, asg, ps, gene, genes, 3, 1)
    assert tuples(rec3) == WANT[:1]
    # more than two junctions: nobody
    assert asj_genes_ref.junctions_genes(batch, rro, rread, asg, ps, gene, genes, 2, 2)[1].tolist() == [0, 0]
    # every read to gene 0: i1 / i2 share bases with nothing of G0 either; b1 / b2 do
    rec0, _ = asj_genes_ref.junctions_genes(batch, rro, rread, asg, ps, np.where(gene >= 0, 0, -1), genes, 2, 1)
    got = {(t[2], t[3]): t for t in tuples(rec0)}
    assert got[(1100, 100)][4:] == (5, 7, 2, 0, 2, 0, 2)     # b2 (ps 9, h2) is a set of its own: 4 rows against 1
    assert got[(1160, 10)][4:] == (2, 7, 2, 2, 0, 2, 0)      # absent: a1 h1, a2 h2, one h2, b1 h1 (ps 7); b2 is set 9; i1 / i2 not counted


def test_read_exon_regions_as_the_script():
    f = asj_genes_ref.read_exon_regions
    assert f(100, [(0, 10), (1, 3), (2, 5), (7, 5), (8, 5)]) == [(101, 125)]                  # I passes; D, =, X extend
    assert f(100, [(0, 10), (3, 20), (2, 10), (0, 5)]) == [(101, 110), (131, 145)]            # 100M20N10D100M's case: D opens the block
    assert f(100, [(4, 5), (3, 7), (0, 1), (3, 0), (0, 2)]) == [(108, 110)]                   # a zero-length N does not split
    assert f(100, [(0, 0), (0, 4)]) == [(101, 104)]                                           # an empty block is extended, never queried alone


# ---- 2. the annotation's introns --------------------------------------------------------------------------------------------------------------
def _attrs(fmt, pairs):
    return " ".join('%s "%s";' % kv for kv in pairs) if fmt == "gtf" else ";".join("%s=%s" % kv for kv in pairs)


@pytest.mark.parametrize("fmt", ["gtf", "gff3"])
def test_annotation_introns(tmp_path, fmt):
    def row(feature, a, b, gid, tid=None, strand="+"):
        at = [("gene_id", gid), ("gene_type", "protein_coding")] + ([("transcript_id", tid)] if tid else [])
        return "\t".join(["chr1", "src", feature, str(a), str(b), ".", strand, ".", _attrs(fmt, at)])
    lines = [row("gene", 101, 1000, "GA"),
             row("exon", 101, 200, "GA", "T1"), row("exon", 301, 400, "GA", "T1"), row("exon", 601, 700, "GA", "T1"),
             row("exon", 601, 1000, "GA", "T2"), row("exon", 151, 200, "GA", "T2"),          # unsorted in the file; shares no intron with T1
             row("exon", 301, 350, "GA", "T3"), row("exon", 101, 200, "GA", "T3"),           # shares T1's first intron
             row("exon", 101, 1000, "GA", "T4"),                                              # a single exon: no intron
             row("gene", 2001, 2400, "GB", strand="-"),
             row("exon", 2001, 2100, "GB", "U1", "-"), row("exon", 2101, 2200, "GB", "U1", "-"),   # abutting: a gap of 0
             row("exon", 2202, 2300, "GB", "U1", "-"),                                        # a gap of one base (2201): dropped
             row("exon", 2303, 2400, "GB", "U1", "-"),                                        # a gap of two bases (2301, 2302): kept
             row("gene", 3001, 3300, "GC"),
             row("exon", 3001, 3100, "GC"), row("exon", 3201, 3300, "GC")]                    # no transcript_id: one nameless transcript
    path = tmp_path / ("a." + fmt)
    path.write_text("\n".join(lines) + "\n")
    g = annotation.load(str(path))["chr1"]
    assert g.gene_id == ["GA", "GB", "GC"] and g.strand == ["+", "-", "+"]
    assert g.introns[0] == frozenset({(200, 100), (400, 200), (200, 400)})       # T1: 201-300, 401-600; T2: 201-600; T3: 201-300 again
    assert g.introns[1] == frozenset({(2300, 2)})
    assert g.introns[2] == frozenset({(3100, 100)})
    assert all(isinstance(s, frozenset) for s in g.introns)
    # nothing else about ContigGenes changes; from_exons without transcripts has no annotated introns
    assert list(zip(g.exon_start0.tolist(), g.exon_end0.tolist()))[:1] == [(100, 1000)]
    h = annotation.ContigGenes.from_exons([("x", [(0, 10), (20, 30)]), ("y", [(5, 8)], "Y", "-", True, [[(40, 50), (5, 8)], [(5, 8)]])])
    assert h.introns == [frozenset(), frozenset({(8, 32)})] and h.gene_name == [".", "Y"]


# ---- 3. the TSV texts and the merge -------------------------------------------------------------------------------------------------------------
def _recs(rows):
    a = np.zeros(len(rows), dtype=_abi.JUNC_GENE_DTYPE)
    for i, r in enumerate(rows):
        for k, v in r.items():
            if k == "cells":
                a["h1_absent"][i], a["h1_present"][i], a["h2_absent"][i], a["h2_present"][i] = v
            else:
                a[k][i] = v
    return a


def _genes():
    return annotation.ContigGenes.from_exons([("g0", [(0, 100), (200, 300)], "ALPHA", "+", True, [[(0, 100), (200, 300)]]),
                                              ("g1", [(50, 400)], ".", "-", True),
                                              ("g2", [(60, 500)], "HIDDEN", "+", False),
                                              ("g3", [(70, 900)], "ALPHA", "-", True)])


def test_gene_tsv_texts():
    genes = _genes()
    assert genes.gene_id == ["g0", "g1", "g2", "g3"]
    rec = _recs([
        dict(gene=0, start0=100, len=100, motif=1, phase_set=5, n_phase_sets=1, cells=(10, 0, 0, 10)),    # A: replaced by F (same name, same junction)
        dict(gene=0, start0=100, len=150, motif=0, phase_set=5, n_phase_sets=1, cells=(5, 5, 5, 5)),      # B: novel, no GT..AG; A's donor: A's set
        dict(gene=0, start0=400, len=50, motif=1, n_reads=12),                                             # C: the zero record: dropped
        dict(gene=1, start0=100, len=100, motif=1, phase_set=0, n_phase_sets=1, cells=(3, 3, 3, 3)),      # D: phase set 0 prints "."
        dict(gene=2, start0=100, len=100, motif=1, phase_set=5, n_phase_sets=1, cells=(50, 0, 0, 50)),    # E: not reported: never printed
        dict(gene=3, start0=100, len=100, motif=1, phase_set=6, n_phase_sets=2, cells=(8, 1, 1, 8)),      # F
        dict(gene=3, start0=500, len=20, motif=1, phase_set=6, n_phase_sets=1, cells=(1, 1, 1, 1)),       # G: 4 < min_count: dropped, not adjusted over
        dict(gene=3, start0=700, len=30, motif=2, phase_set=6, n_phase_sets=1, cells=(0, 9, 9, 0))])      # H: a smaller p than F's
    rec2 = _recs([dict(gene=0, start0=100, len=100, motif=1, phase_set=77, n_phase_sets=1, cells=(0, 9, 9, 0))])   # the same cells as H on another contig
    tables = [("chrA", rec, genes), ("chrB", rec2, _genes())]
    p = [asj.junction_p(rec[i]) for i in (1, 3, 5, 7)] + [asj.junction_p(rec2[0])]
    adj = [float(x) for x in asj.bh_adjust(p)]           # over the five written rows only
    sors = [asj.sor(5, 5, 5, 5), asj.sor(3, 3, 3, 3), asj.sor(8, 1, 1, 8), asj.sor(0, 9, 9, 0)]
    want = [asj.HEADER,
            "chrA:101-250\t+\tchrA:101-200\t5\t5\t5\t5\t5\t%s\t%s\tTrue\tFalse\tALPHA" % (adj[0], sors[0]),
            "chrA:101-200\t-\tchrA:101-200\t.\t3\t3\t3\t3\t%s\t%s\tTrue\tTrue\t." % (adj[1], sors[1]),
            "chrA:101-200\t-\tchrA:101-200\t6\t8\t1\t1\t8\t%s\t%s\tTrue\tTrue\tALPHA" % (adj[2], sors[2]),
            "chrA:701-730\t-\tchrA:701-730\t6\t0\t9\t9\t0\t%s\t%s\tTrue\tTrue\tALPHA" % (adj[3], sors[3]),
            "chrB:101-200\t+\tchrB:101-200\t77\t0\t9\t9\t0\t%s\t%s\tFalse\tTrue\tALPHA" % (adj[4], sors[3]), ""]
    assert asj.format_tsv_genes(tables, 10).split("\n") == want
    assert adj[3] == adj[4] < adj[2]
    # the gene file: ALPHA's smallest adjusted p among its GT_AG events -- H, and at the tie with chrB's row the first seen (chrA) --; B's row
    # (no GT..AG) does not count without no_gtag, so "." is the name seen first
    assert asj.format_gene_tsv(tables, 10) == "#Gene_name\tChr\tP_value\tSOR\n.\tchrA\t%s\t%s\nALPHA\tchrA\t%s\t%s\n" % (adj[1], sors[1], adj[3], sors[3])
    only_b = [("chrA", rec[1:2], genes)]
    assert asj.format_gene_tsv(only_b, 10) == "#Gene_name\tChr\tP_value\tSOR\n"
    assert asj.format_gene_tsv(only_b, 10, no_gtag=True) == "#Gene_name\tChr\tP_value\tSOR\nALPHA\tchrA\t%s\t%s\n" % (asj.junction_p(rec[1]), sors[0])
    # without A (and F) B's set is its own junction; a lower min_count lets G in
    assert asj.format_tsv_genes([("chrA", rec[1:2], genes)], 10).split("\n")[1].split("\t")[2] == "chrA:101-250"
    assert len(asj.format_tsv_genes(tables, 4).split("\n")) == len(want) + 1
    assert asj.format_tsv_genes([], 10) == asj.HEADER + "\n"


def test_cluster_keys_by_pair():
    rec = _recs([dict(region=0, gene=0, start0=100, len=100), dict(region=0, gene=1, start0=100, len=100),
                 dict(region=0, gene=1, start0=150, len=50), dict(region=1, gene=1, start0=100, len=30)])
    assert asj.cluster(rec).tolist() == [0, 1, 1, 3]         # same donor in another gene or region: apart; same acceptor in the pair: joined
    plain = np.zeros(2, dtype=_abi.JUNC_DTYPE)
    plain["start0"], plain["len"] = [100, 100], [100, 50]
    assert asj.cluster(plain).tolist() == [0, 0]             # the region form is what it was


def test_merge_gene_junctions():
    rec = _recs([dict(region=0, gene=3, start0=100, len=100, cells=(8, 1, 1, 8)),
                 dict(region=1, gene=3, start0=100, len=100, cells=(9, 1, 1, 9)),      # the same junction of the gene in another region: 20 > 18
                 dict(region=1, gene=1, start0=100, len=100, cells=(2, 2, 2, 2)),
                 dict(region=2, gene=1, start0=100, len=100, cells=(4, 0, 0, 4)),      # a tie at 8: the first
                 dict(region=2, gene=1, start0=90, len=100, cells=(1, 0, 0, 0))])
    got, idx = asj.merge_gene_junctions(rec, return_index=True)
    assert idx.tolist() == [4, 2, 1] and got.dtype == _abi.JUNC_GENE_DTYPE          # by gene, s, l
    assert asj.merge_gene_junctions(rec)["region"].tolist() == [2, 1, 1]
    assert asj.merge_gene_junctions(rec[:0]).size == 0
    # two chunks of one contig go through the merge in format_tsv_genes
    text = asj.format_tsv_genes([("c", _recs([dict(gene=3, start0=100, len=100, motif=1, phase_set=6, n_phase_sets=1, cells=(8, 1, 1, 8))]), _genes()),
                                 ("c", _recs([dict(gene=3, start0=100, len=100, motif=1, phase_set=9, n_phase_sets=1, cells=(9, 1, 1, 9))]), _genes())], 10)
    assert [l.split("\t")[3:8] for l in text.split("\n")[1:-1]] == [["9", "9", "1", "1", "9"]]


# ---- 4. layouts and bindings ----------------------------------------------------------------------------------------------------------------
RUST = {"i32": 4, "u32": 4, "f32": 4, "i64": 8, "u8": 1}


def _rust_layout(name):
    """field -> offset of a #[repr(C)] struct of INTEGRATION.md (comments dropped; pointers are 8 bytes), and its size"""
    text = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    body = re.search(r"pub struct %s \{(.*?)\}" % name, text, re.S).group(1)
    off, out, align = 0, {}, 1
    for fname, ty in re.findall(r"pub (\w+): ([^,]+?)\s*(?:,|$)", body.strip()):
        m = re.match(r"\[(\w+); (\d+)\]", ty)
        size, al = (RUST[m.group(1)] * int(m.group(2)), RUST[m.group(1)]) if m else (8, 8) if ty.startswith("*") else (RUST[ty], RUST[ty])
        off = (off + al - 1) // al * al
        out[fname] = off
        off += size
        align = max(align, al)
    return out, (off + align - 1) // align * align


def test_struct_layouts_match_the_header(tmp_path):
    fields = {"lcr_junction_gene": list(_abi.JUNC_GENE_DTYPE.names), "lcr_junction_gene_list": [n for n, _ in _abi.LcrJunctionGeneList._fields_]}
    lines = ['#include "lcr.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(){"]
    for name, fs in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in fs]
    lines.append("return 0;}")
    src, exe = tmp_path / "j.c", tmp_path / "j"
    src.write_text("\n".join(lines))
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = {k: int(v) for k, v in (l.split() for l in os.popen(str(exe)).read().strip().split("\n"))}
    assert got["lcr_junction_gene"] == 56 == _abi.JUNC_GENE_DTYPE.itemsize
    assert got["lcr_junction_gene_list"] == C.sizeof(_abi.LcrJunctionGeneList)
    for f in fields["lcr_junction_gene"]:
        assert got["lcr_junction_gene." + f] == _abi.JUNC_GENE_DTYPE.fields[f][1], f
    for f in fields["lcr_junction_gene_list"]:
        assert got["lcr_junction_gene_list." + f] == getattr(_abi.LcrJunctionGeneList, f).offset, f
    # lcr_junction's fields first, in the same order and places
    assert list(_abi.JUNC_GENE_DTYPE.names[:12]) == list(_abi.JUNC_DTYPE.names) and got["lcr_junction_gene.gene"] == _abi.JUNC_DTYPE.itemsize == 48
    for f in _abi.JUNC_DTYPE.names:
        assert _abi.JUNC_GENE_DTYPE.fields[f][1] == _abi.JUNC_DTYPE.fields[f][1]
    for name in fields:
        rust, size = _rust_layout(name)
        assert size == got[name] and list(rust) == fields[name], name
        for f in fields[name]:
            assert rust[f] == got["%s.%s" % (name, f)], (name, f)
    assert re.search(r"pub fn lcr_junctions_genes\(ctx: \*mut lcr_ctx, p: \*const lcr_junction_params, mem: i32,\s*a: \*const lcr_gene_annotation\) -> i32",
                     open(os.path.join(ROOT, "INTEGRATION.md")).read())
    # no new slot of lcr_kernel_ms
    assert _abi.NTIMERS == _abi.NKERNELS + 2


def test_symbols_in_the_library():
    assert {"lcr_junctions_genes", "lcr_get_junctions_genes"} <= set(_lib.SYMBOLS)
    lib = _lib.load()                    # (no GPU is touched by loading it)
    assert lib.lcr_junctions_genes and lib.lcr_get_junctions_genes


# ---- 5. pipeline.run's argument checks ----------------------------------------------------------------------------------------------------------
def test_pipeline_argument_errors(tmp_path):
    gtf = str(tmp_path / "a.gtf")
    with pytest.raises(ValueError, match="asj_annotation needs asj_out"):
        pipeline.run("x.bam", "x.fa", str(tmp_path / "o.vcf"), asj_annotation=gtf)
    with pytest.raises(ValueError, match="same file"):
        pipeline.run("x.bam", "x.fa", str(tmp_path / "o.vcf"), asj_out=str(tmp_path / "o.asj.tsv"), asj_annotation=gtf,
                     ase_out=str(tmp_path / "o.ase.tsv"), ase_annotation=str(tmp_path / "b.gtf"))
    with pytest.raises(ValueError, match="same file"):
        pipeline.run("x.bam", "x.fa", str(tmp_path / "o.vcf"), asj_out=str(tmp_path / "o.asj.tsv"), asj_annotation=gtf,
                     ase_out=str(tmp_path / "o.ase.tsv"), ase_annotation=gtf, ase_gene_types=("lncRNA",))

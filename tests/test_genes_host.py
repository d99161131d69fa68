"""Per-gene allele-specific expression without a GPU: the restatement of the script's read -> gene assignment (tests/genes_ref.py) on
hand-derived answers, the annotation parser (longcallr_amd/annotation.py) on GTF / GFF3 text, merge_gene_records, the per-gene TSV
text, and the layout of the new ABI structs."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import genes_cases
import genes_ref
from longcallr_amd import _abi, _lib, annotation, ase, asj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement itself ----------------------------------------------------------------------------------------------------------
def test_tree_overlap_predicates():
    iv = [(10, 20, "a"), (20, 30, "b")]
    assert genes_ref.tree_overlap(iv, 19, 20) == [iv[0]]            # a.begin 10 < 20 and a.end 20 > 19; b.begin 20 < 20 fails
    assert genes_ref.tree_overlap(iv, 20, 21) == [iv[1]]            # a.end 20 > 20 fails
    assert genes_ref.tree_overlap(iv, 15, 25) == iv
    assert genes_ref.tree_overlap(iv, 15, 15) == [] and genes_ref.tree_overlap(iv, 16, 15) == []     # an empty query finds nothing


def test_splice_regions_as_the_script():
    """1-based inclusive.  pos 100 (0-based): the first base is 101."""
    sr = genes_ref.splice_regions
    assert sr(100, [(0, 10)]) == [(101, 110)]
    assert sr(100, [(4, 5), (0, 10), (1, 3), (2, 2), (0, 8), (4, 1)]) == [(101, 120)]            # S, I add nothing; D adds: 10 + 2 + 8
    assert sr(100, [(0, 10), (3, 50), (7, 5), (8, 5)]) == [(101, 110), (161, 170)]               # = and X add
    assert sr(100, [(0, 10), (3, 0), (0, 10)]) == [(101, 110), (111, 120)]                        # a zero-length N splits
    assert sr(100, [(0, 10), (3, 5), (3, 5), (0, 10)]) == [(101, 110), (121, 130)]                # between two Ns: shift 0, no block
    assert sr(100, [(3, 7), (0, 10), (3, 7)]) == [(108, 117)]
    assert sr(100, [(0, 1), (3, 9), (0, 2)]) == [(101, 101), (111, 112)]                          # a one-base block is listed ...


def test_quirks_by_hand():
    """... and contributes nothing: the script passes (101, 101) to overlap(begin, end), an empty query.  One gene, exon 0-based
    [100, 200) = 1-based [101, 200] = tree interval [101, 201)."""
    genes = annotation.ContigGenes.from_exons([("g", [(100, 200)])])
    tree, gi = genes_ref.script_trees(genes)
    assert tree == [(101, 201, 0)] and gi == {0: [(101, 201, None)]}
    a = lambda pos, cig: genes_ref.assign_read(pos, cig, tree, gi)
    assert a(150, [(0, 1)]) == (0, 0)                  # candidate (query [151, 152) meets [101, 201)), block (151, 151): empty query
    assert a(150, [(0, 2)]) == (0, 2)                  # (151, 152): query [151, 152): min(152, 200) - max(151, 101) + 1 = 2
    # the block's last base is the exon's first: block 0-based [50, 101) = (51, 101): query [51, 101), exon begin 101 < 101 fails
    assert a(50, [(0, 51)]) == (0, 0)
    assert a(50, [(0, 52)]) == (0, 2)                  # (51, 102): min(102, 200) - max(51, 101) + 1 = 2: BOTH bases count once it is met
    # the exon's last base is the block's first: 0-based [199, 260) = (200, 260): exon end 201 > 200: min(260, 200) - 200 + 1 = 1
    assert a(199, [(0, 61)]) == (0, 1)
    assert a(200, [(0, 60)]) == (-1, 0)                # gene ends at pos: no candidate
    assert a(40, [(0, 60)]) == (-1, 0)                 # gene starts at rend
    assert a(40, [(0, 61)]) == (0, 0)                  # one base into the gene: a candidate, the last-base rule gives 0
    assert a(120, [(0, 10), (2, 5), (0, 10), (1, 4), (4, 3)]) == (0, 25)


def test_ties_and_choice_by_hand():
    genes = annotation.ContigGenes.from_exons([("b", [(100, 200)]), ("a", [(100, 200)]), ("c", [(150, 400)])])
    assert genes.gene_id == ["a", "b", "c"]            # equal spans: by gene_id
    tree, gi = genes_ref.script_trees(genes)
    assert genes_ref.assign_read(100, [(0, 100)], tree, gi) == (0, 100)        # a 100, b 100, c 50: the smallest index
    assert genes_ref.assign_read(120, [(0, 200)], tree, gi) == (2, 170)        # [120, 320): a, b 80; c 320 - 150 = 170
    assert genes_ref.assign_read(250, [(0, 10)], tree, gi) == (2, 10)


def test_restatement_on_the_hand_built_instance():
    genes = genes_cases.contig_genes()
    batch, names = genes_cases.batch()
    assert genes.n_genes == 30 and batch.n_reads == len(genes_cases.READS) >= 35
    want_gene, want_ov = genes_cases.expected(names, genes)
    gene, ov = genes_ref.assign(batch, genes)
    for n, g, o, wg, wo in zip(names, gene.tolist(), ov.tolist(), want_gene, want_ov):
        assert (g, o) == (wg, wo), n
    none, zero = genes_ref.assign(batch, None)
    assert (none == -1).all() and not zero.any()


def test_pairs_restatement_by_hand():
    """One region, seven rows (row r is read r), three candidates as in test_ase_host.test_restatement_by_hand:

      row  gene  hap  ps   entries                          gene 0                     gene 1
      0    0     1    101  0: A 30, 1: T 30                 2 / 0 paternal
      1    0     1    101  0: A 30, 1: C 30                 1 / 1 no vote
      2    1     2    101  0: G 30, 1: T 12                                            0 / 1 maternal (q 12 is not seen)
      3    0     2    101  (none)                           no vote
      4    1     2    202  2: A 30                                                     set 202: the votes are over set 202's site 2: paternal
      5    0     0    101  0: G 30                          unassigned: no part
      6    -1    1    101  0: A 30                          no gene: no part in either
    gene 0: set 101 with rows 0, 1, 3: h1 2, h2 1, one set, sites 0 and 1: h1_pat 1.
    gene 1: sets 101 (row 2) and 202 (row 4), one row each: the smaller value 101, h2 1, two sets; sites 0 and 1; row 2 votes maternal."""
    from test_ase_host import _cand

    def v(base, q, p=0):
        return q | p << 5 | "ACGT".index(base) << 6
    fm = dict(row_region_off=np.array([0, 7]), row_ptr=np.array([0, 2, 4, 6, 6, 7, 8, 9]), row_read=np.arange(7),
              col=np.array([0, 1, 0, 1, 0, 1, 2, 0, 0]),
              val=np.array([v("A", 30, 1), v("T", 30), v("A", 30, 1), v("C", 30, 1), v("G", 30), v("T", 12), v("A", 30, 1), v("G", 30), v("A", 30, 1)]))
    asg, ps = np.array([1, 1, 2, 2, 2, 0, 1]), np.array([101, 101, 101, 101, 202, 101, 101])
    gene = np.array([0, 0, 1, 0, 1, 0, -1])
    cands = _cand([dict(pos=500, ref_base=ord("A"), allele1=ord("A"), allele2=ord("G"), phase_set=101),
                   dict(pos=600, ref_base=ord("C"), allele1=ord("T"), allele2=ord("C"), phase_set=101),
                   dict(pos=700, phase_set=202)])
    parental = {500: ("A", "G"), 600: ("T", "C"), 700: ("A", "G")}
    rec, off = genes_ref.pairs(fm, asg, ps, cands, [0, 3], gene, parental, 13, 11.0)
    assert off.tolist() == [0, 2]
    assert rec.tolist() == [(0, 101, 1, 2, 1, 2, 1, 0, 0, 0, 0, 0), (0, 101, 2, 0, 1, 2, 0, 0, 0, 1, 1, 0)]
    # gene 1's set 202 alone (row 2 unassigned): the pair's phase set is now 202 and candidate 2 its one eligible site
    asg2 = asg.copy(); asg2[2] = 0
    rec2, _ = genes_ref.pairs(fm, asg2, ps, cands, [0, 3], gene, parental, 13, 11.0)
    assert rec2.tolist()[1] == (0, 202, 1, 0, 1, 1, 0, 0, 1, 0, 1, 0)
    # a gene with rows but no counting row still is a pair; a region without assigned rows has none
    rec3, off3 = genes_ref.pairs(fm, np.zeros(7, int), ps, cands, [0, 3], gene, None)
    assert rec3.tolist() == [(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0)]
    assert genes_ref.pairs(fm, asg, ps, cands, [0, 3], np.full(7, -1), None)[1].tolist() == [0, 0]


# ---- 2. the annotation parser -------------------------------------------------------------------------------------------------------------
def _gtf(rows):
    out = ["#!genome-build test", "# a comment"]
    for contig, feature, start, end, strand, attrs in rows:
        text = " ".join('%s "%s";' % (k, v) for k, v in attrs)
        out.append("\t".join([contig, "src", feature, str(start), str(end), ".", strand, ".", text]))
    return "\n".join(out) + "\n"


def _gff3(rows):
    out = ["##gff-version 3"]
    for contig, feature, start, end, strand, attrs in rows:
        out.append("\t".join([contig, "src", feature, str(start), str(end), ".", strand, ".", ";".join("%s=%s" % kv for kv in attrs)]))
    return "\n".join(out) + "\n"


def _g(gid, gtype="protein_coding", name=None, tags=(), key="gene_type", tid=None):
    a = [("gene_id", gid), (key, gtype)]
    if tid:
        a.append(("transcript_id", tid))
    if name:
        a.append(("gene_name", name))
    return a + [("tag", t) for t in tags]


ROWS = [
    ("chr1", "gene", 1001, 2000, "+", _g("G1", name="ONE")),
    ("chr1", "transcript", 1001, 2000, "+", _g("G1", tid="T1")),
    ("chr1", "exon", 1001, 1100, "+", _g("G1", tid="T1")),
    ("chr1", "exon", 1051, 1200, "+", _g("G1", tid="T2")),            # overlaps the first: merged to [1000, 1200)
    ("chr1", "exon", 1201, 1300, "+", _g("G1", tid="T2")),            # abuts it (1200 + 1 == 1201): stays apart
    ("chr1", "exon", 1901, 2000, "+", _g("G1", tid="T1")),
    ("chr1", "exon", 1950, 1960, "+", _g("G1", tid="T3")),            # inside the last one
    ("chr1", "gene", 501, 900, "-", _g("G0", "lncRNA")),               # no gene_name: "."
    ("chr1", "exon", 501, 900, "-", _g("G0", "lncRNA", tid="T")),
    ("chr1", "gene", 501, 900, "+", _g("G9", "pseudogene", name="PSEUDO")),      # another gene type: dropped
    ("chr1", "exon", 501, 900, "+", _g("G9", "pseudogene", tid="T")),
    ("chr1", "gene", 3001, 3500, "+", _g("GR", name="RT", tags=("basic", "readthrough_gene"))),   # a readthrough tag: dropped
    ("chr1", "exon", 3001, 3500, "+", _g("GR", tid="T", tags=("readthrough_gene",))),
    ("chr1", "exon", 4001, 4100, "+", _g("GX", tid="T")),             # exons only: competes for reads, never reported
    ("chr1", "gene", 5001, 5100, "+", _g("GM", name="MULTI")),        # exons on two contigs: dropped
    ("chr1", "exon", 5001, 5100, "+", _g("GM", tid="T")),
    ("chr2", "exon", 5001, 5100, "+", _g("GM", tid="T")),
    ("chr2", "gene", 101, 300, "-", _g("GB", "lncRNA", name="BIO", key="gene_biotype")),          # gene_biotype in place of gene_type
    ("chr2", "exon", 101, 300, "-", _g("GB", "lncRNA", tid="T", key="gene_biotype")),
    ("chr1", "gene", 501, 900, "+", _g("G00", name="SAME_SPAN")),     # the span of G0: ordered by gene_id behind it
    ("chr1", "exon", 501, 900, "+", _g("G00", tid="T")),
    ("chr1", "gene", 501, 800, "+", _g("GZ", name="SHORTER")),        # the same start, a smaller end: in front of both
    ("chr1", "exon", 501, 800, "+", _g("GZ", tid="T")),
    ("chr3", "gene", 1, 10, "+", _g("GN", name="NOEXON")),            # a gene without exons takes no reads and is not listed
]


@pytest.mark.parametrize("fmt,gz", [("gtf", False), ("gtf", True), ("gff3", False), ("gff3", True)])
def test_annotation_parser(tmp_path, fmt, gz):
    text = (_gtf if fmt == "gtf" else _gff3)(ROWS)
    path = str(tmp_path / ("a.%s%s" % (fmt, ".gz" if gz else "")))
    if gz:
        with gzip.open(path, "wt") as f:
            f.write(text)
    else:
        open(path, "w").write(text)
    ann = annotation.load(path)
    assert sorted(ann) == ["chr1", "chr2"]
    c1 = ann["chr1"]
    assert c1.gene_id == ["GZ", "G0", "G00", "G1", "GX"]                    # by (span start, span end, gene_id)
    assert c1.gene_name == ["SHORTER", ".", "SAME_SPAN", "ONE", "."] and c1.strand == ["+", "-", "+", "+", "."]
    assert c1.reported.tolist() == [True, True, True, True, False]
    assert c1.span_start0.tolist() == [500, 500, 500, 1000, 4000] and c1.span_end0.tolist() == [800, 900, 900, 2000, 4100]
    assert c1.exon_off.tolist() == [0, 1, 2, 3, 6, 7]
    assert list(zip(c1.exon_start0.tolist(), c1.exon_end0.tolist()))[3:6] == [(1000, 1200), (1200, 1300), (1900, 2000)]
    assert c1.span_start0.dtype == np.int64 and c1.exon_off.dtype == np.int32 and c1.exon_end0.dtype == np.int64
    c2 = ann["chr2"]
    assert c2.gene_id == ["GB"] and c2.gene_name == ["BIO"] and (c2.span_start0[0], c2.span_end0[0]) == (100, 300)
    # gene_types chooses
    only = annotation.load(path, gene_types=("pseudogene",))
    assert sorted(only) == ["chr1"] and only["chr1"].gene_id == ["G9"] and only["chr1"].gene_name == ["PSEUDO"]
    assert annotation.load(path, gene_types=()) == {}


def test_annotation_rejects_other_suffixes(tmp_path):
    p = tmp_path / "a.bed"
    p.write_text("")
    with pytest.raises(ValueError, match="annotation"):
        annotation.load(str(p))


def test_merge_exons_rule():
    m = annotation.merge_exons
    assert m([(10, 20), (19, 30)]) == [(10, 30)]                  # one base in common
    assert m([(10, 20), (20, 30)]) == [(10, 20), (20, 30)]        # abutting: apart
    assert m([(50, 60), (10, 40), (15, 20), (39, 45)]) == [(10, 45), (50, 60)]
    assert annotation.ContigGenes().n_genes == 0 and annotation.ContigGenes().exon_off.tolist() == [0]


# ---- 3. merge_gene_records and the TSV text -----------------------------------------------------------------------------------------------
def _pairs(rows):
    a = np.zeros(len(rows), dtype=_abi.AGENE_DTYPE)
    for i, r in enumerate(rows):
        for k, v in r.items():
            a[k][i] = v
    return a


def test_merge_gene_records():
    pairs = _pairs([
        dict(region=0, gene=2, phase_set=900, n_phase_sets=1, h1=3, h2=4),
        dict(region=0, gene=5, phase_set=900, n_phase_sets=2, h1=30, h2=10, n_sites=3, h1_pat=20, h1_mat=1, h2_mat=7),
        dict(region=1, gene=2, phase_set=1500, n_phase_sets=2, h1=6, h2=6, n_sites=1, h2_pat=2),      # gene 2 again: 12 > 7
        dict(region=2, gene=2, phase_set=1200, n_phase_sets=1, h1=12, h2=0),                           # a tie at 12: the smaller phase set
        dict(region=2, gene=7),                                                                         # rows, none counting
        dict(region=3, gene=7),
        dict(region=3, gene=0, phase_set=40, n_phase_sets=1, h1=1, h2=0)])
    got = ase.merge_gene_records(pairs)
    assert got.dtype == _abi.AGENE_DTYPE
    assert got.tolist() == [(3, 40, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0),
                            (2, 1200, 4, 12, 0, 0, 0, 0, 0, 0, 2, 0),
                            (0, 900, 2, 30, 10, 3, 20, 1, 0, 7, 5, 0),
                            (2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7, 0)]
    assert got.tolist() == genes_ref.genes_of(pairs)
    # the order of the records does not matter (but for `region` of a gene without a read: the first seen)
    assert [r[1:] for r in ase.merge_gene_records(pairs[::-1]).tolist()] == [r[1:] for r in got.tolist()]
    # the filter mask follows the chosen record
    keep = np.array([True, True, True, False, True, True, False])
    rec, k = ase.merge_gene_records(pairs, keep)
    assert rec.tolist() == got.tolist() and k.tolist() == [False, False, True, True]
    assert [x[1] for x in genes_ref.genes_of(pairs, keep)] == k.tolist()
    assert ase.merge_gene_records(pairs[:0]).size == 0 and ase.merge_gene_records(pairs[:0], keep[:0])[1].size == 0


def test_filter_pairs():
    from test_ase_host import _cand
    cands = _cand([dict(region=0, pos=10, af2=0.394, phase_set=1001),       # 39 of 100: significant
                   dict(region=0, pos=20, af2=0.396, phase_set=2002),       # prints 0.40: not significant
                   dict(region=1, pos=30, af2=0.394, phase_set=3003)])      # not in the DNA set
    pairs = _pairs([dict(region=0, gene=0, phase_set=1001), dict(region=0, gene=1, phase_set=2002), dict(region=0, gene=2, phase_set=1001),
                    dict(region=1, gene=2, phase_set=3003), dict(region=1, gene=3, phase_set=1001), dict(region=1, gene=4)])
    keep = ase.filter_pairs(pairs, cands, np.array([10, 20], np.int64), 11.0, 10, 0.001)
    assert keep.tolist() == [True, False, True, False, False, False]       # per pair: its region's sites of ITS phase set
    assert ase.filter_pairs(pairs, cands[:0], np.array([10], np.int64), 11.0).tolist() == [False] * 6


def test_gene_tsv_texts():
    genes = annotation.ContigGenes.from_exons([("g0", [(0, 10)], "ALPHA", "+", True), ("g1", [(5, 20)], ".", "-", True),
                                               ("g2", [(30, 40)], "HIDDEN", "+", False), ("g3", [(50, 60)], "DELTA", "+", True)])
    rec = _pairs([dict(gene=0, phase_set=1001, n_phase_sets=2, h1=30, h2=10, n_sites=3, h1_pat=20, h1_mat=1, h2_mat=7),
                  dict(gene=1, phase_set=2001, n_phase_sets=1, h1=4, h2=5),         # 9 < min_support
                  dict(gene=2, phase_set=3001, n_phase_sets=1, h1=50, h2=50),       # not reported: never printed, not adjusted over
                  dict(gene=3, phase_set=4001, n_phase_sets=1, h1=5, h2=5)])
    rec2 = _pairs([dict(gene=0, h1=0, h2=12, phase_set=77, h2_mat=12, n_sites=1)])
    genes2 = annotation.ContigGenes.from_exons([("x", [(0, 10)], "OTHER", "+", True)])
    tables = [("chrA", rec, genes), ("chrB", rec2, genes2)]
    p = [ase.betabinom_two_sided(30, 40), ase.betabinom_two_sided(5, 10), ase.betabinom_two_sided(0, 12)]
    adj = asj.bh_adjust(p)
    assert ase.format_tsv(tables, 10, 0.001) == ("#Gene_name\tChr\tPS\tH1\tH2\tP_value\n"
                                                 "ALPHA\tchrA\t1001\t30\t10\t%s\nDELTA\tchrA\t4001\t5\t5\t%s\nOTHER\tchrB\t77\t0\t12\t%s\n"
                                                 % tuple(float(x) for x in adj))
    pm = ase.format_tsv(tables, 10, 0.001, patmat=True).split("\n")
    assert pm[0] == ase.HEADER_PATMAT and pm[1] == "ALPHA\tchrA\t1001\t30\t10\t%s\t20\t1\t0\t7" % float(adj[0])
    assert pm[3] == "OTHER\tchrB\t77\t0\t12\t%s\t0\t0\t0\t12" % float(adj[2]) and len(pm) == 5
    low = ase.format_tsv(tables[:1], min_support=0).split("\n")
    assert [l.split("\t")[0] for l in low[1:-1]] == ["ALPHA", ".", "DELTA"]         # a gene without a name prints "."
    flt = ase.format_tsv([("chrA", rec, genes, np.array([True, True, True, False]))], 10).split("\n")
    assert flt == [ase.HEADER, "ALPHA\tchrA\t1001\t30\t10\t%s" % p[0], ""]
    # the region form is what it was
    r0 = np.zeros(1, _abi.ASE_DTYPE); r0["h1"], r0["h2"], r0["phase_set"] = 20, 20, 5
    assert ase.format_tsv([("c", r0, np.array([9]), np.array([10]))]).split("\n")[1].startswith("c:10-19\tc\t5\t20\t20\t")


# ---- 4. layouts and bindings ----------------------------------------------------------------------------------------------------------------
def test_gene_struct_layouts_match_the_header(tmp_path):
    fields = {"lcr_gene_annotation": [n for n, _ in _abi.LcrGeneAnnotation._fields_],
              "lcr_ase_gene": list(_abi.AGENE_DTYPE.names),
              "lcr_ase_gene_list": [n for n, _ in _abi.LcrAseGeneList._fields_]}
    lines = ['#include "lcr.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(){"]
    for name, fs in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in fs]
    lines.append("return 0;}")
    src, exe = tmp_path / "g.c", tmp_path / "g"
    src.write_text("\n".join(lines))
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = {k: int(v) for k, v in (l.split() for l in os.popen(str(exe)).read().strip().split("\n"))}
    assert got["lcr_ase_gene"] == 48 == _abi.AGENE_DTYPE.itemsize
    assert got["lcr_gene_annotation"] == C.sizeof(_abi.LcrGeneAnnotation) and got["lcr_ase_gene_list"] == C.sizeof(_abi.LcrAseGeneList)
    for f in fields["lcr_ase_gene"]:
        assert got["lcr_ase_gene." + f] == _abi.AGENE_DTYPE.fields[f][1], f
    assert list(_abi.AGENE_DTYPE.names[:10]) == list(_abi.ASE_DTYPE.names)          # lcr_ase_region's fields first
    for f in _abi.ASE_DTYPE.names:
        assert _abi.AGENE_DTYPE.fields[f][1] == _abi.ASE_DTYPE.fields[f][1]
    for name, cls in (("lcr_gene_annotation", _abi.LcrGeneAnnotation), ("lcr_ase_gene_list", _abi.LcrAseGeneList)):
        for f in fields[name]:
            assert got["%s.%s" % (name, f)] == getattr(cls, f).offset, (name, f)
    assert {"lcr_assign_genes", "lcr_get_read_genes", "lcr_ase_genes", "lcr_get_ase_genes"} <= set(_lib.SYMBOLS)
    # the two timing slots follow LCR_NKERNELS: the earlier slots keep their numbers
    import re
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcr.h")).read(), flags=re.S)
    assert re.search(r"LCR_K_GENES\s*=\s*LCR_NKERNELS\s*,\s*LCR_K_ASE_GENES\s*,\s*LCR_NTIMERS", hdr)
    assert (_abi.K_GENES, _abi.K_ASE_GENES, _abi.NTIMERS) == (_abi.NKERNELS, _abi.NKERNELS + 1, _abi.NKERNELS + 2)

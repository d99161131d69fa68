"""Exon-only calling, host side (no GPU): the calling annotation's parser and the region clipping of longcallr_amd.annotation against known
answers, and the premise of the GPU tests' yardstick -- a masked run equals the oracle on the batch whose masked-out reference bytes are
'N' (exon_cases.py) -- restated with the Python oracle on the case families and presets the GPU tests use."""
import gzip

import numpy as np
import pytest

import column_cases as cc
import exon_cases as ex
from longcallr_amd import annotation as ann
from oracle import oracle_np as onp


def line(contig, feature, start, end, attrs, strand="+"):
    return "\t".join([contig, "src", feature, str(start), str(end), ".", strand, ".", attrs]) + "\n"


gtf = lambda gid: 'gene_id "%s"; gene_type "protein_coding";' % gid
gff = lambda gid: "ID=x;gene_id=%s;gene_type=protein_coding" % gid

KNOWN = (
    "# a comment\n"
    "#!another\n"
    + line("chr1", "gene", 101, 200, gtf("A"))
    + line("chr1", "transcript", 101, 200, gtf("A"))
    + line("chr1", "exon", 101, 150, gtf("A"))
    + line("chr1", "CDS", 111, 140, gtf("A"))
    + line("chr1", "CDS", 161, 190, gtf("A"))
    + line("chr1", "gene", 150, 300, gff("B"))              # overlaps A: extends the cluster
    + line("chr1", "CDS", 201, 250, gff("B"))
    + line("chr1", "gene", 180, 220, gtf("C"))              # contained; no CDS
    + line("chr1", "gene", 301, 400, gtf("D"))              # 300 + 1 == 301: abutting, a cluster of its own
    + line("chr1", "CDS", 301, 310, gtf("D"))
    + line("chr1", "gene", 1000, 1100, "gene_type \"x\";")  # no gene_id: D's stays
    + line("chr1", "CDS", 1001, 1010, gtf("D"))             # ... so this CDS passes the check and D's list is replaced at the next flush
    + line("chr2", "gene", 11, 20, gtf("A"))                # A again: its earlier list goes
    + line("chr2", "CDS", 12, 13, gtf("A"))
    + line("chr2", "gene", 50, 60, gtf("E"))
    + line("chr2", "CDS", 51, 55, gtf("E"))                 # the last gene: flushed at the end of the file
)


def write(tmp_path, text, name="a.gtf"):
    p = tmp_path / name
    if name.endswith(".gz"):
        with gzip.open(p, "wt") as f:
            f.write(text)
    else:
        p.write_text(text)
    return p


def test_known_answers(tmp_path):
    clusters, cds = ann.calling_annotation(write(tmp_path, KNOWN))
    assert clusters == {"chr1": [(100, 300, ("A", "B", "C")), (300, 400, ("D",)), (999, 1100, ("D",))],
                        "chr2": [(10, 20, ("A",)), (49, 60, ("E",))]}
    # A: chr1's list replaced by chr2's; B; C has none; D: the first flush stored [(300, 310)], the second -- under the id the id-less
    # gene kept -- replaced it; E at the end of the file
    assert cds == {"A": [(11, 13)], "B": [(200, 250)], "D": [(1000, 1010)], "E": [(50, 55)]}


def test_gz_and_plain_agree(tmp_path):
    assert ann.calling_annotation(write(tmp_path, KNOWN, "a.gff3.gz")) == ann.calling_annotation(write(tmp_path, KNOWN))


def test_first_gene_without_an_id(tmp_path):
    text = line("c", "gene", 1, 10, "gene_type x") + line("c", "CDS", 2, 3, "note y") + line("c", "gene", 5, 20, gtf("G"))
    clusters, cds = ann.calling_annotation(write(tmp_path, text))
    assert clusters == {"c": [(0, 20, ("", "G"))]} and cds == {"": [(1, 3)]}


def test_unsorted_genes_raise(tmp_path):
    text = line("c", "gene", 100, 200, gtf("A")) + line("c", "gene", 99, 300, gtf("B"))
    with pytest.raises(ValueError, match=r"line 2: annotation file is not sorted"):
        ann.calling_annotation(write(tmp_path, text))
    # (another contig has a stack of its own)
    ann.calling_annotation(write(tmp_path, line("c", "gene", 100, 200, gtf("A")) + line("d", "gene", 1, 5, gtf("B"))))


def test_cds_of_another_gene_raises(tmp_path):
    text = line("c", "gene", 100, 200, gtf("A")) + line("c", "exon", 100, 120, gtf("Z")) + line("c", "CDS", 100, 120, gtf("B"))
    with pytest.raises(ValueError, match=r"line 3: gene_id in gene and exon are different: gene_id:A, exon_gene_id:B"):
        ann.calling_annotation(write(tmp_path, text))


def test_malformed_line_raises(tmp_path):
    with pytest.raises(ValueError, match="line 2"):
        ann.calling_annotation(write(tmp_path, line("c", "gene", 1, 2, gtf("A")) + "c\tsrc\tgene\tx\t9\n"))


def test_the_scripts_parser_is_untouched(tmp_path):
    """annotation.load still reads the same file its own way: exons, gene types, merged"""
    g = ann.load(write(tmp_path, KNOWN))
    assert list(g) == ["chr1"] and g["chr1"].gene_id == ["A"] and g["chr1"].exon_start0.tolist() == [100]


CLUSTERS = [(100, 300, ("A", "B")), (300, 400, ("D",)), (999, 1100, ("D", "X"))]


def test_intersect_regions():
    # across two clusters: two regions, in cluster order, the query's index with each
    assert ann.intersect_regions([250], [100], CLUSTERS) == [(250, 50, 0, ("A", "B")), (300, 50, 0, ("D",))]
    # touching a cluster at an exclusive end only: [400, 500) against [300, 400), [900, 999) against [999, 1100)
    assert ann.intersect_regions([400, 900], [100, 99], CLUSTERS) == []
    # query order, then cluster order; a region inside a cluster keeps its span
    got = ann.intersect_regions([0, 350, 1050], [150, 10, 500], CLUSTERS)
    assert got == [(100, 50, 0, ("A", "B")), (350, 10, 1, ("D",)), (1050, 50, 2, ("D", "X"))]
    # a contig the annotation does not name
    assert ann.intersect_regions([0], [5000], None) == [] and ann.intersect_regions([0], [5000], {}.get("chrUn")) == []


def test_region_intervals():
    cds = {"A": [(110, 140), (160, 190)], "B": [(200, 250)], "D": [(1000, 1010)]}
    assert ann.region_intervals(("A", "B"), cds) == [(110, 140), (160, 190), (200, 250)]
    assert ann.region_intervals(("D", "X"), cds) == [(1000, 1010)]
    assert ann.region_intervals(("C", "X"), cds) == []          # no id has a CDS: the region is skipped
    assert ann.region_intervals(("A", "A"), cds) == [(110, 140), (160, 190)] * 2


# ---- the yardstick's premise ---------------------------------------------------------------------------------------------------------

def test_mask_helpers():
    k = np.array([1, 1, 0, 1, 0, 0, 1], bool)
    assert ex.runs(k) == [(0, 2), (3, 4), (6, 7)] and ex.runs(~k) == [(2, 3), (4, 6)] and ex.runs(np.zeros(3, bool)) == []
    b = cc.build([cc.case("a", cc._het(5), length=7), cc.case("b", cc._het(5), length=7)])
    lists = ex.lists_of(b, [k, ~k])
    assert lists == [[(100000, 100002), (100003, 100004), (100006, 100007)], [(200002, 200003), (200004, 200006)]]
    assert ex.flat(lists)[0].tolist() == [0, 3, 5]
    assert all(np.array_equal(a, z) for a, z in zip(ex.mask_of_lists(b, lists), [k, ~k]))
    shapes = [[(100003, 100004), (99990, 100002), (100001, 100001), (100006, 100900), (5, 9)], [(200004, 200006), (200002, 200003), (200004, 200005)]]
    assert all(np.array_equal(a, z) for a, z in zip(ex.mask_of_lists(b, shapes), [k, ~k]))
    sub = ex.n_substituted(b, [k, ~k]).ref
    assert np.flatnonzero(sub != b.ref).tolist() == [2, 4, 5, 7, 8, 10, 13] and set(sub[sub != b.ref].tolist()) == {ord("N")}


@pytest.mark.parametrize("preset", ["hifi-masseq", "ont-cdna"])
@pytest.mark.parametrize("family", ["dense", "place", "classes"])
def test_n_substitution_is_the_mask(orc, family, preset):
    """every other record column masked out: the planes keep their values at every unmasked column, exactly the masked records go, and
    the others keep every field"""
    n_records = 0
    for over, cases in cc.groups(cc.all_families(orc)[family]):
        b, p = cc.build(cases), cc.params(preset, over)
        plain = [onp.pileup(b, g, p) for g in range(b.n_regions)]
        recs = [onp.candidates(plain[g], int(b.start0[g]), p) for g in range(b.n_regions)]
        keep = ex.every_other(b, [[r["pos"] - int(b.start0[g]) for r in recs[g]] for g in range(b.n_regions)])
        bn = ex.n_substituted(b, keep)
        n_records += sum(len(r) for r in recs)
        for g in range(b.n_regions):
            pu = onp.pileup(bn, g, p)
            for f in ("cnt", "fwd", "ts", "n", "d", "ni", "hist"):
                assert np.array_equal(pu[f][..., keep[g]], plain[g][f][..., keep[g]]), (family, g, f)
            got = onp.candidates(pu, int(b.start0[g]), p)
            want = [r for r in recs[g] if keep[g][r["pos"] - int(b.start0[g])]]
            assert len(want) == len(recs[g]) // 2
            assert len(got) == len(want)
            for a, z in zip(got, want):
                assert a.keys() == z.keys() and all(np.array_equal(a[f], z[f]) for f in a), (family, g, z["pos"])
    assert n_records >= 10

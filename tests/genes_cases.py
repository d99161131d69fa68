"""The hand-built instance of the read -> gene tests: 30 genes and about 40 reads on one contig, every expected (gene, overlap) derived
by hand below.  Used by tests/test_genes_host.py (the restatement tests/genes_ref.py against these answers) and by
tests/test_genes_gpu.py (lcr_assign_genes against both).  Coordinates 0-based half-open; a block [s, e) and an exon [x, y) contribute
min(e, y) - max(s, x) iff e - s >= 2, y > s and x < e - 1."""
import re

import helpers
from longcallr_amd import annotation

# (gene_id, exons); annotation.ContigGenes sorts them by (span start, span end, gene_id)
GENES = [
    ("GA", [(1000, 1100), (1200, 1300), (1500, 1600)]),
    ("GB", [(10000, 10100), (10200, 20000)]),
    ("GC1", [(30000, 30100)]),
    ("GC2", [(30150, 30300)]),
    ("GD1", [(40000, 40100)]),
    ("GD2", [(40050, 40150)]),
    ("GEo", [(50000, 50100), (50900, 51000)]),          # GEi is nested in its intron
    ("GEi", [(50400, 50500)]),
    ("GF", [(60000, 60100), (60500, 60600)]),
    ("GL", [(70000, 70010), (79990, 80000)]),           # one long early gene spanning the twenty below
] + [("GS%02d" % i, [(70100 + 400 * i, 70300 + 400 * i)]) for i in range(20)]

# (name, pos, CIGAR, expected gene_id or None, expected overlap): the arithmetic of every case
READS = [
    # one block [1010, 1090) inside exon [1000, 1100): 80
    ("one_block", 1010, "80M", "GA", 80),
    # D inside a block counts: 30 + 10 + 40 = the same block [1010, 1090): 80
    ("deletion", 1010, "30M10D40M", "GA", 80),
    # I and S (and H, P) do not count: 30 + 50 = [1010, 1090): 80
    ("ins_clip", 1010, "2H5S30M7I50M3S", "GA", 80),
    ("pad", 1010, "30M2P50M", "GA", 80),
    # = and X add like M
    ("eq_x", 1010, "30=10X40M", "GA", 80),
    # a zero-length N splits a block: [1190, 1201) meets exon [1200, 1300) only with its last base (x = 1200 < e - 1 = 1200 fails): 0;
    # [1201, 1206): min(1206, 1300) - max(1201, 1200) = 5.  (The unsplit block [1190, 1206) would give 1206 - 1200 = 6.)
    ("zero_n", 1190, "11M0N5M", "GA", 5),
    ("unsplit", 1190, "16M", "GA", 6),
    # a one-base block contributes nothing although it lies inside exon [1000, 1100): [1050, 1051) 0; [1200, 1250) 50
    ("one_base", 1050, "1M149N50M", "GA", 50),
    # two-base block: [1050, 1052) 2; [1200, 1250) 50
    ("two_base", 1050, "2M148N50M", "GA", 52),
    # an exon starting at the block's last base: [1150, 1201) against [1200, 1300): x = 1200 < 1200 fails: 0.  GA is the one candidate
    # (span [1000, 1600) meets the read): assigned with overlap 0
    ("last_base_0", 1150, "51M", "GA", 0),
    # the same exon one base earlier in the block: [1150, 1202): x = 1200 < 1201: min(1202, 1300) - 1200 = 2
    ("last_base_2", 1150, "52M", "GA", 2),
    # a block over two exons and the intron between: [1050, 1250): (1100 - 1050) + (1250 - 1200) = 100
    ("two_exons", 1050, "200M", "GA", 100),
    # N N in a row: the block between them has length 0 and is no block: [1010, 1020) 10; [1220, 1230) 10
    ("double_n", 1010, "10M100N100N10M", "GA", 20),
    # a CIGAR that begins and ends with N: blocks [1020, 1030) only: 10
    ("edge_n", 1010, "10N10M10N", "GA", 10),
    # 17 blocks of 10 every 15 (33 ops: three rounds of 16): block i = [10000 + 15 i, 10010 + 15 i).  Exon [10000, 10100): i = 0..6 whole
    # (i = 6 is [10090, 10100)): 70.  Exon [10200, 20000): i = 13 is [10195, 10205): 5; i = 14, 15, 16 whole: 30.  105
    ("blocks17", 10000, "10M5N" * 16 + "10M", "GB", 105),
    # 33 blocks of 7 every 10 (65 ops: five rounds): block i = [10150 + 10 i, 10157 + 10 i).  i = 0..4 end at or before 10197 < 10200 and
    # begin behind 10100: 0.  i = 5 is [10200, 10207): 7, and so is every later one: 28 x 7 = 196
    ("blocks33", 10150, "7M3N" * 32 + "7M", "GB", 196),
    # exactly 16 ops and exactly 32: the carry at a round's edge.  8 blocks of 10 every 20 from 10200: 80; 16 blocks: 160
    ("ops16", 10200, "10M10N" * 8, "GB", 80),
    ("ops32", 10200, "10M10N" * 16, "GB", 160),
    # an N as the last op of a round and the block behind it in the next: ops 0..15 = 7 x (5M 5N) + 5M + 5N(op 15); then 40M:
    # blocks [10200 + 10 i, +5) i = 0..7: 40; [10280, 10320): 40.  80
    ("n_at_15", 10200, "5M5N" * 8 + "40M", "GB", 80),
    # gene ends at pos, gene starts at rend: neither is a candidate.  [30100, 30150): GC1 [30000, 30100) has span_end0 = pos; GC2
    # [30150, 30300) has span_start0 = rend
    ("between", 30100, "50M", None, 0),
    # one base more on either side: [30099, 30151).  GC1: y = 30100 > 30099, x < 30150: 30100 - 30099 = 1.  GC2: a candidate (30150 < 30151),
    # x = 30150 < e - 1 = 30150 fails: 0.  GC1 wins with 1
    ("touch_both", 30099, "52M", "GC1", 1),
    # two genes of equal overlap: [40050, 40100) has 50 in GD1 [40000, 40100) and 50 in GD2 [40050, 40150): the smaller index
    ("tie", 40050, "50M", "GD1", 50),
    # [40060, 40120): GD1 40, GD2 60
    ("no_tie", 40060, "60M", "GD2", 60),
    # a nested gene: [50410, 50490) lies in GEo's intron (0) and in GEi's exon (80)
    ("nested_inner", 50410, "80M", "GEi", 80),
    # [50010, 50090): GEo 80; GEi is no candidate (span_start0 50400 >= rend)
    ("nested_outer", 50010, "80M", "GEo", 80),
    # spliced over the nested gene: [50050, 50100) 50 and [50900, 50950) 50 in GEo; GEi is a candidate with 0
    ("nested_skip", 50050, "50M800N50M", "GEo", 100),
    # a candidate whose exons miss the read: [60200, 60300) in GF's intron: overlap 0, assigned because it is alone
    ("intron_only", 60200, "100M", "GF", 0),
    # the long early gene GL spans the twenty small ones: [77710, 77810) lies in GS19 [77700, 77900): 100; GL is a candidate with 0
    ("late_small", 77710, "100M", "GS19", 100),
    # ... and alone behind the last small gene: [78000, 78100): GL with 0
    ("long_only", 78000, "100M", "GL", 0),
    # inside GL's first exon: [70002, 70010) of [70000, 70010): 8 (the read is [70002, 70052))
    ("long_exon", 70002, "50M", "GL", 8),
    # twenty candidates and GL: blocks [70100 + 400 i, 70300 + 400 i) are the small genes' exons, 200 each, the last block 150: the
    # first nineteen tie at 200: the smallest index, GS00
    ("twenty", 70100, "200M200N" * 19 + "150M", "GS00", 200),
    # the same with a longer first intron: [70100, 70150) 50 in GS00, then GS01 .. GS19 whole: GS01
    ("twenty_b", 70100, "50M350N" + "200M200N" * 18 + "200M", "GS01", 200),
    # outside every gene
    ("outside", 90000, "100M", None, 0),
    ("before_all", 100, "100M", None, 0),
    # ends exactly at the first gene's start / begins exactly at its end
    ("abut_left", 900, "100M", None, 0),
    ("abut_right", 1600, "100M", None, 0),
    # the last base of the read is the first of GA: [901, 1001): x = 1000 < 1000 fails: candidate with 0
    ("last_base_gene", 901, "100M", "GA", 0),
]


def contig_genes():
    return annotation.ContigGenes.from_exons(GENES)


def batch():
    """-> (ReadBatch with the reads sorted by position, [name of read r])"""
    reads = []
    for name, pos, cigar, _, _ in READS:
        n = sum(int(l) for l, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MIS=X")
        reads.append(dict(pos=pos, seq="A" * n, qual=30, cigar=cigar, region=0, name=name))
    reads.sort(key=lambda r: r["pos"])
    return helpers.mk_batch(reads, [(0, "A" * 95000)]), [r["name"] for r in reads]


def expected(names, genes):
    """-> ([gene index or -1], [overlap]) in the batch's read order"""
    want = {name: (genes.gene_id.index(g) if g is not None else -1, ov) for name, _, _, g, ov in READS}
    return [want[n][0] for n in names], [want[n][1] for n in names]

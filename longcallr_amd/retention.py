"""Allele-specific intron retention: the intron-scale host arithmetic behind Engine.intron_retention() (include/lcr.h:
lcr_intron_retention).

The read-scale work -- the reads' junctions and aligned blocks, the introns enough tagged reads splice, the class of every overlapping
read at every kept intron, the counts per haplotype -- is K17 on the GPU; what is left per kept intron is small and plain: the
percent-intron-retention per haplotype, the two tests of the junction table on the 2x2 layout spliced / retained x haplotype, the
Benjamini-Hochberg adjustment and the TSV text.  The tests are asj's (fisher_two_sided, g_test, sor, bh_adjust), imported, not restated."""
from .asj import bh_adjust, fisher_two_sided, g_test, sor

HEADER = ("#Intron\tRegion\tMotif\tSpliced\tRetained\tOther\tPhase_set\tHap1_spliced\tHap1_retained\tHap2_spliced\tHap2_retained\t"
          "PIR_h1\tPIR_h2\tP_value\tSOR")
MOTIFS = (".", "GT-AG", "CT-AC")     # lcr_retained_intron.motif
CELLS = ("h1_spliced", "h1_retained", "h2_spliced", "h2_retained")


def pir(retained, spliced):
    """retained / (retained + spliced) as text, NA on a zero denominator"""
    return str(retained / (retained + spliced)) if retained + spliced else "NA"


def format_tsv(tables, min_count=10, min_retained=1):
    """One row per kept intron whose four cells sum to >= min_count and whose retained cells sum to >= min_retained, in the order given.
    tables: [(chrom, records, region_start0, region_len)] -- per batch the contig's name, the records of Engine.intron_retention() and
    the batch's region arrays (records["region"] indexes them).  Coordinates are 1-based inclusive: Intron is chrom:s+1-s+l, Region
    chrom:start0+1-start0+len.  Spliced, Retained and Other count the overlapping tagged rows of every phase set; the four cells count the
    spliced and retained rows of Phase_set ("." for 0); PIR_h1 / PIR_h2 are retained / (retained + spliced) of a haplotype's two cells.
    P_value is max(Fisher, G-test) of [[h1_spliced, h2_spliced], [h1_retained, h2_retained]], Benjamini-Hochberg adjusted over the written
    rows; SOR the table's symmetric odds ratio."""
    rows, pvals = [], []
    for chrom, records, start0, length in tables:
        for r in records:
            h1s, h1r, h2s, h2r = cells = [int(r[f]) for f in CELLS]
            if sum(cells) < min_count or h1r + h2r < min_retained:
                continue
            g, ps, s, l = int(r["region"]), int(r["phase_set"]), int(r["start0"]), int(r["len"])
            rows.append(("%s:%d-%d\t%s:%d-%d\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%s\t%s" % (
                (chrom, s + 1, s + l, chrom, int(start0[g]) + 1, int(start0[g]) + int(length[g]), MOTIFS[int(r["motif"])], int(r["n_spliced"]),
                 int(r["n_retained"]), int(r["n_other"]), ps if ps else ".") + tuple(cells) + (pir(h1r, h1s), pir(h2r, h2s))), sor(*cells)))
            t = [[h1s, h2s], [h1r, h2r]]
            pvals.append(max(fisher_two_sided(t), g_test(t)[1]))
    lines = [HEADER + "\n"]
    for (head, s_or), p in zip(rows, bh_adjust(pvals)):
        lines.append("%s\t%s\t%s\n" % (head, float(p), s_or))
    return "".join(lines)

"""Allele-specific transcript ends: the site-scale host arithmetic behind Engine.transcript_ends() (include/lcr.h: lcr_transcript_ends,
DESIGN.md section 1o).

The read-scale work -- the reads' ends and strands, the histogram per (region, strand, side), its peaks, the assignment of ends to peaks,
presence and absence per haplotype -- is K16 on the GPU; what is left per kept site is small and plain: the two tests of the junction
table on the same 2x2 layout, the Benjamini-Hochberg adjustment and the TSV text.  The tests are asj's (junction_p, bh_adjust, sor),
imported, not restated."""
from .asj import bh_adjust, junction_p, sor

HEADER = ("#Site\tKind\tStrand\tRegion\tSpread\tReads\tPeak_reads\tH1_reads\tH2_reads\tPhase_set\tHap1_absent\tHap1_present\tHap2_absent\t"
          "Hap2_present\tP_value\tSOR")
KINDS = ("TSS", "TES")        # lcr_end_site.kind: 0 = a 5' end, 1 = a 3' end
STRANDS = (".", "+", "-")     # lcr_end_site.strand: 1 = '+', 2 = '-'


def format_tsv(tables, min_count=10):
    """One row per kept site whose four cells sum to >= min_count, in the order given.  tables: [(chrom, records, region_start0,
    region_len)] -- per batch the contig's name, the records of Engine.transcript_ends() and the batch's region arrays
    (records["region"] indexes them).  Coordinates are 1-based inclusive: Site is chrom:peak0+1, Region chrom:start0+1-start0+len, Spread
    min0+1-max0+1, the smallest and largest end assigned to the site.  Reads, H1_reads and H2_reads are the rows whose end is assigned
    to the site, over every phase set, Peak_reads those that end exactly at it; the four cells count the present and absent rows of
    Phase_set ("." for 0).  P_value is max(Fisher, G-test) of [[h1_absent, h2_absent], [h1_present, h2_present]], Benjamini-Hochberg
    adjusted over the written rows; SOR the table's symmetric odds ratio."""
    rows, pvals = [], []
    for chrom, records, start0, length in tables:
        for r in records:
            cells = [int(r["h1_absent"]), int(r["h1_present"]), int(r["h2_absent"]), int(r["h2_present"])]
            if sum(cells) < min_count:
                continue
            g, ps = int(r["region"]), int(r["phase_set"])
            rows.append(("%s:%d\t%s\t%s\t%s:%d-%d\t%d-%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d" % (
                (chrom, int(r["peak0"]) + 1, KINDS[int(r["kind"])], STRANDS[int(r["strand"])], chrom, int(start0[g]) + 1,
                 int(start0[g]) + int(length[g]), int(r["min0"]) + 1, int(r["max0"]) + 1, int(r["n_reads"]), int(r["n_peak"]), int(r["n_h1"]),
                 int(r["n_h2"]), ps if ps else ".") + tuple(cells)), sor(*cells)))
            pvals.append(junction_p(r))
    lines = [HEADER + "\n"]
    for (head, s_or), p in zip(rows, bh_adjust(pvals)):
        lines.append("%s\t%s\t%s\n" % (head, float(p), s_or))
    return "".join(lines)

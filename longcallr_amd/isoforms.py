"""Allele-specific isoforms: the chain-scale host arithmetic behind Engine.isoforms() (include/lcr.h: lcr_isoforms).

The read-scale work -- junction walk, chain identity, grouping, spanning and presence per haplotype -- is K15 on the GPU; what is left
per kept chain is small and plain: the keys unpacked, the two tests of the junction table on the same 2x2 layout, the
Benjamini-Hochberg adjustment and the TSV text.  The tests are asj's (junction_p, bh_adjust, sor), imported, not restated."""
from .asj import bh_adjust, junction_p, sor

HEADER = ("#Isoform\tRegion\tN_junctions\tChain\tReads\tH1_reads\tH2_reads\tPhase_set\tHap1_absent\tHap1_present\tHap2_absent\tHap2_present\t"
          "P_value\tSOR")


def chains(records, chain):
    """The kept chains of Engine.isoforms() as lists of (s, l): record r's junctions are the keys chain[chain_first .. chain_first +
    n_junc), s << 32 | l each -- s the 0-based contig column of the first skipped base, l the intron's length."""
    out = []
    for r in records:
        f, n = int(r["chain_first"]), int(r["n_junc"])
        out.append([(int(k) >> 32, int(k) & 0xffffffff) for k in chain[f:f + n]])
    return out


def format_tsv(tables, min_count=10):
    """One row per kept chain whose four cells sum to >= min_count, in the order given.  tables: [(chrom, records, chain,
    region_start0, region_len)] -- per batch the contig's name, the records and the pool of Engine.isoforms() and the batch's region
    arrays (records["region"] indexes them).  Coordinates are 1-based inclusive, as the junction table prints them: Isoform is the
    chain's extent chrom:a+1-e, Region chrom:start0+1-start0+len, Chain the comma-joined introns s+1-s+l.  Reads, H1_reads and H2_reads
    are the rows that hold the chain exactly, over every phase set; the four cells count the spanning rows of Phase_set ("." for 0).
    P_value is max(Fisher, G-test) of [[h1_absent, h2_absent], [h1_present, h2_present]], Benjamini-Hochberg adjusted over the written
    rows; SOR the table's symmetric odds ratio."""
    rows, pvals = [], []
    for chrom, records, chain, start0, length in tables:
        for r, ch in zip(records, chains(records, chain)):
            cells = [int(r["h1_absent"]), int(r["h1_present"]), int(r["h2_absent"]), int(r["h2_present"])]
            if sum(cells) < min_count:
                continue
            g, ps = int(r["region"]), int(r["phase_set"])
            rows.append(("%s:%d-%d\t%s:%d-%d\t%d\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d" % (
                (chrom, int(r["start0"]) + 1, int(r["end0"]), chrom, int(start0[g]) + 1, int(start0[g]) + int(length[g]), int(r["n_junc"]),
                 ",".join("%d-%d" % (s + 1, s + l) for s, l in ch), int(r["n_reads"]), int(r["n_h1"]), int(r["n_h2"]), ps if ps else ".")
                + tuple(cells)), sor(*cells)))
            pvals.append(junction_p(r))
    lines = [HEADER + "\n"]
    for (head, s_or), p in zip(rows, bh_adjust(pvals)):
        lines.append("%s\t%s\t%s\n" % (head, float(p), s_or))
    return "".join(lines)

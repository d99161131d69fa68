"""Phased small indels: the event-scale host arithmetic behind Engine.indels() (include/lcr.h: lcr_indels).

The read-scale work -- the reads' gaps, the normalisation of every insertion and deletion over its equivalent placements, the depth at
its anchor, the class of every row at every kept event, the counts per haplotype -- is K18 on the GPU; what is left per kept event is
small and plain: the genotype from the haplotype x {present, absent} table, REF and ALT from the window's reference, and the VCF text.
The test is asj's (fisher_two_sided, bh_adjust), imported, not restated."""
from .asj import bh_adjust, fisher_two_sided

INFO_LINES = ('##INFO=<ID=HRUN,Number=1,Type=Integer,Description="Length of the run of equal reference bases at the left-shifted placement">\n'
              '##INFO=<ID=SHIFT,Number=1,Type=Integer,Description="Columns between the leftmost and the rightmost equivalent placement">\n'
              '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Reads without and with the indel (absent,present)">\n'
              '##FORMAT=<ID=HC,Number=4,Type=Integer,Description="Reads of the phase set: h1 present, h1 absent, h2 present, h2 absent">\n'
              '##FORMAT=<ID=PV,Number=1,Type=Float,Description="Fisher test of the haplotype x presence table, Benjamini-Hochberg adjusted">\n')
BASES = "ACGT"
CELLS = ("h1_present", "h1_absent", "h2_present", "h2_absent")


def cells(rec):
    return [int(rec[f]) for f in CELLS]


def fisher(rec):
    """asj's two-sided Fisher test of [[h1_present, h2_present], [h1_absent, h2_absent]]"""
    h1p, h1a, h2p, h2a = cells(rec)
    return fisher_two_sided([[h1p, h2p], [h1a, h2a]])


def genotype(rec, alpha=0.05, het_high=0.6, het_low=0.2, hom_frac=0.8, min_hap_reads=3, p_adj=None):
    """The genotype of one lcr_indel record -> (GT, FILTER, phase set or None, p), or None for a record without a PRESENT or ABSENT row
    (n_present + n_absent == 0: it is not written).  p_adj: the record's Fisher p-value, Benjamini-Hochberg adjusted over the run's
    records (format_vcf passes it); None: the record's own p-value, a run of one record.
      phased het   "1|0" (haplotype 1 carries it) or "0|1", PASS, with the phase set, when phase_set != 0, both haplotypes have at least
                   min_hap_reads PRESENT + ABSENT rows, the higher present fraction is >= het_high, the lower <= het_low, and p <= alpha
      hom          otherwise "1/1", PASS, when n_present / (n_present + n_absent) >= hom_frac
      else         "0/1", LowQual
    Every threshold is a parameter; the defaults are this feature's own choice -- the reference program calls no indels and offers none to
    follow."""
    n_p, n_a = int(rec["n_present"]), int(rec["n_absent"])
    if n_p + n_a == 0:
        return None
    h1p, h1a, h2p, h2a = cells(rec)
    p = fisher(rec) if p_adj is None else float(p_adj)
    ps = int(rec["phase_set"])
    if ps != 0 and h1p + h1a >= min_hap_reads and h2p + h2a >= min_hap_reads:
        f1, f2 = h1p / (h1p + h1a), h2p / (h2p + h2a)
        if max(f1, f2) >= het_high and min(f1, f2) <= het_low and p <= alpha:
            return ("1|0" if f1 > f2 else "0|1"), "PASS", ps, p
    if n_p / (n_p + n_a) >= hom_frac:
        return "1/1", "PASS", None, p
    return "0/1", "LowQual", None, p


def unpack(seq, length):
    """lcr_indel.seq -> the inserted bases: 2 bits per base, the first base in the lowest bits"""
    return "".join(BASES[(int(seq) >> (2 * k)) & 3] for k in range(length))


def alleles(rec, region_start0, col_off, ref):
    """REF and ALT of one record from the window's reference (ref: the batch's concatenated windows as bytes / uint8, col_off their
    offsets), upper case: the anchor base at s_left - 1, then the deleted bases (DEL: REF) or the inserted ones (INS: ALT)"""
    g, s, n = int(rec["region"]), int(rec["start0"]), int(rec["len"])
    at = int(col_off[g]) + s - 1 - int(region_start0[g])
    if int(rec["type"]) == 0:
        text = bytes(bytearray(ref[at:at + 1 + n])).decode("latin-1").upper()
        return text, text[0]
    anchor = bytes(bytearray(ref[at:at + 1])).decode("latin-1").upper()
    return anchor, anchor + unpack(rec["seq"], n)


def format_vcf(tables, contig_order=None, **thresholds):
    """One VCF line per kept event that genotype() writes -> (text, number of PASS records).  tables: [(chrom, records, [(REF, ALT)])] --
    per batch the contig's name, the records of Engine.indels() and alleles() of each.  POS is s_left, 1-based: the anchor base.  QUAL ".",
    INFO HRUN=..;SHIFT=.., FORMAT GT:DP:AD:AF:PS:HC:PV with DP the depth at the anchor, AD n_absent,n_present, AF n_present / (n_present +
    n_absent) as %.4f, PS "." unless phased, HC the four cells, PV the adjusted p-value as %.3g.  The p-values are adjusted over all
    records that are written.  Records are sorted by contig (contig_order: names in order; default: first appearance) and position,
    then deletions before insertions, length and bases."""
    rows, pvals = [], []
    for chrom, records, als in tables:
        for r, (ref, alt) in zip(records, als):
            if int(r["n_present"]) + int(r["n_absent"]) == 0:
                continue
            rows.append((chrom, r, ref, alt))
            pvals.append(fisher(r))
    order = {}
    for name in (contig_order if contig_order is not None else [x[0] for x in rows]):
        order.setdefault(name, len(order))
    lines, n_pass = [], 0
    for (chrom, r, ref, alt), p in zip(rows, bh_adjust(pvals)):
        gt, flt, ps, p = genotype(r, p_adj=p, **thresholds)
        n_p, n_a = int(r["n_present"]), int(r["n_absent"])
        n_pass += flt == "PASS"
        key = (order.get(chrom, len(order)), int(r["start0"]), int(r["type"]), int(r["len"]), int(r["seq"]))
        lines.append((key, "%s\t%d\t.\t%s\t%s\t.\t%s\tHRUN=%d;SHIFT=%d\tGT:DP:AD:AF:PS:HC:PV\t%s:%d:%d,%d:%.4f:%s:%d,%d,%d,%d:%.3g\n" % (
            (chrom, int(r["start0"]), ref, alt, flt, int(r["hrun"]), int(r["shift"]), gt, int(r["depth"]), n_a, n_p, n_p / (n_p + n_a),
             ps if ps is not None else ".") + tuple(cells(r)) + (float(p),))))
    lines.sort(key=lambda x: x[0])
    return "".join(x[1] for x in lines), n_pass

"""Allele-specific junctions: the junction-scale host arithmetic behind Engine.junctions() (include/lcr.h: lcr_junctions).

The read-scale work -- junction walk, dedupe and count, overlap and presence per haplotype -- is K6 on the GPU; what is left per
kept junction is small and plain: the clusters, the two tests, the Benjamini-Hochberg adjustment and the TSV text of
allele_specific/longcallR-asj.py (cluster_junctions_connected_components, haplotype_event_test, calc_sor, g_test_2x2, the
multipletests(method="fdr_bh") call and AseEvent).  Standard library + NumPy only: fisher_exact, chi2 and multipletests are
restated below.  Not the script's in format_tsv: there is no annotation, so Strand and Novel are "." and Gene_name is the region.
format_tsv_genes / format_gene_tsv are the per-gene form over Engine.junctions_genes() (include/lcr.h: lcr_junctions_genes) and an
annotation.ContigGenes: the script's .asj.tsv and .asj_gene.tsv."""
import math

import numpy as np

HEADER = ("#Junction\tStrand\tJunction_set\tPhase_set\tHap1_absent\tHap1_present\tHap2_absent\tHap2_present\t"
          "P_value\tSOR\tNovel\tGT_AG\tGene_name")


def cluster(junc, exons=None):
    """Connected components of the kept junctions (records of Engine.junctions(), any number of regions) where two junctions of a
    region are joined when they share s or share s + l (donor or acceptor).  Records of Engine.junctions_genes() are joined inside
    their (region, gene) pair only: the script clusters the junctions of one gene's reads.  exons: the kept interior exon blocks of
    Engine.asj_genes(exons=True) (--cluster_with_exons: cluster_junctions_exons_connected_components) -- an exon [a, b) is one more node
    of its pair, joined to an exon that shares a or shares b and to a junction with s == b or s + l == a (the script's +-1 node trick
    in half-open terms), so two junctions on either side of a kept exon fall into one component.  Returns an int array: for every
    junction the index of its component's first junction in output order."""
    n = len(junc)
    gene = junc["gene"] if "gene" in (junc.dtype.names or ()) else None
    m = 0 if exons is None else len(exons)
    if m and gene is None:
        raise ValueError("exon records belong to (region, gene) pairs: the junction records need a gene field")
    parent = list(range(n + m))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    seen = {}
    for i in range(n):
        g, s, l = int(junc["region"][i]), int(junc["start0"][i]), int(junc["len"][i])
        if gene is not None:
            g = (g, int(gene[i]))
        for key in ((g, 0, s), (g, 1, s + l)):
            j = seen.setdefault(key, i)
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)    # the root is the component's first junction
    for e in range(m):   # an exon's nodes come behind the junctions': the root of a component with a junction stays a junction
        g = (int(exons["region"][e]), int(exons["gene"][e]))
        a0, b0 = int(exons["start0"][e]), int(exons["start0"][e]) + int(exons["len"][e])
        for key in ((g, 0, b0), (g, 1, a0)):     # junctions that start at its end / end at its start; exons with the same end / start
            j = seen.setdefault(key, n + e)
            a, b = find(n + e), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int64)


def _log_hyper(x, r1, c1, n):
    """log P(X = x) of the hypergeometric distribution: x of the r1 first-row items among the c1 first-column ones, n in all"""
    lg = math.lgamma
    return (lg(r1 + 1) - lg(x + 1) - lg(r1 - x + 1) + lg(n - r1 + 1) - lg(c1 - x + 1) - lg(n - r1 - c1 + x + 1)
            - (lg(n + 1) - lg(c1 + 1) - lg(n - c1 + 1)))


def fisher_two_sided(table):
    """Two-sided Fisher exact test of a 2x2 table (scipy.stats.fisher_exact's p-value): the sum of the hypergeometric
    probabilities that are <= the observed one, with scipy's relative slack of 1e-7."""
    (a, b), (c, d) = [[int(v) for v in row] for row in table]
    r1, c1, n = a + b, a + c, a + b + c + d
    if n == 0:
        return 1.0
    p_obs = math.exp(_log_hyper(a, r1, c1, n))
    total = 0.0
    for x in range(max(0, r1 + c1 - n), min(r1, c1) + 1):
        p = math.exp(_log_hyper(x, r1, c1, n))
        if p <= p_obs * (1.0 + 1e-7):
            total += p
    return min(total, 1.0)


def g_test(table, pseudocount=1e-10):
    """g_test_2x2 of the script: (G, p) of the log-likelihood-ratio test, the pseudocount on observed and expected alike;
    p = 1 - chi2.cdf(G, 1) = 1 - erf(sqrt(G / 2)) for G > 0 and 1.0 otherwise."""
    t = [[float(v) for v in row] for row in table]
    rows = [t[0][0] + t[0][1], t[1][0] + t[1][1]]
    cols = [t[0][0] + t[1][0], t[0][1] + t[1][1]]
    n = rows[0] + rows[1]
    if n <= 0:
        return 0.0, 1.0
    g = 0.0
    for i in range(2):
        for j in range(2):
            obs = t[i][j] + pseudocount
            exp = rows[i] * cols[j] / n + pseudocount
            g += obs * math.log(obs / exp)
    g *= 2.0
    return g, (1.0 - math.erf(math.sqrt(g / 2.0)) if g > 0 else 1.0)


def sor(h1_absent, h1_present, h2_absent, h2_present):
    """calc_sor of the script (GATK's AS_StrandOddsRatio form): ln(R + 1 / R), R the odds ratio of the table with 1 added to every cell"""
    r = ((h1_absent + 1) * (h2_present + 1)) / ((h1_present + 1) * (h2_absent + 1))
    return math.log(r + 1.0 / r)


def bh_adjust(p):
    """Benjamini-Hochberg adjusted p-values (multipletests(p, method="fdr_bh")[1]), in the order given"""
    p = np.asarray(p, dtype=np.float64)
    n = p.size
    if n == 0:
        return p.copy()
    order = np.argsort(p, kind="stable")
    adj = p[order] * n / np.arange(1, n + 1)
    adj = np.minimum(np.minimum.accumulate(adj[::-1])[::-1], 1.0)
    out = np.empty(n, dtype=np.float64)
    out[order] = adj
    return out


def junction_p(rec):
    """max(Fisher, G-test) of one record's table [[h1_absent, h2_absent], [h1_present, h2_present]] (haplotype_event_test)"""
    t = [[int(rec["h1_absent"]), int(rec["h2_absent"])], [int(rec["h1_present"]), int(rec["h2_present"])]]
    return max(fisher_two_sided(t), g_test(t)[1])


def format_tsv(tables, min_count=10):
    """The script's .asj.tsv text.  tables: [(chrom, junc, region_start0, region_len)] -- per batch the contig's name, the records of
    Engine.junctions() and the batch's region arrays (junc["region"] indexes them).  Written are the junctions whose table sums to
    >= min_count, in the order given; P_value is max(Fisher, G-test), Benjamini-Hochberg adjusted over all written junctions.
    Coordinates are the script's 1-based inclusive ones: junction (s + 1, s + l), region (start0 + 1, start0 + len).  Strand and
    Novel are "." (no annotation), Gene_name is the region, GT_AG is True iff the motif is GT..AG or CT..AC."""
    rows, pvals = [], []
    for chrom, junc, start0, length in tables:
        comp = cluster(junc)
        for i in range(len(junc)):
            r = junc[i]
            cells = [int(r["h1_absent"]), int(r["h1_present"]), int(r["h2_absent"]), int(r["h2_present"])]
            if sum(cells) < min_count:
                continue
            s, l, g, f = int(r["start0"]), int(r["len"]), int(r["region"]), int(comp[i])
            fs, fl = int(junc["start0"][f]), int(junc["len"][f])
            ps = int(r["phase_set"])
            rows.append(("%s:%d-%d\t.\t%s:%d-%d\t%s\t%d\t%d\t%d\t%d" % ((chrom, s + 1, s + l, chrom, fs + 1, fs + fl, ps if ps else ".") + tuple(cells)),
                         sor(*cells), "%s\t%s:%d-%d" % (int(r["motif"]) != 0, chrom, int(start0[g]) + 1, int(start0[g]) + int(length[g]))))
            pvals.append(junction_p(r))
    adj = bh_adjust(pvals)
    lines = [HEADER + "\n"]
    for (head, s_or, tail), p in zip(rows, adj):
        lines.append("%s\t%s\t%s\t.\t%s\n" % (head, float(p), s_or, tail))
    return "".join(lines)


def _cells(r):
    return [int(r["h1_absent"]), int(r["h1_present"]), int(r["h2_absent"]), int(r["h2_present"])]


def merge_gene_junctions(records, return_index=False):
    """One record per (gene, start0, len) out of the (region, gene) records of one contig (Engine.junctions_genes() of its chunks,
    concatenated): where the same junction of a gene occurs in more than one region or chunk, the record with the largest sum of its
    four cells is kept, ties to the first.  That happens only under truncation or with user regions: discovered coverage islands are
    connected by read spans, introns included, so every read that overlaps a junction lies in the junction's island.  -> the kept
    records in (gene, start0, len) order (with return_index: and their indices in `records`)."""
    best = {}
    for i in range(len(records)):
        r = records[i]
        key = (int(r["gene"]), int(r["start0"]), int(r["len"]))
        tot = sum(_cells(r))
        if key not in best or tot > best[key][0]:
            best[key] = (tot, i)
    idx = np.array([best[k][1] for k in sorted(best)], dtype=np.int64)
    out = records[idx] if len(idx) else records[:0]
    return (out, idx) if return_index else out


def gene_events(tables, min_count=10):
    """The events the script writes, with their adjusted p-values.  tables: [(chrom, junc, genes)] -- per batch the contig's name, the
    records of Engine.junctions_genes() and the contig's annotation.ContigGenes (junc["gene"] indexes it); the batches of a contig follow
    one another; a table may carry the batch's exon records of Engine.asj_genes(exons=True) as a fourth element, which cluster() then
    takes.  In the script's order of steps: Junction_set is the first junction (smallest s, then l) of the record's connected
    component inside its (region, gene) pair; the records of a contig are merged per gene (merge_gene_junctions); records without a
    phase set (n_phase_sets == 0: haplotype_event_test returns None) and those of genes that are not reported are dropped; of two
    genes with the same Gene_name and the same junction the later one replaces the earlier (the script's dict keyed by name); events
    whose table sums to less than min_count are dropped; P_value is max(Fisher, G-test), Benjamini-Hochberg adjusted over what is
    left.  -> a list of dicts in contig, gene, s, l order."""
    per_contig, order = {}, []
    for table in tables:
        chrom, junc, genes = table[:3]
        comp = cluster(junc, table[3] if len(table) > 3 else None)
        first = np.zeros((len(junc), 2), dtype=np.int64)
        for i in range(len(junc)):
            first[i] = (int(junc["start0"][comp[i]]), int(junc["len"][comp[i]]))
        if chrom not in per_contig:
            per_contig[chrom] = [[], [], genes]
            order.append(chrom)
        per_contig[chrom][0].append(junc)
        per_contig[chrom][1].append(first)
    events = []
    for chrom in order:
        parts, firsts, genes = per_contig[chrom]
        rec, idx = merge_gene_junctions(np.concatenate(parts), return_index=True)
        first = np.concatenate(firsts)[idx] if len(idx) else np.zeros((0, 2), np.int64)
        by_name = {}     # (s, l, Gene_name) -> position in `kept`
        kept = []
        for i in range(len(rec)):
            r = rec[i]
            k = int(r["gene"])
            if int(r["n_phase_sets"]) == 0 or not genes.reported[k]:
                continue
            s, l = int(r["start0"]), int(r["len"])
            ev = dict(chrom=chrom, start0=s, len=l, strand=genes.strand[k], set_start0=int(first[i][0]), set_len=int(first[i][1]),
                      phase_set=int(r["phase_set"]), cells=_cells(r), novel=(s, l) not in genes.introns[k], gt_ag=int(r["motif"]) != 0,
                      gene_name=genes.gene_name[k], p=junction_p(r))
            key = (s, l, ev["gene_name"])
            if key in by_name:
                kept[by_name[key]] = None
            by_name[key] = len(kept)
            kept.append(ev)
        events += [ev for ev in kept if ev is not None and sum(ev["cells"]) >= min_count]
    adj = bh_adjust([ev["p"] for ev in events])
    for ev, p in zip(events, adj):
        ev["p_adj"] = float(p)
        ev["sor"] = sor(*ev["cells"])
    return events


def format_tsv_genes(tables, min_count=10, events=None):
    """The script's .asj.tsv text with an annotation: format_tsv's header, tests, SOR and Benjamini-Hochberg adjustment over the
    written rows, with Strand and Gene_name from the annotation and Novel = the junction is no annotated intron of its gene.
    tables as in gene_events (or its result as `events`)."""
    events = gene_events(tables, min_count) if events is None else events
    lines = [HEADER + "\n"]
    for ev in events:
        c, s, l, ps = ev["chrom"], ev["start0"], ev["len"], ev["phase_set"]
        lines.append("%s:%d-%d\t%s\t%s:%d-%d\t%s\t%d\t%d\t%d\t%d\t%s\t%s\t%s\t%s\t%s\n" % (
            (c, s + 1, s + l, ev["strand"], c, ev["set_start0"] + 1, ev["set_start0"] + ev["set_len"], ps if ps else ".") + tuple(ev["cells"])
            + (ev["p_adj"], ev["sor"], ev["novel"], ev["gt_ag"], ev["gene_name"])))
    return "".join(lines)


GENE_HEADER = "#Gene_name\tChr\tP_value\tSOR"


def format_gene_tsv(tables, min_count=10, no_gtag=False, events=None):
    """The script's .asj_gene.tsv text: per Gene_name the written event with the smallest adjusted p-value (a strict <: the first seen
    wins a tie) among the events with GT_AG true -- among all of them with no_gtag --, in the order in which the names are first seen."""
    events = gene_events(tables, min_count) if events is None else events
    best = {}
    for ev in events:
        if not no_gtag and not ev["gt_ag"]:
            continue
        name = ev["gene_name"]
        if name not in best or ev["p_adj"] < best[name][1]:
            best[name] = (ev["chrom"], ev["p_adj"], ev["sor"])
    return "".join([GENE_HEADER + "\n"] + ["%s\t%s\t%s\t%s\n" % ((name,) + v) for name, v in best.items()])


COVERAGE_HEADER = "#Gene_name\tChr\tStart\tEnd\tNum_reads"


def format_gene_coverage(rows):
    """The script's .gene_coverage.tsv text (:870-878).  rows: [(gene_name, chrom, start1, end1, n_reads)] -- every `gene` feature of the
    annotation in file order (annotation.gene_features) with the reads Engine.asj_genes(coverage=True) counted for it, 0 for a gene
    nobody was assigned to."""
    return "".join([COVERAGE_HEADER + "\n"] + ["%s\t%s\t%d\t%d\t%d\n" % (name, chrom, int(s), int(e), int(n)) for name, chrom, s, e, n in rows])

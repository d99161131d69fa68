"""Allele-specific expression: the region-scale host arithmetic behind Engine.ase() (include/lcr.h: lcr_ase).

The read-scale work -- the phase set with the most assigned reads, its haplotype counts, the parent-of-origin vote of every read over
the phased heterozygous sites -- is K7 on the GPU; what is left per region is small and plain: the beta-binomial test, the
Benjamini-Hochberg adjustment, the VCF loaders and the three TSV texts of allele_specific/longcallR-ase.py (beta_binomial_p_value,
load_whole_genome_phased_vcf, load_dna_vcf, calculate_ase_pvalue_filtering, the analyze_ase_genes* writers).  Standard library + NumPy
only: scipy.stats.betabinom and multipletests are restated (the latter in asj.bh_adjust).  Without an annotation a region stands where the
script has a gene and Gene_name is the region; with one (annotation.py, Engine.assign_genes / ase_genes) the records are per gene:
merge_gene_records, filter_pairs and the per-gene form of format_tsv."""
import math

import numpy as np

from . import _abi, asj, vcf

HEADER = "#Gene_name\tChr\tPS\tH1\tH2\tP_value"
HEADER_PATMAT = HEADER + "\tH1_Paternal\tH1_Maternal\tH2_Paternal\tH2_Maternal"
HEADER_SITES = "#Chr\tPos\tRef\tAlt\tFilter\tGT\tPS\tH1_ref\tH1_alt\tH2_ref\tH2_alt\tOther_ref\tOther_alt\tP_ase\tP_ase_adj\tP_hap\tP_hap_adj"


def convert_mu_rho_to_alpha_beta(mu, rho):
    """the script's function of that name, as written"""
    phi = (1 - rho) / rho - 1
    alpha = mu * phi
    beta = (1 - mu) * phi
    return alpha, beta


def betabinom_two_sided(k, n, mu=0.5, rho=0.001):
    """beta_binomial_p_value(k, n, mu, rho, "two-sided") of the script: the sum of the beta-binomial probabilities that are <= the
    observed one (with asj.fisher_two_sided's relative slack of 1e-7, so that the mirror image of k counts whatever the rounding), capped at 1."""
    k, n = int(k), int(n)
    if n == 0:
        return 1.0
    a, b = convert_mu_rho_to_alpha_beta(mu, rho)
    lg = math.lgamma
    const = lg(n + 1) + lg(a + b) - lg(a) - lg(b) - lg(n + a + b)
    pmf = [math.exp(const - lg(x + 1) - lg(n - x + 1) + lg(x + a) + lg(n - x + b)) for x in range(n + 1)]
    lim = pmf[k] * (1.0 + 1e-7)
    return min(sum(p for p in pmf if p <= lim), 1.0)


def _acgt(x):
    return (x == 65) | (x == 67) | (x == 71) | (x == 84)


def _pick(vcf_path, contig, f):
    """f(pos0, genotype, ref, alt, phase) of one contig of the VCF, or of every contig (contig None: a dict)"""
    sites = {c: (v[0], v[1]) + v[3:] for c, v in vcf.read_sites(vcf_path, alleles=True).items()}
    if contig is None:
        return {c: f(*v) for c, v in sites.items()}
    z = np.zeros(0, np.uint8)
    return f(*sites.get(contig, (np.zeros(0, np.int64), z, z, z, z)))


def parental_sites(vcf_path, contig=None):
    """load_whole_genome_phased_vcf of the script for one contig (None: a dict of all contigs) -> (pos0, pat, mat), the arrays
    Engine.ase takes: records with genotype 0|1 or 1|0 (phased) and single-base REF and ALT in ACGT; 0|1 gives pat = ALT, mat = REF,
    1|0 gives pat = REF, mat = ALT."""
    def f(pos, gt, ref, alt, ph):
        keep = (gt == 1) & ((ph == 1) | (ph == 2)) & _acgt(ref) & _acgt(alt) & (ref != alt)
        pos, ref, alt, ph = pos[keep], ref[keep], alt[keep], ph[keep]
        return pos, np.where(ph == 1, alt, ref).astype(np.uint8), np.where(ph == 1, ref, alt).astype(np.uint8)
    return _pick(vcf_path, contig, f)


def dna_het_sites(vcf_path, contig=None):
    """load_dna_vcf of the script for one contig (None: a dict of all contigs) -> pos0 of the records with a heterozygous 0/1 genotype,
    phased or not, and single-base alleles"""
    def f(pos, gt, ref, alt, ph):
        return pos[(gt == 1) & (ref != 0) & (alt != 0)]
    return _pick(vcf_path, contig, f)


def eligible_candidates(cands, rec, min_phase_score, join=True):
    """Mask over the candidate records: what the VCF writer prints as PASS with a phased het GT (vcf.format_records), with a phase set,
    and (join) that phase set the one chosen for the candidate's region in `rec` (Engine.ase's records): lcr_ase's eligibility without
    the join with the parental sites."""
    fl = cands["flags"]
    ok = ((fl & (_abi.F_DENSE | _abi.F_NON_SELECTED)) == 0) & (cands["variant_type"] == 1)
    ok &= cands["phase_score"] >= float(min_phase_score)
    ok &= (cands["allele1"] != cands["ref_base"]) | (cands["allele2"] != cands["ref_base"])
    ok &= cands["phase_set"] != 0
    if join and len(cands):
        ok &= cands["phase_set"] == rec["phase_set"][cands["region"]]
    return ok


def filter_regions(rec, cands, dna_pos0, min_phase_score, min_support=10, overdispersion=0.001):
    """calculate_ase_pvalue_filtering's drop rule, from the candidate records: a region is kept when one of its PASS phased-het sites of
    the chosen phase set lies in the DNA set, has dp >= min_support and a beta-binomial p < 0.05 for alt_cnt = int(dp * af) of dp -- dp
    and af as the VCF prints them (af to two decimals), sites with dp == 0 or a NaN af skipped.  -> bool per region."""
    keep = np.zeros(len(rec), dtype=bool)
    dna = np.asarray(dna_pos0, dtype=np.int64)
    ok = eligible_candidates(cands, rec, min_phase_score) & np.isin(cands["pos"], dna)
    for i in np.flatnonzero(ok):
        g = int(cands["region"][i])
        if not keep[g] and _site_imbalanced(cands[i], min_support, overdispersion):
            keep[g] = True
    return keep


def _site_imbalanced(s, min_support, overdispersion):
    """one candidate record under calculate_ase_pvalue_filtering's test: dp >= min_support and p < 0.05 for int(dp * af) of dp"""
    dp = int(s["depth"])
    af = float(vcf._f2(float(s["af1"] if s["allele1"] != s["ref_base"] else s["af2"])))
    if dp == 0 or af != af:
        return False
    return dp >= min_support and betabinom_two_sided(int(dp * af), dp, 0.5, overdispersion) < 0.05


def filter_pairs(pairs, cands, dna_pos0, min_phase_score, min_support=10, overdispersion=0.001):
    """filter_regions for the (region, gene) pair records of Engine.ase_genes: a pair is kept when one of its region's PASS phased-het
    sites of the PAIR's phase set lies in the DNA set and passes the same test.  -> bool per pair."""
    ok = eligible_candidates(cands, None, min_phase_score, join=False)    # every candidate against its own phase set
    ok &= np.isin(cands["pos"], np.asarray(dna_pos0, dtype=np.int64))
    passing = set()     # (region, phase set) with a passing site
    for i in np.flatnonzero(ok):
        key = (int(cands["region"][i]), int(cands["phase_set"][i]))
        if key not in passing and _site_imbalanced(cands[i], min_support, overdispersion):
            passing.add(key)
    return np.array([(int(r["region"]), int(r["phase_set"])) in passing for r in pairs], dtype=bool)


def merge_gene_records(pairs, keep=None, shared_phase_sets=False):
    """The (region, gene) pair records of one contig -- Engine.ase_genes' records of all its chunks, concatenated -- -> one record per
    gene, ascending by gene.  A gene's rows are the union of its pairs' rows, and phase sets of different regions of a contig are
    distinct (a phase set is named after its first site's position), so the gene's phase set with the most reads is that of the pair
    record with the largest h1 + h2, ties to the smallest phase set, and that record's counts, sites and votes are the gene's;
    n_phase_sets is the sum over the pairs.  Exact across regions and across pipeline.run's chunks.  `region` is the chosen record's.
    keep (filter_pairs' mask, parallel to pairs): -> (records, the chosen records' mask).
    Not the script's: under --truncation a read that is a row of both flanks of a cut counts in both flanks' records.
    shared_phase_sets (pipeline.run(haplotag=True): the phase sets are the input VCF's and span the regions of a contig): the pair
    records of one gene with the same phase set are summed first -- h1, h2, the four votes and n_sites added, `region` the first
    one's, keep the OR of theirs -- and the choice above is made among the sums.  n_phase_sets stays the sum over the pairs."""
    pairs = np.asarray(pairs, dtype=_abi.AGENE_DTYPE)
    if shared_phase_sets and len(pairs):
        first = {}      # (gene, phase set) -> index of the summed record
        rows, kept, nps_of = [], [], []
        for i in range(len(pairs)):
            r = pairs[i]
            key = (int(r["gene"]), int(r["phase_set"]))
            j = first.get(key)
            if j is None:
                first[key] = len(rows)
                rows.append(r.copy()); kept.append(bool(keep[i]) if keep is not None else True)
                continue
            for f in ("h1", "h2", "n_sites", "h1_pat", "h1_mat", "h2_pat", "h2_mat", "n_phase_sets"):
                rows[j][f] += r[f]
            kept[j] = kept[j] or (bool(keep[i]) if keep is not None else True)
        pairs = np.array(rows, dtype=_abi.AGENE_DTYPE)
        keep = np.array(kept, dtype=bool) if keep is not None else None
    best = {}    # gene -> index of the chosen pair
    nps = {}
    for i in range(len(pairs)):
        r = pairs[i]
        k = int(r["gene"])
        nps[k] = nps.get(k, 0) + int(r["n_phase_sets"])
        j = best.get(k)
        if j is None:
            best[k] = i
            continue
        tot, tot_j = int(r["h1"]) + int(r["h2"]), int(pairs[j]["h1"]) + int(pairs[j]["h2"])
        if tot > tot_j or (tot == tot_j and int(r["phase_set"]) < int(pairs[j]["phase_set"])):
            best[k] = i
    order = sorted(best)
    out = pairs[[best[k] for k in order]].copy() if order else np.zeros(0, dtype=_abi.AGENE_DTYPE)
    for n, k in enumerate(order):
        out["n_phase_sets"][n] = nps[k]
    if keep is None:
        return out
    keep = np.asarray(keep, dtype=bool)
    return out, (keep[[best[k] for k in order]] if order else np.zeros(0, dtype=bool))


def format_tsv(tables, min_support=10, overdispersion=0.001, patmat=False):
    """The script's table text: .ase.tsv / .filter_ase.tsv (patmat=False) or .patmat_ase.tsv (patmat=True).  tables: [(chrom, rec,
    region_start0, region_len[, keep])] -- per batch the contig's name, the records of Engine.ase(), the batch's region arrays and, for
    the filter mode, filter_regions' mask (a region it drops is not written).  Written are the regions with h1 + h2 >= min_support, in the
    order given; P_value is the two-sided beta-binomial test of h1 among h1 + h2, Benjamini-Hochberg adjusted over all written regions.
    Gene_name is the region in the script's 1-based inclusive coordinates (as asj.format_tsv names it), PS is "." for 0.
    The per-gene form: tables of [(chrom, rec, genes[, keep])] -- rec the contig's merge_gene_records (a "gene" field tells the two forms
    apart), genes its annotation.ContigGenes, keep the mask merge_gene_records returns.  Gene_name is the annotation's; only genes with
    genes.reported are written (a gene without a `gene` feature takes reads and is never printed, as in the script); rows come in the
    order given and inside a table in gene order (the script: in the order its workers finish).  The min_support / Benjamini-Hochberg
    rule is the same."""
    rows, pvals = [], []
    for t in tables:
        chrom, rec = t[:2]
        per_gene = "gene" in (rec.dtype.names or ())
        if per_gene:
            genes, keep = t[2], (t[3] if len(t) > 3 else None)
        else:
            start0, length = t[2:4]
            keep = t[4] if len(t) > 4 else None
        for i in range(len(rec)):
            r = rec[i]
            h1, h2 = int(r["h1"]), int(r["h2"])
            if h1 + h2 < min_support or (keep is not None and not keep[i]):
                continue
            ps = int(r["phase_set"])
            if per_gene:
                k = int(r["gene"])
                if not genes.reported[k]:
                    continue
                head = "%s\t%s\t%s\t%d\t%d" % (genes.gene_name[k], chrom, ps if ps else ".", h1, h2)
            else:
                g = int(r["region"])
                head = "%s:%d-%d\t%s\t%s\t%d\t%d" % (chrom, int(start0[g]) + 1, int(start0[g]) + int(length[g]), chrom, ps if ps else ".", h1, h2)
            tail = "\t%d\t%d\t%d\t%d" % (int(r["h1_pat"]), int(r["h1_mat"]), int(r["h2_pat"]), int(r["h2_mat"])) if patmat else ""
            rows.append((head, tail))
            pvals.append(betabinom_two_sided(h1, h1 + h2, 0.5, overdispersion))
    adj = asj.bh_adjust(pvals)
    lines = [(HEADER_PATMAT if patmat else HEADER) + "\n"]
    for (head, tail), p in zip(rows, adj):
        lines.append("%s\t%s%s\n" % (head, float(p), tail))
    return "".join(lines)


def format_sites_tsv(tables, min_support=10, overdispersion=0.001, min_phase_score=0.0):
    """The per-site table of Engine.site_counts() (include/lcr.h: lcr_site_counts): allele x haplotype counts at every candidate the VCF
    writer prints.  tables: [(chrom, cands, site_records)] -- per batch the contig's name, the candidate records behind the phase stage
    and site_counts()'s records, parallel to them.  One row per candidate for which vcf.format_records(cands, chrom, min_phase_score)
    prints a line, in that order -- min_phase_score is the value the VCF writer gets --, written only when H1_ref + H1_alt + H2_ref +
    H2_alt >= min_support.  Pos (1-based), Ref, Alt, Filter and GT are the writer's own fields; PS is the record's phase set, "." for
    0.  ref = the cell of the upper-cased ref_base (no cell when it is not one of ACGT), alt = the other cells together -- both alleles
    of a triallelic site --, for haplotype 1, haplotype 2 and the other rows (unassigned, without a phase set, or in another set).
    P_ase: betabinom_two_sided(alt, ref + alt, 0.5, overdispersion) over haplotypes 1 + 2, the SNP-level imbalance.  P_hap:
    asj.fisher_two_sided([[H1_ref, H1_alt], [H2_ref, H2_alt]]): is the allele tied to a haplotype -- the question at RnaEdit and
    low-fraction rows.  Each is Benjamini-Hochberg adjusted (asj.bh_adjust) over all written rows."""
    rows, p_ase, p_hap = [], [], []
    for chrom, cands, recs in tables:
        if len(cands) != len(recs):
            raise ValueError("site records and candidates of %s differ in number: %d and %d" % (chrom, len(recs), len(cands)))
        for i in range(len(cands)):
            line = vcf.format_records(cands[i:i + 1], chrom, min_phase_score)
            if not line:
                continue
            f = line.rstrip("\n").split("\t")
            code = "ACGT".find(chr(int(cands["ref_base"][i])).upper())
            cells = []      # H1_ref, H1_alt, H2_ref, H2_alt, Other_ref, Other_alt
            for k in (1, 2, 0):
                n = [int(x) for x in recs["n"][i][k]]
                ref = n[code] if code >= 0 else 0
                cells += [ref, sum(n) - ref]
            if sum(cells[:4]) < min_support:
                continue
            ps = int(recs["phase_set"][i])
            rows.append("%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s" % (f[0], f[1], f[3], f[4], f[6], f[9].split(":")[0], ps if ps else ".",
                                                          "\t".join("%d" % x for x in cells)))
            p_ase.append(betabinom_two_sided(cells[1] + cells[3], sum(cells[:4]), 0.5, overdispersion))
            p_hap.append(asj.fisher_two_sided([cells[0:2], cells[2:4]]))
    adj_ase, adj_hap = asj.bh_adjust(p_ase), asj.bh_adjust(p_hap)
    lines = [HEADER_SITES + "\n"]
    for k, head in enumerate(rows):
        lines.append("%s\t%s\t%s\t%s\t%s\n" % (head, float(p_ase[k]), float(adj_ase[k]), float(p_hap[k]), float(adj_hap[k])))
    return "".join(lines)

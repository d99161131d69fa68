"""Read-backed linkage of nearby sites: the host arithmetic behind Engine.site_pairs() (include/lcr.h: lcr_site_pairs, DESIGN.md section
1r) -- the pair table that checks a phase against the reads themselves, and the multi-nucleotide variants (MNVs) merged from runs of
adjacent calls.  Host formatting only: every count comes from the records."""
import numpy as np

from . import _abi, asj, vcf

HEADER_PAIRS = ("#Chrom\tPos_a\tPos_b\tRef_a\tAlt_a\tRef_b\tAlt_b\tGT_a\tGT_b\tPS_a\tPS_b\tn_rr\tn_ra\tn_ar\tn_aa\tn_other\tn_lowq\t"
                "Orientation\tPhase\tP_value\tP_adj")
INFO_LINES = ('##INFO=<ID=SITES,Number=.,Type=Integer,Description="1-based positions of the merged single-nucleotide sites">\n'
              '##INFO=<ID=RB,Number=4,Type=Integer,Description="Rows that hold the first and the last site, by their bases: alt-alt, alt-ref, ref-alt, ref-ref">\n')


def ref_alt(s):
    """(REF, ALT) of a candidate as upper-case letters: ALT is the one the main VCF prints for a site with one ALT (vcf.format_records'
    one_alt: allele1 where it differs from ref_base, else allele2 where that differs), None without one"""
    r, a1, a2 = chr(int(s["ref_base"])), chr(int(s["allele1"])), chr(int(s["allele2"]))
    alt = a1 if a1 != r else a2 if a2 != r else None
    return r.upper(), (alt.upper() if alt is not None else None)


def cells(rec, cand_a, cand_b):
    """One lcr_site_pair record -> (rr, ra, ar, aa, other): the counted joint rows by (base at a, base at b), "r" the site's ref_base and
    "a" its ALT (ref_alt), first letter site a; other = every counted row with a third base at either site (n_lowq is not part of it)"""
    n = [[int(x) for x in row] for row in rec["n"]]
    (ra_, aa_), (rb_, ab_) = ref_alt(cand_a), ref_alt(cand_b)
    code = lambda x: "ACGT".find(x) if x is not None else -1
    at = lambda x, y: n[x][y] if x >= 0 and y >= 0 else 0
    rr, ra, ar, aa = at(code(ra_), code(rb_)), at(code(ra_), code(ab_)), at(code(aa_), code(rb_)), at(code(aa_), code(ab_))
    return rr, ra, ar, aa, sum(map(sum, n)) - rr - ra - ar - aa


def orientation(rr, ra, ar, aa):
    """the reads' own verdict: "cis" when rr + aa > ra + ar, "trans" when smaller, "tie" when equal"""
    return "cis" if rr + aa > ra + ar else "trans" if rr + aa < ra + ar else "tie"


def phase_check(cand_a, cand_b, orient):
    """orient against the phase: both sites phased hets (variant_type 1, haplotype != 0) of one phase set != 0 -> cis is expected iff
    their haplotype values are equal: "agree" / "disagree"; "." for any other pair and for a tie"""
    if not all(int(s["variant_type"]) == 1 and int(s["haplotype"]) != 0 and int(s["phase_set"]) != 0 for s in (cand_a, cand_b)):
        return "."
    if int(cand_a["phase_set"]) != int(cand_b["phase_set"]) or orient == "tie":
        return "."
    return "agree" if (orient == "cis") == (int(cand_a["haplotype"]) == int(cand_b["haplotype"])) else "disagree"


def _gt_ps(s, chrom, min_phase_score):
    line = vcf.format_records(np.asarray(s).reshape(1), chrom, min_phase_score)
    ps = int(s["phase_set"])
    return (line.rstrip("\n").split("\t")[9].split(":")[0] if line else "."), (str(ps) if ps else ".")


def format_pairs_tsv(tables, min_count=10, min_phase_score=0.0):
    """The pair table of Engine.site_pairs().  tables: [(chrom, cands, pair_records)] -- per batch the contig's name, the candidate records
    behind the phase stage and site_pairs()'s records.  One row per pair with at least min_count counted joint rows (n_rows - n_lowq), in
    record order: both positions (1-based), REF / ALT of both sites (ref_alt; "." without an ALT), GT as the main VCF prints it for
    min_phase_score ("." for a site it does not print) and PS ("." for 0) of both, cells()'s five numbers, n_lowq, orientation(),
    phase_check(), and asj.fisher_two_sided([[rr, ra], [ar, aa]]) with its Benjamini-Hochberg adjustment (asj.bh_adjust) over all written
    rows."""
    rows, pvals = [], []
    for chrom, cands, recs in tables:
        for r in recs:
            if int(r["n_rows"]) - int(r["n_lowq"]) < min_count:
                continue
            a, b = cands[int(r["a"])], cands[int(r["b"])]
            rr, ra, ar, aa, other = cells(r, a, b)
            o = orientation(rr, ra, ar, aa)
            (ref_a, alt_a), (ref_b, alt_b) = ref_alt(a), ref_alt(b)
            (gt_a, ps_a), (gt_b, ps_b) = _gt_ps(a, chrom, min_phase_score), _gt_ps(b, chrom, min_phase_score)
            rows.append("%s\t%d\t%d\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s" % (
                chrom, int(a["pos"]) + 1, int(b["pos"]) + 1, ref_a, alt_a or ".", ref_b, alt_b or ".", gt_a, gt_b, ps_a, ps_b,
                rr, ra, ar, aa, other, int(r["n_lowq"]), o, phase_check(a, b, o)))
            pvals.append(asj.fisher_two_sided([[rr, ra], [ar, aa]]))
    adj = asj.bh_adjust(pvals)
    return "".join([HEADER_PAIRS + "\n"] + ["%s\t%s\t%s\n" % (row, float(p), float(q)) for row, p, q in zip(rows, pvals, adj)])


def callable_gt(s, min_phase_score):
    """The GT of a site that may be part of an MNV, None for any other: not dense, one ALT, and either variant_type 1 without
    LCR_F_NON_SELECTED and with phase_score >= min_phase_score ("0|1" for haplotype 1, else "1|0"), or variant_type 2 without
    LCR_F_RNA_EDIT ("1/1") -- where the main VCF prints such a site, that is a PASS line with this GT.  (The one homozygous site it does
    not print -- selected, with phase_score >= min_phase_score -- is not callable either.)"""
    fl, vt = int(s["flags"]), int(s["variant_type"])
    if fl & _abi.F_DENSE or ref_alt(s)[1] is None:
        return None
    selected = not fl & _abi.F_NON_SELECTED
    scored = float(s["phase_score"]) >= float(min_phase_score)
    if vt == 1 and selected and scored:
        return "0|1" if int(s["haplotype"]) == 1 else "1|0"
    if vt == 2 and not fl & _abi.F_RNA_EDIT and not (selected and scored):
        return "1/1"
    return None


def mnv_records(cands, records, pair_off, refseq, region_start0, min_phase_score, max_dist=2, min_count=3, min_frac=0.8, max_partners=2):
    """Runs of adjacent calls merged into multi-nucleotide variants.  cands / records / pair_off: the candidates behind the phase stage and
    Engine.site_pairs("all", max_partners, max_dist, ...) of them.  refseq: reference bases (str, bytes or uint8 array) whose first one
    lies at the 0-based position region_start0 -- a contig's sequence with 0, or a region's with its start.
    A run is a maximal chain of callable sites (callable_gt) of one region with consecutive positions <= max_dist apart, cut from the left
    into runs of at most max_partners + 1 sites.  It is merged when it is all "1/1", or all phased hets of one phase_set != 0 with equal
    haplotype != 0, AND every pair inside it has a record with aa >= min_count and aa >= min_frac x (aa + ar + ra) (cells()).  A pair
    without a record -- further apart than max_dist -- fails.  Mixed and trans runs are not merged: the pair table shows them.
    -> [dict(pos0, ref, alt, qual, gt, ps, dp, sites, rb)]: pos0 the first site; ref the reference from the first to the last site (the
    sites' own ref_base at the sites), alt the same with the sites' ALT substituted; qual the smallest of the sites' integer QUAL; ps the
    phase set or None; dp the smallest depth; sites the 0-based positions; rb (aa, ar, ra, rr) of the outermost pair."""
    span = lambda lo, hi: (refseq[lo:hi] if isinstance(refseq, str) else bytes(bytearray(refseq[lo:hi])).decode("latin-1")).upper()
    gts = [callable_gt(s, min_phase_score) for s in cands]
    pair_at = {(int(r["a"]), int(r["b"])): r for r in records}
    runs, cur = [], []
    for i in range(len(cands)):
        if gts[i] is None:
            continue
        if cur and (int(cands["region"][i]) != int(cands["region"][cur[-1]]) or int(cands["pos"][i]) - int(cands["pos"][cur[-1]]) > max_dist):
            runs.append(cur)
            cur = []
        cur.append(i)
    if cur:
        runs.append(cur)
    out = []
    for chain in runs:
        for k in range(0, len(chain), max_partners + 1):
            run = chain[k:k + max_partners + 1]
            if len(run) < 2:
                continue
            first = cands[run[0]]
            hom = all(gts[i] == "1/1" for i in run)
            het = all(int(cands["variant_type"][i]) == 1 and int(cands["haplotype"][i]) == int(first["haplotype"]) != 0
                      and int(cands["phase_set"][i]) == int(first["phase_set"]) != 0 for i in run)
            if not (hom or het):
                continue
            ok = True
            for x in range(len(run)):
                for y in range(x + 1, len(run)):
                    r = pair_at.get((run[x], run[y]))
                    if r is None:
                        ok = False
                        continue
                    rr, ra, ar, aa, _ = cells(r, cands[run[x]], cands[run[y]])
                    ok = ok and aa >= min_count and aa >= min_frac * (aa + ar + ra)
            if not ok:
                continue
            p0, p1 = int(first["pos"]), int(cands["pos"][run[-1]])
            ref = list(span(p0 - int(region_start0), p1 + 1 - int(region_start0)))
            alt = list(ref)
            for i in run:
                ref[int(cands["pos"][i]) - p0], alt[int(cands["pos"][i]) - p0] = ref_alt(cands[i])
            rr, ra, ar, aa, _ = cells(pair_at[(run[0], run[-1])], first, cands[run[-1]])
            out.append(dict(pos0=p0, ref="".join(ref), alt="".join(alt), qual=min(vcf._as_i32(float(cands["qual"][i])) for i in run),
                            gt=gts[run[0]], ps=int(first["phase_set"]) if het and not hom else None,
                            dp=min(int(cands["depth"][i]) for i in run), sites=[int(cands["pos"][i]) for i in run], rb=(aa, ar, ra, rr)))
    return out


def format_mnv_vcf(tables, contig_order=None):
    """The MNV file's body -> (text, number of records).  tables: [(chrom, mnv_records(...))] per batch.  One PASS line per record: POS the
    first site (1-based), QUAL, INFO RDS=mnv;SITES=p1,p2[,...];RB=aa,ar,ra,rr, FORMAT GT:PS:DP (PS "." for a 1/1 record); sorted by contig
    (contig_order: names in order; default: first appearance) and position.  INFO_LINES are the header lines of its two tags."""
    order = {}
    for name in (contig_order if contig_order is not None else [x[0] for x in tables]):
        order.setdefault(name, len(order))
    lines = []
    for chrom, recs in tables:
        for m in recs:
            lines.append(((order.get(chrom, len(order)), m["pos0"]), "%s\t%d\t.\t%s\t%s\t%d\tPASS\tRDS=mnv;SITES=%s;RB=%d,%d,%d,%d\tGT:PS:DP\t%s:%s:%d\n" % (
                (chrom, m["pos0"] + 1, m["ref"], m["alt"], m["qual"], ",".join("%d" % (p + 1) for p in m["sites"])) + tuple(m["rb"])
                + (m["gt"], m["ps"] if m["ps"] is not None else ".", m["dp"]))))
    lines.sort(key=lambda x: x[0])
    return "".join(x[1] for x in lines), len(lines)

"""Host side of lcr_somatic (include/lcr.h): the fixed-point tables the driver builds, restated; the somatic score
of a record; and the VCF records of the sites it calls.

The model is the reference's calculate_prob_somatic (somatic.rs) in logs: per haplotype three hypotheses -- reference, heterozygous,
somatic at a given purity -- as sums of llround(log10(x) * 2^40) table entries over the haplotype's counted entries plus a prior.  The
record holds the six sums L[h][ref, het, som]; the score is computed here, in floating point, from the calling haplotype's three."""
import math

from . import vcf

FX = float(1 << 40)
SOM_OK, SOM_ALLELES, SOM_DEEP = 0, 1, 2
DEEP = 1 << 20       # counted entries per haplotype up to which the sums are exact
INFO_LINES = ('##INFO=<ID=SHP,Number=1,Type=Integer,Description="Haplotype carrying the somatic allele">\n'
              '##INFO=<ID=H1,Number=2,Type=Integer,Description="Counted ref,alt reads on haplotype 1">\n'
              '##INFO=<ID=H2,Number=2,Type=Integer,Description="Counted ref,alt reads on haplotype 2">\n')


def _llround(x):
    """C's llround: to nearest, halves away from zero"""
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def check_params(purity, som_rate, het_rate, min_baseq):
    """lcr_somatic's LCR_E_ARG cases as a ValueError, before any GPU work"""
    if isinstance(purity, bool) or not (purity > 0.0 and purity <= 1.0):
        raise ValueError("somatic purity must lie in (0, 1], got %r" % (purity,))
    if not (som_rate > 0.0) or not (het_rate > 0.0) or not (het_rate + som_rate < 1.0):
        raise ValueError("som_rate and het_rate must be positive and add up to less than 1, got %r and %r" % (som_rate, het_rate))
    if isinstance(min_baseq, bool) or int(min_baseq) != min_baseq or not 0 <= int(min_baseq) <= 30:
        raise ValueError("somatic min_baseq must be an integer in [0, 30] (the fragment matrix clamps qualities to 30), got %r" % (min_baseq,))


def table_arguments(purity=0.3, som_rate=5e-6, het_rate=5e-4):
    """the 124 + 3 numbers whose log10 the tables hold, in table order: fe, f1e, fs_ref, fs_alt by q = 0 .. 30 (q = 0 as q = 1), then
    the priors ref, het, som"""
    eps = [math.pow(10.0, -float(max(q, 1)) / 10.0) for q in range(31)]
    return ([e for e in eps] + [1.0 - e for e in eps] + [purity * e + (1.0 - purity) * (1.0 - e) for e in eps]
            + [purity * (1.0 - e) + (1.0 - purity) * e for e in eps], [1.0 - het_rate - som_rate, het_rate, som_rate])


def tables(purity=0.3, som_rate=5e-6, het_rate=5e-4):
    """-> dict(fe, f1e, fs_ref, fs_alt: 31 ints each; prior: [ref, het, som]) -- llround(log10(x) * 2^40), what lcr_somatic builds per call"""
    check_params(purity, som_rate, het_rate, 0)
    args, pri = table_arguments(purity, som_rate, het_rate)
    t = [_llround(math.log10(x) * FX) for x in args]
    return dict(fe=t[0:31], f1e=t[31:62], fs_ref=t[62:93], fs_alt=t[93:124], prior=[_llround(math.log10(x) * FX) for x in pri])


def score_of(l_ref, l_het, l_som):
    """SQ = -10 * (log10(10^lref + 10^lhet) - log10(10^lref + 10^lhet + 10^lsom)), l = L / 2^40: the reference's -10 log10(1 - prob_som),
    each log evaluated after subtracting the maximum of its own terms (its largest term is then 1), so that 1 - prob never cancels to 0
    and nothing underflows: finite at any depth"""
    l = [l_ref / FX, l_het / FX, l_som / FX]
    m2, m3 = max(l[0], l[1]), max(l)
    num = m2 + math.log10(math.pow(10.0, l[0] - m2) + math.pow(10.0, l[1] - m2))
    den = m3 + math.log10(math.pow(10.0, l[0] - m3) + math.pow(10.0, l[1] - m3) + math.pow(10.0, l[2] - m3))
    return -10.0 * (num - den)


def score(rec):
    """the somatic score of one lcr_somatic_site record with call != 0 (the calling haplotype's three sums); None without a call"""
    k = int(rec["call"])
    if k == 0:
        return None
    L = rec["L"][k - 1]
    return score_of(int(L[0]), int(L[1]), int(L[2]))


def format_vcf_records(cands, recs, chrom, min_score=0.0):
    """One VCF line per candidate with call != 0, in the order given (candidate order is position order within a region): QUAL the
    candidate's, FILTER PASS when SQ >= min_score else LowQual, INFO RDS=somatic;SHP=h;H1=r,a;H2=r,a, FORMAT GT:DP:AF:PS:SQ with GT
    0/1, PS "." for 0 and SQ as %.2f.  ALT is the allele that is not the reference base (status OK: one of the two is)."""
    if len(cands) != len(recs):
        raise ValueError("somatic records and candidates of %s differ in number: %d and %d" % (chrom, len(recs), len(cands)))
    out = []
    for s, r in zip(cands, recs):
        if int(r["call"]) == 0:
            continue
        ref, a1, a2 = chr(s["ref_base"]), chr(s["allele1"]), chr(s["allele2"])
        alt, af = (a1, float(s["af1"])) if a1 != ref else (a2, float(s["af2"]))
        sq = score(r)
        ps = int(r["phase_set"])
        n = r["n"]
        out.append("%s\t%d\t.\t%s\t%s\t%d\t%s\tRDS=somatic;SHP=%d;H1=%d,%d;H2=%d,%d\tGT:DP:AF:PS:SQ\t0/1:%d:%s:%s:%.2f\n" % (
            chrom, int(s["pos"]) + 1, ref, alt, vcf._as_i32(float(s["qual"])), "PASS" if sq >= min_score else "LowQual", int(r["call"]),
            int(n[0][0]), int(n[0][1]), int(n[1][0]), int(n[1][1]), int(s["depth"]), vcf._f2(af), ps if ps else ".", sq))
    return "".join(out)

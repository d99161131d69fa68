"""K19 lcr_site_pairs restated in plain Python from its contract (include/lcr.h), sharing nothing with the kernels: the pairs are listed from
the eligible candidates region by region, and a pair's joint rows are the intersection of the two sites' {row: value} maps.  Beside it the
host arithmetic of longcallr_amd/pairs.py once more: the cells, the pair table and the MNV records (the p-values come from asj's functions,
which test_asj_host pins)."""
import numpy as np

from longcallr_amd import _abi, asj, vcf


def eligible(cands, mode):
    out = []
    for i in range(len(cands)):
        ok = not int(cands["flags"][i]) & _abi.F_DENSE
        if mode == "phased":
            ok = ok and int(cands["variant_type"][i]) == 1 and int(cands["haplotype"][i]) != 0 and int(cands["phase_set"][i]) != 0
        if ok:
            out.append(i)
    return out


def pair_list(cands, mode, K, D):
    """[(a, b)] ordered by a, then b"""
    by_region = {}
    for i in eligible(cands, mode):
        by_region.setdefault(int(cands["region"][i]), []).append(i)
    out = []
    for g in sorted(by_region):
        e = by_region[g]
        for i in range(len(e)):
            for k in range(1, K + 1):
                if i + k < len(e) and (D == 0 or int(cands["pos"][e[i + k]]) - int(cands["pos"][e[i]]) <= D):
                    out.append((e[i], e[i + k]))
    return sorted(out)


def site_pairs(row_ptr, col, val, cands, mode, K, D, q):
    """-> (records of _abi.SITE_PAIR_DTYPE, pair_off, n_eligible)"""
    at = [dict() for _ in range(len(cands))]
    for r in range(len(row_ptr) - 1):
        for e in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            at[int(col[e])][r] = int(val[e])
    pl = pair_list(cands, mode, K, D)
    rec = np.zeros(len(pl), dtype=_abi.SITE_PAIR_DTYPE)
    off = np.zeros(len(cands) + 1, np.int32)
    for k, (a, b) in enumerate(pl):
        rec["a"][k], rec["b"][k] = a, b
        off[a + 1] += 1
        for r in sorted(set(at[a]) & set(at[b])):
            va, vb = at[a][r], at[b][r]
            rec["n_rows"][k] += 1
            if (va & 31) < q or (vb & 31) < q:
                rec["n_lowq"][k] += 1
            else:
                rec["n"][k][va >> 6][vb >> 6] += 1
    return rec, np.cumsum(off, dtype=np.int32), len(eligible(cands, mode))


def of_engine(fm, cands, mode, K, D, q):
    return site_pairs(fm["row_ptr"], fm["col"], fm["val"], cands, mode, K, D, q)


# ---- the host arithmetic ----------------------------------------------------------------------------------------------------------------
def printed_alt(s):
    """the ALT letter of the site's line in the main VCF when that line has one ALT, else None"""
    r = chr(int(s["ref_base"]))
    for x in (chr(int(s["allele1"])), chr(int(s["allele2"]))):
        if x != r:
            return x.upper()
    return None


def cells(rec, ca, cb):
    cls = []
    for s in (ca, cb):
        ref, alt = chr(int(s["ref_base"])).upper(), printed_alt(s)
        cls.append(["r" if x == ref else "a" if x == alt else "o" for x in "ACGT"])
    t = dict(rr=0, ra=0, ar=0, aa=0, other=0)
    for x in range(4):
        for y in range(4):
            key = cls[0][x] + cls[1][y]
            t[key if key in t else "other"] += int(rec["n"][x][y])
    return t["rr"], t["ra"], t["ar"], t["aa"], t["other"]


def vcf_fields(s, chrom, min_ps):
    line = vcf.format_records(np.asarray(s).reshape(1), chrom, min_ps)
    return line.rstrip("\n").split("\t") if line else None


def format_pairs_tsv(tables, min_count, min_ps):
    head = ["#Chrom", "Pos_a", "Pos_b", "Ref_a", "Alt_a", "Ref_b", "Alt_b", "GT_a", "GT_b", "PS_a", "PS_b", "n_rr", "n_ra", "n_ar", "n_aa", "n_other",
            "n_lowq", "Orientation", "Phase", "P_value", "P_adj"]
    rows, ps = [], []
    for chrom, cands, recs in tables:
        for r in recs:
            a, b = cands[int(r["a"])], cands[int(r["b"])]
            rr, ra, ar, aa, other = cells(r, a, b)
            if rr + ra + ar + aa + other < min_count:
                continue
            same, cross = rr + aa, ra + ar
            o = "tie" if same == cross else "cis" if same > cross else "trans"
            phased = all(int(s["variant_type"]) == 1 and int(s["haplotype"]) != 0 and int(s["phase_set"]) != 0 for s in (a, b))
            verdict = "."
            if phased and int(a["phase_set"]) == int(b["phase_set"]) and o != "tie":
                want = "cis" if int(a["haplotype"]) == int(b["haplotype"]) else "trans"
                verdict = "agree" if o == want else "disagree"
            f = []
            for s in (a, b):
                v = vcf_fields(s, chrom, min_ps)
                f.append((chr(int(s["ref_base"])).upper(), printed_alt(s) or ".", v[9].split(":")[0] if v else ".", str(int(s["phase_set"]) or ".")))
            rows.append([chrom, int(a["pos"]) + 1, int(b["pos"]) + 1, f[0][0], f[0][1], f[1][0], f[1][1], f[0][2], f[1][2], f[0][3], f[1][3],
                         rr, ra, ar, aa, other, int(r["n_lowq"]), o, verdict])
            ps.append(asj.fisher_two_sided([[rr, ra], [ar, aa]]))
    adj = asj.bh_adjust(ps)
    return "\t".join(head) + "\n" + "".join("\t".join(str(x) for x in row + [float(p), float(q)]) + "\n" for row, p, q in zip(rows, ps, adj))


def vcf_callable(s, chrom, min_ps):
    """the GT of the site's line in the main VCF when that line is PASS with GT 0|1, 1|0 or 1/1 and one ALT, else None"""
    v = vcf_fields(s, chrom, min_ps)
    if v is None or v[6] != "PASS" or "," in v[4]:
        return None
    gt = v[9].split(":")[0]
    return gt if gt in ("0|1", "1|0", "1/1") else None


def mnv_records(cands, records, pair_off, refseq, region_start0, min_ps, max_dist=2, min_count=3, min_frac=0.8, K=2):
    """-> [(pos0, REF, ALT, QUAL, GT, PS or None, DP, [pos0 of the sites], (aa, ar, ra, rr))]; a site is callable by its own line in the
    main VCF (vcf_callable): the restatement goes through the writer, pairs.py through the fields"""
    gt = {i: vcf_callable(cands[i], "c", min_ps) for i in range(len(cands))}
    sites = [i for i in range(len(cands)) if gt[i] is not None and not int(cands["flags"][i]) & _abi.F_DENSE]
    chains = []
    for i in sites:
        if chains and int(cands["region"][chains[-1][-1]]) == int(cands["region"][i]) and int(cands["pos"][i]) - int(cands["pos"][chains[-1][-1]]) <= max_dist:
            chains[-1].append(i)
        else:
            chains.append([i])
    rec_of = {(int(r["a"]), int(r["b"])): r for r in records}
    out = []
    for ch in chains:
        while len(ch) >= 2:
            run, ch = ch[:K + 1], ch[K + 1:]
            if len(run) < 2:
                break
            kinds = {gt[i] for i in run}
            if kinds == {"1/1"}:
                ps = None
            elif len(kinds) == 1 and "1/1" not in kinds and len({int(cands["phase_set"][i]) for i in run}) == 1 and int(cands["phase_set"][run[0]]) != 0 \
                    and len({int(cands["haplotype"][i]) for i in run}) == 1 and int(cands["haplotype"][run[0]]) != 0:
                ps = int(cands["phase_set"][run[0]])
            else:
                continue
            good = True
            for x in range(len(run)):
                for y in range(x + 1, len(run)):
                    r = rec_of.get((run[x], run[y]))
                    if r is None:
                        good = False
                        continue
                    rr, ra, ar, aa, _ = cells(r, cands[run[x]], cands[run[y]])
                    if aa < min_count or aa < min_frac * (aa + ar + ra):
                        good = False
            if not good:
                continue
            p0, p1 = int(cands["pos"][run[0]]), int(cands["pos"][run[-1]])
            ref = [chr(c).upper() if not isinstance(c, str) else c.upper() for c in refseq[p0 - region_start0:p1 + 1 - region_start0]]
            alt = list(ref)
            for i in run:
                ref[int(cands["pos"][i]) - p0] = chr(int(cands["ref_base"][i])).upper()
                alt[int(cands["pos"][i]) - p0] = printed_alt(cands[i])
            rr, ra, ar, aa, _ = cells(rec_of[(run[0], run[-1])], cands[run[0]], cands[run[-1]])
            out.append((p0, "".join(ref), "".join(alt), min(vcf._as_i32(float(cands["qual"][i])) for i in run), gt[run[0]], ps,
                        min(int(cands["depth"][i]) for i in run), [int(cands["pos"][i]) for i in run], (aa, ar, ra, rr)))
    return out

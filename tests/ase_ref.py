"""The contract of lcr_ase (include/lcr.h, DESIGN.md "Allele-specific expression") restated loop for loop in plain Python with dicts: the
counting of allele_specific/longcallR-ase.py's calculate_ase_pvalue and the vote loops of calculate_ase_pvalue_pat_mat, per region
instead of per gene.  Its inputs are the engine's own outputs (rows, assignment, phase set, the fragment matrix, the candidate
records); whether a candidate is a PASS record with a phased het GT is read off the VCF line the writer prints for it.  The one stated
difference from the script: equally large phase sets go to the smallest value.  This is the yardstick of the GPU tests."""
import numpy as np

from longcallr_amd import _abi, vcf


def pass_phased_het(cand, min_phase_score):
    """the candidate's VCF record is PASS with GT 0|1 / 1|0 (load_longcallR_phased_vcf's test on the writer's own text)"""
    text = vcf.format_records(cand, "c", min_phase_score)
    if not text:
        return False
    f = text.rstrip("\n").split("\t")
    return f[6] == "PASS" and f[9].split(":")[0] in ("0|1", "1|0")


def regions(fm, assignment, phase_set, cands, cand_off, parental=None, min_baseq=13, min_phase_score=0.0):
    """fm: Engine.fragmat(); parental: {pos0: (pat, mat)} as one-letter strings, or None (plain mode) -> records as _abi.ASE_DTYPE"""
    rro, row_ptr, col, val = fm["row_region_off"], fm["row_ptr"], fm["col"], fm["val"]
    out = []
    for g in range(len(rro) - 1):
        rows = range(int(rro[g]), int(rro[g + 1]))
        phase_set_hap_count = {}
        for r in rows:
            ps, hp = int(phase_set[r]), int(assignment[r])
            if ps and hp in (1, 2):
                phase_set_hap_count.setdefault(ps, {1: 0, 2: 0})[hp] += 1
        most = 0
        for ps in sorted(phase_set_hap_count):
            c = phase_set_hap_count[ps]
            if most == 0 or c[1] + c[2] > phase_set_hap_count[most][1] + phase_set_hap_count[most][2]:
                most = ps
        rec = dict(region=g, phase_set=most, n_phase_sets=len(phase_set_hap_count), h1=0, h2=0, n_sites=0, h1_pat=0, h1_mat=0, h2_pat=0, h2_mat=0)
        if most:
            rec["h1"], rec["h2"] = phase_set_hap_count[most][1], phase_set_hap_count[most][2]
        if most and parental:
            site = {}    # candidate index -> (pat, mat)
            for i in range(int(cand_off[g]), int(cand_off[g + 1])):
                s = cands[i:i + 1]
                if int(s["phase_set"][0]) == most and pass_phased_het(s, min_phase_score) and int(s["pos"][0]) in parental:
                    site[i] = parental[int(s["pos"][0])]
            rec["n_sites"] = len(site)
            reads_pat_mat_cnt = {}
            for r in rows:
                if int(phase_set[r]) != most or int(assignment[r]) not in (1, 2):
                    continue
                for e in range(int(row_ptr[r]), int(row_ptr[r + 1])):
                    i, v = int(col[e]), int(val[e])
                    if i not in site or (v & 31) < min_baseq:
                        continue
                    base = "ACGT"[v >> 6]
                    cnt = reads_pat_mat_cnt.setdefault(r, {"pat": 0, "mat": 0})
                    if base == site[i][0]:
                        cnt["pat"] += 1
                    elif base == site[i][1]:
                        cnt["mat"] += 1
            for r, cnt in reads_pat_mat_cnt.items():
                h = "h%d" % int(assignment[r])
                if cnt["pat"] > cnt["mat"]:
                    rec[h + "_pat"] += 1
                elif cnt["pat"] < cnt["mat"]:
                    rec[h + "_mat"] += 1
        out.append(tuple(rec[f] for f in _abi.ASE_DTYPE.names))
    return np.array(out, dtype=_abi.ASE_DTYPE)

"""The contract of lcr_site_counts (include/lcr.h) restated loop for loop in plain Python with dicts: per candidate
the entries of the fragment matrix at it, from any row, counted by base and by the haplotype of the row.  Its inputs are the engine's own
outputs -- the fragment matrix, the per-row assignment and phase set, the candidates' own phase sets --, nothing is vectorised.  This is
the yardstick of the GPU tests (tests/test_site_counts_gpu.py), and format_rows below restates ase.format_sites_tsv's table rows."""
import numpy as np

from longcallr_amd import _abi, ase, asj, vcf


def site_counts(row_ptr, col, val, assignment, phase_set, cand_phase_set, min_baseq=13):
    """row_ptr / col / val: the CSR of Engine.fragmat(); assignment / phase_set: per row; cand_phase_set: per candidate (its length is the
    number of candidates) -> records as _abi.SITE_COUNT_DTYPE, one per candidate"""
    n_cand = len(cand_phase_set)
    entries = [[] for _ in range(n_cand)]       # per candidate: (row, value byte) of every entry at it
    for r in range(len(row_ptr) - 1):
        for e in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            entries[int(col[e])].append((r, int(val[e])))
    out = np.zeros(n_cand, dtype=_abi.SITE_COUNT_DTYPE)
    for c in range(n_cand):
        n_lowq = 0
        counted = []                            # (counting row?, its phase set, its assignment, base code)
        for r, v in entries[c]:
            if (v & 31) < min_baseq:
                n_lowq += 1
                continue
            a, ps = int(assignment[r]), int(phase_set[r])
            counted.append((a in (1, 2) and ps != 0, ps, a, v >> 6))
        per_set = {}
        for counting, ps, _, _ in counted:
            if counting:
                per_set[ps] = per_set.get(ps, 0) + 1
        own = int(cand_phase_set[c])
        site_ps = own
        if own == 0:
            for ps in sorted(per_set):          # most entries; a strict > keeps the smallest value
                if site_ps == 0 or per_set[ps] > per_set[site_ps]:
                    site_ps = ps
        n = [[0] * 4 for _ in range(3)]
        for counting, ps, a, b in counted:
            k = a if counting and ps == site_ps else 0
            n[k][b] += 1
        out[c] = (site_ps, len(per_set), len(entries[c]), n_lowq, n)
    return out


def of_engine(fm, pr, cands, min_baseq=13):
    """site_counts on Engine.fragmat(), Engine.phase_result() and the candidate records behind the phase stage"""
    return site_counts(fm["row_ptr"], fm["col"], fm["val"], pr["assignment"], pr["phase_set"], cands["phase_set"], min_baseq)


def format_rows(tables, min_support, overdispersion, min_phase_score):
    """ase.format_sites_tsv's text, restated: per candidate the writer's own line, the cells of the upper-cased reference base against
    the other three, the two tests of the existing functions, Benjamini-Hochberg over all written rows per column"""
    rows, p_ase, p_hap = [], [], []
    for chrom, cands, recs in tables:
        for i in range(len(cands)):
            line = vcf.format_records(cands[i:i + 1], chrom, min_phase_score)
            if not line:
                continue
            f = line.rstrip("\n").split("\t")
            ref_code = "ACGT".find(chr(int(cands["ref_base"][i])).upper())
            cell = []
            for k in (1, 2, 0):
                n = [int(x) for x in recs["n"][i][k]]
                r = n[ref_code] if ref_code >= 0 else 0
                cell += [r, sum(n) - r]
            if cell[0] + cell[1] + cell[2] + cell[3] < min_support:
                continue
            ps = int(recs["phase_set"][i])
            rows.append("\t".join([f[0], f[1], f[3], f[4], f[6], f[9].split(":")[0], str(ps) if ps else "."] + [str(x) for x in cell]))
            p_ase.append(ase.betabinom_two_sided(cell[1] + cell[3], sum(cell[:4]), 0.5, overdispersion))
            p_hap.append(asj.fisher_two_sided([[cell[0], cell[1]], [cell[2], cell[3]]]))
    a_ase, a_hap = asj.bh_adjust(p_ase), asj.bh_adjust(p_hap)
    out = [ase.HEADER_SITES + "\n"]
    for r, p1, q1, p2, q2 in zip(rows, p_ase, a_ase, p_hap, a_hap):
        out.append("%s\t%s\t%s\t%s\t%s\n" % (r, float(p1), float(q1), float(p2), float(q2)))
    return "".join(out)

"""The contract of lcr_junctions (include/lcr.h, DESIGN.md "Allele-specific junctions") restated loop for loop in plain Python: the
haplotype x junction table that allele_specific/longcallR-asj.py builds per gene, per region here.  No vectorisation, no
shortcuts: this is the yardstick of the GPU tests, fed with the GPU's own phasing results (assignment, phase_set)."""
import numpy as np

from longcallr_amd import _abi

REF_CONSUMING = (0, 2, 3, 7, 8)   # M D N = X


def read_junctions(batch, i):
    """([(s, l)] of the read's N ops of length >= 1, rend): s = 0-based contig column of the first skipped base"""
    pos = int(batch.pos[i])
    c0 = int(batch.cig_off[i])
    out = []
    for k in range(int(batch.n_cig[i])):
        w = int(batch.cigar[c0 + k])
        op, ln = w & 15, w >> 4
        if op == 3 and ln >= 1:
            out.append((pos, ln))
        if op in REF_CONSUMING:
            pos += ln
    return out, pos


def junctions(batch, row_region_off, row_read, assignment, phase_set, min_count=10, min_junctions=2):
    """-> (records as _abi.JUNC_DTYPE, junc_region_off)"""
    recs, off = [], [0]
    for g in range(batch.n_regions):
        rows = []     # participating rows: (pos, rend, hap, ps, junctions)
        for r in range(int(row_region_off[g]), int(row_region_off[g + 1])):
            a = int(assignment[r])
            if a not in (1, 2):
                continue
            i = int(row_read[r])
            js, rend = read_junctions(batch, i)
            if not len(js) > min_junctions:
                continue
            rows.append((int(batch.pos[i]), rend, a, int(phase_set[r]), js))
        n_reads = {}
        for _, _, _, _, js in rows:
            for j in set(js):
                n_reads[j] = n_reads.get(j, 0) + 1
        start0, length = int(batch.start0[g]), int(batch.len[g])
        win = bytes(batch.ref[int(batch.col_off[g]):int(batch.col_off[g + 1])]).upper()
        for (s, l) in sorted(n_reads):
            if n_reads[(s, l)] < min_count:
                continue
            per_ps = {}   # ps -> [h1_absent, h1_present, h2_absent, h2_present]
            for pos, rend, a, ps, js in rows:
                if not (pos < s + l and rend > s):
                    continue
                present = 1 if (s, l) in js else 0
                per_ps.setdefault(ps, [0, 0, 0, 0])[(a - 1) * 2 + present] += 1
            best = None
            for ps in sorted(per_ps):
                if best is None or sum(per_ps[ps]) > sum(per_ps[best]):
                    best = ps
            motif = 0
            sl = s - start0
            if l >= 2 and sl >= 0 and sl + l <= length:
                pair = (win[sl:sl + 2], win[sl + l - 2:sl + l])
                motif = 1 if pair == (b"GT", b"AG") else 2 if pair == (b"CT", b"AC") else 0
            cells = per_ps[best] if best is not None else [0, 0, 0, 0]
            recs.append((g, motif, [0, 0, 0], s, l, n_reads[(s, l)], best or 0, len(per_ps)) + tuple(cells))
        off.append(len(recs))
    return np.array(recs, dtype=_abi.JUNC_DTYPE), np.array(off, dtype=np.int32)

"""The contract of lcr_intron_retention (include/lcr.h) restated in plain Python from its text: the haplotype x
{spliced, retained} table per kept intron and region.  Loops over regions, rows and introns, lists of blocks and junctions per read, dicts
keyed by Python ints, no vectorisation and no hashing of anything but Python's own keys: this is the yardstick of the GPU tests, fed with
the GPU's own phasing results (assignment, phase_set)."""
import numpy as np

from longcallr_amd import _abi

COVERING = (0, 2, 7, 8)   # M D = X: they cover and extend the current block


def read_structure(batch, i):
    """-> (pos, rend, junctions [(s, l)], aligned blocks [(bs, be)]) of read i: an N op of length >= 1 is a junction and ends the block;
    I, S, H, P and zero-length ops change nothing"""
    pos = cur = bs = int(batch.pos[i])
    c0 = int(batch.cig_off[i])
    junc, blocks = [], []
    for k in range(int(batch.n_cig[i])):
        w = int(batch.cigar[c0 + k])
        op, n = w & 15, w >> 4
        if n == 0:
            continue
        if op in COVERING:
            cur += n
        elif op == 3:
            blocks.append((bs, cur))
            junc.append((cur, n))
            cur += n
            bs = cur
    blocks.append((bs, cur))
    return pos, cur, junc, blocks


def classify(row, s, l, a):
    """the class of a participating row at the intron [s, s + l) with anchor a: None (no overlap), "S", "R" or "O"; SPLICED is asked first"""
    pos, rend, junc, blocks = row
    e = s + l
    if not (pos < e and rend > s):
        return None
    if (s, l) in junc:
        return "S"
    if s - a >= 0 and any(bs <= s - a and be >= e + a for bs, be in blocks):
        return "R"
    return "O"


def intron_retention(batch, row_region_off, row_read, assignment, phase_set, min_count=10, anchor=10):
    """-> (records as _abi.RETAINED_INTRON_DTYPE, intron_region_off, row_retained, totals {n_part, n_retained})"""
    if anchor > 4096:
        raise ValueError("LCR_E_ARG")
    min_count = max(int(min_count), 1)
    a = int(anchor)
    n_rows = int(row_region_off[batch.n_regions])
    recs, off = [], [0]
    row_retained = [0] * n_rows
    n_part = 0
    for g in range(batch.n_regions):
        rows = []     # participating rows: (row, hap, ps, (pos, rend, junctions, blocks))
        for r in range(int(row_region_off[g]), int(row_region_off[g + 1])):
            hap = int(assignment[r])
            if hap not in (1, 2):
                continue
            rows.append((r, hap, int(phase_set[r]), read_structure(batch, int(row_read[r]))))
        n_part += len(rows)
        n_spliced = {}
        for _, _, _, st in rows:
            for j in st[2]:
                n_spliced[j] = n_spliced.get(j, 0) + 1
        for s, l in sorted(j for j, n in n_spliced.items() if n >= min_count):
            n = dict(S=0, R=0, O=0)
            per_ps = {}   # ps -> [h1_spliced, h1_retained, h2_spliced, h2_retained]
            for r, hap, ps, st in rows:
                cls = classify(st, s, l, a)
                if cls is None:
                    continue
                n[cls] += 1
                if cls == "R":
                    row_retained[r] += 1
                if cls != "O":
                    per_ps.setdefault(ps, [0, 0, 0, 0])[(hap - 1) * 2 + (cls == "R")] += 1
            best = None
            for ps in sorted(per_ps):
                if best is None or sum(per_ps[ps]) > sum(per_ps[best]):
                    best = ps
            recs.append((g, motif(batch, g, s, l), 0, s, l, n["S"], n["R"], n["O"], best or 0, len(per_ps)) + tuple(per_ps[best]))
        off.append(len(recs))
    return (np.array(recs, dtype=_abi.RETAINED_INTRON_DTYPE), np.array(off, dtype=np.int32), np.array(row_retained, dtype=np.int32),
            dict(n_part=n_part, n_retained=sum(row_retained)))


def motif(batch, g, s, l):
    """lcr_junctions' motif of the junction [s, s + l) on the window's reference, either case: 1 = GT-AG, 2 = CT-AC, 0 = neither or not
    inside the window"""
    sl = s - int(batch.start0[g])
    if not (l >= 2 and sl >= 0 and sl + l <= int(batch.len[g])):
        return 0
    w = bytes(batch.ref[int(batch.col_off[g]):int(batch.col_off[g]) + int(batch.len[g])]).upper()
    ends = w[sl:sl + 2] + w[sl + l - 2:sl + l]
    return 1 if ends == b"GTAG" else 2 if ends == b"CTAC" else 0

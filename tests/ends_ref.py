"""The contract of lcr_transcript_ends (include/lcr.h) restated in plain Python from its text: the haplotype x
transcript-end site table per region.  Loops over rows and coordinates, dicts keyed by Python ints, no vectorisation and no hashing of
anything but Python's own keys: this is the yardstick of the GPU tests, fed with the GPU's own phasing results (assignment, phase_set)."""
import numpy as np

from longcallr_amd import _abi

REF_CONSUMING = (0, 2, 3, 7, 8)   # M D N = X


def read_rend(batch, i):
    """pos + the lengths of all M, D, N, = and X ops: exclusive"""
    pos = int(batch.pos[i])
    c0 = int(batch.cig_off[i])
    for k in range(int(batch.n_cig[i])):
        w = int(batch.cigar[c0 + k])
        if (w & 15) in REF_CONSUMING:
            pos += w >> 4
    return pos


def strand(flags, mode):
    """transcript strand of a read: 1 = '+', 2 = '-', 0 = none.  mode "ts": the ts tag alone; "read": the read's own strand without one"""
    rev, ts = flags & 1, (flags >> 1) & 3
    if ts == 1:
        return 2 if rev else 1
    if ts == 2:
        return 1 if rev else 2
    if mode == "read":
        return 2 if rev else 1
    return 0


def transcript_ends(batch, row_region_off, row_read, assignment, phase_set, min_count=10, window=10, mode="ts"):
    """-> (records as _abi.END_SITE_DTYPE, site_region_off, row_site as an (n_rows, 2) array, totals {n_part, n_assigned})"""
    if window > 4096 or mode not in ("ts", "read"):
        raise ValueError("LCR_E_ARG")
    min_count = max(int(min_count), 1)
    W = int(window)
    n_rows = int(row_region_off[batch.n_regions])
    recs, off = [], [0]
    row_site = [[-1, -1] for _ in range(n_rows)]
    n_part = n_assigned = 0
    for g in range(batch.n_regions):
        rows = []     # participating rows: (row, pos, rend, hap, ps, strand)
        for r in range(int(row_region_off[g]), int(row_region_off[g + 1])):
            a = int(assignment[r])
            i = int(row_read[r])
            t = strand(int(batch.flags[i]), mode)
            if a not in (1, 2) or t == 0:
                continue
            rows.append((r, int(batch.pos[i]), read_rend(batch, i), a, int(phase_set[r]), t))
        n_part += len(rows)
        end = lambda row, d: row[1] if d == 0 else row[2] - 1
        sites = []    # (p, t, d, assigned rows)
        target = {}   # (row, d) -> (p, t, d)
        for t in (1, 2):
            for d in (0, 1):
                c = {}
                for row in rows:
                    if row[5] == t:
                        c[end(row, d)] = c.get(end(row, d), 0) + 1
                peaks = set()
                for x in c:
                    ok = True
                    for y in (c if len(c) <= 2 * W + 1 else range(x - W, x + W + 1)):     # (the shorter of two loops over the same y's)
                        if y != x and y in c and abs(y - x) <= W and not (c[x] > c[y] or (c[x] == c[y] and x < y)):
                            ok = False
                    if ok:
                        peaks.add(x)
                held = {p: [] for p in peaks}
                for row in rows:
                    if row[5] != t:
                        continue
                    x = end(row, d)
                    for k in range(W + 1):       # the nearest peak, the smaller coordinate first
                        if x - k in peaks:
                            held[x - k].append(row)
                            break
                        if x + k in peaks:
                            held[x + k].append(row)
                            break
                for p in peaks:
                    if len(held[p]) >= min_count:
                        sites.append((p, t, d, held[p], c[p]))
        sites.sort(key=lambda s: s[:3])
        for p, t, d, held, n_peak in sites:
            j = len(recs)
            present = set(row[0] for row in held)
            for row in held:
                row_site[row[0]][d] = j
            n_assigned += len(held)
            per_ps = {}   # ps -> [h1_absent, h1_present, h2_absent, h2_present]
            for r, pos, rend, hap, ps, ts in rows:
                if pos > p + W + 1:   # (rows come in the order of pos: from here on both ends lie right of the window, and nothing covers it)
                    break
                if ts != t:
                    continue
                if r in present:
                    pres = 1
                elif p - W >= 0 and pos <= p - W and rend >= p + W + 1:
                    pres = 0
                else:
                    continue
                per_ps.setdefault(ps, [0, 0, 0, 0])[(hap - 1) * 2 + pres] += 1
            best = None
            for ps in sorted(per_ps):
                if best is None or sum(per_ps[ps]) > sum(per_ps[best]):
                    best = ps
            cells = per_ps[best] if best is not None else [0, 0, 0, 0]
            xs = [end(row, d) for row in held]
            kind = 0 if (t == 1) == (d == 0) else 1
            recs.append((g, t, d, kind, 0, p, min(xs), max(xs), len(held), sum(1 for x in held if x[3] == 1), sum(1 for x in held if x[3] == 2),
                         n_peak, best or 0, len(per_ps)) + tuple(cells))
        off.append(len(recs))
    return (np.array(recs, dtype=_abi.END_SITE_DTYPE), np.array(off, dtype=np.int32), np.array(row_site, dtype=np.int32).reshape(-1, 2),
            dict(n_part=n_part, n_assigned=n_assigned))

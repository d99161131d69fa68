"""The contract of lcr_indels (include/lcr.h) restated in plain Python from its text: the phased small-indel records
per region.  Loops over regions, rows, gaps and events, Python strings for the reference and the inserted bases, dicts keyed by Python
tuples, no vectorisation and no hashing of anything but Python's own keys: this is the yardstick of the GPU tests, fed with the GPU's own
phasing results (assignment, phase_set).  It shares no code with the library."""
import numpy as np

from longcallr_amd import _abi

COVERING = (0, 2, 7, 8)     # M D = X: they cover and extend the current block
QUERY = (0, 1, 4, 7, 8)     # M I S = X consume the read's bases
ACGT = "ACGT"
MAX_SHIFT = 1024


def read_gaps(batch, i):
    """-> (pos, rend, gaps [(op, s, L, inserted bases or None)], aligned blocks [(bs, be)]) of read i.  Every I, D and N op of length >= 1
    is a gap, but an I or D with s <= pos or s + Lr >= rend is dropped."""
    pos = cur = bs = int(batch.pos[i])
    c0 = int(batch.cig_off[i])
    q = int(batch.seq_off[i])
    raw, blocks = [], []
    for k in range(int(batch.n_cig[i])):
        w = int(batch.cigar[c0 + k])
        op, n = w & 15, w >> 4
        if n == 0:
            continue
        if op == 1:
            raw.append((1, cur, n, bytes(batch.bases[q:q + n]).decode("latin-1")))
        elif op == 2:
            raw.append((2, cur, n, None))
        elif op == 3:
            blocks.append((bs, cur))
            raw.append((3, cur, n, None))
            bs = cur + n
        if op in COVERING or op == 3:
            cur += n
        if op in QUERY:
            q += n
    blocks.append((bs, cur))
    rend = cur
    gaps = [(op, s, n, ins) for op, s, n, ins in raw if op == 3 or (s > pos and s + (0 if op == 1 else n) < rend)]
    return pos, rend, gaps, blocks


def left_shift(ref, w0, typ, s, L, q):
    """ref: the window's reference in upper case, ref[0] = column w0 -> (s_left, rotated q)"""
    steps = 0
    while s > w0 + 1 and steps < MAX_SHIFT:
        a = ref[s - 1 - w0]
        if a not in ACGT:
            break
        if typ == 0:
            if a != ref[s + L - 1 - w0]:
                break
        else:
            if a != q[L - 1]:
                break
            q = a + q[:L - 1]
        s -= 1
        steps += 1
    return s, q


def right_shift(ref, w0, w1, typ, s, L, q):
    steps = 0
    while steps < MAX_SHIFT:
        if typ == 0:
            if not s + L < w1:
                break
            a = ref[s - w0]
            if a not in ACGT or a != ref[s + L - w0]:
                break
        else:
            if not s < w1:
                break
            a = ref[s - w0]
            if a not in ACGT or a != q[0]:
                break
            q = q[1:] + a
        s += 1
        steps += 1
    return s


def pack(q):
    v = 0
    for k, ch in enumerate(q):
        v |= ACGT.index(ch) << (2 * k)
    return v


def event_of(gap, ref, w0, w1, max_ins, max_del):
    """the gap's event as (key, s_left, type, L, rotated q) or None.  key = (s_left, type, payload): a tuple that orders like the 64-bit key"""
    op, s, L, ins = gap
    if op == 2:
        if not (L <= max_del and s >= w0 + 1 and s + L <= w1):
            return None
        sl, _ = left_shift(ref, w0, 0, s, L, None)
        return (sl, 0, L), sl, 0, L, ""
    if op == 1:
        if not (L <= max_ins and s >= w0 + 1 and s <= w1):
            return None
        q = ins.upper()
        if len(q) != L or any(ch not in ACGT for ch in q):
            return None
        sl, q = left_shift(ref, w0, 1, s, L, q)
        return (sl, 1, (L << 24) | pack(q)), sl, 1, L, q
    return None


def classify(row, key, lo_f, hi_f):
    """the class of a participating row at a kept event: None (not looked at), "P", "A" or "O"; PRESENT is asked first"""
    pos, rend, gaps, events = row
    if not (pos < hi_f and rend > lo_f):
        return None
    if key in events:
        return "P"
    touched = False
    for op, s, L, _ in gaps:
        if op == 1:
            touched |= lo_f <= s <= hi_f
        else:
            touched |= s <= hi_f and s + L >= lo_f
    if pos <= lo_f and rend >= hi_f and not touched:
        return "A"
    return "O"


def indels(batch, row_region_off, row_read, assignment, phase_set, min_count=10, min_permille=150, flank=5, max_ins=12, max_del=50, classes=None):
    """-> (records as _abi.INDEL_DTYPE, indel_region_off, row_indels, totals {n_part, n_events, n_present}).  classes: a dict that, when
    given, receives {(region, key): [class of every looked-at row]}"""
    if flank > 4096 or max_ins > 12 or max_del > 65535:
        raise ValueError("LCR_E_ARG")
    min_count = max(int(min_count), 1)
    n_rows = int(row_region_off[batch.n_regions])
    recs, off = [], [0]
    row_indels = [0] * n_rows
    n_part = n_events = 0
    for g in range(batch.n_regions):
        w0, wlen = int(batch.start0[g]), int(batch.len[g])
        w1 = w0 + wlen
        c0 = int(batch.col_off[g])
        ref = bytes(batch.ref[c0:c0 + wlen]).decode("latin-1").upper()
        rows = []     # participating rows: (row, hap, ps, (pos, rend, gaps, event keys), blocks)
        info = {}     # key -> (s_left, type, L, q)
        for r in range(int(row_region_off[g]), int(row_region_off[g + 1])):
            pos, rend, gaps, blocks = read_gaps(batch, int(row_read[r]))
            keys = []
            for gp in gaps:
                ev = event_of(gp, ref, w0, w1, max_ins, max_del)
                if ev is not None:
                    keys.append(ev[0])
                    info[ev[0]] = ev[1:]
            n_events += len(keys)
            rows.append((r, int(assignment[r]), int(phase_set[r]), (pos, rend, gaps, keys), blocks))
        n_part += len(rows)

        def depth(x):
            return sum(1 for row in rows if any(bs <= x < be for bs, be in row[4]))

        cnt = {}
        for row in rows:
            for key in set(row[3][3]):        # a row holds a key once
                cnt[key] = cnt.get(key, 0) + 1
        for key in sorted(cnt):
            sl, typ, L, q = info[key]
            d = depth(sl - 1)
            if not (cnt[key] >= min_count and cnt[key] * 1000 >= min_permille * d):
                continue
            sr = right_shift(ref, w0, w1, typ, sl, L, q)
            lo, hi = sl, (sr + L if typ == 0 else sr)
            lo_f, hi_f = lo - flank, hi + flank
            n = dict(P=0, A=0, O=0)
            per_ps = {}   # ps -> [h1_present, h1_absent, h2_present, h2_absent]
            seen = []
            for r, hap, ps, st, _ in rows:
                cls = classify(st, key, lo_f, hi_f)
                if cls is None:
                    continue
                seen.append(cls)
                n[cls] += 1
                if cls == "P":
                    row_indels[r] += 1
                if cls != "O" and hap in (1, 2):
                    per_ps.setdefault(ps, [0, 0, 0, 0])[(hap - 1) * 2 + (cls == "A")] += 1
            if classes is not None:
                classes[(g, key)] = seen
            best = None
            for ps in sorted(per_ps):
                if best is None or sum(per_ps[ps]) > sum(per_ps[best]):
                    best = ps
            hrun = 0
            while hrun < 255 and sl + hrun < w1 and ref[sl + hrun - w0] == ref[sl - w0]:
                hrun += 1
            cells = tuple(per_ps[best]) if best is not None else (0, 0, 0, 0)
            recs.append((g, typ, hrun, sr - sl, sl, L, pack(q) if typ else 0, d, n["P"], n["A"], n["O"], best or 0, len(per_ps)) + cells)
        off.append(len(recs))
    return (np.array(recs, dtype=_abi.INDEL_DTYPE), np.array(off, dtype=np.int32), np.array(row_indels, dtype=np.int32),
            dict(n_part=n_part, n_events=n_events, n_present=sum(row_indels)))

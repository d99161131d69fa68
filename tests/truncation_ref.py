"""find_isolated_regions_with_depth (reference src/util.rs:236-332) restated loop for loop, with both of its switches
(`truncation`, `truncation_coverage`): spans -> depth -> the column loop.  Written from the Rust text and independent of
longcallr_amd.bamio and of oracle_np.discover_regions (which restates the function with truncation off).

One liberty, for contigs of tens of megabases: the depth vector and the column loop cover only [lo, hi], lo the first covered
column and hi the column behind the last covered one (if the contig has it).  Every column outside has depth 0 and is a break
whatever the cap; in front of lo nothing is pending and max_coverage is 0, so those iterations change no state, and behind hi
the pending region has been emitted at hi (or is emitted after the loop, with the same state), so neither do those.

discover_np is the same function over whole arrays, for windows of millions of columns (tests/scan_regime_cases.py), where the
column loop takes seconds per call; tests/test_scan_regime_cases.py holds it to the loop on every small case."""
import numpy as np


def discover(spans, ref_len, truncation=False, truncation_coverage=200000):
    """spans = [(reference_start, reference_end)] of the filtered reads of one contig.
    Returns ([(start0, len, max_cov)], n_truncated): start0 = Region.start - 1, len = Region.end - Region.start, and the number of
    columns with depth > truncation_coverage (0 with truncation off: the driver's report, not part of the reference)."""
    spans = [(max(int(s), 0), min(int(e), ref_len)) for s, e in spans]
    spans = [(s, e) for s, e in spans if s < e]
    if not spans:
        return [], 0
    lo = min(s for s, _ in spans)
    hi = min(max(e for _, e in spans), ref_len - 1)
    depth = np.zeros(hi - lo + 1, dtype=np.int64)
    for s, e in spans:                       # util.rs:283-285
        depth[s - lo:e - lo] += 1
    depth = depth.tolist()
    out = []
    region_start = region_end = -1
    max_coverage = 0
    n_truncated = 0
    for i in range(lo, hi + 1):              # util.rs:290-319
        d = depth[i - lo]
        if d > max_coverage:
            max_coverage = d
        if truncation and d > truncation_coverage:
            n_truncated += 1
        if d == 0 or (truncation and d > truncation_coverage):
            if region_end > region_start:
                out.append((region_start, region_end - region_start + 1, max_coverage))
                region_start = region_end = -1
                max_coverage = 0
        else:
            if region_start == -1:
                region_start = region_end = i
            else:
                region_end = i
    if region_end > region_start:            # util.rs:320-330
        out.append((region_start, region_end - region_start + 1, max_coverage))
    return out, n_truncated


def window_depth(spans, ref_len):
    """(lo, depth): the int64 depth of the columns [lo, hi] of `discover` (a difference array and its cumsum), or None without a valid span"""
    a = np.asarray(spans, dtype=np.int64).reshape(-1, 2)
    s, e = np.maximum(a[:, 0], 0), np.minimum(a[:, 1], ref_len)
    ok = s < e
    s, e = s[ok], e[ok]
    if s.size == 0:
        return None
    lo = int(s.min())
    n = min(int(e.max()), ref_len - 1) - lo + 1           # e - lo <= n: the difference array has n + 1 entries
    diff = np.bincount(s - lo, minlength=n + 1).astype(np.int64) - np.bincount(e - lo, minlength=n + 1)
    return lo, np.cumsum(diff)[:n]


def regions_of_depth(depth, lo, truncation=False, truncation_coverage=200000):
    """the column loop of `discover` over the window's depth vector (depth[i] = column lo + i), island by island -> (regions, n_truncated)"""
    depth = np.asarray(depth, dtype=np.int64)
    kept = depth > 0
    n_truncated = 0
    if truncation:
        kept &= depth <= truncation_coverage
        n_truncated = int((depth > truncation_coverage).sum())
    edges = np.flatnonzero(np.diff(np.concatenate(([0], kept.view(np.int8), [0]))))
    out = []
    pend, first = -1, 0          # start of the pending region; first column behind the last emission (max_coverage runs from there)
    for s, e in zip(edges[0::2].tolist(), (edges[1::2] - 1).tolist()):      # islands, both ends included
        if pend < 0:
            pend = s
        if e > pend:             # region_end > region_start: emitted at the first break behind the island, or after the loop
            at = min(e + 1, depth.size - 1)
            out.append((pend + lo, e - pend + 1, int(depth[first:at + 1].max())))
            pend, first = -1, at + 1
    return out, n_truncated


def discover_np(spans, ref_len, truncation=False, truncation_coverage=200000):
    """`discover` without the column loop: the same arguments, the same (regions, n_truncated)"""
    w = window_depth(spans, ref_len)
    if w is None:
        return [], 0
    return regions_of_depth(w[1], w[0], truncation, truncation_coverage)

"""find_isolated_regions_with_depth (reference src/util.rs:236-332) restated loop for loop, with both of its switches
(`truncation`, `truncation_coverage`): spans -> depth -> the column loop.  Written from the Rust text and independent of
longcallr_amd.bamio and of oracle_np.discover_regions (which restates the function with truncation off).

One liberty, for contigs of tens of megabases: the depth vector and the column loop cover only [lo, hi], lo the first covered
column and hi the column behind the last covered one (if the contig has it).  Every column outside has depth 0 and is a break
whatever the cap; in front of lo nothing is pending and max_coverage is 0, so those iterations change no state, and behind hi
the pending region has been emitted at hi (or is emitted after the loop, with the same state), so neither do those."""
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

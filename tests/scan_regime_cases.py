"""Inputs of region discovery that drive its depth scan (launch_scan_i32 over nd = window + 2 items, csrc/k2_candidates.hip)
through each of its size regimes, and the small truncation cases that tests/test_truncation_gpu.py shares with the CPU test of
the windowed reference.  Numpy only: nothing here imports longcallr_amd.

The scan works in blocks of TILE = 1024 items.  Up to FUSED_BLOCKS blocks every block adds up the sums of the blocks in front of
it itself, 256 per stride; beyond that a one-block kernel scans the block sums in rounds of 1024 with a carry between rounds.
Item i + 1 of the scan's output is the depth of window column i, so the prefix that scan block k receives from the blocks in
front of it is the depth of window column 1024 k - 1: `case` puts a hand-placed group of spans over each such column it lists
in `borders`, of a depth that differs from border to border, and keeps the random background away from it.  The scan's last
item (window column W, behind the last covered one) is 0 by construction and nothing reads it, so a block that holds only that
item (nd = 1024 m + 1) has no border; the last border of a case is the one of the last block that holds a window column."""
import functools

import numpy as np

import truncation_ref as tr

TILE = 1024
FUSED_BLOCKS = 2048
CAP = 2                                  # the cap of the large cases: about half of their covered columns are deeper
ROUND_BORDERS = (256, 512, 1024, 2048, 3072)
BORDER_DEPTHS = (2, 3, 1, 4, 5, 6)       # pairwise different; above and below CAP
MAX_CONTIG = 0x7FFFFFF0                  # the largest contig_len lcr_discover_regions accepts
HIGH_BASE = 2144000000

# name -> nd; W = nd - 2
SIZES = {
    "tile_exact": TILE,                          # one full block, no second
    "tile_plus1": TILE + 1,                      # the second block holds one item
    "fused_257": 257 * TILE,                     # every thread of the last block adds one block sum
    "fused_258": 258 * TILE,                     # block 257 is the first whose thread 0 takes a second stride (j = 256)
    "fused_513p1": 513 * TILE + 1,               # a third stride; the last block holds one item
    "fused_last": FUSED_BLOCKS * TILE,           # the last fused size
    "three_first": FUSED_BLOCKS * TILE + 1,      # the first three-phase size; the third round of the block-sum scan has one entry
    "three_3072": 3072 * TILE,                   # three full rounds
    "three_3073": 3072 * TILE + 1,               # a fourth round with one entry
    "three_3074": 3074 * TILE,                   # the fourth round's carry reaches columns that are read (borders 3072 and 3073)
}
# name -> (size, keyword arguments of case)
VARIANTS = {
    "three_first_high": ("three_first", dict(base=HIGH_BASE, contig_len=MAX_CONTIG)),
    "three_first_end": ("three_first", dict(base=MAX_CONTIG - (SIZES["three_first"] - 2), contig_len=MAX_CONTIG, clamped_end=True)),
    "fused_257_single": ("fused_257", dict(single_tail=True)),
}
NAMES = list(SIZES) + list(VARIANTS)


def blocks(nd):
    return (nd + TILE - 1) // TILE


def border_column(k):
    """the window column whose depth scan block k takes over from the blocks in front of it"""
    return TILE * k - 1


def borders_of(W):
    last = W // TILE                     # the block of item W = depth of the last covered column
    ks = [k for k in ROUND_BORDERS if k <= last]
    if last >= 1 and last not in ks:
        ks.append(last)
    return ks


def case(W, base=0, seed=1, contig_len=None, clamped_end=False, single_tail=False):
    """(spans, contig_len, borders): the covered window is [base, base + W) exactly.
    clamped_end: contig_len == base + W, and one more span ends at 2^31 - 1 (clamped to the contig: the window ends at the
    contig's last column).  single_tail: the window's last covered stretch is, under CAP, an island of one column (W - 1) behind
    an over-deep column."""
    rng = np.random.default_rng(seed)
    borders = borders_of(W)
    rel = []
    # background: clusters of 2 to 6 chained spans of 200 to 2500 columns, 1 to 3000 uncovered columns between clusters
    pos = 0
    while pos < W - 4000:
        s = end = pos
        for _ in range(int(rng.integers(2, 7))):
            ln = int(rng.integers(200, 2501))
            rel.append((s, s + ln))
            end = max(end, s + ln)
            s += int(rng.integers(50, 501))
        pos = end + (int(rng.integers(1, 4)) if rng.random() < 0.3 else int(rng.integers(1, 3001)))
    if not rel:          # a window of one block: a stretch above CAP, an island of one column, an island
        rel += [(0, 300), (100, 280), (150, 260), (330, 331), (400, 500)]
    # nothing but the hand-placed spans within 500 columns of a border or in the window's last 520 columns
    zones = [(border_column(k) - 500, border_column(k) + 500) for k in borders] + [(W - 520, W + 1)]
    rel = [(s, e) for s, e in rel if s == 0 or not any(s <= z1 and e >= z0 for z0, z1 in zones)]
    assert rel[0][0] == 0 and all(rel[0][1] < z0 for z0, _ in zones)
    for k, d in zip(borders, BORDER_DEPTHS):
        c = border_column(k)
        rel += [(c - 200 - 30 * j, c + 150 + 40 * j) for j in range(d)]      # depth d from c - 200 to c + 149
    if single_tail:      # depth 1, 2, then 3 on [W - 200, W - 2], then 1 on W - 1
        rel += [(W - 450, W - 1), (W - 300, W - 1), (W - 200, W)]
    else:
        rel += [(W - 450, W), (W - 300, W - 100)]
    spans = [(base + s, base + e) for s, e in rel]
    if contig_len is None:
        contig_len = base + W + 1000
    if clamped_end:
        assert contig_len == base + W
        spans.append((base + W - 380, (1 << 31) - 1))
    assert len(spans) <= max(W // 500, 8) and contig_len <= MAX_CONTIG
    return spans, contig_len, borders


def named(name):
    size, kw = VARIANTS.get(name, (name, {}))
    return case(SIZES[size] - 2, seed=11 + NAMES.index(name), **kw)


built = functools.lru_cache(maxsize=None)(named)      # computed once per process; nobody changes what it returns


@functools.lru_cache(maxsize=2)
def depth_of(name):
    """(lo, depth of the window's columns) of the windowed reference"""
    spans, contig_len, _ = built(name)
    return tr.window_depth(spans, contig_len)


@functools.lru_cache(maxsize=None)
def expected(name, cap=None):
    """tr.discover_np of the case: (regions, n_truncated), with truncation at `cap` or (None) without"""
    lo, depth = depth_of(name)
    return tr.regions_of_depth(depth, lo, cap is not None, 0 if cap is None else cap)


@functools.lru_cache(maxsize=None)
def max_depth(name):
    return int(depth_of(name)[1].max())


def small_case(seed):
    """a window of 30 to 3000 columns of short random spans: (spans, contig_len).  Odd seeds sit at a base > 0; every third one has a
    contig that ends inside the window, so some spans are clamped (or dropped) at contig_len"""
    rng = np.random.default_rng(1000 + seed)
    W = int(rng.integers(30, 3001))
    base = int(rng.integers(1, 5000)) if seed % 2 else 0
    n = int(rng.integers(3, max(4, W // 12)))
    st = base + rng.integers(0, W, size=n)
    ln = rng.integers(1, int(rng.choice([4, 40, 400])), size=n)
    spans = list(zip(st.tolist(), (st + ln).tolist()))
    contig_len = base + int(W * 0.8) if seed % 3 == 0 else base + W + int(rng.integers(0, 50))
    return spans, contig_len


# ---- the small truncation cases (tests/test_truncation_gpu.py) ---------------------------------------------------------------------
TRUNC_CAP = 3


def depth_to_spans(depth):
    """spans whose depth vector is `depth`: one span per run of columns with depth >= level, for every level"""
    depth = np.asarray(depth, dtype=np.int64)
    spans = []
    for level in range(1, int(depth.max()) + 1):
        edges = np.flatnonzero(np.diff(np.concatenate(([0], (depth >= level).view(np.int8), [0]))))
        spans += list(zip(edges[0::2].tolist(), edges[1::2].tolist()))
    return spans


def hand_built(variant, tail):
    """depth of a contig of 4096 whose first covered column is 7 (w: window-relative -> contig position), cap = TRUNC_CAP"""
    CAP = TRUNC_CAP
    L, off = 4096, 7
    d = np.zeros(L, dtype=np.int64)
    w = lambda r: r + off
    d[7:10] = 5            # an over-deep stretch on the first covered column: counts for the first region
    d[10:20] = CAP         # exactly the cap: kept
    d[20:22] = CAP + 1     # one above: break; column 20 closes (10, 10) and counts for it, column 21 for the next region
    d[22] = 2              # a single kept column between two over-deep stretches: stays pending ...
    d[23:30] = 6
    d[30:50] = 1           # ... and starts the region that ends here: max over column 21, the column, the stretch, the island
    d[60:70] = 2
    d[70:75] = 9           # two over-deep stretches one kept column apart
    d[75] = 1
    d[76:80] = 7
    d[80:90] = 2
    if variant == 0:       # an island ends at window column 1023, the next starts at 1025
        d[w(1000):w(1024)] = 2; d[w(1024)] = 4; d[w(1025):w(1040)] = 1
    elif variant == 1:     # start at 1023, end at 1024
        d[w(1000):w(1022)] = 2; d[w(1022)] = 4; d[w(1023):w(1025)] = 3; d[w(1025):w(1030)] = 5
    else:                  # start at 1024, end at 1025
        d[w(1000):w(1023)] = 2; d[w(1023)] = 0; d[w(1024):w(1026)] = 1; d[w(1026)] = 8; d[w(1027):w(1040)] = 2
    # an over-deep stretch over more than two whole 1024-column blocks, largest in the middle one; it is the "break run in front" of the island behind it
    d[w(1100):w(3200)] = 5
    d[w(2500)] = 8
    d[w(3200):w(3300)] = 2
    if tail == "deep":     # an over-deep stretch on the contig's last column: counts for nothing
        d[3900:4000] = 1; d[4000:4096] = 6
    else:                  # an island that reaches the contig's last column: emitted after the loop
        d[3990:4000] = 4; d[4000:4096] = 2
    return d, L


HAND_BUILT = [(0, "deep"), (1, "island"), (2, "deep")]


def tiny_islands():
    """depth alternating around the cap every one or two columns over 6000 columns: (depth, contig_len, number of islands)"""
    CAP = TRUNC_CAP
    rng = np.random.default_rng(21)
    L, first = 9000, 1500
    d = np.zeros(L, dtype=np.int64)
    i, kept, n_isl = first, True, 0
    while i < first + 6000:
        n = int(rng.integers(1, 3))
        d[i:i + n] = rng.integers(CAP - 1, CAP + 1) if kept else rng.integers(CAP + 1, CAP + 4)
        n_isl += kept
        i += n
        kept = not kept
    return d, L, n_isl


def random_case():
    rng = np.random.default_rng(3)
    st = np.sort(rng.integers(0, 200000, size=300))
    ln = rng.integers(1, 400, size=300)
    return list(zip(st.tolist(), (st + ln).tolist())), 200100

"""The yardstick of tests/test_scan_regime_cases_gpu.py, checked on the CPU: the windowed reference (truncation_ref.discover_np) is
the loop restatement (truncation_ref.discover) on every small case, and the large cases (tests/scan_regime_cases.py) have the
properties the GPU test relies on -- above all that a scan which lost one block carry could not give their expected regions."""
import numpy as np
import pytest

import scan_regime_cases as sc
import truncation_ref as tr

CAPS = (None, 1, 2, 3)     # None: truncation off


def same_as_loop(spans, contig_len):
    """discover_np == discover with truncation off and at caps 1, 2, 3; returns the cap-free and the cap-1 answer"""
    got = {}
    for cap in CAPS:
        on, c = cap is not None, 200000 if cap is None else cap
        got[cap] = tr.discover_np(spans, contig_len, on, c)
        assert got[cap] == tr.discover(spans, contig_len, on, c), cap
    assert tr.discover_np(spans, contig_len, False, 1) == got[None]      # the cap is ignored while the switch is off
    return got[None], got[1]


@pytest.mark.parametrize("variant,tail", sc.HAND_BUILT)
def test_np_is_the_loop_on_hand_built(variant, tail):
    d, L = sc.hand_built(variant, tail)
    off, cut = same_as_loop(sc.depth_to_spans(d), L)
    assert off != cut[0] and cut[1] > 0


def test_np_is_the_loop_on_tiny_islands_and_random_spans():
    d, L, _ = sc.tiny_islands()
    off, cut = same_as_loop(sc.depth_to_spans(d), L)
    assert off != cut[0]
    off, cut = same_as_loop(*sc.random_case())
    assert off != cut[0]


@pytest.mark.parametrize("name", ["tile_exact", "tile_plus1"])
def test_np_is_the_loop_on_one_tile(name):
    spans, contig_len, _ = sc.built(name)
    same_as_loop(spans, contig_len)
    assert tr.discover(spans, contig_len, True, sc.CAP) == sc.expected(name, sc.CAP)
    assert tr.discover(spans, contig_len) == sc.expected(name)


def test_np_is_the_loop_on_small_random_cases():
    n_based = n_clamped = n_cut = 0
    for seed in range(20):
        spans, contig_len = sc.small_case(seed)
        off, cut = same_as_loop(spans, contig_len)
        n_based += min(s for s, _ in spans) > 0
        n_clamped += any(s < contig_len < e for s, e in spans)
        n_cut += off != cut[0]
    assert n_based >= 8 and n_clamped >= 4 and n_cut >= 15


def test_np_without_a_valid_span():
    for spans in ([], [(5, 5)], [(7, 3)], [(100, 120)]):
        assert tr.discover_np(spans, 50, True, 1) == tr.discover(spans, 50, True, 1) == ([], 0)


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_conditions(name):
    spans, contig_len, borders = sc.built(name)
    size = sc.VARIANTS.get(name, (name,))[0]
    nd = sc.SIZES[size]
    W, nb = nd - 2, sc.blocks(nd)
    lo, depth = sc.depth_of(name)
    a = np.asarray(spans, dtype=np.int64)
    assert a.min() >= 0 and a[:, 0].max() < 1 << 31 and a[:, 1].max() < 1 << 31 and contig_len <= sc.MAX_CONTIG      # int32 spans
    assert lo == int(a[:, 0].min()) and min(int(a[:, 1].max()), contig_len) - lo == W           # the window, exactly
    assert depth[0] > 0 and depth[W - 1] > 0 and depth[:W].size == W
    assert (nb <= 256, 256 < nb <= sc.FUSED_BLOCKS, nb > sc.FUSED_BLOCKS).count(True) == 1
    top = int(depth.max())
    (off, zero), (cut, n_cut) = sc.expected(name), sc.expected(name, sc.CAP)
    assert zero == 0 and sc.expected(name, top) == (off, 0) and top > sc.CAP
    print("%s: nd %d, %d scan blocks, %d regions (%d under cap %d, %d columns above it), maximal depth %d, borders %s"
          % (name, nd, nb, len(off), len(cut), sc.CAP, n_cut, top, borders))
    assert n_cut > 0 and cut != off
    if nb >= 257:
        assert len(off) >= 50 and len(cut) >= 50
    # a region inside the last scan block that holds a window column
    first = lo + max(sc.border_column(W // sc.TILE), 0)
    for regions in (off, cut):
        assert any(s >= first for s, _, _ in regions)
    # the borders: every round border the window has, and the last block's; depths non-zero and pairwise different
    assert borders == sorted(set(borders)) and all(1 <= k <= W // sc.TILE for k in borders)
    assert [k for k in sc.ROUND_BORDERS if k <= W // sc.TILE] == [k for k in borders if k in sc.ROUND_BORDERS]
    assert (W // sc.TILE in borders) == (nb > 2)
    at = [int(depth[sc.border_column(k)]) for k in borders]
    assert at == list(sc.BORDER_DEPTHS[:len(borders)]) and len(set(at)) == len(at) and min(at, default=1) >= 1
    for k, d in zip(borders, at):
        c = lo + sc.border_column(k)
        assert any(s <= c < s + n for s, n, _ in off)                                  # a region of the expected output covers it
        assert any(s <= c < s + n for s, n, _ in cut) == (d <= sc.CAP)                 # (under the cap: where the column is kept)
    # a lost carry must be visible: block k's prefix (the depth of its border column) missing from every item of blocks >= k
    for k in borders:
        c = sc.border_column(k)
        wrong = depth.copy()
        wrong[c:] -= depth[c]
        assert wrong[c] == 0
        assert tr.regions_of_depth(wrong, lo) != (off, 0), k
        assert tr.regions_of_depth(wrong, lo, True, sc.CAP) != (cut, n_cut), k
        assert tr.regions_of_depth(wrong, lo, True, top) != (off, 0), k
    if name == "three_first_high":
        assert lo == sc.HIGH_BASE and contig_len == sc.MAX_CONTIG
    if name == "three_first_end":      # the extra span is clamped: the window ends at the contig's last column, the last region after the loop
        assert a[:, 1].max() == (1 << 31) - 1 and lo + W == contig_len == sc.MAX_CONTIG and depth.size == W
        assert off[-1][0] + off[-1][1] == contig_len == cut[-1][0] + cut[-1][1]
    if name == "fused_257_single":     # under the cap the last column is kept, alone, behind an over-deep one: pending for ever
        assert depth[W - 1] == 1 and depth[W - 2] > sc.CAP and depth[W] == 0
        assert cut[-1][0] + cut[-1][1] < lo + W - 1 and off[-1][0] + off[-1][1] == lo + W

"""Masks for the exon-only tests (lcr_set_exon_mask): plain data and helpers, no tests.

A mask is one boolean array per region of a batch, True = the column lies in a CDS.  Two things are made from it: the interval lists
Engine.set_exon_mask takes, and the yardstick -- the same batch with the reference byte of every masked-out column replaced by 'N'.  A
column whose reference byte is not upper-case ACGT never becomes a candidate (candidate.rs:132) and nothing in front of that test has a
side effect, so the existing oracles on the substituted batch give what a masked run must give; test_exon_host.py restates that premise
with the Python oracle where the GPU tests use it."""
import numpy as np

from longcallr_amd import _abi


def with_reference(b, ref):
    """the batch with another reference (same reads, same regions)"""
    kw = {f: getattr(b, f) for f in _abi.ReadBatch.FIELDS}
    return _abi.ReadBatch(start0=b.start0, len=b.len, read_begin=b.read_begin, ref=ref, names=b.names, **kw)


def n_substituted(b, keep):
    ref = b.ref.copy()
    for g, k in enumerate(keep):
        o = int(b.col_off[g])
        ref[o:o + k.size][~k] = ord("N")
    return with_reference(b, ref)


def runs(k):
    """the True runs of a boolean array as [(first, one past last)]"""
    e = np.flatnonzero(np.diff(np.concatenate([[0], k.astype(np.int8), [0]])))
    return [(int(a), int(z)) for a, z in zip(e[0::2], e[1::2])]


def lists_of(b, keep):
    """per region the mask's runs as reference intervals, ascending and disjoint: [[(start0, end0), ...]]"""
    return [[(int(b.start0[g]) + a, int(b.start0[g]) + z) for a, z in runs(k)] for g, k in enumerate(keep)]


def flat(lists):
    """[[(start0, end0), ...] per region] -> (iv_off, start0, end0) of Engine.set_exon_mask"""
    off = np.zeros(len(lists) + 1, np.int32)
    np.cumsum([len(v) for v in lists], out=off[1:])
    return off, np.array([a for v in lists for a, _ in v], np.int64), np.array([z for v in lists for _, z in v], np.int64)


def mask_of_lists(b, lists):
    """what interval lists of any shape mean, computed the slow way: per region the columns inside some interval"""
    keep = []
    for g, v in enumerate(lists):
        k = np.zeros(int(b.len[g]), bool)
        for a, z in v:
            a, z = max(a - int(b.start0[g]), 0), min(z - int(b.start0[g]), k.size)
            if z > a:
                k[a:z] = True
        keep.append(k)
    return keep


def random_mask(b, seed, n_iv=6):
    """per region a handful of seeded random intervals, 1 to a third of the region long"""
    rng = np.random.default_rng(seed)
    keep = []
    for g in range(b.n_regions):
        L = int(b.len[g])
        k = np.zeros(L, bool)
        for _ in range(int(rng.integers(1, n_iv + 1))):
            a = int(rng.integers(0, L))
            k[a:a + int(rng.integers(1, max(L // 3, 2)))] = True
        keep.append(k)
    return keep


def every_other(b, record_cols):
    """everything in but every other record column of the unmasked result (the 1st, 3rd, ... of each region are masked out)"""
    keep = []
    for g in range(b.n_regions):
        k = np.ones(int(b.len[g]), bool)
        k[np.asarray(record_cols[g], np.int64)[0::2]] = False
        keep.append(k)
    return keep


def one_column(b, g, col, complement=False):
    """every region fully in, region g: only `col` (complement: all but `col`)"""
    keep = [np.ones(int(b.len[h]), bool) for h in range(b.n_regions)]
    keep[g] = np.zeros(int(b.len[g]), bool) if not complement else keep[g]
    keep[g][col] = not complement
    return keep

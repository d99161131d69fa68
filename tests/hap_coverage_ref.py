"""A plain-Python / NumPy restatement of lcr_hap_coverage's contract (include/lcr.h): per read and per op over a dense array, then a
run-length encoding on the host.  Test infrastructure: it shares no code with longcallr_amd/coverage.py or the kernels."""
import numpy as np

from longcallr_amd import _abi

COVER = (0, 2, 7, 8)   # M D = X
GAP = 3                # N


def classes(n_reads, read_begin, row_region_off, row_read, assignment):
    """class per listed read: a row's assignment where it is 1 or 2, else 0 (rows are per region: a read listed twice has two entries)"""
    cls = np.zeros(n_reads, np.int64)
    for g in range(len(read_begin) - 1):
        for r in range(int(row_region_off[g]), int(row_region_off[g + 1])):
            i = int(row_read[r])
            assert read_begin[g] <= i < read_begin[g + 1]
            if int(assignment[r]) in (1, 2):
                cls[i] = int(assignment[r])
    return cls


def blocks(pos, ops):
    """covered blocks [(start, end)] of one read; ops: [(length, code)]"""
    out, p = [], int(pos)
    for n, op in ops:
        if n < 1:
            continue
        if op in COVER:
            out.append((p, p + n))
            p += n
        elif op == GAP:
            p += n
    return out


def dense(start0, length, reads, cls):
    """reads: [(pos, ops)] of one region, cls their classes -> (depth 3 x length uint64, n_reads[3])"""
    d = np.zeros((3, length), np.uint64)
    nr = [0, 0, 0]
    for (pos, ops), k in zip(reads, cls):
        nr[int(k)] += 1
        for s, e in blocks(pos, ops):
            lo, hi = max(s - start0, 0), min(e - start0, length)
            if lo < hi:
                d[int(k), lo:hi] += np.uint64(1)
    return d, nr


def encode(g, start0, d):
    """maximal runs of one non-zero triple -> [(region, len, start0, (n0, n1, n2))]"""
    out, length = [], d.shape[1]
    if length == 0:
        return out
    cuts = [0] + (np.flatnonzero((d[:, 1:] != d[:, :-1]).any(axis=0)) + 1).tolist() + [length]   # a column whose triple differs from the one before
    for c, e in zip(cuts[:-1], cuts[1:]):
        t = (int(d[0, c]), int(d[1, c]), int(d[2, c]))
        if t != (0, 0, 0):
            out.append((g, e - c, start0 + c, t))
    return out


def batch_reads(batch):
    """the batch's reads as [(pos, [(length, code)])]"""
    out = []
    for i in range(len(batch.pos)):
        o, n = int(batch.cig_off[i]), int(batch.n_cig[i])
        out.append((int(batch.pos[i]), [(int(w) >> 4, int(w) & 15) for w in batch.cigar[o:o + n]]))
    return out


def hap_coverage(batch, row_region_off, row_read, assignment):
    """the whole call -> (segments, seg_region_off, region records) as the ABI's structured arrays"""
    rb = [int(x) for x in batch.read_begin]
    ng = len(rb) - 1
    reads = batch_reads(batch)
    cls = classes(len(reads), rb, row_region_off, row_read, assignment)
    segs, off = [], [0]
    reg = np.zeros(ng, dtype=_abi.HAP_COV_REGION_DTYPE)
    for g in range(ng):
        s0, ln = int(batch.start0[g]), int(batch.len[g])
        d, nr = dense(s0, ln, reads[rb[g]:rb[g + 1]], cls[rb[g]:rb[g + 1]])
        segs += encode(g, s0, d)
        off.append(len(segs))
        reg["region"][g] = g
        reg["n_reads"][g] = nr
        reg["bases"][g] = [int(d[k].sum()) for k in range(3)]
        reg["max_depth"][g] = [int(d[k].max()) if ln else 0 for k in range(3)]
    out = np.zeros(len(segs), dtype=_abi.HAP_COV_SEGMENT_DTYPE)
    for j, (g, ln, s, t) in enumerate(segs):
        out["region"][j], out["len"][j], out["start0"][j], out["n"][j] = g, ln, s, t
    return out, np.array(off, np.int32), reg

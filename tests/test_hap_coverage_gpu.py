"""K13 lcr_hap_coverage on the GPU against the plain-Python restatement of its contract (tests/hap_coverage_ref.py): every field of every
segment and region record, exactly, in pinned host memory and in HBM.  Rows are put on chosen haplotypes with Engine.haplotag and
hand-picked sites (a class-1 read carries the reference base at a site, a class-2 read the alternate, a class-0 read N); the restatement
classes the reads by the engine's own assignment, and the tests that depend on a class assert it.

One arm of the contract cannot reach the call through this library: lcr_pileup refuses a batch that holds a P op (K0's verdict 1, as the
reference panics on it), so no batch with a P op gets as far as the phase stage.  The kernel takes P as an op that neither covers nor
advances; the restatement's arm for it is tested in test_hap_coverage_host.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hap_coverage_ref as ref
import helpers
import test_haplotag_gpu as th
import test_junctions_gpu as tj
import test_site_counts_gpu as ts
from longcallr_amd import _abi, _lib, coverage, synth

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "longcallr_amd", "csrc", "k13_hap_coverage.h")) as _f:
    TILE = int(re.search(r"#define\s+K13_TILE\s+(\d+)", _f.read()).group(1))     # window columns per scan / compaction step


def cov_region(start0, length, sites, reads, seed):
    """A region's random reference and its reads.  reads: [(column, CIGAR, class)], columns relative to the window and free to leave it;
    at a column of `sites` inside the window a read of class 1 carries the reference base, of class 2 its tj.ALT, of class 0 an N.
    -> (start0, reference, read dicts sorted by position with the intended class as "cls")"""
    rng = np.random.default_rng(seed)
    refseq = "".join(rng.choice(list("ACGT"), size=length))
    sites = set(sites)
    out = []
    for k, (col, cigar, cls) in enumerate(reads):
        seq, c = [], col
        for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar):
            n = int(n)
            if op in "M=X":
                for x in range(c, c + n):
                    base = refseq[x] if 0 <= x < length else "A"
                    if x in sites and 0 <= x < length:
                        base = {1: base, 2: tj.ALT[base], 0: "N"}[cls]
                    seq.append(base)
                c += n
            elif op in "DN":
                c += n
            elif op in "IS":
                seq += ["A"] * n
        out.append(dict(pos=start0 + col, seq="".join(seq), qual=30, cigar=cigar, rev=k % 2, ts=1 + k % 2, cls=cls))
    out.sort(key=lambda r: r["pos"])
    return start0, refseq, out


def tagged(E, regions, sites_by_region, ps_of=None):
    """the batch staged with a het site imported at every listed column and tagged against them (haplotype 1 = the reference base;
    ps_of: {(region, column): phase set}, default 100 + region) -> (batch, fragmat)"""
    b = tj.batch_of(regions)
    d = {}
    for g, ((s0, refseq, _), cols) in enumerate(zip(regions, sites_by_region)):
        for c in cols:
            d[s0 + c] = (refseq[c], tj.ALT[refseq[c]], (ps_of or {}).get((g, c), 100 + g))
    pos = np.array(sorted(d), np.int64)
    fm, _, _ = th.staged(E, b, (pos, np.ones(pos.size, np.uint8), np.full(pos.size, 30.0, np.float32)))
    E.haplotag(th.site_arrays(d))
    return b, fm


def dev_copy(ptr, dtype, n):
    out = np.zeros(n, dtype=dtype)
    if n:
        assert _lib.load().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


def check(E, b, fm):
    """hap_coverage() against the restatement on the engine's own assignment, host and HBM -> (segments, offsets, region records)"""
    pr = E.phase_result()
    seg, off, reg = E.hap_coverage()
    wseg, woff, wreg = ref.hap_coverage(b, fm["row_region_off"], fm["row_read"], pr["assignment"])
    assert seg.dtype == _abi.HAP_COV_SEGMENT_DTYPE and reg.dtype == _abi.HAP_COV_REGION_DTYPE
    assert off.tolist() == woff.tolist()
    for f in _abi.HAP_COV_SEGMENT_DTYPE.names:
        assert seg[f].tolist() == wseg[f].tolist(), f
    for f in _abi.HAP_COV_REGION_DTYPE.names:
        assert reg[f].tolist() == wreg[f].tolist(), f
    o = E._hap_coverage_list()
    assert (o.n_regions, o.n_segments) == (len(reg), len(seg))
    assert dev_copy(o.dev_seg, _abi.HAP_COV_SEGMENT_DTYPE, o.n_segments).tobytes() == seg.tobytes()     # HBM and host hold the same records
    assert dev_copy(o.dev_reg, _abi.HAP_COV_REGION_DTYPE, o.n_regions).tobytes() == reg.tobytes()
    return seg, off, reg


def got_classes(b, fm, E):
    return ref.classes(len(b.pos), [int(x) for x in b.read_begin], fm["row_region_off"], fm["row_read"], E.phase_result()["assignment"]).tolist()


def intended(regions):
    return [r["cls"] for _, _, rs in regions for r in rs]


def runs(seg, g=None):
    return [(int(s["start0"]), int(s["start0"]) + int(s["len"]), tuple(int(x) for x in s["n"])) for s in seg if g is None or int(s["region"]) == g]


def engine(engine_cls, seed=5):
    return engine_cls(0, _abi.make_params("hifi-masseq", seed=seed, min_linkers=1, dist_to_end=0))


# ---- 1. the worked instance of the contract -------------------------------------------------------------------------------------------
WORKED = [(0, "10M", 1), (5, "5M10N5M", 2), (8, "4M2D4M", 0), (20, "3S5M2I5M", 1)]
WORKED_SEGS = [(1000, 1005, (0, 1, 0)), (1005, 1008, (0, 1, 1)), (1008, 1010, (1, 1, 1)), (1010, 1018, (1, 0, 0)),
               (1020, 1025, (0, 1, 1)), (1025, 1030, (0, 1, 0))]


def test_worked_instance(engine_cls):
    regs = [cov_region(1000, 40, (6, 22), WORKED, 11)]
    E = engine(engine_cls)
    b, fm = tagged(E, regs, [(6, 22)])
    assert got_classes(b, fm, E) == [1, 2, 0, 1]
    seg, off, reg = check(E, b, fm)
    assert runs(seg) == WORKED_SEGS and off.tolist() == [0, 6] and not seg["pad_"].any() and not reg["pad_"].any()
    assert reg["bases"][0].tolist() == [10, 20, 10] and reg["max_depth"][0].tolist() == [1, 1, 1] and reg["n_reads"][0].tolist() == [1, 2, 1]
    assert (coverage.expand(seg, 1000, 40) == ref.dense(1000, 40, ref.batch_reads(b), [1, 2, 0, 1])[0]).all()
    E.close()


# ---- 2. CIGAR arms --------------------------------------------------------------------------------------------------------------------
ARMS = [(0, "20=", 1),                          # = covers
        (2, "8M3X20M", 2),                      # X covers (the site under it)
        (5, "5M5D5M", 0),                       # D covers: one block [5, 20), the site inside the deletion
        (0, "4M6N4M", 1),                       # N does not: [0, 4) and [10, 14)
        (8, "2H3S4M2I4M0M0N0D4M3S2H", 2),       # H S I and zero-length M / N / D change nothing: one block [8, 20)
        (20, "5M0N5M", 0),                      # a zero-length N is no gap: one block [20, 30)
        (40, "5M5D5M", 0),                      # D abutting M: one block [40, 55), no breakpoint at 45 or 50
        (100, "1M1D" * 65, 0),                  # 130 ops, one block [100, 230)
        (240, "1M1N" * 65, 1)]                  # 130 ops, 65 blocks of one column; the site at 300 is under the 31st


def test_cigar_arms(engine_cls):
    regs = [cov_region(7000, 400, (10, 300), ARMS, 12)]
    E = engine(engine_cls)
    b, fm = tagged(E, regs, [(10, 300)])
    assert max(int(n) for n in b.n_cig) == 130
    seg, off, reg = check(E, b, fm)
    d = coverage.expand(seg, 7000, 400).astype(np.int64).sum(axis=0)
    assert d[40:55].tolist() == [1] * 15 and d[39] == 0 and d[55] == 0                      # D abutting M
    assert d[100:230].tolist() == [1] * 130 and d[230:240].tolist() == [0] * 10            # the 130-op read, all of it
    assert d[240:370].tolist() == [1, 0] * 65                                              # N gaps of one column
    assert [r for r in runs(seg) if 7040 <= r[0] < 7056] == [(7040, 7055, (1, 0, 0))]
    assert int(reg["n_reads"][0].sum()) == len(ARMS)
    E.close()


# ---- 3. clipping ----------------------------------------------------------------------------------------------------------------------
CLIP = [(-10, "30M", 1),           # pos left of the window, a block starting before it: [0, 20)
        (80, "40M", 2),            # a block ending behind it: [80, 100)
        (90, "10M", 1),            # ending exactly at start0 + len
        (0, "10M", 2),             # starting exactly at start0
        (-20, "10M20N10M", 1),     # the first block wholly outside on the left: [10, 20) only
        (70, "10M40N10M", 2)]      # the second wholly outside on the right: [70, 80) only


def test_clipping(engine_cls):
    regs = [cov_region(5000, 100, (5, 15, 75, 95), CLIP, 13)]
    E = engine(engine_cls)
    b, fm = tagged(E, regs, [(5, 15, 75, 95)])
    seg, off, reg = check(E, b, fm)
    assert int(seg["start0"].min()) == 5000 and int((seg["start0"] + seg["len"]).max()) == 5100      # nothing outside the window
    d = coverage.expand(seg, 5000, 100).astype(np.int64).sum(axis=0)
    assert d.tolist() == [2] * 10 + [2] * 10 + [0] * 50 + [1] * 10 + [1] * 10 + [2] * 10
    assert int(reg["n_reads"][0].sum()) == len(CLIP) and int(reg["bases"][0].sum()) == int(d.sum())
    E.close()


# ---- 4. cancelling breakpoints --------------------------------------------------------------------------------------------------------
def test_cancelling_breakpoints(engine_cls):
    regs = [cov_region(3000, 100, (5, 25), [(0, "20M", 1), (20, "20M", 1)], 14),      # class 1 ends where class 1 starts: no split
            cov_region(4000, 100, (5, 25), [(0, "20M", 1), (20, "20M", 2)], 15)]      # class 2 follows class 1: a split
    E = engine(engine_cls)
    b, fm = tagged(E, regs, [(5, 25), (5, 25)])
    assert got_classes(b, fm, E) == [1, 1, 1, 2]
    seg, off, reg = check(E, b, fm)
    assert runs(seg, 0) == [(3000, 3040, (0, 1, 0))]
    assert runs(seg, 1) == [(4000, 4020, (0, 1, 0)), (4020, 4040, (0, 0, 1))]
    E.close()


# ---- 5. scan and compaction boundaries ------------------------------------------------------------------------------------------------
def window_reads(n):
    """the whole window, its first, middle and last column"""
    return [(0, "%dM" % n, 1), (0, "1M", 2), (n // 2, "1M", 0), (n - 1, "1M", 0)]


def test_window_lengths(engine_cls):
    lens = [63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1]
    regs = [cov_region(10000 * (g + 1), n, (0,), window_reads(n), 20 + g) for g, n in enumerate(lens)]
    E = engine(engine_cls)
    b, fm = tagged(E, regs, [(0,)] * len(lens))
    seg, off, reg = check(E, b, fm)
    for g, n in enumerate(lens):
        r = runs(seg, g)
        assert r[0][0] == 10000 * (g + 1) and r[-1][1] == 10000 * (g + 1) + n and len(r) == 5, (g, n)       # first, run, middle, run, last
        assert int(reg["bases"][g].sum()) == n + 3
    E.close()


def test_regions_inside_one_tile_and_runs_across_tiles(engine_cls):
    assert TILE >= 700
    small = [100, 7, 200, 1, 300]      # five regions, 608 columns: depth in every last column, none in the first of the next
    regs = []
    for g, n in enumerate(small):
        reads = [(n - 1, "1M", 0)] + ([(1, "%dM" % (n - 2), 0)] if n > 2 else [])
        regs.append(cov_region(1000 * (g + 1), n, (), reads, 30 + g))
    # one segment over more than three tiles; a run from a tile's first column and one to a tile's last
    regs.append(cov_region(50000, 4 * TILE + 10, (7,), [(5, "%dM" % (3 * TILE + 20), 1)], 40))
    regs.append(cov_region(90000, 3 * TILE, (TILE + 2,), [(TILE, "7M", 2), (2 * TILE - 9, "9M", 0)], 41))
    E = engine(engine_cls)
    b, fm = tagged(E, regs, [()] * 5 + [(7,), (TILE + 2,)])
    seg, off, reg = check(E, b, fm)
    for g, n in enumerate(small):
        s0 = 1000 * (g + 1)
        assert runs(seg, g) == [(s0 + min(1, n - 1), s0 + n, (1, 0, 0))], g       # the scan restarts at every window
    assert runs(seg, 5) == [(50005, 50005 + 3 * TILE + 20, (0, 1, 0))]
    assert runs(seg, 6) == [(90000 + TILE, 90000 + TILE + 7, (0, 0, 1)), (90000 + 2 * TILE - 9, 90000 + 2 * TILE, (1, 0, 0))]
    assert off.tolist() == [0, 1, 2, 3, 4, 5, 6, 8]
    E.close()


# ---- 6. classes -----------------------------------------------------------------------------------------------------------------------
def test_classes(engine_cls):
    regs = [cov_region(1000, 200, (), [(10, "50M", 0), (30, "50M", 0), (30, "20M10N20M", 0)], 50),      # no candidate: every read class 0
            cov_region(2000, 300, (50,), [(0, "100M", 1), (20, "100M", 2), (40, "100M", 0),              # the third carries N at the site
                                          (50, "10M", 2), (51, "100M", 1), (200, "50M", 2)], 51),         # the last two start behind the candidate
            cov_region(3000, 600, (50, 60, 400, 410),                                                    # two phase sets
                       [(0, "100M", 1), (10, "100M", 2), (350, "100M", 2), (360, "100M", 1), (100, "200M", 0)], 52),
            cov_region(4000, 100, (), [], 53),                                                           # no reads
            cov_region(5000, 50, (10,), [(0, "30M", 1)], 54)]
    E = engine(engine_cls)
    ps_of = {(2, 50): 700, (2, 60): 700, (2, 400): 900, (2, 410): 900}
    b, fm = tagged(E, regs, [(), (50,), (50, 60, 400, 410), (), (10,)], ps_of)
    want = intended(regs)
    want[7], want[8] = 0, 0          # (the two reads of region 1 that start behind its last candidate are no rows)
    assert got_classes(b, fm, E) == want
    pr = E.phase_result()
    rro = fm["row_region_off"]
    assert rro[1] - rro[0] == 0 and rro[2] - rro[1] == 4 and sorted(set(pr["phase_set"][rro[2]:rro[3]].tolist())) == [0, 700, 900]
    seg, off, reg = check(E, b, fm)
    assert all(t[1] == 0 and t[2] == 0 for _, _, t in runs(seg, 0)) and reg["n_reads"][0].tolist() == [3, 0, 0]
    assert reg["n_reads"][1].tolist() == [3, 1, 2] and reg["n_reads"][2].tolist() == [1, 2, 2]
    assert off[4] == off[3] and reg[3]["n_reads"].tolist() == [0, 0, 0] and not reg[3]["bases"].any() and not reg[3]["max_depth"].any()
    assert int(reg["region"][3]) == 3 and runs(seg, 4) == [(5000, 5030, (0, 1, 0))]
    E.close()


# ---- 7. depth beyond 16 bits, one hot address -----------------------------------------------------------------------------------------
def test_deep_columns(engine_cls):
    deep = 70000
    regs = [cov_region(1000, 64, (), [(10, "4M", 0)] * deep, 60),
            cov_region(9000, 50, (10,), [(0, "30M", 1), (5, "30M", 2)], 61)]
    E = engine(engine_cls)
    b, fm = tagged(E, regs, [(), (10,)])
    seg, off, reg = check(E, b, fm)
    assert runs(seg, 0) == [(1010, 1014, (deep, 0, 0))] and deep > 65535
    assert reg["bases"][0].tolist() == [4 * deep, 0, 0] and reg["max_depth"][0].tolist() == [deep, 0, 0] and reg["n_reads"][0].tolist() == [deep, 0, 0]
    E.close()


# ---- 8. behind lcr_phase: synthetic and real data -------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ont-cdna", "masseq", "demo"])
def test_synth_and_demo(engine_cls, which):
    if which == "demo":
        b, prm = helpers.demo_batch(), _abi.make_params("hifi-masseq")
    else:
        b, prm = synth.make_batch(which, n_genes=4), _abi.make_params(synth.preset_for(which))
    E = engine_cls(0, prm)
    E.load_batch(b).run_all()
    fm = E.fragmat()
    seg, off, reg = check(E, b, fm)
    print("%s: regions %d, columns %d, segments %d, reads per class %r, bases per class %r, maxima %r, longest CIGAR %d" % (
        which, len(reg), int(np.sum(b.len)), len(seg), reg["n_reads"].sum(axis=0).tolist(), reg["bases"].sum(axis=0).tolist(),
        reg["max_depth"].max(axis=0).tolist(), int(max(b.n_cig))))
    assert reg["n_reads"][:, 1].any() and reg["n_reads"][:, 2].any() and len(seg) > 0
    E.close()


# ---- 9. independence from the batch ---------------------------------------------------------------------------------------------------
def test_region_alone_and_in_the_batch(engine_cls):
    regs = [cov_region(7000, 400, (10, 300), ARMS, 12), cov_region(15000, 100, (5, 15, 75, 95), CLIP, 13),
            cov_region(30000, TILE + 1, (0,), window_reads(TILE + 1), 28)]
    cols = [(10, 300), (5, 15, 75, 95), (0,)]
    E = engine(engine_cls)
    b, fm = tagged(E, regs, cols)
    seg, off, reg = check(E, b, fm)
    for g in range(3):
        b1, fm1 = tagged(E, [regs[g]], [cols[g]], {(0, c): 100 + g for c in cols[g]})
        seg1, off1, reg1 = check(E, b1, fm1)
        part, r = seg[off[g]:off[g + 1]].copy(), reg[g:g + 1].copy()
        assert set(part["region"].tolist()) == {g} and int(r["region"][0]) == g
        part["region"], r["region"] = 0, 0
        assert seg1.tobytes() == part.tobytes() and reg1.tobytes() == r.tobytes() and off1.tolist() == [0, len(part)], g
    E.close()


# ---- 10. order and lifetime on one context --------------------------------------------------------------------------------------------
def test_order_and_lifetime(engine_cls):
    b1, b2 = tj.batch_of([tj.allele_specific_region()]), tj.batch_of(th.edge_regions()[2:4])
    prm = _abi.make_params("hifi-masseq", seed=7)
    E = engine_cls(0, prm)
    lib = E.lib
    o = _abi.LcrHapCovList()
    call = lambda: lib.lcr_hap_coverage(E.h)
    get = lambda: lib.lcr_get_hap_coverage(E.h, C.byref(o))
    assert lib.lcr_hap_coverage(None) == E_ARG and lib.lcr_get_hap_coverage(E.h, None) == E_ARG
    E.load_batch(b1).fill_data_into_freq_vec().get_candidate_snps()
    assert call() == E_STATE and get() == E_STATE
    E.get_fragments()
    assert get() == E_STATE and call() == E_STATE and b"before lcr_phase" in lib.lcr_last_error(E.h)     # before the phase stage
    E.phase()
    assert get() == E_STATE                                                                              # phased, not counted yet
    fm = E.fragmat()
    sites = E.site_counts(13)
    junc, joff = E.junctions(2, 0)
    snap = th.snapshot(E)
    first = check(E, b1, fm)
    assert th.snapshot(E) == snap                                                                        # (the call writes nothing a getter reads)
    assert ts.dev_records(E).tobytes() == sites.tobytes()                                                # ... nor the site counts' records
    jl = _abi.LcrJunctionList()
    assert lib.lcr_get_junctions(E.h, C.byref(jl)) == 0 and jl.n_junctions == len(junc)
    assert dev_copy(jl.dev_junc, _abi.JUNC_DTYPE, jl.n_junctions).tobytes() == junc.tobytes()            # ... nor the junction table
    again = check(E, b1, fm)                                                                             # a repeated call: the same bytes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
    float_ms = C.c_float()
    assert lib.lcr_hap_coverage_ms(E.h, C.byref(float_ms)) == E_STATE                                    # no timing on this context
    # the next candidate stage ends the records' life; so does the next batch
    E.get_candidate_snps()
    assert get() == E_STATE and call() == E_STATE
    E.get_fragments().phase()
    re_ = check(E, b1, E.fragmat())                                                                      # stage re-entry: the same records
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, re_))
    E.load_batch_async(b2, 0).bind_batch(0)                                                              # lcr_bind_batch
    assert get() == E_STATE and call() == E_STATE
    E.run_all()
    assert get() == E_STATE                                                                              # (nothing stale from the last batch)
    got2 = check(E, b2, E.fragmat())
    E.close()
    # behind an asynchronous phase stage: the call settles it
    A = engine_cls(0, prm)
    A.set_async_phase(True)
    A.load_batch(b2).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
    fm2 = A.fragmat()
    A.phase()
    assert A.lib.lcr_hap_coverage(A.h) == 0
    gota = check(A, b2, fm2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got2, gota))
    A.close()
    # the timer
    T = engine_cls(0, prm, timing=True)
    with pytest.raises(Exception):
        T.hap_coverage_ms()
    T.load_batch(b1).run_all()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(T.hap_coverage(), first)) and T.hap_coverage_ms() > 0.0
    T.close()

"""K15 lcr_isoforms on the GPU against the plain-Python restatement of its contract (tests/isoforms_ref.py): every field of every record,
the offsets, the chain pool and row_isoform, exactly, in pinned host memory and in HBM.  Rows are put on chosen haplotypes and phase
sets with Engine.haplotag and hand-picked sites (test_hap_coverage_gpu's `tagged`: a class-1 read carries the reference base at a site,
a class-2 read the alternate, a class-0 read N); the restatement takes the engine's own assignment and phase sets, and the tests that
depend on a class or a phase set assert it.  Haplotag never hands out phase set 0 with an assignment, so the one test that needs it
rewrites the read records in HBM, which is what the kernels read."""
import ctypes as C

import numpy as np
import pytest

import helpers
import isoforms_ref as ref
import test_hap_coverage_gpu as tc
import test_haplotag_gpu as th
import test_isoforms_host as ih
import test_junctions_gpu as tj
from longcallr_amd import _abi, _lib, isoforms, synth

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
CELLS = ih.CELLS


def outputs(E):
    """the last isoforms()'s four outputs, from pinned host memory and from HBM"""
    o = E._isoform_list()
    pinned = []
    for ptr, dt, n in ((o.iso, _abi.ISOFORM_DTYPE, o.n_isoforms), (o.iso_region_off, np.int32, o.n_regions + 1), (o.chain, np.uint64, o.n_chain),
                       (o.row_isoform, np.int32, o.n_rows)):
        assert bool(ptr) == (n > 0)                               # NULL exactly where a count is 0
        buf = (C.c_char * (np.dtype(dt).itemsize * n)).from_address(ptr) if n else b""
        pinned.append(np.frombuffer(buf, dtype=dt, count=n).copy())
    for ptr, n in ((o.dev_iso, o.n_isoforms), (o.dev_chain, o.n_chain), (o.dev_row_isoform, o.n_rows)):
        assert bool(ptr) == (n > 0)
    hbm = [tc.dev_copy(o.dev_iso, _abi.ISOFORM_DTYPE, o.n_isoforms), pinned[1], tc.dev_copy(o.dev_chain, np.uint64, o.n_chain),
           tc.dev_copy(o.dev_row_isoform, np.int32, o.n_rows)]
    return pinned, hbm


def as_bytes(outs):
    return [x.tobytes() for x in outs]


def check(E, b, fm, min_count, min_junctions, assignment=None, phase_set=None):
    """isoforms() against the restatement on the engine's own assignment and phase sets, host and HBM; row_isoform against the pool
    -> (records, offsets, pool, row_isoform)"""
    pr = E.phase_result()
    asg = pr["assignment"] if assignment is None else assignment
    ps = pr["phase_set"] if phase_set is None else phase_set
    rec, off, pool, row_iso = E.isoforms(min_count, min_junctions)
    want = ref.isoforms(b, fm["row_region_off"], fm["row_read"], asg, ps, min_count, min_junctions)
    assert rec.dtype == _abi.ISOFORM_DTYPE and pool.dtype == np.uint64 and off.dtype == np.int32 and row_iso.dtype == np.int32
    for f in _abi.ISOFORM_DTYPE.names:
        assert rec[f].tolist() == want[0][f].tolist(), f
    assert off.tolist() == want[1].tolist()
    assert pool.tolist() == want[2].tolist()
    assert row_iso.tolist() == want[3].tolist() and row_iso.size == int(fm["row_region_off"][-1])
    pinned, hbm = outputs(E)
    assert as_bytes(pinned) == as_bytes((rec, off, pool, row_iso)) == as_bytes(hbm)          # HBM and host hold the same bytes
    # row_isoform: for every j the rows with value j number n_reads[j], and each of them holds exactly pool chain j
    ch = isoforms.chains(rec, pool)
    assert np.bincount(row_iso[row_iso >= 0], minlength=rec.size).tolist() == rec["n_reads"].tolist()
    for r in np.flatnonzero(row_iso >= 0):
        assert ref.read_chain(b, int(fm["row_read"][r]))[0] == ch[row_iso[r]] and asg[r] in (1, 2)
    return rec, off, pool, row_iso


def summary(rec, pool):
    return ih.summary(rec, pool)


def cells(r):
    return tuple(int(r[f]) for f in CELLS)


def region(start0, length, sites, reads, seed):
    """test_hap_coverage_gpu.cov_region with the reads' order kept: [(column, CIGAR, class)] must come sorted by column"""
    assert [c for c, _, _ in reads] == sorted(c for c, _, _ in reads)
    return tc.cov_region(start0, length, sites, reads, seed)


# ---- 1. the worked instance of the contract -------------------------------------------------------------------------------------------
def test_worked_instance(engine_cls):
    regs = [region(1000, 300, (5,), [(0, cig, cls) for cig, cls in ih.WORKED], 31)]
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(5,)], {(0, 5): 7})
    assert tc.got_classes(b, fm, E) == [cls for _, cls in ih.WORKED]
    rec, off, pool, row_iso = check(E, b, fm, 1, 1)
    assert summary(rec, pool) == ih.WORKED_WANT and off.tolist() == [0, 4]
    assert rec["phase_set"].tolist() == [7] * 4 and rec["n_phase_sets"].tolist() == [1] * 4
    assert row_iso.tolist() == [1, 1, 1, 2, 0, -1, -1, 3]
    rec, off, pool, row_iso = check(E, b, fm, 2, 1)
    assert summary(rec, pool) == [ih.WORKED_WANT[1]] and row_iso.tolist() == [0, 0, 0, -1, -1, -1, -1, -1]
    E.close()


# ---- 2. chain identity ----------------------------------------------------------------------------------------------------------------
def long_cigar(k, last_len):
    """k junctions of length 10 (the last one last_len) between exons of I / D / S / = / X / M ops: 5 reference columns each, more than
    2 k ops in all, so the CIGAR crosses the walk's rounds of 16 ops (k = 7: once, 17: three times, 33: six times)"""
    exons = ["5=", "2M2I3M", "2X1D2M", "5M"]
    out = ["3S20M"]
    for j in range(k):
        out.append("%dN" % (last_len if j == k - 1 else 10))
        out.append(exons[j % len(exons)])
    return "".join(out) + "2S"


IDENTITY = ["20M10N10M10N10M",                 # P = [(20, 10), (40, 10)]
            "20M10N5M0N5M10N10M",              # P again: the 0N in the middle is no junction
            "20M10N30M",                       # its proper prefix
            "20M10N10M11N9M",                  # equal but for one l
            "20M10N10M10N10M10N10M",           # Q = [(20, 10), (40, 10), (60, 10)]
            "20M10N11M9N10M10N10M"]            # Q's first and last junction, a different middle: (41, 9)
IDENTITY += [long_cigar(k, last) for k in (7, 17, 33) for last in (10, 11)]


def test_chain_identity(engine_cls):
    import re
    n_ops = [len(re.findall(r"\d+[MIDNSHP=X]", long_cigar(k, 10))) for k in (7, 17, 33)]
    assert [n // 16 for n in n_ops] == [1, 3, 6]
    regs = [region(20000, 800, (5,), [(0, cig, 1 + k % 2) for k, cig in enumerate(IDENTITY)], 32)]
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(5,)])
    assert tc.got_classes(b, fm, E) == [1 + k % 2 for k in range(len(IDENTITY))]
    rec, off, pool, row_iso = check(E, b, fm, 1, 1)
    ch = [[(s - 20000, l) for s, l in c] for c in isoforms.chains(rec, pool)]
    assert rec.size == 11 and row_iso[0] == row_iso[1] and sorted(row_iso.tolist()[1:]) == list(range(11))      # the 0N read joins P; every other read has a chain of its own
    P, Q = [(20, 10), (40, 10)], [(20, 10), (40, 10), (60, 10)]
    assert ch[0] == [(20, 10)]                                           # a proper prefix comes first
    assert [c for c in ch if len(c) <= 3] == [[(20, 10)], P, Q, [(20, 10), (40, 11)], [(20, 10), (41, 9), (60, 10)]]
    assert ch.index(P) == row_iso[0] and [int(n) for n in rec["n_reads"]] == [2 if c == P else 1 for c in ch]
    for k in (7, 17, 33):        # the twins differ in the last junction only, and are two records with one read each
        a, t = sorted(c for c in ch if len(c) == k)
        assert a[:-1] == t[:-1] and a[-1][0] == t[-1][0] and (a[-1][1], t[-1][1]) == (10, 11)
    E.close()


# ---- 3. presence ----------------------------------------------------------------------------------------------------------------------
PRESENCE = [("50M30N20M40N60M", 1), ("50M30N20M40N60M", 1),        # X = [(50, 30), (100, 40)], extent [50, 140)
            ("50M90N60M", 2),                                       # exon skipping: one junction covers both: absent
            ("50M30N20M45N55M", 2),                                 # a junction that straddles e: absent
            ("45M35N20M40N60M", 2),                                 # a junction that straddles a: absent
            ("10M10N30M30N20M40N20M10N30M", 1),                     # extra introns on either side of the extent: present
            ("50M30N20M", 2),                                       # ends inside the extent: neither
            ("50M30N20M39N1M", 1)]                                  # rend == e behind (100, 39): spans, absent


def test_presence(engine_cls):
    regs = [region(30000, 260, (5,), [(0, cig, cls) for cig, cls in PRESENCE], 33)]
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(5,)])
    assert tc.got_classes(b, fm, E) == [cls for _, cls in PRESENCE]
    rec, off, pool, row_iso = check(E, b, fm, 2, 1)
    assert isoforms.chains(rec, pool) == [[(30050, 30), (30100, 40)]]
    assert (int(rec["start0"][0]), int(rec["end0"][0]), int(rec["n_reads"][0])) == (30050, 30140, 2)
    assert cells(rec[0]) == (1, 3, 3, 0)
    check(E, b, fm, 1, 1)
    E.close()


def test_chain_at_the_read_ends(engine_cls):
    """pos == a (a CIGAR that begins with N) and rend == e (one that ends with N): both span and are present"""
    reads = [(0, "20M30N20M", 1), (0, "20M30N", 1), (0, "21M29N20M", 1), (20, "30N20M", 2), (21, "29N20M", 2)]
    regs = [region(35000, 100, (5, 60), reads, 34)]
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(5, 60)])
    assert tc.got_classes(b, fm, E) == [1, 1, 1, 2, 2]
    rec, off, pool, row_iso = check(E, b, fm, 1, 1)
    ch = [[(s - 35000, l) for s, l in c] for c in isoforms.chains(rec, pool)]
    assert ch == [[(20, 30)], [(21, 29)]] and rec["n_reads"].tolist() == [3, 2]
    assert cells(rec[0]) == (1, 2, 0, 1)        # the read at column 21 starts inside the extent: neither
    E.close()


# ---- 4. phase sets --------------------------------------------------------------------------------------------------------------------
def ps_reads(n5, n15, n25):
    """n5 / n15 / n25 reads that cover the site at column 5 / 15 / 25 only (a D op steps over the others) and hold one chain, (60, 30)"""
    return ([(0, "10M30D20M30N20M", 1 + k % 2) for k in range(n5)] + [(10, "10M20D20M30N20M", 1 + k % 2) for k in range(n15)]
            + [(20, "10M10D20M30N20M", 1 + k % 2) for k in range(n25)])


def test_phase_sets(engine_cls):
    E = tc.engine(engine_cls)
    for g, (counts, pss, want_ps) in enumerate([((2, 4, 3), (30, 20, 10), 20),        # a majority
                                                ((3, 2, 3), (30, 20, 10), 10),        # a tie goes to the smaller value
                                                ((3, 3, 3), (5, 9, 7), 5)]):
        regs = [region(40000, 200, (5, 15, 25), ps_reads(*counts), 35 + g)]
        b, fm = tc.tagged(E, regs, [(5, 15, 25)], {(0, 5): pss[0], (0, 15): pss[1], (0, 25): pss[2]})
        pr = E.phase_result()
        assert pr["phase_set"].tolist() == [pss[0]] * counts[0] + [pss[1]] * counts[1] + [pss[2]] * counts[2] and (pr["assignment"] != 0).all()
        rec, off, pool, row_iso = check(E, b, fm, 1, 1)
        assert rec.size == 1 and int(rec["n_reads"][0]) == sum(counts) and int(rec["n_phase_sets"][0]) == 3
        n = counts[pss.index(want_ps)]
        assert int(rec["phase_set"][0]) == want_ps and cells(rec[0]) == (0, (n + 1) // 2, 0, n // 2)
        assert (int(rec["n_h1"][0]), int(rec["n_h2"][0])) == tuple(sum((c + 1 - h) // 2 for c in counts) for h in (0, 1))
    # phase set 0 as the winner: the rows of the largest group lose their phase set in the read records the kernels read
    ptr, n = E.read_records_device()
    recs = tc.dev_copy(ptr, _abi.READ_REC_DTYPE, n)
    ps = pr["phase_set"].copy()
    ps[ps == 9] = 0
    recs["phase_set"] = ps
    assert _lib.load().hipMemcpy(C.c_void_p(ptr), C.c_void_p(recs.ctypes.data), C.c_size_t(recs.nbytes), 1) == 0
    rec, off, pool, row_iso = check(E, b, fm, 1, 1, phase_set=ps)
    assert (int(rec["phase_set"][0]), int(rec["n_phase_sets"][0])) == (0, 3) and cells(rec[0]) == (0, 2, 0, 1)
    E.close()


# ---- 5. thresholds --------------------------------------------------------------------------------------------------------------------
def test_thresholds(engine_cls):
    k1, k2, k3 = "20M10N60M", "20M10N20M10N30M", "20M10N20M10N10M10N10M"
    reads = [(0, "90M", 1)] * 2 + [(0, k1, 1)] * 3 + [(0, k2, 2)] * 4 + [(0, k3, 1)] * 4
    regs = [region(50000, 120, (5,), reads, 38)]
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(5,)])
    assert tc.got_classes(b, fm, E) == [c for _, _, c in reads]
    C1, C2, C3 = [(50020, 10)], [(50020, 10), (50050, 10)], [(50020, 10), (50050, 10), (50070, 10)]
    rec, _, pool, _ = check(E, b, fm, 4, 1)          # n_reads at min_count - 1 (k1: 3 rows) and at min_count
    assert isoforms.chains(rec, pool) == [C2, C3] and rec["n_reads"].tolist() == [4, 4]
    assert cells(rec[0]) == (3, 4, 0, 4)              # the rows of the chain that is not kept still count: absent in C2's extent
    rec, _, pool, _ = check(E, b, fm, 3, 1)          # k = 0 takes no part at min_junctions 1, k = 1 does
    assert isoforms.chains(rec, pool) == [C1, C2, C3] and cells(rec[0]) == (0, 7, 0, 4)
    rec, _, pool, row_iso = check(E, b, fm, 4, 3)    # k = 2 takes no part at min_junctions 3, k = 3 does
    assert isoforms.chains(rec, pool) == [C3] and cells(rec[0]) == (0, 4, 0, 0) and row_iso.tolist() == [-1] * 9 + [0] * 4
    rec, _, pool, _ = check(E, b, fm, 4, 2)
    assert isoforms.chains(rec, pool) == [C2, C3] and cells(rec[0]) == (0, 4, 0, 4)
    rec, _, _, _ = check(E, b, fm, 5, 1)
    assert rec.size == 0
    E.close()


# ---- 6. regions -----------------------------------------------------------------------------------------------------------------------
def region_batch():
    """Regions 0 and 1 hold the same chain (1020, 1500): region 1's reads start left of its window.  Region 2 has no participating
    row, region 3 one row whose chain nobody shares."""
    return ([region(1000, 100, (5,), [(0, "20M1500N20M", 1), (0, "20M1500N20M", 2)], 41),
             region(2500, 100, (25,), [(-1500, "20M1500N20M", 1), (-1500, "20M1500N20M", 2), (-1500, "20M1500N20M", 2)], 42),
             region(5000, 100, (5,), [(0, "90M", 1), (0, "90M", 2)], 43),
             region(6000, 100, (5,), [(0, "20M10N20M", 1), (0, "90M", 2)], 44)], [(5,), (25,), (5,), (5,)])


def test_regions(engine_cls):
    regs, sites = region_batch()
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, sites)
    assert tc.got_classes(b, fm, E) == [1, 2, 1, 2, 2, 1, 2, 1, 2]
    rec, off, pool, row_iso = check(E, b, fm, 2, 1)
    assert off.tolist() == [0, 1, 2, 2, 2] and rec["region"].tolist() == [0, 1] and rec["n_reads"].tolist() == [2, 3]
    assert isoforms.chains(rec, pool) == [[(1020, 1500)]] * 2 and rec["chain_first"].tolist() == [0, 1]      # the same chain stays two records
    assert row_iso.tolist() == [0, 0, 1, 1, 1, -1, -1, -1, -1]
    rec, off, pool, row_iso = check(E, b, fm, 1, 1)
    assert off.tolist() == [0, 1, 2, 2, 3]
    # nothing kept in the whole batch: counts 0, NULL pointers (outputs() asserts them), row_isoform all -1
    rec, off, pool, row_iso = check(E, b, fm, 4, 1)
    o = E._isoform_list()
    assert (o.n_regions, o.n_isoforms, o.n_chain, o.n_rows) == (4, 0, 0, 9) and not o.iso and not o.dev_iso and not o.chain and not o.dev_chain
    assert off.tolist() == [0] * 5 and row_iso.tolist() == [-1] * 9
    rec, off, pool, row_iso = check(E, b, fm, 1, 2)      # no participating row in the whole batch
    assert rec.size == 0 and row_iso.tolist() == [-1] * 9
    E.close()


# ---- 7. collisions, 10. determinism ---------------------------------------------------------------------------------------------------
def many_chain_regions():
    """region 0: 48 distinct chains (40 of one junction, 8 of two), some held by two or three reads; regions 1 and 2: a few of the same shapes"""
    cig = ["20M%dN20M" % (10 + j) for j in range(40)] + ["20M10N10M%dN20M" % (10 + j) for j in range(8)]
    reads0 = [(0, cig[j % len(cig)], 1 + (j // 3) % 2) for j in range(80)]
    return ([region(60000, 140, (5,), reads0, 45), region(61000, 140, (5,), [(0, cig[j], 1 + j % 2) for j in (0, 1, 0, 41, 41, 7)], 46),
             region(62000, 140, (5,), [(0, cig[3], 2)] * 5, 47)], [(5,), (5,), (5,)])


def test_collisions_and_determinism(engine_cls):
    regs, sites = many_chain_regions()
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, sites)
    got = {}
    for bits in (0, 1, 64):
        E.debug_set("iso_hash_bits", bits)
        rec, off, pool, row_iso = check(E, b, fm, 1, 1)
        got[bits] = as_bytes((rec, off, pool, row_iso))
        assert off.tolist() == [0, 48, 52, 53]
    assert got[0] == got[1] == got[64]
    assert E.lib.lcr_debug_set(E.h, b"iso_hash_bits", 7) == 0
    again = as_bytes(check(E, b, fm, 1, 1))               # a second call on the same engine
    F = tc.engine(engine_cls)                             # and one on a fresh engine
    b2, fm2 = tc.tagged(F, regs, sites)
    fresh = as_bytes(check(F, b2, fm2, 1, 1))
    assert again == got[64] == fresh
    F.close()
    E.close()


# ---- 9. state and arguments -----------------------------------------------------------------------------------------------------------
def test_state_and_arguments(engine_cls):
    s0, refseq, rs = tj.allele_specific_region()
    b = tj.batch_of([(s0, refseq, rs)])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=7))
    lib, lst = E.lib, _abi.LcrIsoformList()
    p10, p0 = _abi.LcrIsoformParams(10, 1), _abi.LcrIsoformParams(10, 0)
    E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
    assert lib.lcr_isoforms(E.h, C.byref(p10)) == E_STATE and lib.lcr_get_isoforms(E.h, C.byref(lst)) == E_STATE
    E.phase()
    assert lib.lcr_get_isoforms(E.h, C.byref(lst)) == E_STATE                   # no records yet
    assert lib.lcr_isoforms(E.h, None) == E_ARG and lib.lcr_isoforms(E.h, C.byref(p0)) == E_ARG
    assert lib.lcr_get_isoforms(E.h, C.byref(lst)) == E_STATE                   # a refused call leaves nothing behind
    before = (E.phase_result(), E.candidates(), E.junctions(10, 0))
    fm = E.fragmat()
    rec, off, pool, row_iso = check(E, b, fm, 10, 1)
    assert (before[0]["assignment"] != 0).all()
    assert isoforms.chains(rec, pool) == [[(5800, 300), (6400, 500)], [(5800, 1100)]] and rec["n_reads"].tolist() == [20, 20]
    assert sorted([cells(rec[0]), cells(rec[1])]) == [(0, 20, 20, 0), (20, 0, 0, 20)]
    first = as_bytes(outputs(E)[0])
    assert lib.lcr_isoforms(E.h, None) == E_ARG and lib.lcr_isoforms(E.h, C.byref(p0)) == E_ARG
    assert as_bytes(outputs(E)[0]) == first                                     # the previous records still answer
    assert check(E, b, fm, 21, 1)[0].size == 0 and check(E, b, fm, 10, 2)[0].size == 1     # repetition with other parameters
    assert as_bytes(check(E, b, fm, 10, 1)) == first
    after = (E.phase_result(), E.candidates(), E.junctions(10, 0))
    for k in before[0]:
        assert before[0][k].tobytes() == after[0][k].tobytes(), k
    assert as_bytes(before[1]) == as_bytes(after[1]) and as_bytes(before[2]) == as_bytes(after[2])     # junctions(): the same bytes before and after
    with pytest.raises(Exception):
        E.isoforms_ms()                                                         # timing is off
    # the asynchronous phase stage is collected first
    A = engine_cls(0, _abi.make_params("hifi-masseq", seed=7))
    A.set_async_phase(True)
    A.load_batch(b).run_all()
    assert as_bytes(A.isoforms(10, 1)) == first
    A.close()
    # the same batch behind haplotag(): the same chains, tagged on the sites' haplotypes (A's reads carry the alternate base: class 2)
    d = {s0 + c: (refseq[c].upper(), tj.ALT[refseq[c].upper()], 77) for c in (150, 300, 450, 600, 2050, 2200, 2350, 2500)}
    pos = np.array(sorted(d), np.int64)
    fm, _, _ = th.staged(E, b, (pos, np.ones(pos.size, np.uint8), np.full(pos.size, 30.0, np.float32)))
    assert lib.lcr_get_isoforms(E.h, C.byref(lst)) == E_STATE                   # a new candidate stage drops the phase results, and the records with them
    assert lib.lcr_isoforms(E.h, C.byref(p10)) == E_STATE
    E.haplotag(th.site_arrays(d))
    assert lib.lcr_get_isoforms(E.h, C.byref(lst)) == E_STATE
    rec, off, pool, row_iso = check(E, b, fm, 10, 1)
    assert isoforms.chains(rec, pool) == [[(5800, 300), (6400, 500)], [(5800, 1100)]] and rec["phase_set"].tolist() == [77, 77]
    assert [cells(rec[0]), cells(rec[1])] == [(20, 0, 0, 20), (0, 20, 20, 0)]
    assert lib.lcr_enable_timing(E.h, 1) == 0
    check(E, b, fm, 10, 1)
    assert E.isoforms_ms() > 0.0
    E.load_batch(b)
    assert lib.lcr_get_isoforms(E.h, C.byref(lst)) == E_STATE                   # ... and so does a new binding
    E.close()


# ---- 11. the three-isoform region of test_junctions_gpu --------------------------------------------------------------------------------
def test_three_isoforms(engine_cls):
    iso = ["600M50N40M50N40M50N40M50N40M50N40M", "600M50N40M140N40M50N40M50N40M30N40M", "600M70N20M50N40M140N40M50N40M50N20M"]
    reads = []
    for k in range(600):       # isoform 0: 300 reads, 70 % on haplotype A; 1: 200 reads, 30 %; 2: 100 reads, half
        i = 0 if k < 300 else 1 if k < 500 else 2
        reads.append((0, iso[i], (k * 7 % 10) < (7, 3, 5)[i]))
    refseq, rs = tj.build_region(8000, 1300, tj.ANCHOR, reads, 21)
    b = tj.batch_of([(8000, refseq, rs)])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    E.load_batch(b).run_all()
    fm = E.fragmat()
    assert (E.phase_result()["assignment"] != 0).all()
    rec, off, pool, row_iso = check(E, b, fm, 10, 1)
    assert rec.size == 3 and sorted(rec["n_reads"].tolist()) == [100, 200, 300] and rec["n_junc"].tolist() == [5, 5, 5]
    assert (rec["n_h1"] + rec["n_h2"]).tolist() == rec["n_reads"].tolist()
    k = int(np.argmax(rec["n_reads"]))      # the 300-read chain ends first: all 600 rows span it, its own are present
    assert sum(cells(rec[k])) == 600 and int(rec["h1_present"][k]) + int(rec["h2_present"][k]) == 300
    E.close()


# ---- 12. larger workloads --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ont-cdna", "demo"])
def test_synth_and_demo(engine_cls, which):
    """The counts these workloads give are printed and recorded in DESIGN.md section 1m; nothing is asserted beyond equality with the
    restatement."""
    if which == "demo":
        b, prm = helpers.demo_batch(), _abi.make_params("hifi-masseq")
    else:
        b, prm = synth.make_batch("ont-cdna", n_genes=4), _abi.make_params("ont-cdna")
    E = engine_cls(0, prm)
    E.load_batch(b).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    n = {}
    for mc, mj in ((10, 1), (2, 1)):
        rec, off, pool, row_iso = check(E, b, fm, mc, mj)
        n[(mc, mj)] = (int(rec.size), int(pool.size), int((row_iso >= 0).sum()))
    print("%s: rows %d, assigned %d, (kept chains, pool entries, rows with a kept chain) %r"
          % (which, pr["assignment"].size, int((pr["assignment"] != 0).sum()), n))
    E.close()

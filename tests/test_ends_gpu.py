"""K16 lcr_transcript_ends on the GPU against the plain-Python restatement of its contract (tests/ends_ref.py): every field of every record,
the offsets, row_site and the totals, exactly, in pinned host memory and in HBM.  Rows are put on chosen haplotypes and phase sets with
Engine.haplotag and hand-picked sites (test_hap_coverage_gpu's `tagged`: a class-1 read carries the reference base at a site, a class-2
read the alternate, a class-0 read N), and on chosen transcript strands through their flags; the restatement takes the engine's own
assignment and phase sets, and every test asserts the property it was built for on the restatement's output."""
import ctypes as C

import numpy as np
import pytest

import ends_ref as ref
import helpers
import test_ends_host as eh
import test_hap_coverage_gpu as tc
import test_haplotag_gpu as th
import test_junctions_gpu as tj
from longcallr_amd import _abi, _lib, synth

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
CELLS = eh.CELLS
PLUS, MINUS, NONE = eh.PLUS, eh.MINUS, eh.NONE
MODES = {"ts": 0, "read": 1}


def outputs(E):
    """the last transcript_ends()'s outputs, from pinned host memory and from HBM, and its totals"""
    o = E._end_list()
    pinned = []
    for ptr, dt, n in ((o.site, _abi.END_SITE_DTYPE, o.n_sites), (o.site_region_off, np.int32, o.n_regions + 1), (o.row_site, np.int32, 2 * o.n_rows)):
        assert bool(ptr) == (n > 0)                               # NULL exactly where a count is 0
        buf = (C.c_char * (np.dtype(dt).itemsize * n)).from_address(ptr) if n else b""
        pinned.append(np.frombuffer(buf, dtype=dt, count=n).copy())
    for ptr, n in ((o.dev_site, o.n_sites), (o.dev_row_site, o.n_rows)):
        assert bool(ptr) == (n > 0)
    hbm = [tc.dev_copy(o.dev_site, _abi.END_SITE_DTYPE, o.n_sites), pinned[1], tc.dev_copy(o.dev_row_site, np.int32, 2 * o.n_rows)]
    return pinned, hbm, (int(o.n_part), int(o.n_assigned))


def as_bytes(outs):
    return [x.tobytes() for x in outs[:3]] + [sorted(outs[3].items())]


def check(E, b, fm, min_count, window, mode="ts", assignment=None, phase_set=None):
    """transcript_ends() against the restatement on the engine's own assignment and phase sets, host and HBM
    -> (records, offsets, row_site, totals)"""
    pr = E.phase_result()
    asg = pr["assignment"] if assignment is None else assignment
    ps = pr["phase_set"] if phase_set is None else phase_set
    rec, off, row_site, tot = E.transcript_ends(min_count, window, mode)
    want = ref.transcript_ends(b, fm["row_region_off"], fm["row_read"], asg, ps, min_count, window, mode)
    assert rec.dtype == _abi.END_SITE_DTYPE and off.dtype == np.int32 and row_site.dtype == np.int32
    for f in _abi.END_SITE_DTYPE.names:
        assert rec[f].tolist() == want[0][f].tolist(), f
    assert off.tolist() == want[1].tolist()
    assert row_site.shape == (int(fm["row_region_off"][-1]), 2) and row_site.tolist() == want[2].tolist()
    assert tot == want[3]
    assert [x.tobytes() for x in (rec, off, row_site)] == [x.tobytes() for x in want[:3]]          # all output bytes
    pinned, hbm, totals = outputs(E)
    assert [x.tobytes() for x in pinned] == [x.tobytes() for x in (rec, off, row_site)] == [x.tobytes() for x in hbm]     # HBM and host hold the same bytes
    assert totals == (tot["n_part"], tot["n_assigned"])
    # row_site: for every record j the ends with value j number n_reads[j]
    assert np.bincount(row_site[row_site >= 0], minlength=rec.size).tolist() == rec["n_reads"].tolist()
    assert int((row_site >= 0).sum()) == tot["n_assigned"]
    return rec, off, row_site, tot


def summary(rec):
    return eh.summary(rec)


def cells(r):
    return tuple(int(r[f]) for f in CELLS)


def region(start0, length, sites, reads, seed):
    """test_hap_coverage_gpu.cov_region with the reads' order kept and their flags set: [(column, CIGAR, class, (ts, rev))] must come
    sorted by column"""
    assert [r[0] for r in reads] == sorted(r[0] for r in reads)
    s0, refseq, out = tc.cov_region(start0, length, sites, [r[:3] for r in reads], seed)
    for d, r in zip(out, reads):        # (the sort by position is stable)
        d["ts"], d["rev"] = r[3]
    return s0, refseq, out


def classes_of(regs):
    return [r["cls"] for _, _, rs in regs for r in rs]


def sites_at(rec, g, strand, side):
    return [s for s, r in zip(summary(rec), rec) if int(r["region"]) == g and s[1] == strand and s[2] == side]


# ---- 1. the worked instance of the contract -------------------------------------------------------------------------------------------
def test_worked_instance(engine_cls):
    regs = [region(1000, 300, (5,), eh.WORKED, 31)]
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(5,)], {(0, 5): 7})
    assert tc.got_classes(b, fm, E) == [r[2] for r in eh.WORKED]
    rec, off, row_site, tot = check(E, b, fm, 2, 2)
    assert summary(rec) == eh.WORKED_WANT and off.tolist() == [0, 5] and row_site.tolist() == eh.WORKED_ROW_SITE
    assert rec["phase_set"].tolist() == [7] * 5 and rec["n_phase_sets"].tolist() == [1] * 5 and tot == dict(n_part=9, n_assigned=15)
    rec, off, row_site, tot = check(E, b, fm, 2, 2, "read")
    assert tot == dict(n_part=10, n_assigned=17) and summary(rec)[0][5] == (6, 4, 2, 4)
    rec, off, row_site, tot = check(E, b, fm, 1, 2)
    assert [s[0] for s in summary(rec)] == [1000, 1004, 1059, 1059, 1062, 1119] and row_site[7].tolist() == [-1, 4]
    E.close()


# ---- 2. the peak rule -------------------------------------------------------------------------------------------------------------------
def stack(cols_counts, right_col, cls0=1):
    """count reads per left column, all ending at right_col; classes alternate"""
    out, k = [], cls0
    for col, n in cols_counts:
        for _ in range(n):
            out.append((col, "%dM" % (right_col + 1 - col), 1 + k % 2, PLUS))
            k += 1
    return out


def test_peak_rule(engine_cls):
    W = 4
    regs = [region(1000, 200, (50,), stack([(0, 3), (W, 3)], 99), 32),                   # (3, 3) at x and x + W: one peak, the smaller
            region(2000, 200, (50,), stack([(0, 3), (W + 1, 3)], 99), 33),               # (3, 3) at x and x + W + 1: two
            region(3000, 200, (50,), stack([(0, 3), (W, 5), (2 * W, 7)], 99), 34)]       # (3, 5, 7): only the last is a peak
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(50,)] * 3)
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    rec, off, row_site, tot = check(E, b, fm, 1, W)
    assert [(s[0], s[5][0]) for s in sites_at(rec, 0, 1, 0)] == [(1000, 6)]
    assert [(s[0], s[5][0]) for s in sites_at(rec, 1, 1, 0)] == [(2000, 3), (2005, 3)]
    assert [(s[0], s[4], s[5]) for s in sites_at(rec, 2, 1, 0)] == [(3008, (3004, 3008), (12, 6, 6, 7))]
    ro = fm["row_region_off"]
    assert row_site[ro[2]:ro[2] + 3, 0].tolist() == [-1] * 3 and (row_site[ro[2] + 3:ro[3], 0] >= 0).all()     # x's ends unassigned, the middle one's assigned
    assert tot["n_assigned"] == 2 * tot["n_part"] - 3
    # W == 0: every distinct coordinate is a peak
    rec, off, _, tot = check(E, b, fm, 1, 0)
    assert off.tolist() == [0, 3, 6, 10] and tot["n_assigned"] == 2 * tot["n_part"]
    # a window of 4096: one peak per class and region, the largest count, the smaller coordinate among equals
    rec, off, _, tot = check(E, b, fm, 1, 4096)
    assert [(s[0], s[2], s[5][0]) for s in summary(rec)] == [(1000, 0, 6), (1099, 1, 6), (2000, 0, 6), (2099, 1, 6), (3008, 0, 15), (3099, 1, 15)]
    E.close()


# ---- 3. assignment ----------------------------------------------------------------------------------------------------------------------
def test_assignment(engine_cls):
    W = 3
    regs = [region(1000, 200, (50,), stack([(0, 2), (3, 1), (6, 2)], 99), 35),           # an end exactly between two peaks 2 k apart
            region(2000, 200, (50,), stack([(0, 5), (W, 2), (W + 1, 1)], 99), 36)]       # an end at distance W, one at W + 1 behind it
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(50,)] * 2)
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    rec, off, row_site, tot = check(E, b, fm, 1, W)
    assert [(s[0], s[4], s[5][0]) for s in sites_at(rec, 0, 1, 0)] == [(1000, (1000, 1003), 3), (1006, (1006, 1006), 2)]
    assert row_site[2, 0] == 0                                                            # ... goes to the smaller
    assert [(s[0], s[4], s[5][0]) for s in sites_at(rec, 1, 1, 0)] == [(2000, (2000, 2003), 7)]
    ro = fm["row_region_off"]
    assert row_site[ro[1]:ro[2], 0].tolist() == [int(off[1])] * 7 + [-1]                  # distance W: assigned; W + 1: a shoulder of a shoulder
    E.close()


# ---- 4. classes -------------------------------------------------------------------------------------------------------------------------
def test_classes(engine_cls):
    """column 50 is the right end of '+' and '-' rows and the left end of '+', '-' and untagged rows"""
    reads = ([(0, "51M", 1 + k % 2, PLUS) for k in range(2)] + [(0, "51M", 1 + k % 2, MINUS) for k in range(2)]
             + [(50, "40M", 1 + k % 2, PLUS) for k in range(2)] + [(50, "40M", 1 + k % 2, MINUS) for k in range(2)]
             + [(50, "40M", 1 + k % 2, NONE) for k in range(2)])
    regs = [region(1000, 120, (10, 60), reads, 37)]
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(10, 60)])
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    rec, off, row_site, tot = check(E, b, fm, 2, 2)
    at = [s for s in summary(rec) if s[0] == 1050]
    assert [(s[1], s[2], s[3], s[5][0]) for s in at] == [(1, 0, 0, 2), (1, 1, 1, 2), (2, 0, 1, 2), (2, 1, 0, 2)]     # '+' before '-', left before right; TSS / TES
    assert tot["n_part"] == 8 and row_site[8:].tolist() == [[-1, -1]] * 2                                            # untagged reads are dropped in "ts" mode
    rec, off, row_site, tot = check(E, b, fm, 2, 2, "read")
    at = [s for s in summary(rec) if s[0] == 1050]
    assert [(s[1], s[2], s[5][0]) for s in at] == [(1, 0, 4), (1, 1, 2), (2, 0, 2), (2, 1, 2)] and tot["n_part"] == 10   # ... and '+' rows in "read" mode
    E.close()


# ---- 5. spanning edges ------------------------------------------------------------------------------------------------------------------
def test_spanning_edges(engine_cls):
    W = 3
    reads = ([(50, "51M", 1 + k % 2, PLUS) for k in range(3)]          # a 3' site of '+' at column 100
             + [(97, "40M", 1, PLUS),                                    # pos == p - W, rend beyond p + W: absent
                (98, "40M", 2, PLUS),                                    # pos == p - W + 1: neither
                (150, "54M", 1, PLUS),                                   # rend == p + W + 1 at the 5' site at column 200: absent
                (150, "53M", 2, PLUS),                                   # rend == p + W: neither
                (150, "20M100N20M", 2, PLUS)]                            # an N op covers the window: absent
             + [(200, "50M", 1 + k % 2, PLUS) for k in range(3)])
    regs = [region(0, 100, (1,), [(0, "3M", 1 + k % 2, PLUS) for k in range(3)] + [(0, "60M", 1, PLUS), (0, "60M", 2, PLUS)], 39),     # p < W
            region(1000, 400, (60, 110, 160, 210), reads, 38)]
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(1,), (60, 110, 160, 210)])
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    rec, off, row_site, tot = check(E, b, fm, 3, W)
    tes = [s for s in sites_at(rec, 1, 1, 1) if s[0] == 1100]
    tss = [s for s in sites_at(rec, 1, 1, 0) if s[0] == 1200]
    assert [(s[5][0], s[6]) for s in tes] == [(3, (1, 2, 0, 1))]                          # h1_absent: the read at p - W alone
    assert [(s[5][0], s[6]) for s in tss] == [(3, (1, 2, 1, 1))]                          # absent: the 54M read (h1) and the intron read (h2)
    low = sites_at(rec, 0, 1, 1)
    assert [(s[0], s[5][0], s[6]) for s in low] == [(2, 3, (0, 2, 0, 1))]                 # p = 2 < W: the two long reads cover [0, 60) and are not absent
    E.close()


# ---- 6. ends outside the window -----------------------------------------------------------------------------------------------------------
def test_ends_outside_the_window(engine_cls):
    """region 1's reads start left of its window and are region 0's reads again, as the flanks of a truncated region share reads"""
    regs = [region(1000, 100, (5,), [(0, "20M1500N20M", 1, PLUS), (0, "20M1500N20M", 2, PLUS)], 41),
            region(2500, 100, (25,), [(-1500, "20M1500N20M", 1, PLUS), (-1500, "20M1500N20M", 2, PLUS), (-1500, "20M1500N20M", 2, PLUS)], 42)]
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(5,), (25,)])
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    rec, off, row_site, tot = check(E, b, fm, 2, 10)
    assert [(int(r["region"]), s[0], s[2], s[5][0]) for r, s in zip(rec, summary(rec))] == [(0, 1000, 0, 2), (0, 2539, 1, 2), (1, 1000, 0, 3), (1, 2539, 1, 3)]
    assert row_site.tolist() == [[0, 1]] * 2 + [[2, 3]] * 3                               # the same coordinates stay two sites, one per region
    E.close()


# ---- 7. phase sets ----------------------------------------------------------------------------------------------------------------------
def ps_reads(n5, n15, n25):
    """n5 / n15 / n25 reads that cover the site at column 5 / 15 / 25 only (a D op steps over the others); all end at column 109"""
    return ([(0, "10M30D20M30N20M", 1 + k % 2, PLUS) for k in range(n5)] + [(10, "10M20D20M30N20M", 1 + k % 2, PLUS) for k in range(n15)]
            + [(20, "10M10D20M30N20M", 1 + k % 2, PLUS) for k in range(n25)])


def test_phase_sets(engine_cls):
    E = tc.engine(engine_cls)
    for g, (counts, pss, want_ps) in enumerate([((2, 4, 3), (30, 20, 10), 20),        # a majority
                                                ((3, 2, 3), (30, 20, 10), 10),        # a tie goes to the smaller value
                                                ((3, 3, 3), (5, 9, 7), 5)]):
        regs = [region(40000, 200, (5, 15, 25), ps_reads(*counts), 43 + g)]
        b, fm = tc.tagged(E, regs, [(5, 15, 25)], {(0, 5): pss[0], (0, 15): pss[1], (0, 25): pss[2]})
        pr = E.phase_result()
        assert pr["phase_set"].tolist() == [pss[0]] * counts[0] + [pss[1]] * counts[1] + [pss[2]] * counts[2] and (pr["assignment"] != 0).all()
        rec, off, row_site, tot = check(E, b, fm, 1, 2)
        assert [s[0] for s in summary(rec)] == [40000, 40010, 40020, 40109]
        r = rec[3]                                                                    # the 3' site every row ends at
        n = counts[pss.index(want_ps)]
        assert int(r["n_reads"]) == sum(counts) and int(r["n_phase_sets"]) == 3 and int(r["phase_set"]) == want_ps
        assert cells(r) == (0, (n + 1) // 2, 0, n // 2)
    # phase set 0 as the winner: the rows of the largest group lose their phase set in the read records the kernels read
    ptr, n = E.read_records_device()
    recs = tc.dev_copy(ptr, _abi.READ_REC_DTYPE, n)
    ps = pr["phase_set"].copy()
    ps[ps == 9] = 0
    recs["phase_set"] = ps
    assert _lib.load().hipMemcpy(C.c_void_p(ptr), C.c_void_p(recs.ctypes.data), C.c_size_t(recs.nbytes), 1) == 0
    rec, off, row_site, tot = check(E, b, fm, 1, 2, phase_set=ps)
    assert (int(rec["phase_set"][3]), int(rec["n_phase_sets"][3])) == (0, 3) and cells(rec[3]) == (0, 2, 0, 1)
    E.close()


# ---- 8. thresholds ----------------------------------------------------------------------------------------------------------------------
def test_thresholds(engine_cls):
    reads = stack([(0, 4), (20, 3)], 99)
    regs = [region(50000, 120, (50,), reads, 46)]
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(50,)])
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    rec, _, _, tot = check(E, b, fm, 4, 5)            # n_reads at min_count (4 rows) and at min_count - 1 (3 rows)
    assert [(s[0], s[2], s[5][0]) for s in summary(rec)] == [(50000, 0, 4), (50099, 1, 7)] and tot == dict(n_part=7, n_assigned=11)
    rec, _, _, _ = check(E, b, fm, 3, 5)
    assert [(s[0], s[5][0]) for s in summary(rec)] == [(50000, 4), (50020, 3), (50099, 7)]
    assert check(E, b, fm, 8, 5)[0].size == 0
    one = as_bytes(check(E, b, fm, 1, 5))
    assert as_bytes(check(E, b, fm, 0, 5)) == one     # min_count 0 is 1
    E.close()


# ---- 9. regions -------------------------------------------------------------------------------------------------------------------------
def test_regions(engine_cls):
    regs = [region(1000, 100, (5,), [(0, "60M", 1, PLUS), (0, "60M", 2, PLUS)], 47),
            region(2000, 100, (), [], 48),                                                                       # no reads
            region(3000, 100, (5,), [(0, "60M", 1, NONE), (0, "60M", 2, NONE), (0, "60M", 0, PLUS)], 49),       # rows, none participating
            region(4000, 100, (5,), [(0, "60M", 1, MINUS), (0, "60M", 2, MINUS), (0, "60M", 1, MINUS)], 50)]
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(5,), (), (5,), (5,)])
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    rec, off, row_site, tot = check(E, b, fm, 2, 10)
    assert off.tolist() == [0, 2, 2, 2, 4] and rec["region"].tolist() == [0, 0, 3, 3] and tot == dict(n_part=5, n_assigned=10)
    assert rec["kind"].tolist() == [0, 1, 1, 0]
    rec, off, row_site, tot = check(E, b, fm, 3, 10)
    assert off.tolist() == [0, 0, 0, 0, 2] and row_site[:5].tolist() == [[-1, -1]] * 5
    # nothing kept in the whole batch: counts 0, NULL record pointers (outputs() asserts them), row_site all -1
    rec, off, row_site, tot = check(E, b, fm, 4, 10)
    o = E._end_list()
    assert (o.n_regions, o.n_sites, o.n_rows, o.n_part, o.n_assigned) == (4, 0, 8, 5, 0) and not o.site and not o.dev_site
    assert off.tolist() == [0] * 5 and row_site.tolist() == [[-1, -1]] * 8
    E.close()
    # no participating row in the whole batch
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs[2:3], [(5,)])
    rec, off, row_site, tot = check(E, b, fm, 1, 10)
    assert rec.size == 0 and tot == dict(n_part=0, n_assigned=0) and row_site.tolist() == [[-1, -1]] * 3
    assert check(E, b, fm, 1, 10, "read")[3] == dict(n_part=2, n_assigned=4)
    E.close()


# ---- 10. table stress and determinism -----------------------------------------------------------------------------------------------------
def test_table_stress_and_determinism(engine_cls):
    """600 rows with all-distinct ends in one region: 1 200 keys in a segment of 4 096 slots"""
    reads = [(k, "%dM" % (700 + k), 1 + k % 2, (PLUS, MINUS)[(k // 2) % 2]) for k in range(600)]      # [k, 2 k + 700): every read covers column 650
    regs = [region(70000, 2000, (650,), reads, 51)]
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(650,)])
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    rec0, _, _, tot0 = check(E, b, fm, 1, 0)
    assert rec0.size == 1200 and tot0 == dict(n_part=600, n_assigned=1200)               # all ends distinct
    got = {}
    for bits in (32, 0, 3):
        E.debug_set("ends_hash_bits", bits)
        got[bits] = as_bytes(check(E, b, fm, 2, 10))
    assert got[0] == got[3] == got[32]
    assert E.lib.lcr_debug_set(E.h, b"ends_hash_bits", 32) == 0
    again = as_bytes(check(E, b, fm, 2, 10))              # a second call on the same engine
    F = tc.engine(engine_cls)                             # and one on a fresh engine
    b2, fm2 = tc.tagged(F, regs, [(650,)])
    fresh = as_bytes(check(F, b2, fm2, 2, 10))
    assert again == got[32] == fresh
    F.close()
    E.close()


# ---- 11. state and arguments ------------------------------------------------------------------------------------------------------------
def test_state_and_arguments(engine_cls):
    s0, refseq, rs = tj.allele_specific_region()
    b = tj.batch_of([(s0, refseq, rs)])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=7))
    lib, lst = E.lib, _abi.LcrEndList()
    p10 = _abi.LcrEndParams(10, 10, 0, 0)
    bad = [_abi.LcrEndParams(10, 4097, 0, 0), _abi.LcrEndParams(10, 10, 2, 0)]
    E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
    assert lib.lcr_transcript_ends(E.h, C.byref(p10)) == E_STATE and lib.lcr_get_transcript_ends(E.h, C.byref(lst)) == E_STATE
    E.phase()
    assert lib.lcr_get_transcript_ends(E.h, C.byref(lst)) == E_STATE            # no records yet
    assert lib.lcr_transcript_ends(E.h, None) == E_ARG and [lib.lcr_transcript_ends(E.h, C.byref(p)) for p in bad] == [E_ARG] * 2
    assert lib.lcr_get_transcript_ends(E.h, C.byref(lst)) == E_STATE            # a refused call leaves nothing behind
    alone_iso, alone_junc = [x.tobytes() for x in E.isoforms(10, 1)], [x.tobytes() for x in E.junctions(10, 0)]
    before = (E.phase_result(), E.candidates())
    fm = E.fragmat()
    rec, off, row_site, tot = check(E, b, fm, 10, 10)
    assert (before[0]["assignment"] != 0).all() and rec.size >= 2 and tot["n_part"] == row_site.shape[0] == 40
    first = as_bytes((rec, off, row_site, tot))
    assert lib.lcr_transcript_ends(E.h, None) == E_ARG and [lib.lcr_transcript_ends(E.h, C.byref(p)) for p in bad] == [E_ARG] * 2
    pinned, _, totals = outputs(E)
    assert [x.tobytes() for x in pinned] == first[:3] and totals == (tot["n_part"], tot["n_assigned"])      # the previous records still answer
    assert check(E, b, fm, 41, 10)[0].size == 0 and check(E, b, fm, 1, 0, "read")[0].size >= rec.size       # repetition with other parameters
    assert check(E, b, fm, 10, 4096)[0].size >= 2                                                           # the largest window
    assert as_bytes(check(E, b, fm, 10, 10)) == first
    # alongside lcr_isoforms and lcr_junctions, in either order: each call's bytes equal its bytes alone
    assert [x.tobytes() for x in E.isoforms(10, 1)] == alone_iso and [x.tobytes() for x in E.junctions(10, 0)] == alone_junc
    assert [x.tobytes() for x in outputs(E)[0]] == first[:3]
    assert as_bytes(check(E, b, fm, 10, 10)) == first
    assert [x.tobytes() for x in E.junctions(10, 0)] == alone_junc and [x.tobytes() for x in E.isoforms(10, 1)] == alone_iso
    after = (E.phase_result(), E.candidates())
    for k in before[0]:
        assert before[0][k].tobytes() == after[0][k].tobytes(), k
    assert [x.tobytes() for x in before[1]] == [x.tobytes() for x in after[1]]
    with pytest.raises(Exception):
        E.transcript_ends_ms()                                                  # timing is off
    with pytest.raises(ValueError):
        E.transcript_ends(10, 10, "both")
    # the asynchronous phase stage is collected first
    A = engine_cls(0, _abi.make_params("hifi-masseq", seed=7))
    A.set_async_phase(True)
    A.load_batch(b).run_all()
    assert as_bytes(A.transcript_ends(10, 10)) == first
    A.close()
    # the same batch behind haplotag()
    d = {s0 + c: (refseq[c].upper(), tj.ALT[refseq[c].upper()], 77) for c in (150, 300, 450, 600, 2050, 2200, 2350, 2500)}
    pos = np.array(sorted(d), np.int64)
    fm, _, _ = th.staged(E, b, (pos, np.ones(pos.size, np.uint8), np.full(pos.size, 30.0, np.float32)))
    assert lib.lcr_get_transcript_ends(E.h, C.byref(lst)) == E_STATE            # a new candidate stage drops the phase results, and the records with them
    assert lib.lcr_transcript_ends(E.h, C.byref(p10)) == E_STATE
    E.haplotag(th.site_arrays(d))
    assert lib.lcr_get_transcript_ends(E.h, C.byref(lst)) == E_STATE
    rec2, off2, _, tot2 = check(E, b, fm, 10, 10)
    assert rec2["peak0"].tolist() == rec["peak0"].tolist() and rec2["phase_set"].tolist() == [77] * rec.size and tot2 == tot
    assert lib.lcr_enable_timing(E.h, 1) == 0
    check(E, b, fm, 10, 10)
    assert E.transcript_ends_ms() > 0.0
    E.load_batch(b)
    assert lib.lcr_get_transcript_ends(E.h, C.byref(lst)) == E_STATE            # ... and so does a new binding
    E.close()


# ---- 12. larger workloads --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ont-cdna", "demo"])
def test_synth_and_demo(engine_cls, which):
    """The counts these workloads give are printed and recorded in DESIGN.md section 1o; beyond equality with the restatement only the
    peak rule's guarantee is asserted: W == 0 and min_count 1 keep a site whenever a row participates."""
    if which == "demo":
        b, prm = helpers.demo_batch(), _abi.make_params("hifi-masseq")
    else:
        b, prm = synth.make_batch("ont-cdna", n_genes=4), _abi.make_params("ont-cdna")
    E = engine_cls(0, prm)
    E.load_batch(b).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    n = {}
    for mc, w, mode in ((3, 10, "ts"), (10, 10, "ts"), (1, 0, "read")):
        rec, off, row_site, tot = check(E, b, fm, mc, w, mode)
        n[(mc, w, mode)] = (int(rec.size), tot["n_part"], tot["n_assigned"], int(((rec["h1_absent"] + rec["h2_absent"]) > 0).sum()),
                            sorted(set(zip(rec["strand"].tolist(), rec["side"].tolist()))))
    assert n[(1, 0, "read")][0] >= 1 or n[(1, 0, "read")][1] == 0
    print("%s: rows %d, assigned %d, (min_count, W, mode) -> (kept sites, participating rows, assigned ends, sites with absent rows, classes) %r"
          % (which, pr["assignment"].size, int((pr["assignment"] != 0).sum()), n))
    E.close()

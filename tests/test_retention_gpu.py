"""K17 lcr_intron_retention on the GPU against the plain-Python restatement of its contract (tests/retention_ref.py): every field of every
record, the offsets, row_retained and the totals, exactly, in pinned host memory and in HBM.  Rows are put on chosen haplotypes and phase
sets with Engine.haplotag and hand-picked sites (test_hap_coverage_gpu's `tagged`: a class-1 read carries the reference base at a site, a
class-2 read the alternate, a class-0 read N -- it stays untagged); the restatement takes the engine's own assignment and phase sets, and
every test asserts the property it was built for."""
import ctypes as C

import numpy as np
import pytest

import retention_ref as ref
import test_hap_coverage_gpu as tc
import test_haplotag_gpu as th
import test_junctions_gpu as tj
import test_retention_host as rh
from longcallr_amd import _abi, _lib

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
CELLS = rh.CELLS
BLOCK = 256     # LCR_BLOCK: threads of the workgroup that serves one kept intron


def outputs(E):
    """the last intron_retention()'s outputs, from pinned host memory and from HBM, and its totals"""
    o = E._retention_list()
    pinned = []
    for ptr, dt, n in ((o.intron, _abi.RETAINED_INTRON_DTYPE, o.n_introns), (o.intron_region_off, np.int32, o.n_regions + 1),
                       (o.row_retained, np.int32, o.n_rows)):
        assert bool(ptr) == (n > 0)                               # NULL exactly where a count is 0
        buf = (C.c_char * (np.dtype(dt).itemsize * n)).from_address(ptr) if n else b""
        pinned.append(np.frombuffer(buf, dtype=dt, count=n).copy())
    for ptr, n in ((o.dev_intron, o.n_introns), (o.dev_row_retained, o.n_rows)):
        assert bool(ptr) == (n > 0)
    hbm = [tc.dev_copy(o.dev_intron, _abi.RETAINED_INTRON_DTYPE, o.n_introns), pinned[1], tc.dev_copy(o.dev_row_retained, np.int32, o.n_rows)]
    return pinned, hbm, (int(o.n_part), int(o.n_retained_total))


def as_bytes(outs):
    return [x.tobytes() for x in outs[:3]] + [sorted(outs[3].items())]


def check(E, b, fm, min_count, anchor, assignment=None, phase_set=None):
    """intron_retention() against the restatement on the engine's own assignment and phase sets, host and HBM, and the invariants
    -> (records, offsets, row_retained, totals)"""
    pr = E.phase_result()
    asg = pr["assignment"] if assignment is None else assignment
    ps = pr["phase_set"] if phase_set is None else phase_set
    rec, off, row_ret, tot = E.intron_retention(min_count, anchor)
    want = ref.intron_retention(b, fm["row_region_off"], fm["row_read"], asg, ps, min_count, anchor)
    assert rec.dtype == _abi.RETAINED_INTRON_DTYPE and off.dtype == np.int32 and row_ret.dtype == np.int32
    for f in _abi.RETAINED_INTRON_DTYPE.names:
        assert rec[f].tolist() == want[0][f].tolist(), f
    assert off.tolist() == want[1].tolist()
    assert row_ret.shape == (int(fm["row_region_off"][-1]),) and row_ret.tolist() == want[2].tolist()
    assert tot == want[3]
    assert [x.tobytes() for x in (rec, off, row_ret)] == [x.tobytes() for x in want[:3]]          # all output bytes
    pinned, hbm, totals = outputs(E)
    assert [x.tobytes() for x in pinned] == [x.tobytes() for x in (rec, off, row_ret)] == [x.tobytes() for x in hbm]     # HBM and host hold the same bytes
    assert totals == (tot["n_part"], tot["n_retained"])
    # the invariants: the three sums of retained rows; n_spliced is lcr_junctions' count wherever that call keeps the junction
    assert int(row_ret.sum()) == int(rec["n_retained"].sum()) == tot["n_retained"]
    junc, _ = E.junctions(min_count, 0)
    mine = {(int(r["region"]), int(r["start0"]), int(r["len"])): int(r["n_spliced"]) for r in rec}
    for j in junc:
        assert mine[(int(j["region"]), int(j["start0"]), int(j["len"]))] == int(j["n_reads"])
    assert len(junc) == len(rec)
    return rec, off, row_ret, tot


def summary(rec):
    return rh.summary(rec)


def region(start0, length, sites, reads, seed):
    """test_hap_coverage_gpu.cov_region with the reads' order kept: [(column, CIGAR, class)] must come sorted by column"""
    assert [r[0] for r in reads] == sorted(r[0] for r in reads)
    return tc.cov_region(start0, length, sites, reads, seed)


def classes_of(regs):
    return [r["cls"] for _, _, rs in regs for r in rs]


def at(rec, g, s, l):
    hit = [x for r, x in zip(rec, summary(rec)) if int(r["region"]) == g and x[:2] == (s, l)]
    assert len(hit) == 1, (g, s, l)
    return hit[0]


SPLICED2 = [(0, "50M20N50M", 1), (0, "50M20N50M", 2)]     # the intron [1050, 1070) of most tests, spliced once per haplotype


# ---- 1. the worked instance of the contract -------------------------------------------------------------------------------------------
def worked_regions():
    return [region(1000, 400, (5,), rh.WORKED, 61)]


def test_worked_instance(engine_cls):
    regs = worked_regions()
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(5,)], {(0, 5): 7})
    assert tc.got_classes(b, fm, E) == [r[2] for r in rh.WORKED]
    rec, off, row_ret, tot = check(E, b, fm, 2, 10)
    assert summary(rec) == rh.WORKED_WANT and off.tolist() == [0, 2] and row_ret.tolist() == rh.WORKED_ROW_RETAINED
    assert rec["phase_set"].tolist() == [7, 7] and rec["n_phase_sets"].tolist() == [1, 1] and tot == dict(n_part=8, n_retained=6)
    rec, off, row_ret, tot = check(E, b, fm, 2, 50)
    assert summary(rec)[0] == rh.WORKED_WANT[0] and summary(rec)[1][2:] == ((4, 0, 3), (1, 0, 3, 0)) and tot == dict(n_part=8, n_retained=3)
    E.close()


# ---- 2. CIGAR arms --------------------------------------------------------------------------------------------------------------------
ARMS = SPLICED2 + [
    (0, "2H3S30M2I10=5X0M0N0D15D60M3S2H", 1),     # D = X cover, I S H and zero-length M / N / D change nothing: one block [0, 120), RETAINED
    (0, "5M1D" * 7 + "5M20N50M", 2),              # 15 ops in front of it: the N op is the last lane of the first round of 16 -> (47, 20)
    (0, "5M1D" * 8 + "20N50M", 1),                # ... and the first lane of the second round -> (48, 20)
    (0, "1M1D" * 20 + "100M", 2),                 # 41 ops, one block [0, 140): RETAINED at all three
    (0, "30M" + "5N5M" * 17, 1)]                  # 17 junction keys (30, 5), (40, 5), ...: the nested (50, 5) makes it OTHER at (50, 20)


def arms_regions():
    return [region(1000, 400, (2,), ARMS, 62)]


def test_cigar_arms(engine_cls):
    regs = arms_regions()
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(2,)])
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    assert [int(b.n_cig[i]) for i in (3, 4, 5, 6)] == [17, 18, 41, 35] and [int(b.cigar[int(b.cig_off[i]) + k]) & 15 for i, k in ((3, 15), (4, 16))] == [3, 3]
    rec, off, row_ret, tot = check(E, b, fm, 1, 10)
    assert rec.size == 3 + 17 and at(rec, 0, 1050, 20)[2:] == ((2, 2, 3), (1, 1, 1, 1))
    assert at(rec, 0, 1047, 20)[2] == (1, 2, 4) and at(rec, 0, 1048, 20)[2] == (1, 2, 4)
    assert [at(rec, 0, 1030 + 10 * k, 5)[2][0] for k in range(17)] == [1] * 17
    assert row_ret[2] >= 3 and row_ret[5] >= 3 and row_ret[6] == 0 and int(row_ret.sum()) == 40     # (the short introns of the last read are retained by most)
    E.close()


# ---- 3. anchor boundaries ---------------------------------------------------------------------------------------------------------------
def anchor_regions():
    reads = SPLICED2 + [(0, "80M", 1), (0, "79M", 2), (40, "40M", 1), (41, "39M", 2), (50, "20M", 1), (51, "19M", 2)]
    low = [(0, "30M", 1), (3, "2M5N20M", 1), (3, "2M5N20M", 2)]                       # the intron [5, 10) of a region at column 0
    return [region(1000, 200, (5, 55), reads, 63), region(0, 100, (3,), low, 64)]


def test_anchor_boundaries(engine_cls):
    regs = anchor_regions()
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(5, 55), (3,)])
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    rec, off, row_ret, tot = check(E, b, fm, 2, 10)
    assert at(rec, 0, 1050, 20)[2] == (2, 2, 4) and row_ret[2:8].tolist() == [1, 0, 1, 0, 0, 0]     # bs == s - a and be == e + a; one column short each
    assert at(rec, 1, 5, 5)[2] == (2, 0, 1)                                                           # s - a = -5: covered by no row
    rec, off, row_ret, tot = check(E, b, fm, 2, 0)
    assert at(rec, 0, 1050, 20)[2] == (2, 5, 1) and row_ret[2:8].tolist() == [1, 1, 1, 1, 1, 0]     # a = 0: the block [50, 70) is enough, [51, 70) is not
    assert at(rec, 1, 5, 5)[2] == (2, 1, 0)
    assert at(check(E, b, fm, 2, 5)[0], 1, 5, 5)[2] == (2, 1, 0)                                     # s - a == 0 with pos == 0
    assert at(check(E, b, fm, 2, 6)[0], 1, 5, 5)[2] == (2, 0, 1)                                     # s - a == -1
    rec, off, row_ret, tot = check(E, b, fm, 2, 4096)
    assert at(rec, 0, 1050, 20)[2] == (2, 0, 6) and tot["n_retained"] == 0
    E.close()


# ---- 4. OTHER's four causes -----------------------------------------------------------------------------------------------------------
def other_regions():
    reads = SPLICED2 + [(0, "50M30N40M", 1),       # another acceptor
                        (0, "40M30N50M", 2),       # another donor
                        (0, "55M3N62M", 1),        # a nested junction
                        (0, "30M15N75M", 2),       # a junction that ends inside [s - a, s)
                        (0, "60M", 1)]             # the read ends inside the intron
    return [region(1000, 200, (5,), reads, 65)]


def test_other_causes(engine_cls):
    regs = other_regions()
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(5,)])
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    rec, off, row_ret, tot = check(E, b, fm, 2, 10)
    assert summary(rec) == [(1050, 20, (2, 0, 5), (1, 0, 1, 0))] and not row_ret.any()
    rec, off, row_ret, tot = check(E, b, fm, 2, 5)               # the junction that ends at 1045 lies outside [s - 5, e + 5)
    assert summary(rec) == [(1050, 20, (2, 1, 4), (1, 0, 1, 1))] and row_ret.tolist() == [0, 0, 0, 0, 0, 1, 0]
    E.close()


# ---- 5. regions and batch composition ---------------------------------------------------------------------------------------------------
def region_cases():
    unspliced = [(0, "120M", 1), (0, "120M", 2), (0, "50M20N50M", 0)]       # tagged rows all unspliced: an empty table segment
    with_rec = SPLICED2 + [(0, "120M", 1), (0, "120M", 2), (0, "60M", 2)]
    return [region(1000, 200, (5,), unspliced, 66), region(2000, 200, (5,), with_rec, 67), region(3000, 200, (), [], 68),
            region(4000, 200, (5,), unspliced, 69)]


def test_regions_and_batch_order(engine_cls):
    regs = region_cases()
    E = tc.engine(engine_cls)
    ps9 = {(g, 5): 9 for g in range(4)}                    # one phase set value whatever the region's index
    b, fm = tc.tagged(E, regs, [(5,), (5,), (), (5,)], ps9)
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    rec, off, row_ret, tot = check(E, b, fm, 1, 10)
    assert off.tolist() == [0, 0, 1, 1, 1] and summary(rec) == [(2050, 20, (2, 2, 1), (1, 1, 1, 1))] and tot == dict(n_part=9, n_retained=2)
    assert row_ret.tolist() == [0, 0, 0] + [0, 0, 1, 1, 0] + [0, 0, 0]
    first = rec.copy()
    # the same regions in another batch order: the empty segment first, last and in between; the records are the same but for the region
    for order in ([1, 0, 3, 2], [3, 2, 0, 1]):
        b2, fm2 = tc.tagged(E, [regs[k] for k in order], [((5,), (5,), (), (5,))[k] for k in order], ps9)
        rec2, off2, row2, tot2 = check(E, b2, fm2, 1, 10)
        g = order.index(1)
        assert rec2["region"].tolist() == [g] and off2.tolist() == [0] * (g + 1) + [1] * (4 - g) and tot2 == tot
        rec2["region"] = 1
        assert rec2.tobytes() == first.tobytes()
    # the unspliced region alone: participating rows, no pair, no record, NULL record pointers (outputs() asserts them)
    b3, fm3 = tc.tagged(E, regs[:1], [(5,)])
    rec3, off3, row3, tot3 = check(E, b3, fm3, 1, 10)
    o = E._retention_list()
    assert (o.n_regions, o.n_introns, o.n_rows, o.n_part, o.n_retained_total) == (1, 0, 3, 2, 0) and not o.intron and not o.dev_intron
    assert off3.tolist() == [0, 0] and row3.tolist() == [0, 0, 0]
    E.close()


# ---- 6. the keep rule -------------------------------------------------------------------------------------------------------------------
def keep_regions():
    reads = [(0, "50M20N50M", 1), (0, "50M20N50M", 2), (0, "50M20N50M", 1), (0, "50M20N50M", 0),     # three tagged rows splice [50, 70)
             (0, "80M30N20M", 0), (0, "80M30N20M", 0),                                               # [80, 110) is held by untagged reads only
             (0, "150M", 2)]
    return [region(1000, 200, (5,), reads, 70)]


def test_keep_rule(engine_cls):
    regs = keep_regions()
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(5,)])
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    rec, off, row_ret, tot = check(E, b, fm, 3, 10)               # min_count at n_spliced
    assert summary(rec) == [(1050, 20, (3, 1, 0), (2, 0, 1, 1))] and tot == dict(n_part=4, n_retained=1)
    rec, off, row_ret, tot = check(E, b, fm, 4, 10)               # ... and one above: nothing kept, row_retained all 0, the totals stay
    assert rec.size == 0 and off.tolist() == [0, 0] and not row_ret.any() and tot == dict(n_part=4, n_retained=0)
    one = as_bytes(check(E, b, fm, 1, 10))
    assert len(one[0]) == _abi.RETAINED_INTRON_DTYPE.itemsize                                         # the untagged reads' intron is no event
    assert as_bytes(check(E, b, fm, 0, 10)) == one                # min_count 0 is 1
    E.close()


# ---- 7. phase sets ----------------------------------------------------------------------------------------------------------------------
def ps_reads(n5, n15, n25):
    """n5 / n15 / n25 reads that cover the site at column 5 / 15 / 25 only (a D op steps over the others); per site the reads alternate
    between splicing [60, 90) and retaining it, and between the haplotypes every two reads"""
    out = []
    for col, d, n in ((0, 30, n5), (10, 20, n15), (20, 10, n25)):
        out += [(col, "10M%dD20M30N20M" % d if k % 2 == 0 else "10M%dD70M" % d, 1 + (k // 2) % 2) for k in range(n)]
    return out


def test_phase_sets(engine_cls):
    E = tc.engine(engine_cls)
    for g, (counts, pss, want_ps) in enumerate([((2, 4, 3), (30, 20, 10), 20),        # a majority
                                                ((3, 2, 3), (30, 20, 10), 10),        # a tie goes to the smaller value
                                                ((3, 3, 3), (5, 9, 7), 5)]):
        regs = [region(40000, 200, (5, 15, 25), ps_reads(*counts), 71 + g)]
        b, fm = tc.tagged(E, regs, [(5, 15, 25)], {(0, 5): pss[0], (0, 15): pss[1], (0, 25): pss[2]})
        pr = E.phase_result()
        assert pr["phase_set"].tolist() == [pss[0]] * counts[0] + [pss[1]] * counts[1] + [pss[2]] * counts[2] and (pr["assignment"] != 0).all()
        rec, off, row_ret, tot = check(E, b, fm, 1, 10)
        assert [s[:2] for s in summary(rec)] == [(40060, 30)]
        r, n = rec[0], counts[pss.index(want_ps)]
        assert int(r["n_spliced"]) + int(r["n_retained"]) == sum(counts) and int(r["n_phase_sets"]) == 3 and int(r["phase_set"]) == want_ps
        assert sum(int(r[f]) for f in CELLS) == n and int(r["h1_spliced"]) == (n + 3) // 4
    # phase set 0 as the winner: the rows of the largest group lose their phase set in the read records the kernels read
    ptr, n = E.read_records_device()
    recs = tc.dev_copy(ptr, _abi.READ_REC_DTYPE, n)
    ps = pr["phase_set"].copy()
    ps[ps == 9] = 0
    recs["phase_set"] = ps
    assert _lib.load().hipMemcpy(C.c_void_p(ptr), C.c_void_p(recs.ctypes.data), C.c_size_t(recs.nbytes), 1) == 0
    rec, off, row_ret, tot = check(E, b, fm, 1, 10, phase_set=ps)
    assert (int(rec["phase_set"][0]), int(rec["n_phase_sets"][0])) == (0, 3) and tuple(int(rec[f][0]) for f in CELLS) == (1, 1, 1, 0)
    E.close()


# ---- 8. workgroup stride, table stress and determinism ------------------------------------------------------------------------------------
def many_rows_region():
    """600 rows that all overlap [50, 70): more than two strides of the workgroup.  A third splice it, a third retain it, a third end inside
    it; six reads in seven also hold a junction of one of six lengths behind it, at one of two places, so the segment holds thirteen keys"""
    reads = []
    for k in range(600):
        tail = "30M%dN10M" % (10 + k % 7 * 3) if k % 7 else "80M"
        reads.append((0, ("50M20N" + tail, "70M20=" + tail, "60M")[k % 3], 1 + (k // 3) % 2))
    return [region(70000, 400, (5,), reads, 74)]


def test_stride_hash_and_determinism(engine_cls):
    regs = many_rows_region()
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, [(5,)])
    assert tc.got_classes(b, fm, E) == classes_of(regs)
    rec, off, row_ret, tot = check(E, b, fm, 10, 10)
    assert at(rec, 0, 70050, 20)[2] == (200, 200, 200) and at(rec, 0, 70050, 20)[3] == (100, 100, 100, 100) and 200 > BLOCK // 2 and 600 > 2 * BLOCK
    assert rec.size == 13 and tot["n_part"] == 600
    got = {}
    for bits in (32, 0, 3):
        E.debug_set("ir_hash_bits", bits)
        got[bits] = as_bytes(check(E, b, fm, 2, 10))
    assert got[0] == got[3] == got[32]                    # every key of the region down one probe chain: the same bytes
    assert E.lib.lcr_debug_set(E.h, b"ir_hash_bits", 32) == 0
    again = as_bytes(check(E, b, fm, 2, 10))              # a second call on the same engine
    F = tc.engine(engine_cls)                             # and one on a fresh engine
    b2, fm2 = tc.tagged(F, regs, [(5,)])
    fresh = as_bytes(check(F, b2, fm2, 2, 10))
    assert again == got[32] == fresh
    F.close()
    E.close()


# ---- 9. state and arguments ------------------------------------------------------------------------------------------------------------
def test_state_and_arguments(engine_cls):
    s0, refseq, rs = tj.allele_specific_region()
    b = tj.batch_of([(s0, refseq, rs)])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=7))
    lib, lst = E.lib, _abi.LcrRetentionList()
    p10 = _abi.LcrRetentionParams(10, 10)
    bad = [_abi.LcrRetentionParams(10, 4097)]
    E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
    assert lib.lcr_intron_retention(E.h, C.byref(p10)) == E_STATE and lib.lcr_get_intron_retention(E.h, C.byref(lst)) == E_STATE
    E.phase()
    assert lib.lcr_get_intron_retention(E.h, C.byref(lst)) == E_STATE            # no records yet
    assert lib.lcr_intron_retention(E.h, None) == E_ARG and [lib.lcr_intron_retention(E.h, C.byref(p)) for p in bad] == [E_ARG]
    assert lib.lcr_get_intron_retention(E.h, C.byref(lst)) == E_STATE            # a refused call leaves nothing behind
    others = [lambda: [x.tobytes() for x in E.junctions(10, 0)], lambda: [x.tobytes() for x in E.isoforms(10, 1)],
              lambda: [x.tobytes() for x in E.transcript_ends(10, 10, "read")[:3]]]
    alone = [f() for f in others]
    before = (E.phase_result(), E.candidates())
    fm = E.fragmat()
    rec, off, row_ret, tot = check(E, b, fm, 10, 10)
    assert (before[0]["assignment"] != 0).all() and [s[:3] for s in summary(rec)] == [(5800, 300, (20, 0, 20)), (5800, 1100, (20, 0, 20)),
                                                                                       (6400, 500, (20, 0, 20))]
    assert rec["motif"].tolist() == [1, 0, 2] and tot == dict(n_part=40, n_retained=0) and row_ret.shape[0] == 40
    first = as_bytes((rec, off, row_ret, tot))
    assert lib.lcr_intron_retention(E.h, None) == E_ARG and [lib.lcr_intron_retention(E.h, C.byref(p)) for p in bad] == [E_ARG]
    pinned, _, totals = outputs(E)
    assert [x.tobytes() for x in pinned] == first[:3] and totals == (tot["n_part"], tot["n_retained"])      # the previous records still answer
    assert check(E, b, fm, 21, 10)[0].size == 0 and check(E, b, fm, 1, 0)[0].size == 3                      # repetition with other parameters
    assert check(E, b, fm, 10, 4096)[0].size == 3                                                           # the largest anchor
    assert as_bytes(check(E, b, fm, 10, 10)) == first
    # alongside lcr_junctions, lcr_isoforms and lcr_transcript_ends, in either order: each call's bytes equal its bytes alone
    assert [f() for f in others] == alone
    assert [x.tobytes() for x in outputs(E)[0]] == first[:3]
    assert as_bytes(check(E, b, fm, 10, 10)) == first
    assert [f() for f in others[::-1]] == alone[::-1]
    after = (E.phase_result(), E.candidates())
    for k in before[0]:
        assert before[0][k].tobytes() == after[0][k].tobytes(), k
    assert [x.tobytes() for x in before[1]] == [x.tobytes() for x in after[1]]
    with pytest.raises(Exception):
        E.intron_retention_ms()                                                 # timing is off
    # the asynchronous phase stage is collected first
    A = engine_cls(0, _abi.make_params("hifi-masseq", seed=7))
    A.set_async_phase(True)
    A.load_batch(b).run_all()
    assert as_bytes(A.intron_retention(10, 10)) == first
    A.close()
    # the same batch behind haplotag()
    d = {s0 + c: (refseq[c].upper(), tj.ALT[refseq[c].upper()], 77) for c in (150, 300, 450, 600, 2050, 2200, 2350, 2500)}
    pos = np.array(sorted(d), np.int64)
    fm, _, _ = th.staged(E, b, (pos, np.ones(pos.size, np.uint8), np.full(pos.size, 30.0, np.float32)))
    assert lib.lcr_get_intron_retention(E.h, C.byref(lst)) == E_STATE            # a new candidate stage drops the phase results, and the records with them
    assert lib.lcr_intron_retention(E.h, C.byref(p10)) == E_STATE
    E.haplotag(th.site_arrays(d))
    assert lib.lcr_get_intron_retention(E.h, C.byref(lst)) == E_STATE
    rec2, off2, _, tot2 = check(E, b, fm, 10, 10)
    assert rec2["start0"].tolist() == rec["start0"].tolist() and rec2["phase_set"].tolist() == [77] * 3 and tot2 == tot
    assert lib.lcr_enable_timing(E.h, 1) == 0
    check(E, b, fm, 10, 10)
    assert E.intron_retention_ms() > 0.0
    E.load_batch(b)
    assert lib.lcr_get_intron_retention(E.h, C.byref(lst)) == E_STATE            # ... and so does a new binding
    E.close()

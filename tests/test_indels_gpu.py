"""K18 lcr_indels on the GPU against the plain-Python restatement of its contract (tests/indels_ref.py): every field of every record, the
offsets, row_indels and the totals, exactly, in pinned host memory and in HBM.  Rows are put on chosen haplotypes and phase sets with
Engine.haplotag and hand-picked sites (test_hap_coverage_gpu's `tagged`: a class-1 read carries the reference base at a site, a class-2
read the alternate, a class-0 read N -- it stays untagged); read dicts are built here so that inserted bases can be chosen.  The
restatement takes the engine's own assignment and phase sets, and every test asserts the property it was built for.

The worked instance (test_worked_instance).  Window [1000, 1100), reference ACGT repeated with AAAAAA at columns 40 .. 45 (column 39 is
T, column 46 G), a het site at column 2, min_count 2, min_permille 150, flank 5.  Eleven rows, all from column 0:
    rows 0-2   haplotype 1   42M1D57M      a deletion of column 1042
    row  3     haplotype 1   45M1D54M      the same deletion, placed at column 1045
    rows 4-6   haplotype 2   100M
    row  7     haplotype 2   44M           ends inside the homopolymer
    row  8     untagged      100M
    rows 9-10  haplotype 2   70M2I28M      TT inserted in front of column 1070
The deletion left-shifts to 1040 and right-shifts to 1045: shift 5, extent [1040, 1046), hrun 6, flanked [1035, 1051].  Depth at 1039 is
11, four rows hold it (4000 >= 150 x 11), rows 4-6 and 8-10 are ABSENT (one clean block over the flanked extent), row 7 is OTHER; the
cells count the tagged rows only: h1 4 / 0, h2 0 / 5.  The insertion does not move (column 1069 is C, 1070 G): extent [1070, 1070), hrun 1,
flanked [1065, 1075]; depth at 1069 is 10, rows 9-10 hold it, rows 0-6 and 8 are ABSENT, row 7 ends left of it and is not looked at;
cells h1 0 / 4, h2 2 / 3.  seq of TT is 0b1111.  row_indels is 1 for rows 0-3 and 9-10; n_events 6.

One arm cannot reach the call through this library: lcr_pileup refuses a batch that holds a P op, so the restatement's P arm is tested in
test_indels_host.py only."""
import ctypes as C
import re

import numpy as np
import pytest

import indels_ref as ref
import test_hap_coverage_gpu as tc
import test_haplotag_gpu as th
import test_junctions_gpu as tj
from longcallr_amd import _abi, _lib

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
BLOCK = 256     # LCR_BLOCK: threads of the workgroup that serves one kept event
CELLS = ("h1_present", "h1_absent", "h2_present", "h2_absent")
DEFAULTS = dict(min_count=1, min_permille=0, flank=5, max_ins=12, max_del=50)


def bg(n, patches=()):
    """ACGT repeated -- no 1- or 2-base indel shifts in it -- with `patches` = [(column, text)] written into it"""
    s = list(("ACGT" * (n // 4 + 1))[:n])
    for col, text in patches:
        s[col:col + len(text)] = text
    return "".join(s)


def mk(refseq, s0, col, cigar, cls, sites=(2,), ins=""):
    """one read dict: M / = / X bases from the reference (outside the window or no ACGT letter there: A), at a column of `sites` the
    reference base (class 1), its tj.ALT (class 2) or N (class 0); the bases of the I ops taken from `ins` in order (then A); S bases C"""
    seq, c, it = [], col, iter(ins)
    for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar):
        n = int(n)
        if op in "M=X":
            for x in range(c, c + n):
                base = refseq[x].upper() if 0 <= x < len(refseq) else "A"
                base = base if base in "ACGT" else "A"
                if x in sites:
                    base = {1: base, 2: tj.ALT[base], 0: "N"}[cls]
                seq.append(base)
            c += n
        elif op in "DN":
            c += n
        elif op == "I":
            seq += [next(it, "A") for _ in range(n)]
        elif op == "S":
            seq += ["C"] * n
    return dict(pos=s0 + col, seq="".join(seq), qual=30, cigar=cigar, rev=0, ts=1, cls=cls)


def region(s0, refseq, sites, reads):
    """reads: [(column, CIGAR, class[, inserted bases])] -> (start0, reference, read dicts sorted by position)"""
    out = [mk(refseq, s0, r[0], r[1], r[2], sites, r[3] if len(r) > 3 else "") for r in reads]
    out.sort(key=lambda r: r["pos"])
    return s0, refseq, out


def outputs(E):
    """the last indels()'s outputs, from pinned host memory and from HBM, and its totals"""
    o = E._indel_list()
    pinned = []
    for ptr, dt, n in ((o.indel, _abi.INDEL_DTYPE, o.n_indels), (o.indel_region_off, np.int32, o.n_regions + 1), (o.row_indels, np.int32, o.n_rows)):
        assert bool(ptr) == (n > 0)                               # NULL exactly where a count is 0
        buf = (C.c_char * (np.dtype(dt).itemsize * n)).from_address(ptr) if n else b""
        pinned.append(np.frombuffer(buf, dtype=dt, count=n).copy())
    for ptr, n in ((o.dev_indel, o.n_indels), (o.dev_row_indels, o.n_rows)):
        assert bool(ptr) == (n > 0)
    hbm = [tc.dev_copy(o.dev_indel, _abi.INDEL_DTYPE, o.n_indels), pinned[1], tc.dev_copy(o.dev_row_indels, np.int32, o.n_rows)]
    return pinned, hbm, dict(n_part=int(o.n_part), n_events=int(o.n_events), n_present=int(o.n_present_total))


def as_bytes(outs):
    return [x.tobytes() for x in outs[:3]] + [sorted(outs[3].items())]


def check(E, b, fm, phase_set=None, classes=None, **kw):
    """indels() against the restatement on the engine's own assignment and phase sets, host and HBM, and the invariants
    -> (records, offsets, row_indels, totals)"""
    p = dict(DEFAULTS, **kw)
    pr = E.phase_result()
    ps = pr["phase_set"] if phase_set is None else phase_set
    rec, off, rows, tot = E.indels(**p)
    want = ref.indels(b, fm["row_region_off"], fm["row_read"], pr["assignment"], ps, classes=classes, **p)
    assert rec.dtype == _abi.INDEL_DTYPE and off.dtype == np.int32 and rows.dtype == np.int32
    for f in _abi.INDEL_DTYPE.names:
        assert rec[f].tolist() == want[0][f].tolist(), f
    assert off.tolist() == want[1].tolist()
    assert rows.shape == (int(fm["row_region_off"][-1]),) and rows.tolist() == want[2].tolist()
    assert tot == want[3]
    assert [x.tobytes() for x in (rec, off, rows)] == [x.tobytes() for x in want[:3]]          # all output bytes
    pinned, hbm, totals = outputs(E)
    assert [x.tobytes() for x in pinned] == [x.tobytes() for x in (rec, off, rows)] == [x.tobytes() for x in hbm]     # HBM and host hold the same bytes
    assert totals == tot
    assert int(rows.sum()) == int(rec["n_present"].sum()) == tot["n_present"]
    return rec, off, rows, tot


def summary(rec):
    """[(start0, type, len, seq, (present, absent, other), cells)]"""
    return [(int(r["start0"]), int(r["type"]), int(r["len"]), int(r["seq"]), (int(r["n_present"]), int(r["n_absent"]), int(r["n_other"])),
             tuple(int(r[f]) for f in CELLS)) for r in rec]


def at(rec, g, s, typ, n):
    hit = [r for r in rec if (int(r["region"]), int(r["start0"]), int(r["type"]), int(r["len"])) == (g, s, typ, n)]
    assert len(hit) == 1, (g, s, typ, n)
    return hit[0]


def counts(r):
    return int(r["n_present"]), int(r["n_absent"]), int(r["n_other"])


def run(engine_cls, regs, sites, ps_of=None, n_part=None):
    E = tc.engine(engine_cls)
    b, fm = tc.tagged(E, regs, sites, ps_of)
    if n_part is not None:
        assert int(fm["row_region_off"][-1]) == n_part          # every read is a fragment row
    return E, b, fm


# ---- 1. the worked instance of the contract -------------------------------------------------------------------------------------------
WORKED_REF = bg(100, [(40, "AAAAAA")])
WORKED = ([(0, "42M1D57M", 1)] * 3 + [(0, "45M1D54M", 1)] + [(0, "100M", 2)] * 3 + [(0, "44M", 2), (0, "100M", 0)]
          + [(0, "70M2I28M", 2, "TT")] * 2)


def test_worked_instance(engine_cls):
    regs = [region(1000, WORKED_REF, (2,), WORKED)]
    E, b, fm = run(engine_cls, regs, [(2,)], {(0, 2): 7}, 11)
    assert tc.got_classes(b, fm, E) == [r[2] for r in WORKED]
    rec, off, rows, tot = check(E, b, fm, min_count=2, min_permille=150)
    assert summary(rec) == [(1040, 0, 1, 0, (4, 6, 1), (4, 0, 0, 5)), (1070, 1, 2, 15, (2, 8, 0), (0, 4, 2, 3))]
    assert rec["hrun"].tolist() == [6, 1] and rec["shift"].tolist() == [5, 0] and rec["depth"].tolist() == [11, 10]
    assert rec["phase_set"].tolist() == [7, 7] and rec["n_phase_sets"].tolist() == [1, 1] and off.tolist() == [0, 2]
    assert rows.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1] and tot == dict(n_part=11, n_events=6, n_present=6)
    E.close()


# ---- 2. CIGAR arms --------------------------------------------------------------------------------------------------------------------
ARMS = [
    (0, "2H3S30M2I68M", 1, "TT"),                 # I after H and S: its bases lie at query offset 33
    (0, "2I50M", 2, "GG"),                        # a leading I,
    (0, "50M2I", 1, "GG"),                        # a trailing I
    (0, "3D50M", 2),                              # and a leading D: ignored entirely
    (0, "105M2I3D5M", 1, "TT"),                   # I and D at one column: both events, each in the other's flank
    (0, "10M0I0D0N40M", 2),                       # zero-length ops are no gaps
    (0, "10=5X35M1D10=", 1),                      # = and X align
    (0, "3M1D" * 8 + "50M", 2),                   # 17 ops: the eighth D is lane 15 of the first round
    (0, "3M1D" * 7 + "3M2M1D50M", 1),             # 18 ops: the eighth D is lane 0 of the second round
    (0, "2M1D" * 15 + "1I30M", 0, "T"),           # 32 ops: the I is lane 14, the M behind it lane 15
    (0, "2M1D" * 16 + "30M", 0),                  # 33 ops
    (0, "3S5M2I" + "2M1D" * 7 + "4M3I40M", 0, "TTGCA")]     # the second I sits in the second round behind S, I and M: query offset 28


def test_cigar_arms(engine_cls):
    regs = [region(1000, bg(300), (2,), ARMS)]
    E, b, fm = run(engine_cls, regs, [(2,)], None, len(ARMS))
    assert [int(b.n_cig[i]) for i in (7, 8, 9, 10)] == [17, 18, 32, 33]
    assert [int(b.cigar[int(b.cig_off[i]) + k]) & 15 for i, k in ((7, 15), (8, 16), (9, 30))] == [2, 2, 1]
    rec, off, rows, tot = check(E, b, fm)
    assert counts(at(rec, 0, 1030, 1, 2))[0] == 1 and int(at(rec, 0, 1030, 1, 2)["seq"]) == 15
    assert rows[1] == 0 and rows[2] == 0 and rows[3] == 0 and rows[5] == 0              # the ignored ops and the zero-length ops are no events
    assert counts(at(rec, 0, 1105, 1, 2))[0] == 1 and counts(at(rec, 0, 1105, 0, 3))[0] == 1 and rows[4] == 2     # PRESENT at both
    assert rows[6] == 1 and counts(at(rec, 0, 1050, 0, 1))[0] == 1
    assert rows[7] == 8 and rows[8] == 8 and rows[9] == 16 and rows[10] == 16           # every op of the long CIGARs is seen, in both rounds
    assert int(at(rec, 0, 1005, 1, 2)["seq"]) == 15 and int(at(rec, 0, 1030, 1, 3)["seq"]) == ref.pack("GCA") and rows[11] == 9
    E.close()


# ---- 3. normalisation -------------------------------------------------------------------------------------------------------------------
def test_normalisation(engine_cls):
    ref0 = bg(200, [(40, "A" * 10), (80, "CACACA")])                       # column 39 T, 50 G; column 79 T, 86 G
    reads0 = [(0, "%dM1D%dM" % (40 + k, 159 - k), 1 + k % 2) for k in range(10)]       # one deletion at every column of the homopolymer
    reads0 += [(0, "86M2I114M", 1, "CA"), (0, "85M2I115M", 2, "AC")]                  # CA behind CACACA, AC inside it
    ref1 = bg(100, [(0, "T" * 8), (40, "aAaAaA"), (60, "AANAAAA")])
    reads1 = [(0, "5M1D94M", 1),                  # shifts to w0 + 1 and stops there, whatever column w0 holds
              (0, "45M1D54M", 2),                 # lower-case letters do not stop the shift
              (0, "65M1D34M", 1),                 # an N does
              (0, "95M5D10M", 2), (0, "96M5D10M", 1),                   # the raw placement ends on w1 / one behind it
              (0, "100M2I5M", 2, "GG"), (0, "101M2I5M", 1, "GG")]       # an insertion in front of column w1 / one behind it
    ref2 = bg(1300, [(50, "A" * 1100)])
    reads2 = [(0, "1140M1D100M", 1), (0, "100M1D1140M", 2)]                # 1024 steps from 1140 end at 116; from 100 the run's start ends the shift
    regs = [region(1000, ref0, (2,), reads0), region(5000, ref1, (20,), reads1), region(9000, ref2, (2,), reads2)]
    E, b, fm = run(engine_cls, regs, [(2,), (20,), (2,)], None, 12 + 7 + 2)
    rec, off, rows, tot = check(E, b, fm)
    r = at(rec, 0, 1040, 0, 1)
    assert counts(r)[0] == 10 and (int(r["shift"]), int(r["hrun"])) == (9, 10)         # one record, all ten rows
    r = at(rec, 0, 1080, 1, 2)
    assert counts(r)[0] == 2 and int(r["seq"]) == ref.pack("CA") and int(r["shift"]) == 6
    assert off.tolist()[1] == 2
    g1 = [(int(x["start0"]), int(x["type"]), int(x["len"])) for x in rec if int(x["region"]) == 1]
    assert g1 == [(5001, 0, 1), (5040, 0, 1), (5063, 0, 1), (5095, 0, 5), (5100, 1, 2)]      # 96M5D and 101M2I are no events
    assert int(at(rec, 1, 5001, 0, 1)["hrun"]) == 7 and int(at(rec, 1, 5040, 0, 1)["shift"]) == 5
    g2 = [(int(x["start0"]), int(x["shift"]), int(x["hrun"])) for x in rec if int(x["region"]) == 2]
    assert g2 == [(9050, 1024, 255), (9116, 1024, 255)]                                 # the cap splits one deletion into two records
    E.close()


# ---- 4. identity ------------------------------------------------------------------------------------------------------------------------
def test_identity(engine_cls):
    reads = [(0, "30M2I70M", 1, "TT"), (0, "30M2I70M", 2, "GG"),          # same anchor and length, other bases
             (0, "32M2I68M", 1, "TN"),                                     # an N among the inserted bases: a gap only
             (0, "60M12I40M", 2, "ACGTTGCATGCA"), (0, "60M13I40M", 1, "ACGTTGCATGCAT"),
             (0, "80M50D20M", 2), (0, "80M51D19M", 1)]
    regs = [region(1000, bg(200), (2,), reads)]
    E, b, fm = run(engine_cls, regs, [(2,)], None, 7)
    cls = {}
    rec, off, rows, tot = check(E, b, fm, classes=cls)
    assert [(s[0], s[1], s[2], s[3]) for s in summary(rec)] == [(1030, 1, 2, ref.pack("GG")), (1030, 1, 2, ref.pack("TT")),
                                                                 (1060, 1, 12, ref.pack("ACGTTGCATGCA")), (1080, 0, 50, 0)]
    assert rows.tolist() == [1, 1, 0, 1, 0, 1, 0] and tot["n_events"] == 4
    assert counts(rec[0]) == (1, 4, 2) and counts(rec[1]) == (1, 4, 2)     # the other insertion's row and the TN row (its gap lies in the flank) are OTHER
    assert check(E, b, fm, max_ins=11, max_del=49)[0].size == 2
    E.close()


# ---- 5. classes -------------------------------------------------------------------------------------------------------------------------
B0 = 4000     # the event of the class tests: a 2-base deletion at column B0 + 100; flanked extent [B0 + 95, B0 + 107] at flank 5


def class_reads():
    hold = [(B0, "100M2D98M", 1), (B0, "100M2D98M", 2)]
    edge = [(B0 + 95, "105M", 1), (B0 + 96, "104M", 2),                   # pos == lo_f: ABSENT; lo_f + 1: OTHER
            (B0, "107M", 1), (B0, "106M", 2)]                              # rend == hi_f: ABSENT; hi_f - 1: OTHER
    gaps = [(B0, "95M1I105M", 1, "T"), (B0, "94M1I106M", 2, "T"),         # a foreign I exactly at lo_f touches; one column outside it does not
            (B0, "107M1I93M", 1, "T"), (B0, "108M1I92M", 2, "T"),         # ... at hi_f / outside
            (B0, "90M5D105M", 1), (B0, "89M5D106M", 2),                   # a foreign D that ends at lo_f / one column before it
            (B0, "107M3D90M", 1), (B0, "108M3D89M", 2)]                   # ... that starts at hi_f / one column behind it
    far = [(10, "10M%dN150M" % (B0 + 96 - 20), 1),                         # an N from column 20 that ends inside the flank: OTHER
           (10, "10M%dN152M" % (B0 + 94 - 20), 2)]                         # ... that ends one column before the flank: ABSENT
    many = [(B0 - 200, "1M1D" * 70 + "200M", 1),                           # 70 gaps left of the flank: ABSENT
            (B0 - 200, "1M1D" * 70 + "160M2D50M", 2)]                      # 71 gaps, the last one the event: PRESENT
    return hold + edge + gaps + far + many


CLASS_WANT = ["P", "P", "A", "O", "A", "O", "O", "A", "O", "A", "O", "A", "O", "A", "O", "A", "A", "P"]


def test_classes(engine_cls):
    rs = class_reads()
    refseq = bg(5000)
    regs = [region(1000, refseq, (B0 + 150,), rs)]
    order = sorted(range(len(rs)), key=lambda k: rs[k][0])        # (the sort is stable: the rows' order)
    E, b, fm = run(engine_cls, regs, [(B0 + 150,)], None, len(rs))
    cls = {}
    rec, off, rows, tot = check(E, b, fm, min_count=3, classes=cls)
    key = (1000 + B0 + 100, 0, 2)
    assert [s[:3] for s in summary(rec)] == [key] and cls[(0, key)] == [CLASS_WANT[k] for k in order]
    assert counts(rec[0]) == (3, 8, 7)
    assert int(b.n_cig[order.index(17)]) == 143
    rec, off, rows, tot = check(E, b, fm, min_count=3, flank=0, classes=cls)      # flank 0: only what touches [lo, hi] itself counts
    assert counts(rec[0]) == (3, 15, 0)
    # lo_f < 0: covered by no row; lo_f == 0 with pos == 0 is
    low = [(0, "3M2D95M", 1), (0, "3M2D95M", 2), (0, "100M", 1)]
    b2, fm2 = tc.tagged(E, [region(0, bg(100), (20,), low)], [(20,)])
    assert counts(check(E, b2, fm2, min_count=2, flank=5)[0][0]) == (2, 0, 1)
    assert counts(check(E, b2, fm2, min_count=2, flank=3)[0][0]) == (2, 1, 0)
    E.close()


# ---- 6. filters -------------------------------------------------------------------------------------------------------------------------
def filter_reads(extra):
    return ([(0, "50M2D48M", 1), (0, "50M2D48M", 2), (0, "50M2D48M", 0)]          # three rows hold it, one of them untagged
            + [(0, "100M", 1 + k % 2) for k in range(13)] + [(0, "100M", 0)] * 2  # 15 plain rows, two of them untagged
            + [(0, "45M10D45M", 1), (0, "45M10D45M", 2)]                          # a D covers the anchor column 49: counted
            + [(0, "40M20N40M", 1)]                                               # an N spans it: not counted
            + [(0, "100M", 2)] * extra)


def test_filters(engine_cls):
    regs = [region(1000, bg(100), (2,), filter_reads(0)), region(3000, bg(100), (2,), filter_reads(1))]
    E, b, fm = run(engine_cls, regs, [(2,), (2,)], None, 21 + 22)
    rec, off, rows, tot = check(E, b, fm, min_count=3, min_permille=150)
    r = at(rec, 0, 1050, 0, 2)
    assert int(r["depth"]) == 20 and counts(r)[0] == 3 and 3 * 1000 == 150 * 20           # equality keeps
    assert not [x for x in rec if int(x["region"]) == 1 and int(x["start0"]) == 3050]     # one more covering row: 3000 < 150 x 21
    assert check(E, b, fm, min_count=4, min_permille=0)[0].size == 0                      # cnt == min_count - 1
    rec = check(E, b, fm, min_count=3, min_permille=0)[0]
    assert [(int(x["region"]), int(x["start0"]), int(x["depth"])) for x in rec] == [(0, 1050, 20), (1, 3050, 21)]
    one = as_bytes(check(E, b, fm, min_count=1, min_permille=0))
    assert as_bytes(check(E, b, fm, min_count=0, min_permille=0)) == one and len(one[0]) == 4 * 64      # min_count 0 is 1
    E.close()


# ---- 7. phase sets ----------------------------------------------------------------------------------------------------------------------
def ps_reads(n5, n15, n25):
    """n5 / n15 / n25 reads that cover the site at column 5 / 15 / 25 only (a D op, longer than max_del, steps over the others); per site
    the reads alternate between holding the deletion [70, 72) and covering it cleanly, and between the haplotypes every two reads"""
    out = []
    for col, d, n in ((0, 30, n5), (10, 20, n15), (20, 10, n25)):
        out += [(col, "10M%dD30M2D30M" % d if k % 2 == 0 else "10M%dD62M" % d, 1 + (k // 2) % 2) for k in range(n)]
    return out


def test_phase_sets(engine_cls):
    E = tc.engine(engine_cls)
    for g, (cnts, pss, want_ps) in enumerate([((2, 4, 3), (30, 20, 10), 20),        # a majority
                                              ((3, 2, 3), (30, 20, 10), 10),        # a tie goes to the smaller value
                                              ((3, 3, 3), (5, 9, 7), 5)]):
        regs = [region(40000, bg(200), (5, 15, 25), ps_reads(*cnts))]
        b, fm = tc.tagged(E, regs, [(5, 15, 25)], {(0, 5): pss[0], (0, 15): pss[1], (0, 25): pss[2]})
        pr = E.phase_result()
        assert pr["phase_set"].tolist() == [pss[0]] * cnts[0] + [pss[1]] * cnts[1] + [pss[2]] * cnts[2] and (pr["assignment"] != 0).all()
        rec, off, rows, tot = check(E, b, fm, max_del=5)
        assert [s[:3] for s in summary(rec)] == [(40070, 0, 2)]
        r, n = rec[0], cnts[pss.index(want_ps)]
        assert int(r["n_present"]) + int(r["n_absent"]) == sum(cnts) and int(r["n_phase_sets"]) == 3 and int(r["phase_set"]) == want_ps
        assert sum(int(r[f]) for f in CELLS) == n and int(r["h1_present"]) == (n + 3) // 4
    # phase set 0 as the winner: the rows of the largest group lose their phase set in the read records the kernels read
    ptr, n = E.read_records_device()
    recs = tc.dev_copy(ptr, _abi.READ_REC_DTYPE, n)
    ps = pr["phase_set"].copy()
    ps[ps == 9] = 0
    recs["phase_set"] = ps
    assert _lib.load().hipMemcpy(C.c_void_p(ptr), C.c_void_p(recs.ctypes.data), C.c_size_t(recs.nbytes), 1) == 0
    rec, off, rows, tot = check(E, b, fm, phase_set=ps, max_del=5)
    assert (int(rec["phase_set"][0]), int(rec["n_phase_sets"][0])) == (0, 3) and tuple(int(rec[f][0]) for f in CELLS) == (1, 1, 1, 0)
    E.close()


# ---- 8. table and layout ------------------------------------------------------------------------------------------------------------------
def many_rows_region():
    """600 rows that are all looked at at the deletion [50, 52): more than two strides of the workgroup.  A third hold it, a third cover it
    cleanly, a third end inside its flank; most also hold a deletion or an insertion of one of a few forms behind it, so the segment holds
    nine kept keys"""
    reads = []
    for k in range(600):
        tail = ("30M%dD20M" % (1 + k % 4), "30M1I20M", "50M")[k % 7 % 3] if k % 7 else "50M"
        reads.append((0, ("50M2D" + tail, "52M" + tail, "55M")[k % 3], 1 + (k // 3) % 2, "ACGT"[k % 4]))
    return region(70000, bg(200), (2,), reads)


def test_table_and_layout(engine_cls):
    plain = [(0, "100M", 1), (0, "100M", 2), (0, "40M30N30M", 0)]             # rows, gaps, no event
    with_rec = [(0, "50M2D48M", 1), (0, "50M2D48M", 2), (0, "100M", 1), (0, "100M", 2), (0, "60M", 2)]
    regs = [region(1000, bg(200), (2,), plain), region(2000, bg(200), (2,), with_rec), region(3000, bg(200), (), []),
            region(4000, bg(200), (2,), plain), many_rows_region()]
    sites = [(2,), (2,), (), (2,), (2,)]
    ps9 = {(g, 2): 9 for g in range(5)}                     # one phase set value whatever the region's index
    E, b, fm = run(engine_cls, regs, sites, ps9, 3 + 5 + 0 + 3 + 600)
    rec, off, rows, tot = check(E, b, fm, min_count=2)
    assert off.tolist()[:5] == [0, 0, 1, 1, 1] and summary(rec)[0] == (2050, 0, 2, 0, (2, 3, 0), (1, 1, 1, 2))
    r = at(rec, 4, 70050, 0, 2)
    assert counts(r) == (200, 200, 200) and tuple(int(r[f]) for f in CELLS) == (100, 100, 100, 100) and 600 > 2 * BLOCK
    assert off[5] - off[4] == 9
    got = {}
    for bits in (32, 0, 3):
        E.debug_set("indel_hash_bits", bits)
        got[bits] = as_bytes(check(E, b, fm, min_count=2))
    assert got[0] == got[3] == got[32]                    # every key of a region down one probe chain: the same bytes
    assert E.lib.lcr_debug_set(E.h, b"indel_hash_bits", 32) == 0
    per_region = {g: rec[off[g]:off[g + 1]].copy() for g in range(5)}
    # the same regions in another batch order, and each region alone: the per-region records are the same but for the region's index
    for order in ([4, 1, 0, 3, 2], [3, 2, 4, 0, 1], [1], [4], [0]):
        b2, fm2 = tc.tagged(E, [regs[k] for k in order], [sites[k] for k in order], {(g, 2): 9 for g in range(len(order))})
        rec2, off2, rows2, tot2 = check(E, b2, fm2, min_count=2)
        for g2, k in enumerate(order):
            part = rec2[off2[g2]:off2[g2 + 1]].copy()
            assert (part["region"] == g2).all()
            part["region"] = k
            assert part.tobytes() == per_region[k].tobytes()
    o = E._indel_list()                                     # the last batch: rows, gaps, no event at all
    assert (o.n_regions, o.n_indels, o.n_rows, o.n_part, o.n_events, o.n_present_total) == (1, 0, 3, 3, 0, 0) and not o.indel and not o.dev_indel
    E.close()


# ---- 9. state and arguments ------------------------------------------------------------------------------------------------------------
def state_region():
    reads = [(0, "50M2D48M", 1)] * 12 + [(0, "100M", 2)] * 12
    return region(1000, bg(100), (2, 30, 60, 90), reads)


def test_state_and_arguments(engine_cls):
    regs = [state_region()]
    b = tj.batch_of(regs)
    E = tc.engine(engine_cls)
    lib, lst = E.lib, _abi.LcrIndelList()
    p10 = _abi.LcrIndelParams(10, 150, 5, 12, 50)
    bad = [_abi.LcrIndelParams(10, 150, 4097, 12, 50), _abi.LcrIndelParams(10, 150, 5, 13, 50), _abi.LcrIndelParams(10, 150, 5, 12, 65536)]
    E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
    assert lib.lcr_indels(E.h, C.byref(p10)) == E_STATE and lib.lcr_get_indels(E.h, C.byref(lst)) == E_STATE
    E.phase()
    assert lib.lcr_get_indels(E.h, C.byref(lst)) == E_STATE              # no records yet
    assert lib.lcr_indels(E.h, None) == E_ARG and [lib.lcr_indels(E.h, C.byref(p)) for p in bad] == [E_ARG] * 3
    assert lib.lcr_get_indels(E.h, C.byref(lst)) == E_STATE              # a refused call leaves nothing behind
    others = [lambda: [x.tobytes() for x in E.junctions(10, 0)], lambda: [x.tobytes() for x in E.intron_retention(10, 10)[:3]],
              lambda: [x.tobytes() for x in E.hap_coverage()], lambda: [E.site_counts().tobytes()]]
    alone = [f() for f in others]
    before = (E.phase_result(), E.candidates())
    fm = E.fragmat()
    rec, off, rows, tot = check(E, b, fm, min_count=10, min_permille=150)             # behind lcr_phase
    assert (before[0]["assignment"] != 0).all() and [s[:3] for s in summary(rec)] == [(1050, 0, 2)] and counts(rec[0]) == (12, 12, 0)
    assert sorted(tuple(int(rec[f][0]) for f in CELLS)) == [0, 0, 12, 12] and tot == dict(n_part=24, n_events=12, n_present=12)
    first = as_bytes((rec, off, rows, tot))
    assert lib.lcr_indels(E.h, None) == E_ARG and [lib.lcr_indels(E.h, C.byref(p)) for p in bad] == [E_ARG] * 3
    pinned, _, totals = outputs(E)
    assert [x.tobytes() for x in pinned] == first[:3] and totals == tot               # the previous records still answer
    assert check(E, b, fm, min_count=13)[0].size == 0 and check(E, b, fm, min_count=1, flank=4096, max_ins=0, max_del=65535)[0].size == 1
    assert check(E, b, fm, min_count=1, max_del=1)[0].size == 0                       # repetition with other parameters
    assert as_bytes(check(E, b, fm, min_count=10, min_permille=150)) == first
    # alongside the other calls behind the phase stage, in either order: each call's bytes equal its bytes alone
    assert [f() for f in others] == alone
    assert [x.tobytes() for x in outputs(E)[0]] == first[:3]
    assert as_bytes(check(E, b, fm, min_count=10, min_permille=150)) == first
    assert [f() for f in others[::-1]] == alone[::-1]
    after = (E.phase_result(), E.candidates())
    for k in before[0]:
        assert before[0][k].tobytes() == after[0][k].tobytes(), k
    assert [x.tobytes() for x in before[1]] == [x.tobytes() for x in after[1]]
    with pytest.raises(Exception):
        E.indels_ms()                                                   # timing is off
    # the same batch behind haplotag()
    s0, refseq, _ = regs[0]
    d = {s0 + c: (refseq[c], tj.ALT[refseq[c]], 77) for c in (2, 30, 60, 90)}
    pos = np.array(sorted(d), np.int64)
    fm, _, _ = th.staged(E, b, (pos, np.ones(pos.size, np.uint8), np.full(pos.size, 30.0, np.float32)))
    assert lib.lcr_get_indels(E.h, C.byref(lst)) == E_STATE              # a new candidate stage drops the phase results, and the records with them
    assert lib.lcr_indels(E.h, C.byref(p10)) == E_STATE
    E.haplotag(th.site_arrays(d))
    assert lib.lcr_get_indels(E.h, C.byref(lst)) == E_STATE
    rec2, off2, _, tot2 = check(E, b, fm, min_count=10, min_permille=150)
    assert rec2["start0"].tolist() == [1050] and rec2["phase_set"].tolist() == [77] and tot2 == tot
    assert tuple(int(rec2[f][0]) for f in CELLS) == (12, 0, 0, 12)
    assert lib.lcr_enable_timing(E.h, 1) == 0
    check(E, b, fm, min_count=10)
    assert E.indels_ms() > 0.0
    E.load_batch(b)
    assert lib.lcr_get_indels(E.h, C.byref(lst)) == E_STATE              # ... and so does a new binding
    E.close()


# ---- 10. random batches -------------------------------------------------------------------------------------------------------------------
def random_regions(seed, n_regions=4, n_reads=70, length=400):
    """Per region a low-complexity reference (A and C, a few G and T) with het sites at columns 2 and 200, eight planted indels that each
    haplotype's reads carry with its own probability, and per-read noise: random short I / D and a few N, so that equal events arrive at
    different raw placements and every class is reached"""
    rng = np.random.default_rng(seed)
    regs, sites = [], []
    for g in range(n_regions):
        letters = rng.choice(list("ACGT"), size=length, p=[0.45, 0.45, 0.05, 0.05])
        letters[2], letters[200] = "G", "T"
        refseq = "".join(letters)
        planted = [(int(c), int(rng.integers(1, 3)), int(rng.integers(1, 4)), float(rng.random()), float(rng.random()))
                   for c in sorted(rng.choice(np.arange(20, length - 40, 12), size=8, replace=False))]
        reads = []
        for k in range(n_reads):
            cls = int(rng.integers(0, 3))
            col = int(rng.integers(0, 3)) if k % 3 else int(rng.integers(3, 190))
            end = int(rng.integers(length - 150, length - 5))
            ops = []    # (column, op, len)
            for c, op, n, p1, p2 in planted:
                if col + 5 < c < end - 10 and rng.random() < (p1, p1, p2)[cls]:
                    ops.append((c + int(rng.integers(0, 2)), "ID"[op - 1], n))
            for _ in range(int(rng.integers(0, 4))):
                c = int(rng.integers(col + 3, end - 10))
                ops.append((c, "IDDN"[int(rng.integers(0, 4))], int(rng.integers(1, 3))))
            ops.sort()
            cigar, cur, ins = "", col, ""
            for c, op, n in ops:
                if c - cur < 2 or c in (2, 200) or (op != "I" and c <= 200 < c + n + 1) or (op != "I" and c <= 2 < c + n + 1):
                    continue
                if op == "N":
                    n = 15
                    if c + n >= end - 5:
                        continue
                cigar += "%dM%d%s" % (c - cur, n, op)
                cur = c + (0 if op == "I" else n)
                if op == "I":
                    ins += "".join(rng.choice(list("AC"), size=n))
            if end - cur < 2:
                end = cur + 2
            cigar += "%dM" % (end - cur)
            reads.append((col, cigar, cls, ins))
        regs.append(region(10000 * (g + 1), refseq, (2, 200), reads))
        sites.append((2, 200))
    return regs, sites


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_random_batches(engine_cls, seed):
    regs, sites = random_regions(seed)
    E, b, fm = run(engine_cls, regs, sites, None, 4 * 70)
    cls = {}
    rec, off, rows, tot = check(E, b, fm, min_count=3, min_permille=100, flank=3, classes=cls)
    # on the restatement's own output, so that an empty comparison cannot pass
    pr = E.phase_result()
    want = ref.indels(b, fm["row_region_off"], fm["row_read"], pr["assignment"], pr["phase_set"], 3, 100, 3)
    assert len(want[0]) >= 20 and {c for v in cls.values() for c in v} == {"P", "A", "O"}
    assert set(want[0]["type"].tolist()) == {0, 1} and int(want[0]["shift"].max()) > 0 and len(set(pr["assignment"].tolist())) == 3
    E.close()

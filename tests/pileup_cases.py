"""Recipes for the pileup stage (csrc/k0_ops.hip, k1_pileup.hip: K0, K1 and the poly-A mask K1z): plain data and builders, no tests.

A case is one small batch for helpers.mk_batch -- one region per sub-case, reads and CIGARs written out --, the params it runs under in each
form, and the facts it was designed for: plane values at its design columns, written down from the recipe (interval counts of the runs
the recipe lists, tallies of the bases the recipe places, literals), by neither oracle.  tests/test_pileup_cases.py runs the two CPU
oracles against each other on every case, holds both to the facts and reads the preconditions (records per tile, pieces per K1 batch,
the K1z kernel a (D, L) pair reaches, the bytes behind the last piece) off the batch; tests/test_pileup_cases_gpu.py puts the same
cases in front of every form of the tally.

Every design column derives from LCR_TILE (T below), read from lcr_dev.h.  A region of 600 columns has tiles of 256, 256 and 88 columns.
Reads carry the reference base on every aligned column but where the recipe says otherwise; references have no two equal neighbours
(no homopolymer for the HiFi presets' poly-A mask to find) unless a recipe forces one.  Read bases stay inside the ABI's alphabet
(include/lcr.h: upper case).

Forms (FORMS of a case): "hifi" the HiFi preset (full tally, K1z behind it), "fused" / "lean" / "tiles" the ONT preset.  The ONT forms of
the families whose facts are about record geometry (seg, ins, intron, piece, alphabet, batch) run with dist_to_end = 0, so that one set
of facts holds under both platforms; the end trim has its own family (trim), at dist_to_end 20 and 30.

Facts of a region: plane name (longcallr_amd._abi.PLANE_NAMES, and "depth" = a + c + g + t) -> {column: value}.
"""
import functools
import os
import re

import numpy as np

import helpers
from longcallr_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "longcallr_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


TILE = int(re.search(r"#define LCR_TILE (\d+)", _src("lcr_dev.h")).group(1))
K1_RPB = int(re.search(r"#define K1_RPB (\d+)", _src("k1_pileup.hip")).group(1))
K1_BATCH = K1_RPB * TILE                                                                            # record slots of a K1 batch (K1_THREADS = LCR_TILE)
K1_PMAP = int(re.search(r"#define K1_PMAP \((\d+) \* K1_THREADS\)", _src("k1_pileup.hip")).group(1)) * TILE
K0_OPB = (int(re.search(r"#define K0_THREADS (\d+)", _src("k0_ops.hip")).group(1)) *
          int(re.search(r"#define K0_OPT (\d+)", _src("k0_ops.hip")).group(1)))                     # CIGAR ops of a K0 block
T = TILE
START0, STEP = 5000, 20000
ALT_OF = {"A": "C", "C": "A", "G": "T", "T": "G"}
BASE_PLANES = ("a", "c", "g", "t")


def make_ref(length, seed, force=()):
    """random ACGT without two equal neighbours; force: (column, string) written over it"""
    rng = np.random.default_rng(seed)
    ref = [str(rng.choice(list("ACGT")))]
    while len(ref) < length:
        ref.append(str(rng.choice([b for b in "ACGT" if b != ref[-1]])))
    for x, s in force:
        ref[x:x + len(s)] = list(s)
    return "".join(ref[:length])


def cyc_ref(length, force=()):
    """ACGTACGT...: the base of column x is CYC(x)"""
    ref = list(("ACGT" * (length // 4 + 1))[:length])
    for x, s in force:
        ref[x:x + len(s)] = list(s)
    return "".join(ref)


def CYC(x):
    return "ACGT"[x % 4]


def pick(*avoid):
    return next(b for b in "ACGT" if b not in avoid)


def ops_of(cigar):
    return [(int(n), c) for n, c in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]


def rd(ref, lo, cigar, over=None, at=None, ins=None, clip="GT", rev=0, ts=0, qual=30):
    """one read whose first aligned base stands on region column lo (may be negative).  Aligned bases: the reference base (upper case;
    A under a reference byte that is no ACGT, ACGT[x % 4] outside the region), over: column -> base.  Inserted bases: `ins` repeated, by
    default a base that differs from the reference base of the column behind the insertion, then TGTG...; clipped bases: `clip` repeated.
    at: read offset -> base, applied last.  "placed" lists (column, base) of the aligned bases inside the region."""
    over, at = over or {}, at or {}
    seq, cols, p = [], [], lo
    for n, c in ops_of(cigar):
        if c in "M=X":
            for x in range(p, p + n):
                b = ref[x].upper() if 0 <= x < len(ref) else "ACGT"[x % 4]
                seq.append(over.get(x, b if b in "ACGT" else "A"))
                cols.append(x)
            p += n
        elif c in "DN":
            p += n
        elif c == "I":
            s = ins or ((ALT_OF.get(ref[p].upper(), "T") if 0 <= p < len(ref) else "T") + "TG" * n)
            seq += list((s * n)[:n]); cols += [None] * n
        elif c == "S":
            seq += list((clip * n)[:n]); cols += [None] * n
    for o, b in at.items():
        seq[o] = b
    placed = [(x, b) for x, b in zip(cols, seq) if x is not None and 0 <= x < len(ref)]
    return dict(lo=lo, seq="".join(seq), cigar=cigar, rev=rev, ts=ts, qual=qual, placed=placed)


def cover(runs, col):
    """how many of the runs [lo, hi) hold the column"""
    return sum(lo <= col < hi for lo, hi in runs)


def tally(reads, cols):
    """counts of the bases the recipe placed on the columns: facts of the four count planes and the four forward planes (valid where nothing
    trims or masks)"""
    out = {k: {c: 0 for c in cols} for k in BASE_PLANES + tuple("fwd_" + k for k in BASE_PLANES)}
    want = set(cols)
    for r in reads:
        for x, b in r["placed"]:
            if x in want and b in "ACGT":
                out[b.lower()][x] += 1
                if not r["rev"]:
                    out["fwd_" + b.lower()][x] += 1
    return out


def region(label, ref, reads, facts, **meta):
    lo = [r["lo"] for r in reads]
    assert lo == sorted(lo), label          # (a region's reads are sorted by position: the ABI's precondition)
    return dict(label=label, ref=ref, reads=reads, facts=facts, meta=meta)


def build(regions):
    """(batch, {label: facts}, {label: region index}, {label: meta}); meta["reads"] = the batch indices of the region's reads"""
    reads, regs, n = [], [], 0
    for g, R in enumerate(regions):
        s0 = START0 + STEP * g
        for r in R["reads"]:
            reads.append(dict(pos=s0 + r["lo"], seq=r["seq"], qual=r["qual"], cigar=r["cigar"], rev=r["rev"], ts=r["ts"], region=g))
        R["meta"]["reads"] = list(range(n, n + len(R["reads"])))
        n += len(R["reads"])
        regs.append((s0, R["ref"]))
    labels = [R["label"] for R in regions]
    assert len(set(labels)) == len(labels)
    return (helpers.mk_batch(reads, regs), {R["label"]: R["facts"] for R in regions}, {R["label"]: g for g, R in enumerate(regions)},
            {R["label"]: R["meta"] for R in regions})


def hets(seed):
    """twelve reads over 600 columns, the alt base on every other read at the first and the last column of tile 1: two het calls under the
    ONT preset (min_depth 10) -- what the candidate stage's two histogram forms read K0's records for"""
    ref = make_ref(600, seed)
    cols = (T, 2 * T - 1)
    reads = [rd(ref, 0, "600M", over={x: ALT_OF[ref[x]] for x in cols} if k % 2 == 0 else {}, rev=k // 2 % 2, ts=1 + k // 2 % 2) for k in range(12)]
    return region("hets", ref, reads, dict(depth={x: 12 for x in cols}, **{k: v for k, v in tally(reads, cols).items()}), het_cols=list(cols))


# ---- seg: record geometry at tile borders ---------------------------------------------------------------------------------------------

# runs [lo, hi): ends on T - 1 (col0 + len = the pad slot); starts on T; spans T - 1 | T; spans all three tiles; exactly one tile (twice);
# length 1 on 0, T - 1, T and 599; clipped by the region's start; clipped by its end
SEG_RUNS = [(200, T), (T, 300), (250, 262), (100, 560), (0, T), (T, 2 * T), (0, 1), (T - 1, T), (T, T + 1), (599, 600), (-10, 5), (590, 610)]
SEG_COLS = sorted({0, 1, 4, 5, 99, 100, 199, 200, 249, 250, T - 2, T - 1, T, T + 1, 261, 262, 299, 300, 2 * T - 1, 2 * T, 559, 560, 589, 590, 598, 599})


def seg_region(kind):
    """kind M: a read of one M op per run; D / N: 5M <run> 5M around every run"""
    ref = make_ref(600, {"M": 11, "D": 12, "N": 13}[kind])
    reads, runs, m_runs = [], [], []
    for k, (lo, hi) in enumerate(sorted(SEG_RUNS)):
        if kind == "M":
            reads.append(rd(ref, lo, "%dM" % (hi - lo), rev=k % 2, ts=k % 3))
            m_runs.append((lo, hi))
        else:
            reads.append(rd(ref, lo - 5, "5M%d%s5M" % (hi - lo, kind), rev=k % 2, ts=k % 3))
            runs.append((lo, hi))
            m_runs += [(lo - 5, lo), (hi, hi + 5)]
    reads.sort(key=lambda r: r["lo"])
    facts = dict(depth={c: cover(m_runs, c) for c in SEG_COLS}, **tally(reads, SEG_COLS))
    if kind != "M":
        facts[kind.lower()] = {c: cover(runs, c) for c in SEG_COLS}
    return region("seg_" + kind, ref, reads, facts)


def seg():
    return build([seg_region("M"), seg_region("D"), seg_region("N"), hets(14)])


SEG_LENGTHS = [1, T - 1, None, T, T + 1, 2 * T]       # None: a region of 300 columns without reads


def seg_lengths():
    """regions of 1, T - 1, T, T + 1 and 2 T columns, a read-free one between them: a read over both ends, a read over exactly the region,
    a deletion and an intron over the whole region"""
    regions = []
    for g, L in enumerate(SEG_LENGTHS):
        if L is None:
            regions.append(region("len_free", make_ref(300, 20), [], dict(depth={0: 0, 299: 0}, n={0: 0, 299: 0})))
            continue
        ref = make_ref(L, 20 + g)
        reads = [rd(ref, -10, "%dM" % (L + 20), rev=1, ts=1), rd(ref, -3, "3M%dD3M" % L), rd(ref, -3, "3M%dN3M" % L, ts=2), rd(ref, 0, "%dM" % L)]
        regions.append(region("len_%d" % L, ref, reads, dict(depth={0: 2, L - 1: 2}, d={0: 1, L - 1: 1}, n={0: 1, L - 1: 1}, ni={0: 0, L - 1: 0})))
    return build(regions)


# ---- ins: insertions ---------------------------------------------------------------------------------------------------------------------

def ins():
    """p = the column behind the insertion; the record goes to column p - 1 for 1 <= p < len"""
    ref = make_ref(600, 31)
    reads = [
        rd(ref, -20, "10M1I40M"),            # p = -10: left of the window, no record
        rd(ref, -20, "20M1I30M"),            # p = 0: no record
        rd(ref, -20, "21M1I30M"),            # p = 1: column 0
        rd(ref, -20, "30M2I30M", rev=1),     # p = 10: column 9, in a read that starts left of the window
        rd(ref, 0, "2I50M"),                 # p = 0 as the read's first op: no record
        rd(ref, 0, "%dM2I100M" % T),         # p = T: tile 0, column T - 1
        rd(ref, 0, "%dM1I100M" % (T + 1)),   # p = T + 1: tile 1, column 0
        rd(ref, 300, "3H4S2I50M", ts=1),     # a leading insertion behind a hard and a soft clip: p = 300, column 299
        rd(ref, 500, "99M1I1M"),             # p = 599 = len - 1: column 598
        rd(ref, 500, "100M2I5M"),            # p = 600 = len: no record
    ]
    facts = dict(ni={0: 1, 1: 0, 9: 1, 10: 0, T - 2: 0, T - 1: 1, T: 1, T + 1: 0, 298: 0, 299: 1, 300: 0, 598: 1, 599: 0},
                 depth={0: 7, T - 1: 2, T: 2, 299: 2, 300: 3, 599: 2})
    return build([region("ins", ref, reads, facts)])


# ---- intron: tile_ndiff / tile_nbase ---------------------------------------------------------------------------------------------------------

def intron_read(ref, lo, hi, **kw):
    return rd(ref, lo - 10, "10M%dN10M" % (hi - lo), **kw)


def intron():
    assert T == 256                       # (the literals below are columns of tiles of 256)
    regions = []
    ref = make_ref(600, 41)
    regions.append(region("one_tile", ref, [intron_read(ref, 50, 150)], dict(n={49: 0, 50: 1, 149: 1, 150: 0, 255: 0, 256: 0}, depth={49: 1, 50: 0, 150: 1})))
    ref = make_ref(600, 42)
    regions.append(region("adjacent", ref, [intron_read(ref, 200, 300)], dict(n={199: 0, 200: 1, 255: 1, 256: 1, 299: 1, 300: 0, 512: 0})))
    ref = make_ref(600, 43)               # first tile 0, last tile 2: tile 1 is covered whole and holds no record
    regions.append(region("one_between", ref, [intron_read(ref, 200, 560)], dict(n={199: 0, 200: 1, 255: 1, 256: 1, 300: 1, 511: 1, 512: 1, 559: 1, 560: 0})))
    ref = make_ref(1100, 44)              # [256, 768): tiles 1 and 2 covered whole, by a record each; [256, 1024): tile 2 by nbase, tiles 1 and 3 by records
    regions.append(region("aligned", ref, [intron_read(ref, 256, 768), intron_read(ref, 256, 1024, rev=1, ts=1)],
                          dict(n={255: 0, 256: 2, 511: 2, 512: 2, 767: 2, 768: 1, 1023: 1, 1024: 0}, depth={255: 2, 256: 0, 768: 1, 1024: 1})))
    ref = make_ref(600, 45)               # clipped by the region's end: [300, 700) -> tiles 1 and 2; [100, 700) -> tiles 0 and 2, tile 1 by nbase
    regions.append(region("clipped", ref, [intron_read(ref, 100, 700), intron_read(ref, 300, 700)], dict(n={99: 0, 100: 1, 255: 1, 256: 1, 299: 1, 300: 2, 511: 2, 512: 2, 599: 2})))
    # two introns over whole tiles: A [100, 1100) on two reads covers tiles 1 .. 3, and tiles 1 and 2 hold records of other reads (nbase + the
    # tile's own difference array); B [1300, 2250) on three reads covers tiles 6 and 7, which stay record-free (k1_empty_tiles' constant)
    ref = make_ref(2304, 46)
    reads = [intron_read(ref, 100, 1100), intron_read(ref, 100, 1100, rev=1), rd(ref, 300, "50M", over={310: ALT_OF[ref[310]]}), rd(ref, 700, "50M", rev=1),
             intron_read(ref, 1300, 2250), intron_read(ref, 1300, 2250, ts=1), intron_read(ref, 1300, 2250, ts=2)]
    regions.append(region("two_introns", ref, reads,
                          dict(n={99: 0, 100: 2, 255: 2, 256: 2, 300: 2, 349: 2, 511: 2, 512: 2, 700: 2, 767: 2, 768: 2, 1023: 2, 1024: 2, 1099: 2, 1100: 0, 1299: 0, 1300: 3,
                                  1535: 3, 1536: 3, 1791: 3, 1792: 3, 2047: 3, 2048: 3, 2249: 3, 2250: 0},
                               depth={300: 1, 310: 1, 349: 1, 350: 0, 700: 1, 1536: 0, 2047: 0}, **{ALT_OF[ref[310]].lower(): {310: 1}})))
    return build(regions)


# ---- piece: K1 phase 2 ---------------------------------------------------------------------------------------------------------------------

PIECE_SIZES = [1, 15, 16, 17, 31, 32, 33, T - 1, T]


def piece():
    """A region per segment size n: sixteen reads nM 1I tM on columns 0 .. 15 (all column residues mod 4), t chosen so that a read has 1 mod 16
    bases -- the sixteen segments start on all sixteen byte residues.  Mismatches on the segment's first and last byte and on bytes 15 and
    16; the inserted base behind the segment differs from the reference base of the next column, which is where an unmasked last piece
    would count it."""
    regions = []
    for n in PIECE_SIZES:
        ref = make_ref(320, 100 + n)
        t = (-n) % 16 or 16
        reads, cols, segs = [], set(), []
        for j in range(16):
            mm = [x for x in (j, j + n - 1, j + 15, j + 16) if j <= x < j + n]
            reads.append(rd(ref, j, "%dM1I%dM" % (n, t), over={x: ALT_OF[ref[x]] for x in mm}, ins=ALT_OF[ref[j + n]], rev=j % 2, ts=j % 3))
            cols |= set(mm) | {j + n}
            segs.append((j, n))
        cols = sorted(cols)
        regions.append(region("piece_%d" % n, ref, reads, tally(reads, cols), segs=segs))
    regions.append(hets(150))
    return build(regions)


TAIL_REMS = [1, 3, 4, 8, 15, 0]


def tail(rem, last):
    """three reads on one column; the batch's last read is one M segment whose final 16-byte piece has `rem` bytes (0: all sixteen) before the
    base array ends.  last = "long": the read of 32 + rem bases; "short": the same reads with the one of 40 bases (8 bytes) last."""
    ref = make_ref(100, 200 + rem)
    m = 32 + rem
    r1 = rd(ref, 10, "20M", rev=1, ts=1)
    r2 = rd(ref, 10, "40M", over={12: ALT_OF[ref[12]], 49: ALT_OF[ref[49]]}, ts=2)
    r3 = rd(ref, 10, "%dM" % m, over={10: ALT_OF[ref[10]], 10 + m - 1: ALT_OF[ref[10 + m - 1]]})
    reads = [r1, r2, r3] if last == "long" else [r3, r1, r2]
    cols = [10, 11, 12, 29, 30, 49, 50, 10 + m - 1, 10 + m]
    return build([region("tail", ref, reads, dict(depth={10: 3, 29: 3, 30: 2, 9: 0}, **tally(reads, cols)), last_bytes=(rem or 16) if last == "long" else 8)])


# ---- alphabet --------------------------------------------------------------------------------------------------------------------------------

def alphabet():
    """six reads of every (strand, ts) with N / R / = in turn on columns 0, T - 1, T and 599 and N on column 300, two plain reads; reference
    N on T - 1 and 100, lower case on T, 110 and 111"""
    ref = make_ref(600, 51)
    force = [(T - 1, "N"), (100, "N"), (T, ref[T].lower()), (110, ref[110].lower()), (111, ref[111].lower())]
    ref = make_ref(600, 51, force=force)
    edge = [0, T - 1, T, 599]
    reads = []
    for k, (rev, ts) in enumerate([(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]):
        over = {x: "NR="[(k + i) % 3] for i, x in enumerate(edge)}
        over[300] = "N"
        over[111] = ALT_OF[ref[111].upper()] if k % 2 else ref[111].upper()
        reads.append(rd(ref, 0, "600M", over=over, rev=rev, ts=ts))
    for rev in (0, 1):
        reads.append(rd(ref, 0, "600M", over={300: "N", 111: ALT_OF[ref[111].upper()] if rev else ref[111].upper()}, rev=rev, ts=1))
    cols = edge + [100, 110, 111, 300]
    # transcript strand: (fwd, ts 1) and (rev, ts 2) count on ts_fwd, (fwd, ts 2) and (rev, ts 1) on ts_rev, whatever the base
    facts = dict(depth={0: 2, T - 1: 2, T: 2, 599: 2, 300: 0, 100: 8, 110: 8, 111: 8}, ts_fwd={c: 3 for c in cols}, ts_rev={c: 3 for c in cols}, **tally(reads, cols))
    assert facts["a"][100] == 8 and facts[ref[110].lower()][110] == 8 and facts[ref[111].lower()][111] == 4 and facts[ALT_OF[ref[111].upper()].lower()][111] == 4
    return build([region("alphabet", ref, reads, facts), hets(52)])


# ---- batch: slots, groups, maps ------------------------------------------------------------------------------------------------------------------

def short_reads(seed, n, per_col, label):
    """n reads of 4M, per_col of them on every start column: one op and one record each, all in tile 0"""
    ref = make_ref(T, seed)
    reads = [rd(ref, k // per_col, "4M", over={k // per_col + 1: ALT_OF[ref[k // per_col + 1]]} if k % 5 == 0 else {}, rev=k % 2, ts=k % 3) for k in range(n)]
    assert reads[-1]["lo"] + 4 <= T
    cols = [0, 1, 2, 3, 4, 5, (n - 1) // per_col, (n - 1) // per_col + 3, (n - 1) // per_col + 4]
    return region(label, ref, reads, tally(reads, cols), n_records=n)


def groups():
    """tiles of 15, 16, 17 and 512 records from one K0 block: a short group, a full one, a full and a group of one (odd count), and exactly one
    K1 batch of full groups"""
    return build([short_reads(61, 15, 4, "r15"), short_reads(62, 16, 4, "r16"), short_reads(63, 17, 4, "r17"), short_reads(64, K1_BATCH, 4, "r512")])


def one_more():
    return build([short_reads(65, K1_BATCH + 1, 4, "r513")])


def two_blocks():
    """8 + 1 100 one-op reads: the second region's tile gets 1 016 records from K0's first block (63 full groups and one of 8) and 84 from the second"""
    return build([short_reads(66, 8, 4, "r8"), short_reads(67, 1100, 8, "r1100")])


def many_pieces():
    """512 reads in one tile, 80M but every 32nd, which is 60M 2D 60M 1I 60M: the first K1 batch of 512 records has more than K1_PMAP pieces (map
    stride 2), and D and I records without pieces lie between the M records"""
    ref = make_ref(T, 68)
    reads = []
    for k in range(512):
        lo = k // 8
        if k % 32 == 0:
            reads.append(rd(ref, lo, "60M2D60M1I60M", over={lo + 70: ALT_OF[ref[lo + 70]]}, rev=1, ts=1))
        else:
            reads.append(rd(ref, lo, "80M", over={lo + 79: ALT_OF[ref[lo + 79]]} if k % 7 == 0 else {}, rev=k % 2, ts=k % 3))
    assert T == 256                       # the special reads start on 0, 4, ..., 60: deletions [lo + 60, lo + 62), insertions behind column lo + 121
    facts = dict(d={59: 0, 60: 1, 61: 1, 62: 0, 63: 0, 64: 1, 65: 1, 120: 1, 121: 1, 122: 0}, ni={120: 0, 121: 1, 122: 0, 125: 1, 181: 1, 182: 0},
                 depth={0: 8, 1: 16, 255: 0, 250: 0})
    return build([region("pmap", ref, reads, facts)])


# ---- trim: the ONT end trim ------------------------------------------------------------------------------------------------------------------------

def trim(D):
    """aligned read offsets c with |c - lead| < D or |c - reb| < D are dropped (util.rs:745-751): a read keeps [lead + D, reb - D]"""
    assert T == 256 and D in (20, 30)
    regions = []
    ref = make_ref(600, 71)               # an M block over lead + D; the same behind clips: lead > 0 shifts the zone with the read, not against the columns
    reads = [rd(ref, 100, "100M"), rd(ref, 400, "3H10S100M5S", rev=1, ts=1)]
    regions.append(region("straddle", ref, reads, dict(depth={100: 0, 100 + D - 1: 0, 100 + D: 1, 200 - D: 1, 200 - D + 1: 0, 199: 0,
                                                              400: 0, 400 + D - 1: 0, 400 + D: 1, 500 - D: 1, 500 - D + 1: 0}, ts_rev={400 + D - 1: 0, 400 + D: 1})))
    ref = make_ref(600, 72)               # an M block wholly inside the trimmed zone (offsets 0 .. 9): no record, the deletion behind it counts
    short = "10M2D5M1I10M3N5M"            # 31 bases < 2 D: no base kept; columns 20 .. 29 | D 30, 31 | 32 .. 36 | I | 37 .. 46 | N 47 .. 49 | 50 .. 54
    reads = [rd(ref, 20, short, ts=2), rd(ref, 300, "10M5D200M")]
    regions.append(region("inside", ref, reads, dict(depth={20: 0, 29: 0, 32: 0, 40: 0, 54: 0, 300: 0, 309: 0, 315: 0, 315 + D - 10 - 1: 0, 315 + D - 10: 1, 315 + 200 - D: 1, 315 + 200 - D + 1: 0},
                                                     d={29: 0, 30: 1, 31: 1, 32: 0, 309: 0, 310: 1, 314: 1, 315: 0}, n={46: 0, 47: 1, 49: 1, 50: 0}, ni={35: 0, 36: 1, 37: 0},
                                                     ts_fwd={25: 0, 40: 0}, ts_rev={25: 0, 40: 0})))
    ref = make_ref(600, 73)               # the trim boundary on the tile border: one read keeps [195 + D.., 255], the other [256, ...]
    reads = [rd(ref, 155 + D, "100M"), rd(ref, 256 - D, "100M", rev=1)]
    regions.append(region("edge", ref, reads, dict(depth={155 + 2 * D - 1: 0, 155 + 2 * D: 1, 254: 1, 255: 1, 256: 1, 257: 1, 356 - 2 * D: 1, 356 - 2 * D + 1: 0},
                                                   **{"fwd_" + ref[255].lower(): {255: 1}, "fwd_" + ref[256].lower(): {256: 0}})))
    ref = make_ref(600, 74)               # reads, and no record in any tile
    regions.append(region("free", ref, [rd(ref, 300, "15M"), rd(ref, 305, "%dM" % (2 * D - 1))], dict(depth={300: 0, 310: 0, 320: 0}, n={310: 0}, d={310: 0})))
    return build(regions)


# ---- zone: K1z ---------------------------------------------------------------------------------------------------------------------------------------

ZONE_PAIRS = [(40, 5), (63, 16), (63, 2), (1, 2), (64, 6), (64, 7), (40, 17), (40, 1)]
ZL, Z0, ZN = 700, 50, 400                 # region length, first column and aligned length of a zone read


def k1z_kernel(D, L):
    """launch_k1_zonefix's choice, restated"""
    return "k1_zonefix_ends" if 1 <= D <= 63 and 2 <= L <= 16 else "k1_zonefix"


def zone(D, L):     # noqa: C901
    """A region per read; reference ACGTACGT... (column x holds CYC(x)).  The base at aligned read offset c inside a zone (c - lead < D or
    reb - c < D) is dropped when a window of L equal bases X in ACGT starts in [c - L, c + 1] and X is not the reference byte of c's column
    (util.rs:754-789): a run of X over [t, t + R) masks [t - 1, t + R].  A region's facts say 0 / 1 for the read's base on the design column.
    L = 1 makes every base a window: a base is then masked by any neighbour that differs from its reference base, which turns most of the
    `not masked` facts over; they are written for both."""
    L2, D2 = L >= 2, D >= 2
    col = lambda c: Z0 + c                # of a read without a leading clip
    regions, n_bases = [], [0]

    def add(label, reads, facts, ref=None, **meta):
        regions.append(region(label, ref or cyc_ref(ZL), reads, facts, **meta))
        n_bases[0] += sum(len(r["seq"]) for r in reads)

    def run(t, n, X):
        return {o: X for o in range(t, t + n)}
    ref = cyc_ref(ZL)
    M = "%dM" % ZN
    z = ZN - D + 1                        # first offset of the trailing zone (reb = ZN)
    # the leading zone's last offset D - 1 against windows that start on c + 1 and on c + 2
    X = pick(CYC(col(D - 1)), CYC(col(D + L)))
    f = dict(depth={col(D - 1): 0, col(D): 1})
    if D2:
        f["depth"][col(D - 2)] = 1 if L2 else 0
    add("lead_c+1", [rd(ref, Z0, M, at=run(D, L, X))], f, runs=[(0, 0, D)])
    X = pick(CYC(col(D - 1)), CYC(col(D)), CYC(col(D + 1 + L)))
    add("lead_c+2", [rd(ref, Z0, M, at=run(D + 1, L, X))], dict(depth={col(D - 1): 1 if L2 else 0, col(D): 1}))
    # the same with ts = 0 on the reverse strand, and with N as the masked base: only ts is subtracted
    X = pick(CYC(col(D - 1)), CYC(col(D + L)))
    add("lead_ts0", [rd(ref, Z0, M, at=run(D, L, X), rev=1, ts=0)], dict(depth={col(D - 1): 0}, ts_fwd={col(D - 1): 0, col(D): 0}, ts_rev={col(D - 1): 0, col(D): 0}))
    at = run(D, L, X); at[D - 1] = "N"
    add("masked_N", [rd(ref, Z0, M, at=at, ts=2)], dict(ts_rev={col(D - 1): 0, col(D): 1}, a={col(D - 1): 0}, c={col(D - 1): 0}, g={col(D - 1): 0}, t={col(D - 1): 0}))
    # the trailing zone's first offset z against windows that start on c - L and on c - L - 1 (D = 1: |c - reb| < 1 holds for no aligned offset)
    if D2:
        X = pick(CYC(col(z)), CYC(col(z - L - 1)))
        add("trail_c-L", [rd(ref, Z0, M, at=run(z - L, L, X))], dict(depth={col(z): 0, col(z - 1): 1, col(z + 1): 1 if L2 else 0}), runs=[(0, 1, z - L)])
        X = pick(CYC(col(z)), CYC(col(z - 1)), CYC(col(z - L - 2)))
        add("trail_c-L-1", [rd(ref, Z0, M, at=run(z - L - 1, L, X))], dict(depth={col(z): 1 if L2 else 0, col(z - 1): 1}))
    else:
        add("trail_none", [rd(ref, Z0, M, at=run(ZN - L, L, pick(CYC(col(ZN - 1)), CYC(col(ZN - L - 1)))))], dict(depth={col(ZN - 1): 1, col(ZN - 2): 1}))
    # runs inside the soft clips that reach the aligned zone: [lead - L, lead) masks offset lead, [lead - L - 1, lead - 1) does not; [reb, reb + L) masks reb - 1
    add("clip_in", [rd(ref, Z0, "%dS%s" % (L + 2, M), at=run(2, L, "A"))], dict(depth={Z0: 0, Z0 + 1: 1 if L2 or not D2 else 0}), runs=[(0, 0, 2)])
    at = run(1, L, "A"); at.update({0: "G", L + 1: "T"})
    add("clip_out", [rd(ref, Z0, "%dS%s" % (L + 2, M), at=at)], dict(depth={Z0: 1 if L2 else 0}))
    X = pick(CYC(col(ZN - 1)))
    at = run(ZN, L, X); at.update({ZN + L: pick(X), ZN + L + 1: pick(X)})
    add("clip_trail", [rd(ref, Z0, "%s%dS" % (M, L + 2), at=at)], dict(depth={col(ZN - 1): 0 if D2 else 1}), runs=[(0, 1, ZN)])
    # runs at read offset 0 and at seq_len - 1
    X = pick(CYC(Z0), CYC(col(L)))
    add("run_at_0", [rd(ref, Z0, M, at=run(0, L, X))], dict(depth={Z0: 0, col(L): 0 if L < D else 1}))
    X = pick(CYC(col(ZN - 1)), CYC(col(ZN - 1 - L)))
    add("run_at_end", [rd(ref, Z0, M, at=run(ZN - L, L, X))], dict(depth={col(ZN - 1): 0 if D2 else 1}))
    # a run that equals the reference base (upper case: not masked; lower case: masked), a run of N
    X = pick(CYC(Z0 + L + 2))
    r2 = cyc_ref(ZL, force=[(Z0, X * (L + 2))])
    add("ref_equal", [rd(r2, Z0, M)], dict(depth={Z0: 1, Z0 + 1: 1}), ref=r2)
    r2 = cyc_ref(ZL, force=[(Z0, X.lower() * (L + 2))])
    add("ref_lower", [rd(r2, Z0, M)], dict(depth={Z0: 0, Z0 + 1: 0 if D2 else 1}), ref=r2)
    add("n_run", [rd(ref, Z0, M, at=run(0, L + 2, "N"), ts=1)], dict(depth={Z0: 0, Z0 + 1: 0}, ts_fwd={Z0: 1, Z0 + 1: 1}))
    # two runs of different bases reach offset lead: A in the clip (the reference base of its column), C behind it -- masked by C; without C, not masked
    r2 = cyc_ref(ZL, force=[(Z0, "A")])
    at = run(1, L, "A"); at.update({0: "G", L + 1: "T"}); at.update(run(L + 2, L, "C"))
    add("two_runs", [rd(r2, Z0, "%dS%s" % (L + 1, M), at=at)], dict(depth={Z0: 0}), ref=r2)
    at = run(1, L, "A"); at[0] = "G"
    add("equal_only", [rd(r2, Z0, "%dS%s" % (L + 1, M), at=at)], dict(depth={Z0: 1 if L2 else 0}), ref=r2)
    # a read shorter than L (one base for L <= 2), and a read whose zones overlap: every offset of [n - D + 1, D) lies in both, a base leaves once
    add("short", [rd(ref, Z0, "%dM" % max(L - 1, 1))], dict(depth={Z0: 1}))
    n = max(1, 3 * D // 2)
    t = n - D + 1
    if D2 and t + L <= n:
        X = pick(CYC(col(t)), CYC(col(t - 1)))
        add("overlap", [rd(ref, Z0, "%dM" % n, at=run(t, L, X))], dict(depth={col(t): 0, col(t - 1): 0}))
    else:
        add("overlap", [rd(ref, Z0, "%dM" % n)], dict(depth={Z0: 1}))
    # zones that cross an insertion, a deletion and an intron, forwards and backwards.  Leading: offsets 0-3 columns 50-53 | 4, 5 inserted | 6-9 columns
    # 54-57 | D 58-60 | 10-13 columns 61-64 | N 65-94 | 14 .. columns 95 ..; a run of A over [2, 2 + R), R = max(L, 13), masks [1, 2 + R]
    R = max(L, 13)
    f = dict(ni={53: 1}, d={58: 1, 60: 1}, n={65: 1, 94: 1})
    if D >= 17:
        f["depth"] = {51: 0, 55: 0, 62: 0, 95: 0, 52: 1 if L2 else 0, 56: 1, 64: 1}       # (columns 52, 56, 64 hold A: not masked by A)
    else:
        f["depth"] = {50: 1}
    add("lead_indel", [rd(ref, Z0, "4M2I4M3D4M30N400M", at=run(2, R, "A"))], f)
    # trailing: offsets 0-399 columns 50-449 | N 450-479 | 400-403 columns 480-483 | D 484-486 | 404-407 columns 487-490 | 408, 409 inserted | 410-413
    # columns 491-494; reb = 414; a run of T over [412 - R, 412) masks [411 - R, 412]: offset 413 is behind it
    f = dict(ni={490: 1}, d={484: 1, 486: 1}, n={450: 1, 479: 1})
    if D >= 17:
        f["depth"] = {449: 0, 481: 0, 488: 0, 492: 0, 493: 0, 494: 1 if L2 else 0, 483: 1, 487: 1, 491: 1}
    else:
        f["depth"] = {494: 1}
    add("trail_indel", [rd(ref, Z0, "400M30N4M3D4M2I4M", at=run(412 - R, R, "T"))], f)
    # zones whose columns lie outside the window
    add("left_of_window", [rd(ref, -30, "130M", at=run(0, L, pick(CYC(-30), CYC(-30 + L))))], dict(depth={0: 1 if L2 or D <= 30 else 0, 99: 1 if L2 else 0}))
    add("right_of_window", [rd(ref, 650, "100M", at=run(100 - L, L, pick(CYC(749), CYC(749 - L))))], dict(depth={699: 1 if L2 or D <= 49 else 0, 650: 1 if L2 else 0}))
    # a run of 70 C from offset 0: column 50 (G) masked, column 53 (C) not
    add("long_run", [rd(ref, Z0, M, at=run(0, 70, "C"))], dict(depth={Z0: 0, Z0 + 1: 0 if D2 else 1, Z0 + 3: 1}))
    # the batch's last read: a run in its trailing clip, the read placed (by the filler in front of it) so that the trailing zone's window bytes
    # start on byte 15 of a 16-byte line -- sh = 15 in zonefix_ends_body, and the run's window start falls on mask bit sh + (reb - lo) >= 64 for D + L > 49
    lo_win = max(max(ZN - D + 1, D) - L, 0)
    k = (15 - (n_bases[0] + lo_win)) % 16 or 16
    X = pick(CYC(col(ZN - 1)))
    at = run(ZN, L, X); at.update({ZN + L: pick(X), ZN + L + 1: pick(X)})
    add("last_read", [rd(ref, 10, "%dM" % k), rd(ref, Z0, "%s%dS" % (M, L + 2), at=at)], dict(depth={col(ZN - 1): 0 if D2 else 1}), runs=[(1, 1, ZN)])
    return build(regions)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------

GEOMETRY_ONT = dict(dist_to_end=0)


def case(name, family, builder, forms, hifi=None, ont=None):
    return dict(name=name, family=family, builder=builder, forms=tuple(forms), hifi=hifi or {}, ont=GEOMETRY_ONT if ont is None else ont)


BOTH = ("hifi", "fused", "lean")
CASES = [
    case("seg", "seg", seg, BOTH + ("tiles",)),
    case("seg_lengths", "seg", seg_lengths, BOTH),
    case("ins", "ins", ins, BOTH),
    case("intron", "intron", intron, BOTH),
    case("piece", "piece", piece, BOTH + ("tiles",)),
]
CASES += [case("tail_%d_%s" % (rem, last), "piece", functools.partial(tail, rem, last), BOTH) for rem in TAIL_REMS for last in ("long", "short")]
CASES += [
    case("alphabet", "alphabet", alphabet, BOTH + ("tiles",)),
    case("groups", "batch", groups, BOTH),
    case("one_more", "batch", one_more, BOTH),
    case("two_blocks", "batch", two_blocks, BOTH),
    case("many_pieces", "batch", many_pieces, BOTH),
]
CASES += [case("trim_%d" % D, "trim", functools.partial(trim, D), ("fused", "lean"), ont=dict(dist_to_end=D)) for D in (20, 30)]
CASES += [case("zone_%d_%d" % (D, L), "zone", functools.partial(zone, D, L), ("hifi",), hifi=dict(dist_to_end=D, polya_len=L)) for D, L in ZONE_PAIRS]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]
FAMILIES = ["seg", "ins", "intron", "piece", "alphabet", "batch", "trim", "zone"]
ONT_FORMS = ("fused", "lean", "tiles")


def names(form=None, family=None):
    return [c["name"] for c in CASES if (form is None or form in c["forms"]) and (family is None or c["family"] == family)]


@functools.lru_cache(maxsize=None)
def built(name):
    return BY_NAME[name]["builder"]()


def batch(name):
    return built(name)[0]


def facts(name):
    return built(name)[1]


def region_of(name, label):
    return built(name)[2][label]


def meta(name):
    return built(name)[3]


def platform_of(form):
    return "ont" if form in ONT_FORMS else "hifi"


@functools.lru_cache(maxsize=None)
def params(name, platform):
    c = BY_NAME[name]
    assert any(platform_of(f) == platform for f in c["forms"]), (name, platform)
    if platform == "ont":
        return _abi.make_params("ont-cdna", **dict(dict(seed=6), **c["ont"]))
    return _abi.make_params("hifi-masseq", **dict(dict(seed=6), **c["hifi"]))


def platforms(name):
    return sorted({platform_of(f) for f in BY_NAME[name]["forms"]})


# ---- the census: what the kernels will meet, counted from the batch alone --------------------------------------------------------------------------------

def records(b, prm):
    """K0's records, restated from k0_ops.hip: per global tile the list of (kind, first column in the tile, length, byte offset of the first base
    or None, flat op index) in the order of the flat CIGAR array.  M blocks clipped to the region and, on ONT, to the offsets the end trim keeps;
    D runs in every tile they touch; an insertion on the column in front of it; an intron in its first and its last tile -- the tiles between
    them count it in nbase (tile_ndiff's prefix sum).  Returns (records per tile, nbase per tile, first tile of every region)."""
    ont, D = int(prm.platform) == _abi.LCR_PLATFORM_ONT, int(prm.dist_to_end)
    first = np.concatenate([[0], np.cumsum([(int(n) + T - 1) // T for n in b.len])])
    tiles = [[] for _ in range(int(first[-1]))]
    nbase = [0] * int(first[-1])
    for g in range(b.n_regions):
        vec, s0 = int(b.len[g]), int(b.start0[g])
        for r in range(int(b.read_begin[g]), int(b.read_begin[g + 1])):
            lead, reb = int(b.lead_clip[r]), int(b.seq_len[r]) - int(b.trail_clip[r])
            p, q, c0 = int(b.pos[r]) - s0, max(lead, 0), int(b.cig_off[r])
            for j, w in enumerate(b.cigar[c0:c0 + int(b.n_cig[r])].tolist()):
                op, n = w & 15, w >> 4
                m = op in (0, 7, 8)
                if m or op in (2, 3):
                    a, e = max(p, 0), min(p + n, vec)
                    if m and ont:
                        a, e = max(a, p + (lead + D - q)), min(e, p + (reb - D + 1 - q))
                    if n > 0 and e > a:
                        ts = range(a // T, (e - 1) // T + 1) if op != 3 else sorted({a // T, (e - 1) // T})
                        if op == 3:
                            for t in range(a // T + 1, (e - 1) // T):
                                nbase[int(first[g]) + t] += 1
                        for t in ts:
                            lo, hi = max(a, t * T), min(e, (t + 1) * T)
                            off = int(b.seq_off[r]) + q + (lo - p) if m else None
                            tiles[int(first[g]) + t].append(("MDN"[0 if m else op - 1], lo - t * T, hi - lo, off, c0 + j))
                    p += n
                elif op == 1 and n > 0 and 1 <= p < vec:
                    tiles[int(first[g]) + (p - 1) // T].append(("I", (p - 1) % T, 1, None, c0 + j))
                if m or op == 1:
                    q += n
    return tiles, nbase, first


def k1_batches(recs):
    """a tile's records as K1 meets them: the records of one K0 block (K0_OPB consecutive ops) lie back to back and are cut into groups of at
    most 16, a group takes 16 slots, K1 takes K1_BATCH slots at a time.  Returns (group sizes, pieces per K1 batch)."""
    sizes = []
    blocks = {}
    for rec in recs:
        blocks.setdefault(rec[4] // K0_OPB, []).append(rec)
    slots = []
    for blk in sorted(blocks):
        rs = blocks[blk]
        for i in range(0, len(rs), 16):
            grp = rs[i:i + 16]
            sizes.append(len(grp))
            slots += grp + [None] * (16 - len(grp))
    pieces = [sum((x[2] + 15) // 16 for x in slots[i:i + K1_BATCH] if x is not None and x[0] == "M") for i in range(0, len(slots), K1_BATCH)]
    return sizes, pieces


def zone_window(b, r, end, D, L):
    """zonefix_ends_body's window of read r's leading (0) / trailing (1) zone, restated: (zlo, lo, n, sh) or None when the kernel leaves early"""
    seq_len, lead = int(b.seq_len[r]), int(b.lead_clip[r])
    reb = seq_len - int(b.trail_clip[r])
    zlo = lead if end == 0 else max(reb - D + 1, lead + D)
    zhi = min(lead + D, reb) - 1 if end == 0 else reb - 1
    if zlo > zhi:
        return None
    lo, hi = max(zlo - L, 0), min(zhi + L, seq_len - 1)
    if hi - lo + 1 < L:
        return None
    return zlo, lo, hi - lo + 1, (int(b.seq_off[r]) + lo) % 16

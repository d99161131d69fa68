"""Recipes for K0's indel fold (csrc/k0_ops.hip: REC_F_INS / REC_F_DEL, lcr_dev.h): plain data, builders and a model of the rule, no tests.

The rule.  A 1-base indel that directly follows an M op of its read leaves no record of its own: its count travels as a flag of that M op's
record in the M's last tile.  With end = the M's unclipped end column, ee = its kept end (region clip, ONT end trim), vec = the region's
length, T = LCR_TILE, and the next op of the SAME read inside the same wave's ops (64 * K0_OPT consecutive ops of the batch's flat CIGAR
array; a wave's last op never folds):
    next is I with len > 0:   ee == end, 1 <= end < vec                     -> the point on column end - 1 is the M record's last column
    next is D with len == 1:  ee == end, 0 <= end < vec, end % T != 0       -> the deleted column end lies in the M's last tile
Everything else keeps its record: a D of length >= 2, a D on the first column of the next tile, an M whose end is trimmed or clipped or
that is trimmed away, an indel that opens a read or follows anything but an M, the second of M I D / M D I, a pair split by a wave's end.
A folded op still counts as an item (lcr_pileup_records: items stay, records fall).

fold_model() restates that rule -- from the text above, not from the kernel -- on top of pileup_cases.records (the records WITHOUT the fold).
The cases follow pileup_cases: one region per recipe, reads written out, facts for the d / ni planes (and depth) at the design columns
written down by hand.  A fact key "plane@ont" / "plane@hifi" holds under that platform only (the end trim is ONT's).  Every case says what
the rule does in it: folds (it folds at least one op), keeps (it leaves at least one counting indel op a record of its own).
"""
import functools
import re

import numpy as np

import helpers
import pileup_cases as pc
from longcallr_amd import _abi
from pileup_cases import ALT_OF, T, build, make_ref, rd, region

K0_OPB = pc.K0_OPB
K0_OPT = int(re.search(r"#define K0_OPT (\d+)", pc._src("k0_ops.hip")).group(1))
WOPS = 64 * K0_OPT                  # ops of a K0 wave
K0_WIN = int(re.search(r"#define K0_THREADS (\d+)", pc._src("k0_ops.hip")).group(1))     # tiles of a block's LDS window (K0_WIN = K0_THREADS)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------

def fold_model(b, prm):
    """(items, records, folded): the counting M / D / I / N ops of the batch, the records K0 emits for them under the rule, and the folded
    ops as (flat op index, "I" | "D", flat op index of the M in front)"""
    ont, D = int(prm.platform) == _abi.LCR_PLATFORM_ONT, int(prm.dist_to_end)
    cig0 = int(b.cig_off[0]) if b.n_reads else 0
    items, folded = 0, []
    for g in range(b.n_regions):
        vec, s0 = int(b.len[g]), int(b.start0[g])
        for r in range(int(b.read_begin[g]), int(b.read_begin[g + 1])):
            lead, reb = int(b.lead_clip[r]), int(b.seq_len[r]) - int(b.trail_clip[r])
            p, q, c0 = int(b.pos[r]) - s0, max(lead, 0), int(b.cig_off[r])
            ops = b.cigar[c0:c0 + int(b.n_cig[r])].tolist()
            for i, w in enumerate(ops):
                op, n = w & 15, w >> 4
                m = op in (0, 7, 8)
                counts = False
                if m or op in (2, 3):
                    a, e = max(p, 0), min(p + n, vec)
                    if m and ont:
                        a, e = max(a, p + (lead + D - q)), min(e, p + (reb - D + 1 - q))
                    counts = n > 0 and e > a
                    j = c0 - cig0 + i
                    if m and counts and i + 1 < len(ops) and j % WOPS != WOPS - 1 and e == p + n:
                        op2, n2, end = ops[i + 1] & 15, ops[i + 1] >> 4, p + n
                        if op2 == 1 and n2 > 0 and 1 <= end < vec:
                            folded.append((j + 1, "I", j))
                        elif op2 == 2 and n2 == 1 and 0 <= end < vec and end % T != 0:
                            folded.append((j + 1, "D", j))
                    p += n
                elif op == 1:
                    counts = n > 0 and 1 <= p < vec
                if m or op == 1:
                    q += n
                items += counts
    unfolded = sum(len(t) for t in pc.records(b, prm)[0])
    return items, unfolded - len(folded), folded


def unfolded_records(b, prm):
    """the records K0 emits without the fold (lcr_debug_set("fold_indels", 0))"""
    return sum(len(t) for t in pc.records(b, prm)[0])


def kept_indels(b, prm):
    """counting I ops and D ops of length 1 that stay records: flat op indices"""
    gone = {j for j, _, _ in fold_model(b, prm)[2]}
    return [x[4] for t in pc.records(b, prm)[0] for x in t if (x[0] == "I" or (x[0] == "D" and _d_len(b, x[4]) == 1)) and x[4] - int(b.cig_off[0]) not in gone]


def _d_len(b, j):
    return int(b.cigar[j]) >> 4


# ---- the recipes --------------------------------------------------------------------------------------------------------------------------

def hets_fold(seed):
    """pileup_cases.hets with folded indels in every read: 200M 1D 155M 1I 244M -- the M behind the deletion crosses T (its insertion flag rides on
    tile 1's record only, beside the het column T), the last M crosses 2 T (het column 2 T - 1 in front of the border)"""
    ref = make_ref(600, seed)
    cols = (T, 2 * T - 1)
    reads = [rd(ref, 0, "200M1D155M1I244M", over={x: ALT_OF[ref[x]] for x in cols} if k % 2 == 0 else {}, rev=k // 2 % 2, ts=1 + k // 2 % 2) for k in range(12)]
    facts = dict(depth={T: 12, 2 * T - 1: 12, 200: 0, 199: 12, 201: 12}, d={199: 0, 200: 12, 201: 0}, ni={T - 1: 0, 354: 0, 355: 12, 356: 0},
                 **pc.tally(reads, cols))
    return region("hets", ref, reads, facts, het_cols=list(cols))


def mid():
    """the common case in the middle of a tile: M / = / X in front, I of 1 and of 5 bases, a D of 1; a D of 2 stays"""
    ref = make_ref(600, 301)
    reads = [rd(ref, 10, "30M1I30M"),                    # M [10, 40): point on 39
             rd(ref, 12, "30=5I30X", rev=1, ts=1),       # = [12, 42): point on 41
             rd(ref, 14, "30X1D30M", ts=2),              # X [14, 44): column 44 deleted
             rd(ref, 16, "30M1D30=", rev=1, ts=2),       # column 46 deleted
             rd(ref, 100, "20M2D20M")]                   # columns 120, 121: a record
    facts = dict(ni={38: 0, 39: 1, 40: 0, 41: 1, 42: 0}, d={43: 0, 44: 1, 45: 0, 46: 1, 47: 0, 119: 0, 120: 1, 121: 1, 122: 0},
                 depth={20: 4, 39: 4, 44: 3, 46: 3, 120: 0})
    return build([region("mid", ref, reads, facts), hets_fold(302)])


def tile_end():
    """an M that ends on column T - 1 (end % T == 0): the I folds onto T - 1, the D on column T stays a record of the next tile; an M with
    end % T == T - 1: the D folds onto T - 1, its end marker onto the pad slot T, the I onto T - 2"""
    ref = make_ref(600, 303)
    reads = [rd(ref, 200, "%dM1I20M" % (T - 200)),
             rd(ref, 200, "%dM1D20M" % (T - 200), rev=1),
             rd(ref, 205, "%dM1D20M" % (T - 206), ts=1),
             rd(ref, 206, "%dM2I20M" % (T - 207), rev=1, ts=2)]
    facts = dict(ni={T - 3: 0, T - 2: 1, T - 1: 1, T: 0}, d={T - 2: 0, T - 1: 1, T: 1, T + 1: 0}, depth={T - 1: 3, T: 3}, n={0: 0, T: 0})
    return build([region("tile_end", ref, reads, facts)])


def cross():
    """an M over one tile border and over two: the flags ride on the last tile's record only"""
    ref = make_ref(600, 304)
    reads = [rd(ref, 100, "450M1I10M", ts=1),            # M [100, 550): point on 549
             rd(ref, 100, "450M1D10M", rev=1, ts=2),     # column 550 deleted
             rd(ref, 250, "20M1I10M"),                   # M [250, 270): point on 269
             rd(ref, 250, "20M1D10M", rev=1)]            # column 270 deleted
    facts = dict(ni={T - 1: 0, T: 0, 268: 0, 269: 1, 270: 0, 2 * T - 1: 0, 2 * T: 0, 548: 0, 549: 1, 550: 0},
                 d={T: 0, T + 1: 0, 269: 0, 270: 1, 271: 0, 2 * T: 0, 2 * T + 1: 0, 549: 0, 550: 1, 551: 0}, n={0: 0, T: 0, 2 * T: 0},
                 depth={T - 1: 4, T: 4, 269: 4, 270: 3, 550: 1})
    return build([region("cross", ref, reads, facts)])


def region_end():
    """a last tile of 88 columns; an M that ends at the region's last column, one before it, and beyond it"""
    ref = make_ref(600, 305)
    reads = [rd(ref, 520, "20M1D10M"),                   # inside the short tile: column 540
             rd(ref, 560, "40M1I5M"),                    # end == vec: the I is counted nowhere
             rd(ref, 560, "39M1I5M", rev=1),             # end == vec - 1: folds, point on 598
             rd(ref, 561, "38M1D5M"),                    # end == vec - 1: column 599 deleted, folds
             rd(ref, 570, "40M1I5M", ts=1),              # M clipped by the region: no fold, and the I lies outside
             rd(ref, 575, "25M1D5M", ts=2)]              # end == vec: the D lies outside
    facts = dict(ni={597: 0, 598: 1, 599: 0}, d={539: 0, 540: 1, 541: 0, 598: 0, 599: 1}, depth={540: 0, 599: 4, 598: 5})
    return build([region("region_end", ref, reads, facts)])


def region_start():
    """M ops that start before the region: clipped at their start they still fold; one that ends on column 0 has no record to carry a flag"""
    ref = make_ref(600, 306)
    reads = [rd(ref, -30, "20M1I30M"),                   # M [-30, -10): none; the I lies outside
             rd(ref, -25, "25M1D20M"),                   # M [-25, 0): none -- column 0 deleted, a record
             rd(ref, -24, "25M1I20M"),                   # M [-24, 1): one column; point on 0, folds
             rd(ref, -20, "50M1I20M"),                   # point on 29, folds
             rd(ref, -20, "50M1D20M", rev=1)]            # column 30 deleted, folds
    facts = dict(ni={0: 1, 1: 0, 28: 0, 29: 1, 30: 0}, d={0: 1, 1: 0, 29: 0, 30: 1, 31: 0}, depth={0: 4, 30: 1})
    return build([region("region_start", ref, reads, facts)])


def trim():
    """ONT end trim at dist_to_end 20 cutting an M's end, and the whole M, in front of an I and of a D: both stay records, the counts stay on
    their columns.  At dist_to_end 0 (and under the HiFi preset) the same reads fold."""
    ref = make_ref(600, 307)
    reads = [rd(ref, 100, "100M1I10M"),                  # 111 bases: offsets 20 .. 91 kept, M [100, 200) -> [120, 192): point on 199
             rd(ref, 100, "100M1D10M", rev=1),           # 110 bases: offsets 20 .. 90 kept: column 200 deleted
             rd(ref, 300, "10M1I100M"),                  # offsets 0 .. 9 trimmed: no M record; point on 309
             rd(ref, 300, "10M1D100M", ts=1),            # column 310 deleted
             rd(ref, 400, "50M1I50M", ts=2)]             # offset 49 is kept either way: folds, point on 449
    return ref, reads, dict(ni={198: 0, 199: 1, 200: 0, 308: 0, 309: 1, 310: 0, 449: 1}, d={199: 0, 200: 1, 201: 0, 309: 0, 310: 1, 311: 0})


def trim_20():
    ref, reads, facts = trim()
    facts.update({"depth@ont": {199: 0, 150: 2, 192: 0, 191: 1, 305: 0, 449: 1}, "depth@hifi": {199: 2, 150: 2, 305: 2, 449: 1}})
    return build([region("trim", ref, reads, facts)])


def trim_0():
    ref, reads, facts = trim()
    facts.update(depth={199: 2, 150: 2, 305: 2, 449: 1})
    return build([region("trim", ref, reads, facts)])


def neighbours():
    """M I D, M D I, M 2D, M N, M S, M D D; I and D as a read's first op, an I behind a soft clip"""
    ref = make_ref(600, 308)
    reads = [rd(ref, 10, "20M1I1D20M"),                  # I folds (point on 29), the D behind it (column 30) is a record
             rd(ref, 12, "20M1D1I20M", rev=1),           # D folds (column 32), the I behind it (point on 32) is a record
             rd(ref, 14, "20M2D20M"),                    # columns 34, 35
             rd(ref, 16, "20M50N20M", ts=1),             # intron [36, 86)
             rd(ref, 100, "20M5S"),
             rd(ref, 120, "1I20M"),                      # point on 119
             rd(ref, 140, "1D20M", ts=2),                # column 140
             rd(ref, 200, "3S1I20M"),                    # point on 199
             rd(ref, 300, "20M1D1D20M", rev=1)]          # column 320 folds, column 321 is a record
    facts = dict(ni={28: 0, 29: 1, 30: 0, 31: 0, 32: 1, 33: 0, 118: 0, 119: 1, 120: 0, 199: 1},
                 d={29: 0, 30: 1, 31: 0, 32: 1, 33: 0, 34: 1, 35: 1, 36: 0, 140: 1, 141: 0, 319: 0, 320: 1, 321: 1, 322: 0}, n={35: 0, 36: 1, 85: 1, 86: 0})
    return build([region("neighbours", ref, reads, facts)])


def read_border():
    """the last M of a read in front of the next read's first op, an I or a D: the columns of a wrong fold (39, 90) stay empty.  The rule
    touches nothing here."""
    ref = make_ref(600, 309)
    reads = [rd(ref, 10, "30M"), rd(ref, 50, "1I30M"), rd(ref, 60, "30M", rev=1), rd(ref, 100, "1D30M", ts=1)]
    facts = dict(ni={39: 0, 49: 1, 50: 0}, d={90: 0, 100: 1, 101: 0})
    return build([region("read_border", ref, reads, facts)])


def strands():
    """every (strand, transcript strand) with an I and with a D behind an M: the flags beside the strand bits"""
    ref = make_ref(600, 310)
    combos = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]
    reads = [rd(ref, 10 + k, "30M1I30M", rev=rev, ts=ts) for k, (rev, ts) in enumerate(combos)]       # points on 39 + k
    reads += [rd(ref, 110 + k, "30M1D30M", rev=rev, ts=ts) for k, (rev, ts) in enumerate(combos)]     # columns 140 + k deleted
    facts = dict(ni={38: 0, 39: 1, 40: 1, 41: 1, 42: 1, 43: 1, 44: 1, 45: 0}, d={139: 0, 140: 1, 141: 1, 142: 1, 143: 1, 144: 1, 145: 1, 146: 0},
                 depth={20: 6, 125: 6, 142: 5}, ts_fwd={20: 2, 125: 2, 142: 2}, ts_rev={20: 2, 125: 2, 142: 1})      # (column 142: the (fwd, ts 2) read's deletion)
    return build([region("strands", ref, reads, facts)])


LONG_UNITS = K0_OPB // 4 + 20       # units "2M1D2M1I" of the long read: 4 ops and 5 columns each
LONG_LO = 10
FILLER = {0: None, 1: "5M", 2: "5M2S", 3: "5M2D5M"}


def long_read(shift):
    """one read of 2S + LONG_UNITS x (2M 1D 2M 1I), more than K0_OPB ops, behind `shift` ops of a read in a region in front of it: over the four shifts
    an M / indel pair falls on every thread border, on every wave border and on the block border (tests/test_indel_fold_cases.py reads that
    off the op indices)"""
    regions = []
    if FILLER[shift]:
        ref = make_ref(100, 320 + shift)
        regions.append(region("filler", ref, [rd(ref, 10, FILLER[shift])], dict(depth={10: 1, 9: 0})))
    ref = make_ref(5 * LONG_UNITS + 40, 330 + shift)
    reads = [rd(ref, LONG_LO, "2S" + "2M1D2M1I" * LONG_UNITS)]
    u = LONG_UNITS - 1
    facts = dict(d={LONG_LO + 1: 0, LONG_LO + 2: 1, LONG_LO + 3: 0, LONG_LO + 7: 1, LONG_LO + 5 * u + 2: 1},
                 ni={LONG_LO + 3: 0, LONG_LO + 4: 1, LONG_LO + 5: 0, LONG_LO + 9: 1, LONG_LO + 5 * u + 4: 1},
                 depth={LONG_LO: 1, LONG_LO + 2: 0, LONG_LO + 4: 1})
    regions.append(region("long", ref, reads, facts))
    return build(regions)


OVF_L, OVF_S, OVF_READS = 102000, 500, 6


def overflow():
    """six reads 100M 100000N (3M1D) x 10 (3M1I) x 10: the records behind the intron lie outside their block's LDS window of K0_WIN tiles and take
    the overflow path, flags and all (the shape of test_gpu_parity.test_k0_thousands_of_records_beyond_the_tile_window)"""
    rng = np.random.default_rng(311)
    ref = "".join(rng.choice(list("ACGT"), size=OVF_L))
    t0 = OVF_S + 100 + 100000
    reads = [rd(ref, OVF_S, "100M100000N" + "3M1D" * 10 + "3M1I" * 10, rev=k % 2, ts=k % 3) for k in range(OVF_READS)]
    t1 = t0 + 40
    facts = dict(d={t0 + 2: 0, t0 + 3: OVF_READS, t0 + 4: 0, t0 + 39: OVF_READS, t1: 0}, ni={t1 + 1: 0, t1 + 2: OVF_READS, t1 + 3: 0, t1 + 29: OVF_READS},
                 n={OVF_S + 99: 0, OVF_S + 100: OVF_READS, t0 - 1: OVF_READS, t0: 0})
    return build([region("overflow", ref, reads, facts)])


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------

FORMS = ("hifi", "fused", "lean")


def case(name, builder, folds, keeps, ont=None, hets=False):
    """folds / keeps: the rule folds at least one op / leaves at least one counting I or 1-base D a record (under the ONT form's params)"""
    return dict(name=name, builder=builder, folds=folds, keeps=keeps, ont=dict(dist_to_end=0) if ont is None else ont, hets=hets)


CASES = [
    case("mid", mid, True, False, hets=True),
    case("tile_end", tile_end, True, True),
    case("cross", cross, True, False),
    case("region_end", region_end, True, False),
    case("region_start", region_start, True, True),
    case("trim_20", trim_20, True, True, ont=dict(dist_to_end=20)),
    case("trim_0", trim_0, True, False),
    case("neighbours", neighbours, True, True),
    case("read_border", read_border, False, True),       # the rule does not touch this case
    case("strands", strands, True, False),
]
CASES += [case("long_%d" % s, functools.partial(long_read, s), True, True) for s in range(4)]
CASES += [case("overflow", overflow, True, False)]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]
PLATFORMS = ("hifi", "ont")


@functools.lru_cache(maxsize=None)
def built(name):
    return BY_NAME[name]["builder"]()


def batch(name):
    return built(name)[0]


def facts(name, platform):
    """{label: {plane: {column: value}}} with the platform's own facts folded in"""
    out = {}
    for label, f in built(name)[1].items():
        out[label] = {}
        for key, at in f.items():
            plane, _, only = key.partition("@")
            if only in ("", platform):
                out[label].setdefault(plane, {}).update(at)
    return out


def region_of(name, label):
    return built(name)[2][label]


def meta(name):
    return built(name)[3]


@functools.lru_cache(maxsize=None)
def params(name, platform):
    if platform == "ont":
        return _abi.make_params("ont-cdna", **dict(dict(seed=6), **BY_NAME[name]["ont"]))
    return _abi.make_params("hifi-masseq", seed=6)


@functools.lru_cache(maxsize=None)
def model(name, platform):
    return fold_model(batch(name), params(name, platform))

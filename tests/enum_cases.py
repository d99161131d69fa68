"""Recipes for the enumeration branch of the phase stage (csrc/k4_enum.hip, host control csrc/k4_phase.hip): plain data and builders, no tests.

A case is one small batch (one region unless stated), its parameters, the kernel class its size gives it (predicted_class, a restatement of
the host's class rule) and its census: what the CPU restatement of the restarts (Census below) must have met for the case to count as a visit
of the limit it was built for.  tests/test_enum_cases.py runs the two CPU oracles against each other and checks every census;
tests/test_enum_cases_gpu.py puts the same cases in front of k4_enum_bits, k4_enum_reg, k4_enum_big and their resolve / repair kernels.

The limits (csrc/k4_kernels.h, csrc/k4_phase.hip), copied below the way tests/test_stage_forms_gpu.py copies STG_E:
  ENUM_TQ = 126       tied rows of more than two entries a wave queues per sigma step; beyond it k4_enum_reg scores them on their lanes and
                      k4_enum_bits in place
  ENUM_TCAP = 256     configurations of maximal objective k4_enum_resolve compares at a time; resolve_tlcap(S) sizes the list of them
  ENUM_LDS_MAX        63 KB: the image of a region of the bit-state class (enum_layout(bits)), of the streaming class (enum_layout) and
                      of k4_enum_resolve (resolve_layout); beyond them, or with a lane that owns more than 64 rows, the global-memory class
  REDO_GRID = 512     workgroups of k4_enum_redo: a longer repair list gives a workgroup several restarts
  ENUM_BITS_PER = 64  restarts per tile of k4_enum_bits; enum_bits_sp rounds S up to 8

Reads are short: SITE_GAP bases between neighbouring sites, MARGIN bases in front of a read's first and behind its last site (beyond every
preset's dist_to_end), so a read covers exactly the sites of its range and 100 bases never hold five sites (the dense filter).  A het site's
alt is never A>G / T>C (ALT_OF), so no site is of the RNA-editing class.

How the tied rows are built.  A row's sigma decision ties when its signed fixed-point weights cancel: sum over its entries at het sites of
+-w[q], w[q] = f1e[q] - fe[q].  Rows whose entries all have ONE quality tie whenever as many of them match as mismatch -- under the winning
delta the `recombinant' rows (alt allele on half of their sites) do, and so does every equal-quality row of an even number of entries in the
first sigma step of a restart whose start delta has as many +1 as -1.  The tq_* cases therefore give their clean rows a different quality at
every site (no signed sum of four different w[q] is zero): the recombinant rows are the ONLY rows of more than two entries that can tie, in
any step of any restart, and their number is the case's number.

The tied rows have quality TIED_Q = 26: with two matches and two mismatches at that quality the f64 scores of the two signs differ for all
six patterns, so about half of the tied rows FLIP when they are scored (at quality 30 the two scores are one double and a tied row stays
as it is, whoever scores or forgets it).  A flip that is lost stays hidden in the region's result all the same -- the restarts that did
not need it outvote the one that lost it, and assign_reads_haplotype scores every row again -- so the GPU tests hold the tie census to
the oracle's count for count (test_enum_cases_gpu.test_sigma_ties_alone), which no lost flip passes.

Left out, and why:
  * a delta / eta tie at the maximum (tie class 2) in an enumeration region.  The enumeration restarts choose among (delta, het), (-delta,
    het), hom-ref and hom-var.  The two het scores tie when the weights of the entries that match under delta and under -delta are equal,
    W / 2 each; the entries with the reference base and those with the alt base also split W, so one hom genotype explains at least
    W / 2 -- and its prior (log10 0.9985 or log10 0.0005) beats the het prior (log10 0.001 - n log10 2) for n >= 2 entries: the maximum
    is a hom score, not the tie.  For n = 1 the het and the hom-var prior are one fixed-point number, but there hom-ref is the maximum:
    it takes the one entry as a match, or as an error that costs at most 3.0 against 3.3 for the other priors.  (Any other tie between
    a het and a hom score would need the data terms to differ by exactly the priors' fixed-point difference.)  So redo_over_grid does not start from the flipped-allele construction of test_gpu_parity.test_chain_ties_of_classes_2_and_4
    -- with ten sites its flipped sites simply go hom: 6 and 12 restarts of 1 024 on the repair list -- but fills the list with tie-only
    steps (class 4), the only way in; its census asks for class2_ties == 0;
  * base quality 0 in single_entry_rows: eps = 1 makes log10(1 - eps) infinite, the reference panics there (phase.rs:307) and
    oracle_np_phase with it; liblcr and the C++ oracle treat it as q = 1, which tests/test_gpu_parity.py::test_edge_cases covers.
"""
import functools
import math

import numpy as np

import helpers
from longcallr_amd import _abi
from oracle import oracle_np_phase as onp2

# ---- the constants of csrc/k4_kernels.h and csrc/k4_phase.hip ----------------------------------------------------------------------
ENUM_WAVES = 4
ENUM_LDS_MAX = 63 * 1024
ENUM_TQ = 126
ENUM_TCAP = 256
ENUM_BITS_PER = 64
REDO_CAP, REDO_GRID = 8192, 512


def enum_bits_sp(S):
    return (S + 7) & ~7


def enum_bits_stride(R, S):
    return ((R + 15) & ~7) + 8 * 8 * enum_bits_sp(S) + 8 * 32 + 4 * 24 + 4 * (ENUM_TQ + 2)


def enum_layout(R, E, bits=False, S=32):
    """EnumLayout.total"""
    o = 256 + 512
    o += 8 * (E + (64 * min(S, 31) if bits else 0))
    o += 4 * E
    o += 2 * (R + 1)
    o += 2 * 65 + (2 * 64 if bits else 0)
    o = (o + 7) & ~7
    o += 2 * ((E + 3) & ~3)
    if bits:
        o += 2 * ((R + 3) & ~3) + 2 * ((R + 4) & ~3)
    o = (o + 15) & ~15
    stride = enum_bits_stride(R, S) if bits else 8 * ((R + 63) // 64 + 1) + 8 * 32 + 4 * (ENUM_TQ + 2)
    return o + ENUM_WAVES * stride


def enum_state_words(R):
    return (R + 63) // 64 + 3


def resolve_tlcap(S):
    return 4096 if S >= 12 else 64 if S < 6 else 1 << S


def resolve_layout(R, E, S):
    """ResolveLayout.total"""
    nk = (R + 63) // 64
    o = 512 + 2 * (R + 2)
    o = (o + 15) & ~15
    o += 2 * ((E + 7) & ~7)
    o = (o + 15) & ~15
    o += 8 * ((E + 8) & ~7)
    o += 8 * (nk + 1) * 2
    o += 8 * nk * (S or 1)
    o += 4 * (R + 1)
    o = (o + 7) & ~7
    o += ENUM_TCAP * 16 + 96 * 10 + 16 + 2 * resolve_tlcap(S)
    return (o + 15) & ~15


def enum_chunk(E):
    return (E + 63) // 64 if E else 1


def lane_rows(row_ptr):
    """k4_stage's row partition of k4_enum_reg: lane l owns the rows whose first entry lies in [l c, (l + 1) c), c = enum_chunk(E).
    Returns the lane of every row (row_ptr: the phase matrix's, R + 1 values)."""
    row_ptr = np.asarray(row_ptr, np.int64)
    return row_ptr[:-1] // enum_chunk(int(row_ptr[-1]))


def max_rows(row_ptr):
    return int(np.bincount(lane_rows(row_ptr)).max()) if len(row_ptr) > 1 else 0


def predicted_class(R, E, S, max_rows=0):
    """the class rule of PhaseHost (k4_phase.hip, `kernel classes`): "bits", "stream" or "big".  max_rows: the largest number of rows a lane
    of lane_rows owns (uniform rows of 3 entries stay far below 64; max_rows_65 is the case that passes it)."""
    bits = S <= 31 and enum_layout(R, E, True, min(S, 32)) <= ENUM_LDS_MAX
    total = enum_layout(R, E, True, min(S, 32)) if bits else enum_layout(R, E)
    cls = "big"
    if R < 65536 and E < 65536 and S <= 31 and total <= ENUM_LDS_MAX and resolve_layout(R, E, S) <= ENUM_LDS_MAX and max_rows <= 64:
        cls = "bits" if bits else "stream"
    if cls != "big" and (1 << min(S, 62)) * enum_state_words(R) > 1 << 27:
        cls = "big"
    return cls


def class_edges(S, per_row):
    """the largest R of uniform rows of per_row entries in the bit-state class and in the streaming class"""
    edge, R, cur = {}, 1, "bits"
    while cur != "big":
        nxt = predicted_class(R + 1, (R + 1) * per_row, S)
        if nxt != cur:
            edge[cur] = R
            if cur == "bits" and nxt == "big":
                edge["stream"] = R
            cur = nxt
        R += 1
    return edge["bits"], edge["stream"]


# ---- the fixed-point table of the phase stage (oracle/lcr_oracle.cpp: PhaseLut; include/lcr.h) --------------------------------------

def _llround(x):
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


FX_SCALE = 1099511627776.0
FX_E = [_llround(math.log10(math.pow(10.0, -float(q or 1) / 10.0)) * FX_SCALE) for q in range(31)]
FX_1E = [_llround(math.log10(1.0 - math.pow(10.0, -float(q or 1) / 10.0)) * FX_SCALE) for q in range(31)]
FX_HOMREF = _llround(math.log10(1 - 1.5 * 0.001) * FX_SCALE)
FX_HOMVAR = _llround(math.log10(0.5 * 0.001) * FX_SCALE)
FX_HET0 = _llround(math.log10(0.001) * FX_SCALE)
FX_LOG2 = _llround(math.log10(2.0) * FX_SCALE)

# ---- reads ---------------------------------------------------------------------------------------------------------------------------
START0 = 5000
SITE_GAP, MARGIN = 50, 45
ALT_OF = {"A": "C", "C": "A", "G": "T", "T": "G"}


def row(alt, lo=0, qual=30):
    """a read over the sites lo .. lo + len(alt) - 1: alt[j] truthy = the alt allele at site lo + j; qual: one value or one per covered site"""
    return dict(lo=lo, alt=list(alt), qual=qual)


def region_reads(n_sites, rows, seed, region=0, start0=START0):
    """(reads, (start0, reference)) of one region: sites at MARGIN + SITE_GAP k; reads sorted by position, reads of one position in list order"""
    rng = np.random.default_rng(seed)
    length = 2 * MARGIN + SITE_GAP * (n_sites - 1) + 1
    ref = "".join(rng.choice(list("ACGT"), size=length))
    at = [MARGIN + SITE_GAP * k for k in range(n_sites)]
    reads = []
    for k, r in enumerate(rows):
        lo, n = r["lo"], len(r["alt"])
        a, b = at[lo] - MARGIN, at[lo + n - 1] + MARGIN + 1
        s, q = list(ref[a:b]), [30] * (b - a)
        qs = r["qual"] if isinstance(r["qual"], (list, tuple)) else [r["qual"]] * n
        for j in range(n):
            x = at[lo + j]
            if r["alt"][j]:
                s[x - a] = ALT_OF[ref[x]]
            q[x - a] = qs[j]
        rev = k // 2 % 2
        reads.append(dict(pos=start0 + a, seq="".join(s), qual=q, cigar="%dM" % (b - a), rev=rev, ts=1 + rev, region=region))
    reads.sort(key=lambda r: r["pos"])
    return reads, (start0, ref)


def build(n_sites, rows, seed):
    reads, reg = region_reads(n_sites, rows, seed)
    return helpers.mk_batch(reads, [reg])


def clean(n, S, qual=30, hom=()):
    """n error-free rows over all S sites, alternating haplotype A (alt at every het site) and B; hom: sites with the alt in every read"""
    return [row([k % 2 == 0 or j in hom for j in range(S)], qual=qual) for k in range(n)]


# ---- the builders --------------------------------------------------------------------------------------------------------------------
DISTINCT_Q = (30, 27, 28, 26)     # no signed sum of the four w[q] is zero (the census shows it: max_tied_rows)
TIED_Q = 26                       # two matches and two mismatches at this quality: the f64 scores of the two signs DIFFER for each of the six
#                                   patterns (at q = 30 they are one double, and a tied row would never flip: whoever dropped a tied row
#                                   would drop a row that stays as it is)


def tq(n_tied, n_clean, n_hom=0):
    """n_clean clean rows over four het sites with a different quality at every site, then n_tied recombinant rows of quality TIED_Q: the alt on
    two of the four het sites, the six choices of two in turn -- no delta fits more than a third of them, and a site that went hom would
    cost the clean rows more than it saves the recombinant ones even if all of those mismatched there (n_clean > 1.6 n_tied + 3 at these
    qualities, the het prior of 3 + 0.3 per entry included), so the clean rows' delta wins and every recombinant row ties under it.  n_hom: further sites behind the four, under the recombinant rows only, alt in every read (eta = -1):
    the ties are ties of the het entries."""
    pairs = [(0, 1), (2, 3), (0, 2), (1, 3), (0, 3), (1, 2)]
    rows = clean(n_clean, 4, qual=list(DISTINCT_Q))
    rows += [row([j in pairs[k % 6] for j in range(4)] + [1] * n_hom, qual=TIED_Q) for k in range(n_tied)]
    return build(4 + n_hom, rows, seed=5)


def tcap(S, n_clean, n_rec, rec_sites):
    """n_clean clean rows over S sites and n_rec recombinant rows over the first rec_sites (even) sites, all of quality 30: the alt on the
    first half of their sites (even rows) or on the second half (odd rows).  The recombinant rows tie under the winning delta, their sigma is
    what the f64 scores or the start draw make of it: restarts of one objective and many term sequences."""
    h = rec_sites // 2
    rows = clean(n_clean, S)
    rows += [row([(j < h) == (k % 2 == 0) for j in range(rec_sites)]) for k in range(n_rec)]
    return build(S, rows, seed=5)


REDO_Q = (30, 29, 28, 27, 26, 25, 24, 23, 22, 21)


def redo_region():
    """40 clean rows over ten sites with a different quality at every site (they never tie) and 24 rows of quality 30 with the alt on five
    of the ten sites, twelve patterns: after the first sigma step the clean rows agree with the start delta's majority, the first delta
    step reaches the winning delta, and the second sigma step finds no row to flip but the equal-quality rows, which tie NOW and are
    decided by their f64 scores for the first time -- a step whose only changes are tie changes, in nearly every restart."""
    rng = np.random.default_rng(31)
    rows = clean(40, 10, qual=list(REDO_Q))
    for k in range(24):
        if k % 2 == 0:
            on = set(rng.choice(10, size=5, replace=False).tolist())
        rows.append(row([(j in on) == (k % 2 == 0) for j in range(10)]))
    return build(10, rows, seed=31)


def class_rows(R):
    """R uniform rows of three entries: two clean haplotypes and one recombinant row of 2 + 1 in twenty"""
    return [row([1, 1, 0] if k % 40 == 19 else [0, 0, 1] if k % 40 == 39 else [k % 2 == 0] * 3) for k in range(R)]


def class_region(R):
    return build(3, class_rows(R), seed=7)


def class_mixed(sizes):
    reads, regs = [], []
    for g, R in enumerate(sizes):
        rd, reg = region_reads(3, class_rows(R), 7 + g, region=g, start0=START0 + 10000 * g)
        reads += rd
        regs.append(reg)
    return helpers.mk_batch(reads, regs)


def max_rows_65():
    """70 rows of one entry (site 0 only) in front of 513 clean rows over eight sites: E = 4 174, a lane owns 66 entries -- lane 0 owns 66
    rows.  (k4_enum_reg's image of 583 rows and 4 174 entries is 63 926 bytes of the 64 512: with rows of five entries it no longer fits.)"""
    return build(8, [row([k % 2 == 0]) for k in range(70)] + clean(513, 8), seed=3)


def rows_case(R):
    """R rows over three sites.  rows_65: row 3 has two entries, which puts the first entries of rows 63 and 64 into one lane's four"""
    rows = clean(R, 3)
    if R == 65:
        rows[3] = row([0, 0])
    return build(3, rows, seed=11)


def entries_case(n3, n2):
    """n3 rows of three entries, then n2 rows over the first two sites"""
    return build(3, clean(n3, 3) + [row([k % 2 == 0] * 2) for k in range(n2)], seed=12)


SINGLE_Q = (1, 2, 3, 4, 5, 29, 30, 31, 60, 93)


def single_entry_rows():
    """24 clean rows over four sites; per site 40 rows of that one entry, haplotypes alternating, the qualities of SINGLE_Q in turn"""
    rows = clean(24, 4)
    for j in range(4):
        rows += [row([k % 2 == 0], lo=j, qual=SINGLE_Q[(k // 2 + j) % len(SINGLE_Q)]) for k in range(40)]
    return build(4, rows, seed=13)


def tile(S):
    return build(S, clean(24, S), seed=20 + S)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
# census: key -> value it must equal, or (">=", bound).  Keys: Census.report().  cls: the predicted class, per region.

BITS_LAST, STREAM_LAST = class_edges(3, 3)
MIXED_SIZES = (200, BITS_LAST + 20, STREAM_LAST + 10, 40)


def case(name, builder, S, cls, census, seed=5, **over):
    return dict(name=name, builder=builder, S=S, cls=cls if isinstance(cls, tuple) else (cls,), census=census, over=dict(over, seed=seed))


CASES = [
    case("tq_126", functools.partial(tq, 126, 240), 4, "bits", dict(tied_rows_final=126, max_tied_rows=126, overflow_flips=0)),
    case("tq_127", functools.partial(tq, 127, 240), 4, "bits", dict(tied_rows_final=127, max_tied_rows=127, overflow_flips=(">=", 1))),
    case("tq_300", functools.partial(tq, 300, 520), 4, "bits", dict(tied_rows_final=300, max_tied_rows=300, winner_overflow_flips=(">=", 1))),
    case("tq_300_hom", functools.partial(tq, 300, 520, n_hom=2), 6, "stream", dict(tied_rows_final=300, max_tied_rows=300, hom_sites=2, winner_overflow_flips=(">=", 1))),
    case("tcap_1024", functools.partial(tcap, 10, 200, 140, 10), 10, "stream", dict(maxima=(">=", 257), term_sequences=(">=", 2))),
    case("tcap_512", functools.partial(tcap, 9, 160, 130, 8), 9, "bits", dict(maxima=(">=", 257), term_sequences=(">=", 2))),
    case("redo_over_grid", redo_region, 10, "bits", dict(redo_restarts=(">=", REDO_GRID + 1), class2_ties=0)),
    case("class_bits_last", functools.partial(class_region, BITS_LAST), 3, "bits", dict()),
    case("class_stream_first", functools.partial(class_region, BITS_LAST + 1), 3, "stream", dict()),
    case("class_stream_last", functools.partial(class_region, STREAM_LAST), 3, "stream", dict()),
    case("class_big_first", functools.partial(class_region, STREAM_LAST + 1), 3, "big", dict()),
    case("class_mixed", functools.partial(class_mixed, MIXED_SIZES), 3, ("bits", "stream", "big", "bits"), dict()),
    case("max_rows_65", max_rows_65, 8, "big", dict(max_rows=(">=", 65))),
    case("rows_63", functools.partial(rows_case, 63), 3, "bits", dict(first_step_flips=[(62,)]), seed=9),
    case("rows_64", functools.partial(rows_case, 64), 3, "bits", dict(first_step_flips=[(63,)]), seed=9),
    case("rows_65", functools.partial(rows_case, 65), 3, "bits", dict(first_step_flips=[(63, 64)], one_lane=(63, 64)), seed=9),
    case("rows_128", functools.partial(rows_case, 128), 3, "bits", dict(first_step_flips=[(63, 64), (127,)]), seed=9),
    case("rows_129", functools.partial(rows_case, 129), 3, "bits", dict(first_step_flips=[(63, 64), (127, 128)], one_lane=(127, 128)), seed=9),
    case("entries_60", functools.partial(entries_case, 20, 0), 3, "bits", dict(E=60)),
    case("entries_64", functools.partial(entries_case, 20, 2), 3, "bits", dict(E=64)),
    case("entries_65", functools.partial(entries_case, 21, 1), 3, "bits", dict(E=65)),
    case("single_entry_rows", single_entry_rows, 4, "bits", dict(one_entry_rows=160, q_le_3=(">=", 1), q_30=(">=", 1)), min_baseq=0),
] + [case("tile_s%d" % S, functools.partial(tile, S), S, "bits", dict()) for S in (5, 6, 7, 8, 9)]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def batch(name):
    return BY_NAME[name]["builder"]()


def params(name, **more):
    return _abi.make_params("hifi-masseq", **dict(BY_NAME[name]["over"], **more))


def shape(name):
    """per region (R, E, S, max_rows) of the phase matrix as the recipe implies it: every read is a phasing row (min_linkers = 1) with an
    entry at each site of its range, every site is a phase site.  test_enum_cases.py holds it against the oracle's fragment matrix."""
    b, out = batch(name), []
    for g in range(b.n_regions):
        n = (b.seq_len[int(b.read_begin[g]):int(b.read_begin[g + 1])].astype(np.int64) - 2 * MARGIN - 1) // SITE_GAP + 1
        rp = np.concatenate([[0], np.cumsum(n)])
        out.append((len(n), int(rp[-1]), (int(b.len[g]) - 2 * MARGIN - 1) // SITE_GAP + 1, max_rows(rp)))
    return out


def classes(name, force_stream=False):
    """the class of every region; force_stream: with the bit-state class closed (lcr_debug_set("enum_force_stream"))"""
    out = []
    for R, E, S, mr in shape(name):
        cls = predicted_class(R, E, S, mr)
        if force_stream and cls == "bits":
            cls = "stream" if enum_layout(R, E) <= ENUM_LDS_MAX and mr <= 64 else "big"
        out.append(cls)
    return out


def phase_matrix(fm, cands):
    """(R, E, row_ptr) of the phase matrix (k4_stage: the phasing rows restricted to the phase sites) from an oracle region's
    fragmat() and candidate records as of the fragment stage"""
    fp = (cands["flags"] & _abi.F_FOR_PHASING) != 0
    rp = [0]
    for k in np.flatnonzero(fm["row_for_phasing"]):
        rp.append(rp[-1] + int(fp[fm["col"][fm["row_ptr"][k]:fm["row_ptr"][k + 1]]].sum()))
    return len(rp) - 1, rp[-1], np.array(rp, np.int64)


# ---- the census ------------------------------------------------------------------------------------------------------------------------

def _seq_sum(t, axis):
    """running sum in index order along `axis`, as the reference's loops add (no pairwise reduction)"""
    acc = np.zeros(np.delete(t.shape, axis), t.dtype)
    for j in range(t.shape[axis]):
        acc = acc + np.take(t, j, axis)
    return acc


class Census(onp2.SNPFrag):
    """oracle_np_phase.SNPFrag whose enumeration restarts (cross_optimize with the genotype, nothing conserved) run on arrays -- the same f64
    terms added in the same order, so the same decisions: test_enum_cases.py holds its result against the C++ oracle's like that of the
    unchanged class -- and keep, per restart, what the limits are about.  The exact fixed-point sums are taken beside the f64 scores to
    say which decisions TIE (they decide nothing here)."""

    def __init__(self, *a):
        super().__init__(*a)
        self.restarts = []
        self._m = None

    def _matrix(self):
        if self._m is None:
            rows = [k for k, f in enumerate(self.fragments) if f.for_phasing]
            ents = [[fe for fe in self.fragments[k].list if fe.phase_site] for k in rows]
            R, L = len(rows), max(len(e) for e in ents)
            m = dict(rows=rows, n=np.array([len(e) for e in ents]), valid=np.zeros((R, L), bool), col=np.zeros((R, L), np.int64),
                     p=np.zeros((R, L), np.int64), lm=np.zeros((R, L)), le=np.zeros((R, L)), fm=np.zeros((R, L), np.int64),
                     fe=np.zeros((R, L), np.int64), q=np.zeros((R, L), np.int64))
            for r, es in enumerate(ents):
                for j, e in enumerate(es):
                    m["valid"][r, j], m["col"][r, j], m["p"][r, j], m["q"][r, j] = True, e.snp_idx, e.p, e.baseq
                    m["lm"][r, j], m["le"][r, j] = math.log10(1.0 - e.prob), math.log10(e.prob)
                    m["fm"][r, j], m["fe"][r, j] = FX_1E[e.baseq], FX_E[e.baseq]
            m["cols"] = [np.argwhere(m["valid"] & (m["col"] == i)) for i in range(len(self.candidate_snps))]   # (row order)
            self._m = m
        return self._m

    def cross_optimize(self, conserved, keep_conserved, with_genotype):   # noqa: C901
        if keep_conserved or not with_genotype:
            return super().cross_optimize(conserved, keep_conserved, with_genotype)
        self.n_cross += 1
        m, snps = self._matrix(), self.candidate_snps
        valid, col, p = m["valid"], m["col"], m["p"]
        delta = np.array([s.haplotype for s in snps])
        eta = np.array([s.genotype for s in snps])
        sigma = np.array([self.fragments[k].haplotag for k in m["rows"]])
        assert np.all(sigma != 0) and all(s.for_phasing for s in snps)
        rec = dict(start=delta.copy(), tied=[], class2=0, class4=0, sigma_ties=0, first_flips=None, overflow_flips=0)
        hg_inc = h_inc = True
        iters = 0
        while hg_inc or h_inc:
            # ---- sigma step
            xp = np.where(eta == 0, delta, eta)[col]
            xm = np.where(eta == 0, -delta, eta)[col]
            lp = _seq_sum(np.where(valid, np.where(p == xp, m["lm"], m["le"]), 0.0), 1)
            ln = _seq_sum(np.where(valid, np.where(p == xm, m["lm"], m["le"]), 0.0), 1)
            den = lp + ln
            q = 1.0 - np.where(sigma == 1, lp, ln) / den
            qn = 1.0 - np.where(sigma == 1, ln, lp) / den
            flip = q < qn
            ap = np.where(valid, np.where(p == xp, m["fm"], m["fe"]), 0).sum(1)
            an = np.where(valid, np.where(p == xm, m["fm"], m["fe"]), 0).sum(1)
            d_fx = np.where(sigma == 1, ap - an, an - ap)
            tie = d_fx == 0
            rec["sigma_ties"] += int(tie.sum())
            queued = tie & (m["n"] > 2)
            rec["tied"].append(np.flatnonzero(queued))
            rec["overflow_flips"] += int((queued & flip & (np.cumsum(queued) > ENUM_TQ)).sum())     # (k4_enum_reg queues in row order)
            if not np.any(d_fx < 0) and np.any(tie & flip):
                rec["class4"] += 1
            if rec["first_flips"] is None:
                rec["first_flips"] = np.flatnonzero(flip)
            logp, pre = _seq_sum(np.where(flip, qn, q), 0), _seq_sum(q, 0)
            sigma = np.where(flip, -sigma, sigma)
            if logp > pre:
                h_inc = hg_inc = True
            else:
                h_inc = False
            # ---- delta / eta step
            logp = pre = 0.0
            strict = tie_change = False
            new = []
            for i in range(len(snps)):
                at = m["cols"][i]
                if not len(at):
                    continue
                r_, c_ = at[:, 0], at[:, 1]
                sg, pp, lm, le, fm, fe = sigma[r_], p[r_, c_], m["lm"][r_, c_], m["le"][r_, c_], m["fm"][r_, c_], m["fe"][r_, c_]
                match = [pp == sg * delta[i], pp == -sg * delta[i], pp == 1, pp == -1]
                Sd, Sn, Shr, Shv = (float(np.cumsum(np.where(k, lm, le))[-1]) for k in match)
                N = [int(np.where(k, fm, fe).sum()) for k in match]
                n = len(r_)
                het = math.log10(0.001) - n * math.log10(2.0)
                hr, hv = math.log10(1 - 1.5 * 0.001), math.log10(0.5 * 0.001)
                den_d = (Shv + hv) + (Sd + het) + (Shr + hr) + (Sn + het)
                den_n = (Shv + hv) + (Sn + het) + (Shr + hr) + (Sd + het)
                qs = [1.0 - (Sd + het) / den_d, 1.0 - (Sn + het) / den_n, 1.0 - (Shr + hr) / den_d, 1.0 - (Shv + hv) / den_d]
                N = [N[0] + FX_HET0 - n * FX_LOG2, N[1] + FX_HET0 - n * FX_LOG2, N[2] + FX_HOMREF, N[3] + FX_HOMVAR]
                mx = max(qs[0], max(qs[1], max(qs[2], qs[3])))
                ch = 0 if qs[0] == mx else 1 if qs[1] == mx else 2 if qs[2] == mx else 3
                cur = {0: 0, 1: 2, -1: 3}[int(eta[i])]
                rec["class2"] += sum(1 for t in range(4) if N[t] == max(N)) > 1
                if N[ch] > N[cur]:
                    strict = True
                elif ch != cur:
                    tie_change = True
                logp += qs[ch]
                pre += qs[cur]
                new.append((i, [(delta[i], 0), (-delta[i], 0), (delta[i], 1), (delta[i], -1)][ch]))
            if not strict and tie_change:
                rec["class4"] += 1
            for i, (h, g) in new:
                delta[i], eta[i] = h, g
            if logp > pre:
                hg_inc = h_inc = True
            else:
                hg_inc = False
            iters += 1
            if iters > 20:
                break
        for s, h, g in zip(snps, delta.tolist(), eta.tolist()):
            s.haplotype, s.genotype = h, g
        for k, h in zip(m["rows"], sigma.tolist()):
            self.fragments[k].haplotag = h
        match = (p == np.where(eta[col] == 0, sigma[:, None] * delta[col], eta[col]))[valid]      # (row-major: the reference's entry order)
        prob = float(np.cumsum(np.where(match, m["lm"][valid], m["le"][valid]))[-1])
        rec.update(prob=prob, obj_fx=int(np.where(match, m["fm"][valid], m["fe"][valid]).sum()), terms=np.packbits(match).tobytes(),
                   iters=iters, delta=delta.copy(), eta=eta.copy())
        self.restarts.append(rec)
        return prob

    def report(self):
        rs, m = self.restarts, self._matrix()
        win, best = 0, float("-inf")
        for k, r in enumerate(rs):                      # `prob > largest_prob`, phase.rs:1117
            if r["prob"] > best:
                win, best = k, r["prob"]
        top = max(r["obj_fx"] for r in rs)
        maxima = [r for r in rs if r["obj_fx"] == top]
        compares, largest = 0, None                     # restarts that meet the running maximum with an equal objective
        for r in rs:
            if largest is not None and r["obj_fx"] == largest:
                compares += 1
            if largest is None or r["obj_fx"] > largest:
                largest = r["obj_fx"]
        flips = [set(r["first_flips"].tolist()) for r in rs]
        w = rs[win]
        # the rows of more than two entries whose weights cancel under the winner's delta / eta, from the matrix alone
        x = np.where(w["eta"] == 0, w["delta"], 0)[m["col"]]
        signed = np.where(m["valid"] & (x != 0), np.where(m["p"] == x, 1, -1) * (m["fm"] - m["fe"]), 0).sum(1)
        return dict(n_restarts=len(rs), winner=win, R=len(m["rows"]), E=int(m["valid"].sum()),
                    sigma_ties=sum(r["sigma_ties"] for r in rs), class2_ties=sum(r["class2"] for r in rs),
                    class4_steps=sum(r["class4"] for r in rs), equal_objective_compares=compares,
                    max_tied_rows=max(len(t) for r in rs for t in r["tied"]),
                    tied_rows_final=int(((signed == 0) & (m["n"] > 2)).sum()),
                    winner_last_step_tied=w["tied"][-1].tolist(),
                    zero_weight_rows=np.flatnonzero((signed == 0) & (m["n"] > 2)).tolist(),
                    maxima=len(maxima), term_sequences=len({r["terms"] for r in maxima}),
                    redo_restarts=sum(1 for r in rs if r["class2"] or r["class4"]),
                    overflow_flips=sum(r["overflow_flips"] for r in rs), winner_overflow_flips=w["overflow_flips"],
                    first_step_flips=flips,
                    hom_sites=int((w["eta"] != 0).sum()), one_entry_rows=int((m["n"] == 1).sum()),
                    q_le_3=int((m["valid"] & (m["q"] <= 3)).sum()), q_30=int((m["valid"] & (m["q"] == 30)).sum()),
                    max_iters=max(r["iters"] for r in rs))


def census_holds(want, got):
    """the entries of `want` that `got` does not meet (empty: the census holds).  first_step_flips: groups of rows; the rows of a group must
    all change sigma in the first sigma step of ONE restart."""
    bad = {}
    for k, v in want.items():
        if k in ("one_lane", "max_rows"):
            continue                         # (properties of the matrix, checked by the test from lane_rows)
        if isinstance(v, tuple) and v and v[0] == ">=":
            ok = got[k] >= v[1]
        elif k == "first_step_flips":
            ok = all(any(set(grp) <= f for f in got[k]) for grp in v)
        else:
            ok = got[k] == v
        if not ok:
            bad[k] = (v, "(per restart)" if k == "first_step_flips" else got[k])
    return bad

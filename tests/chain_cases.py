"""Recipes for the chain branch of the phase stage (regions with S > max_enum_snps: csrc/k4_grid.hip, csrc/k4_grid_batch.h, the workgroup
cross_optimize of csrc/k4_dev.h, host control PhaseHost::launch_chain in csrc/k4_phase.hip): plain data and builders, no tests.

A case is one small batch, its parameters and what it was built to stand at: the form launch_chain gives each of its regions
(predicted_form, a restatement of the selection rules) and a census -- what the CPU restatement of the chain (ChainCensus below) must have met
for the case to count as a visit of its limit.  tests/test_chain_cases.py runs the two CPU oracles against each other and checks every
census; tests/test_chain_cases_gpu.py puts the same cases in front of k4_chain_wg and k4_chain_grid in every form they have.

The limits, copied below the way tests/enum_cases.py copies its own:
  CROSS_MACC = 2048     SNPs with a per-column accumulator in LDS: beyond it the workgroup cross_optimize takes its plain form
  RACC_CAP = 4160       rows with an accumulator in the stage rows (NW * 4 * SSTR words): beyond it cols_balanced only
  SCN = 256             SNPs whose four constants k4_chain_wg keeps in LDS
  STAGE_BYTES = 33280   the stage rows as ld_pair_table's scratch: 8 S W + 4 n_ent + 16 bytes must fit for the LDS form of the table
  WG_LDS = 64 KB        dynamic LDS of k4_chain_wg: the state (R + 2 S rounded up to 64, of the launch's LARGEST region) lives there up to
                        3/4 of it, a region's matrix behind it while state + matview_bytes + 64 fit
  grid_min              stat.E >= grid_min: all CUs (2^17 unless "grid_min_entries" is set)
  64                    the window of ld_components_wave (cur - 64), ld_seed_wave (base += 64), block_flip's nodes, col_sums4's entries
                        and the prefetch of objective_f64_greater_wg (base + 64 + lane < E)
  TIE_CAP = 256         tied (row, state) pairs a workgroup of the batched all-CU rounds queues per sigma step; beyond it: decided in place

Reads are those of tests/enum_cases.py (SITE_GAP, MARGIN, ALT_OF; a read covers exactly the sites of its range); a row's alt value 2 is a
SECOND non-reference base (ALT2_OF), which gives a site both of whose major alleles are non-reference.

Limits that cannot be met as the constants stand, and why:
  * k4_grid_fast_lds / k4_grid_batch_lds beyond 96 KB: 8 ceil(R / 64) + 3 S + 64 and 12 (S + 2) + 24 KB pass 96 KB from S > 6 000 sites or
    R > 780 000 rows on -- a batch of tens of megabases, minutes of oracle time;
  * n_rounds > BATCH_ROUNDS: S > 16 * 8 * (workgroups of the launch) = 32 768 sites on a 256-CU device, and a number that changes with the
    device;
  * the n_ent >= 65536 and S >= 32768 guards of the LDS pair table: the byte rule 8 S W + 4 n_ent + 16 <= 33 280 closes the LDS form at
    n_ent <= 8 314 and S <= 4 158 (W >= 1) long before either guard;
  * tie8's `copy` bound (2 S <= 33 280 bytes): S > 16 640 sites in a region of workgroup scope.
"""
import functools

import numpy as np

import enum_cases as ec
import helpers
from longcallr_amd import _abi
from oracle import oracle_np_phase as onp2

# ---- the constants of csrc/k4_dev.h, csrc/k4_grid.hip, csrc/k4_grid_batch.h, csrc/k4_phase.hip -----------------------------------------
CROSS_MACC = 2048
NW, SSTR = 16, 65
RACC_CAP = NW * 4 * SSTR
STAGE_BYTES = 8 * RACC_CAP
SCN = 256
WG_LDS = 64 * 1024
GRID_MIN = 1 << 17
TIE_CAP = 256
WINDOW = 64


def matview_bytes(R, S, E):
    return 4 * (R + 1) + 4 * (S + 1) + 8 * E + 2 * ((E + 3) & ~3) + 2 * ((S + 3) & ~3)


def state_stride(max_state):
    return (max_state + 63) & ~63


def pair_table_bytes(S, W, n_ent):
    return 8 * S * max(1, min(W, S)) + 4 * n_ent + 16


def predicted_form(R, S, E, n_ent, W, batch_max_state, grid_min=GRID_MIN):
    """the form PhaseHost::launch_chain and k4_chain_wg give a chain region of R phasing rows, S sites, E phase entries, n_ent entries of
    all its fragment rows and band width W, in a launch whose largest workgroup-scope region has R + 2 S = batch_max_state"""
    if E >= grid_min:
        return dict(scope="all-CU", state="global", matrix="global", cross="grid", scn="global", pair_table="global")
    stride = state_stride(batch_max_state)
    lds_state = stride <= WG_LDS * 3 // 4
    lds_mat = lds_state and stride + matview_bytes(R, S, E) + 64 <= WG_LDS
    cross = "plain" if S > CROSS_MACC else "rows_balanced" if R <= RACC_CAP else "cols_balanced"
    tbl = S < 32768 and n_ent < 65536 and pair_table_bytes(S, W, n_ent) <= STAGE_BYTES
    return dict(scope="workgroup", state="LDS" if lds_state else "global", matrix="LDS" if lds_mat else "global", cross=cross,
                scn="LDS" if S <= SCN else "global", pair_table="LDS" if tbl else "global")


def form_line(g, f):
    """the line PhaseHost::report_prof prints for region g in form f (LCR_PHASE_PROF=1)"""
    return "chain region %d: scope %s, state %s, matrix %s, cross_optimize %s, constants %s, pair table %s" % (
        g, f["scope"], f["state"], f["matrix"], f["cross"], f["scn"], f["pair_table"])


# ---- reads ---------------------------------------------------------------------------------------------------------------------------------
row, clean = ec.row, ec.clean
SITE_GAP, MARGIN = ec.SITE_GAP, ec.MARGIN
ALT2_OF = {"A": "T", "C": "G", "G": "C", "T": "A"}     # (never A>G / T>C either)


def region_reads(n_sites, rows, seed, region=0, start0=ec.START0):
    """enum_cases.region_reads with alt value 2 = the site's second non-reference base"""
    rng = np.random.default_rng(seed)
    length = 2 * MARGIN + SITE_GAP * (n_sites - 1) + 1
    ref = "".join(rng.choice(list("ACGT"), size=length))
    reads = []
    for k, r in enumerate(rows):
        lo, n = r["lo"], len(r["alt"])
        a, b = SITE_GAP * lo, SITE_GAP * (lo + n - 1) + 2 * MARGIN + 1
        s, q = list(ref[a:b]), [30] * (b - a)
        qs = r["qual"] if isinstance(r["qual"], (list, tuple)) else [r["qual"]] * n
        for j in range(n):
            x = MARGIN + SITE_GAP * (lo + j)
            if r["alt"][j]:
                s[x - a] = (ALT2_OF if r["alt"][j] == 2 else ec.ALT_OF)[ref[x]]
            q[x - a] = qs[j]
        rev = r.get("rev", k // 2 % 2)
        reads.append(dict(pos=start0 + a, seq="".join(s), qual=q, cigar="%dM" % (b - a), rev=rev, ts=1 + rev, region=region))
    reads.sort(key=lambda r: r["pos"])
    return reads, (start0, ref)


def build(*regions):
    """regions: (n_sites, rows, seed) each; region g starts at START0 + 1 000 000 g"""
    reads, regs = [], []
    for g, (n_sites, rows, seed) in enumerate(regions):
        rd, reg = region_reads(n_sites, rows, seed, region=g, start0=ec.START0 + 1000000 * g)
        reads += rd
        regs.append(reg)
    return helpers.mk_batch(reads, regs)


def span_rows(S, R, width=2, step=1):
    """R error-free rows of `width` neighbouring sites, dealt in turn to the windows lo = 0, step, 2 step, ... (the last one ends at site
    S - 1), haplotype A (alt everywhere) and B alternating inside every window"""
    los = list(range(0, S - width, step)) + [S - width]
    out = []
    for k in range(R):
        w, n = k % len(los), k // len(los)
        out.append(dict(row([n % 2 == 0] * width, lo=los[w]), rev=n // 2 % 2))      # (both strands under both alleles of every window)
    return out


# ---- the recipes ---------------------------------------------------------------------------------------------------------------------------
SMALL = (12, clean(24, 12), 41)        # a small chain region: one block of twelve sites, everything in LDS


def complete(S):
    """24 clean rows over all S sites: a complete LD graph (degree S - 1, one block of S nodes, the DFS S - 1 deep); S W alone is
    beyond the pair table's scratch"""
    return build((S, clean(24, S), 100 + S))


def path(S, per_pair=12, wide=0):
    """rows of two neighbouring sites: the path graph 0 - 1 - ... - S - 1, W = 1; wide: ONE more row over the first `wide` sites, which
    alone sets the band (W = wide - 1)"""
    rows = span_rows(S, per_pair * (S - 1))
    if wide:
        rows.append(row([1] * wide))
    return build((S, rows, 200 + S))


def columns(n):
    """n clean rows over twelve sites: every column of the block has n phase entries"""
    return build((12, clean(n, 12), 300 + n))


BLOCK_SITES = dict(X=(0, 1, 2), A=(3, 4, 5, 6, 7), N1=8, B=(9, 10), C=(11, 12, 13, 14, 15, 16), two_alt=17, hom=18, D=(19, 20, 21))


def blocks(seed):
    """Twenty-two sites and four blocks.  A = sites 3-7 (cis), B = 9-10 (two nodes), C = 11-16 (the alt on haplotype A at the odd, on
    haplotype B at the even sites: every pair of neighbours is TRANS, the seed signs negative), D = 19-21.  X = sites 0-2 are coherent but
    for three rows with one allele flipped each, which give every pair of them cis AND trans support: eligible sites without an edge, in
    front of block A.  Site 8 has the alt on every other read of each haplotype (no edge either).  Site 17 has two non-reference major
    alleles and site 18 the alt in every read: inside the band of the rows over 15-21, not eligible.  The rows that join two blocks are half
    cis, half trans (no edge between the blocks); those that join X and A are cis but for two:
      over 3-7      wholly inside block A -- the block the reference visits last, device block 0
      over 0-3      first entries outside every block, then block A.  Their sigma follows X, whose sign against A is the start draws':
                    where it comes out wrong, flipping A (and the rows that begin in it) is what repairs these rows -- block 0 FLIPS
      over 6-10     start in A, the leading in-block run ends in the middle of the row (at site 8)
      over 8-12     first entry outside every block, then B and C
      over 9-10, 11-16, 19-21   start in another block
      over 15-21    C, then 17 and 18, then D"""
    h = lambda k: k % 2 == 0
    cpat = lambda hx, sites: [hx == (j % 2 == 1) for j in sites]
    other = lambda k: h(k) == (k % 4 < 2)                 # the same haplotype in half of the rows of each haplotype, the other one in the rest
    rows = [row([h(k)] * 5, lo=3) for k in range(24)]
    rows += [row([h(k)] * 3, lo=0) for k in range(24)] + [row([0, 1, 1]), row([1, 0, 1]), row([1, 1, 0])]
    rows += [row([h(k)] * 4, lo=0) for k in range(8)] + [row([1, 1, 1, 0]), row([0, 0, 0, 1])]
    rows += [row([h(k)] * 2, lo=9) for k in range(24)]
    rows += [row(cpat(h(k), range(11, 17)), lo=11) for k in range(24)]
    rows += [row([h(k)] * 3, lo=19) for k in range(24)]
    rows += [row([h(k), h(k), k // 4 % 2 == 0, other(k), other(k)], lo=6) for k in range(16)]
    rows += [row([k // 4 % 2 == 0, h(k), h(k)] + cpat(other(k), (11, 12)), lo=8) for k in range(16)]
    rows += [row(cpat(h(k), (15, 16)) + [1 + k % 2, 1] + [other(k)] * 3, lo=15) for k in range(16)]
    return build((22, rows, seed))


def pair_table_edge(more):
    """twelve sites, W = 11 (8 S W = 1 056 bytes): 669 clean rows over all of them and two more rows -- twelve and twelve entries: n_ent =
    8 052, the table's last LDS size; twelve, eleven and two: 8 053"""
    rows = clean(669, 12) + [row([1] * 12), row([0] * 12)]
    if more:
        rows[-1] = row([0] * 11)
        rows.append(row([0, 0], lo=10))
    return build((12, rows, 51))


def rows_edge(R):
    return build((41, span_rows(41, R), 52))


def sites_edge(S):
    return build((S, span_rows(S, 12 * (S - 1)), 53))


def wide_edge(S):
    """rows of eight sites on windows four sites apart, eight rows a window"""
    return build((S, span_rows(S, 8 * len(range(0, S - 8, 4)) + 8, width=8, step=4), 54))


def _edge_R(S, key, hi):
    """the largest R of two-site rows over S sites whose region alone still has form[key] == "LDS" (E = n_ent = 2 R, W = 1)"""
    f = lambda R: predicted_form(R, S, 2 * R, 2 * R, 1, R + 2 * S)[key] == "LDS"
    lo = S
    assert f(lo) and not f(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if f(mid) else (lo, mid)
    return lo


MATRIX_S, STATE_S = 41, 101
MATRIX_LAST = _edge_R(MATRIX_S, "matrix", 10000)        # the matrix's byte edge: stride + matview_bytes + 64 <= 64 KB
STATE_LAST = _edge_R(STATE_S, "state", 100000)          # R + 2 S = 49 152


def matrix_edge(R):
    return build((MATRIX_S, span_rows(MATRIX_S, R), 55))


def state_edge(R):
    return build((STATE_S, span_rows(STATE_S, R), 56))


def mixed_state():
    """the small region beside the region beyond the state edge: one launch, so the small region's state goes to global memory too"""
    return build(SMALL, (STATE_S, span_rows(STATE_S, STATE_LAST + 1), 56))


def mixed_matrix():
    """a region whose matrix is copied into LDS and one whose matrix is not, in one launch"""
    return build(SMALL, (41, span_rows(41, RACC_CAP + 1), 52))


def ties_2_4(n_reads, seed):
    """test_gpu_parity.test_chain_ties_of_classes_2_and_4's recipe -- twelve het sites, three of them with the allele flipped in half the
    reads of each haplotype, equal qualities -- with n_reads rows: from 560 rows on the matrix is no longer copied into LDS"""
    rng = np.random.default_rng(seed)
    flipped = set(rng.choice(12, size=3, replace=False).tolist())
    rows = [row([(k % 2 == 0) != (j in flipped and k // 2 % 2 == 0) for j in range(12)]) for k in range(n_reads)]
    return build((12, rows, seed))


def class8(extra):
    """32 clean rows over twelve sites and 32 rows of TWO entries of quality 30 (sites 5 and 6), the alt on one of them: those tie, and their
    two scores are one double (a + b against b + a), so a row stays on the side the perturbation rounds leave it on -- configurations of one
    objective and other match bits, which the chain compares by their ordered f64 sums.  E = 448 = 7 * 64; extra = 1: a row of one entry
    more (E % 64 = 1); extra = -1: the last row has one entry (E % 64 = 63)"""
    rows = clean(32, 12) + [row([k % 2 == 0, k % 2 == 1], lo=5) for k in range(32)]
    if extra == 1:
        rows.append(row([1], lo=11))
    if extra == -1:
        rows[-1] = row([1], lo=5)
    return build((12, rows, 61))


def tie_queue(n_tied):
    """192 clean rows over twelve sites (three blocks of 64 rows of three groups of four entries), a different quality at each of the first
    four sites, and n_tied rows of enum_cases' tied-row recipe over those four sites (four entries at TIED_Q, the alt on two of them): one
    more block of rows of ONE group.  Under the best delta every one of them ties, in every speculative state whose perturbation left the
    four sites alone: with 64 of them more than TIE_CAP (row, state) pairs in one sigma step of one workgroup."""
    pairs = [(0, 1), (2, 3), (0, 2), (1, 3), (0, 3), (1, 2)]
    rows = clean(192, 12, qual=list(ec.DISTINCT_Q) + [30] * 8)
    rows += [row([j in pairs[k % 6] for j in range(4)], qual=ec.TIED_Q) for k in range(n_tied)]
    return build((12, rows, 62))


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
# shape: per region (R, S, E, n_ent, W) as the recipe implies it (tests/test_chain_cases.py holds it against the oracle's fragment matrix);
# census: key -> value, or (">=", bound); keys: ChainCensus.report().  heavy: only the default all-CU form on the GPU.

def case(name, builder, shape, census, heavy=False, seed=5, **over):
    return dict(name=name, builder=builder, shape=shape if isinstance(shape, list) else [shape], census=census, heavy=heavy,
                over=dict(over, seed=seed))


def _span_shape(S, R, width=2):
    return (R, S, R * width, R * width, width - 1)


_SMALL_SHAPE = (24, 12, 288, 288, 11)
_N_WIDE = lambda S: 8 * len(range(0, S - 8, 4)) + 8

CASES = [
    case("complete_%d" % S, functools.partial(complete, S), (24, S, 24 * S, 24 * S, S - 1),
         dict(max_degree=S - 1, min_degree=S - 1, block_sizes=[S], dfs_depth=S - 1)) for S in (63, 64, 65, 66, 130)
] + [
    case("path_70", functools.partial(path, 70), _span_shape(70, 12 * 69), dict(max_degree=2, block_sizes=[70], dfs_depth=69)),
    case("path_70_wide_row", functools.partial(path, 70, wide=10), (12 * 69 + 1, 70, 24 * 69 + 10, 24 * 69 + 10, 9),
         dict(block_sizes=[70])),
] + [
    case("columns_%d" % n, functools.partial(columns, n), (n, 12, 12 * n, 12 * n, 11), dict(block_sizes=[12], block_column_lengths=[n]))
    for n in (63, 64, 65, 128, 129)
] + [
    case("blocks_flip", functools.partial(blocks, 71), None, dict(block0_flips=True), seed=5),
    case("blocks_stay", functools.partial(blocks, 71), None, dict(block0_flips=False), seed=3),
    case("pair_table_lds_last", functools.partial(pair_table_edge, False), (671, 12, 8052, 8052, 11), dict(block_sizes=[12])),
    case("pair_table_global_first", functools.partial(pair_table_edge, True), (672, 12, 8053, 8053, 11), dict(block_sizes=[12])),
    case("rows_4160", functools.partial(rows_edge, RACC_CAP), _span_shape(41, RACC_CAP), dict(block_sizes=[41]), heavy=True),
    case("rows_4161", functools.partial(rows_edge, RACC_CAP + 1), _span_shape(41, RACC_CAP + 1), dict(block_sizes=[41]), heavy=True),
    case("sites_256", functools.partial(sites_edge, SCN), _span_shape(SCN, 12 * (SCN - 1)), dict(block_sizes=[SCN])),
    case("sites_257", functools.partial(sites_edge, SCN + 1), _span_shape(SCN + 1, 12 * SCN), dict(block_sizes=[SCN + 1])),
    case("sites_2048", functools.partial(wide_edge, CROSS_MACC), _span_shape(CROSS_MACC, _N_WIDE(CROSS_MACC), 8), dict(block_sizes=[CROSS_MACC]), heavy=True),
    case("sites_2049", functools.partial(wide_edge, CROSS_MACC + 1), _span_shape(CROSS_MACC + 1, _N_WIDE(CROSS_MACC + 1), 8), dict(block_sizes=[CROSS_MACC + 1]), heavy=True),
    case("matrix_lds_last", functools.partial(matrix_edge, MATRIX_LAST), _span_shape(MATRIX_S, MATRIX_LAST), dict(block_sizes=[MATRIX_S])),
    case("matrix_global_first", functools.partial(matrix_edge, MATRIX_LAST + 1), _span_shape(MATRIX_S, MATRIX_LAST + 1), dict(block_sizes=[MATRIX_S])),
    case("state_lds_last", functools.partial(state_edge, STATE_LAST), _span_shape(STATE_S, STATE_LAST), dict(block_sizes=[STATE_S]), heavy=True),
    case("state_global_first", functools.partial(state_edge, STATE_LAST + 1), _span_shape(STATE_S, STATE_LAST + 1), dict(block_sizes=[STATE_S]), heavy=True),
    case("mixed_state", mixed_state, [_SMALL_SHAPE, _span_shape(STATE_S, STATE_LAST + 1)], dict(), heavy=True),
    case("mixed_matrix", mixed_matrix, [_SMALL_SHAPE, _span_shape(41, RACC_CAP + 1)], dict(), heavy=True),
    case("ties_2_4_matrix_global", functools.partial(ties_2_4, 600, 16), (600, 12, 7200, 7200, 11), dict(class2_ties=(">=", 1)), seed=16),
    case("class8_e448", functools.partial(class8, 0), (64, 12, 448, 448, 11), dict(f64_sum_compares=(">=", 1))),
    case("class8_e449", functools.partial(class8, 1), (65, 12, 449, 449, 11), dict(f64_sum_compares=(">=", 1))),
    case("class8_e447", functools.partial(class8, -1), (64, 12, 447, 447, 11), dict(f64_sum_compares=(">=", 1))),
    case("tie_queue_64", functools.partial(tie_queue, 64), (256, 12, 2560, 2560, 11), dict(max_tied_rows=(">=", 64))),
    case("tie_queue_24", functools.partial(tie_queue, 24), (216, 12, 2400, 2400, 11), dict(max_tied_rows=24)),
    case("scope", functools.partial(build, SMALL), _SMALL_SHAPE, dict(block_sizes=[12])),
]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]
# the cases whose pure-Python run stops behind the LD blocks (the S >= 2048 pair and the state-edge pair: minutes of oracle_np_phase)
BLOCKS_ONLY = ("sites_2048", "sites_2049", "state_lds_last", "state_global_first")
TIE_CASES = ("ties_2_4_matrix_global", "class8_e448", "class8_e449", "class8_e447")
TIE_QUEUE_CASES = ("tie_queue_64", "tie_queue_24")


@functools.lru_cache(maxsize=4)
def batch(name):
    return BY_NAME[name]["builder"]()


def params(name, **more):
    return _abi.make_params("hifi-masseq", **dict(BY_NAME[name]["over"], **more))


def region_shape(fm, cands):
    """(R, S, E, n_ent, W) of a region from an oracle region's fragmat() and candidate records as of the fragment stage: what k4_stage
    writes into StageStat (W: the largest distance between the first and the last phase site of any fragment row)"""
    fp = (cands["flags"] & _abi.F_FOR_PHASING) != 0
    R = E = W = 0
    for k in range(len(fm["row_ptr"]) - 1):
        c = fm["col"][fm["row_ptr"][k]:fm["row_ptr"][k + 1]]
        c = c[fp[c]]
        if len(c):
            W = max(W, int(c[-1] - c[0]))
        if fm["row_for_phasing"][k]:
            R, E = R + 1, E + len(c)
    return R, len(cands), E, int(fm["row_ptr"][-1]), W


def forms(shapes, grid_min=GRID_MIN):
    """predicted_form of every region of a batch from their region_shape()s"""
    wg = [s[0] + 2 * s[1] for s in shapes if s[2] < grid_min]
    return [predicted_form(*s, batch_max_state=max(wg) if wg else 0, grid_min=grid_min) for s in shapes]


# ---- the census ----------------------------------------------------------------------------------------------------------------------------

class ChainCensus(onp2.SNPFrag):
    """oracle_np_phase.SNPFrag that keeps what a chain region's run met.  Its cross_optimize runs on arrays -- the same f64 terms added in the
    same order, so the same decisions (tests/test_chain_cases.py holds its result against the C++ oracle's) -- and takes the exact
    fixed-point sums beside the f64 scores to say which decisions TIE (they decide nothing here)."""

    def __init__(self, *a):
        super().__init__(*a)
        self.c = dict(sigma_ties=0, class2_ties=0, class4_steps=0, equal_objective_compares=0, f64_sum_compares=0, max_tied_rows=0,
                      cross_calls=0, flipped_blocks=None)
        self._m = None
        self._best = None         # (f64 objective, fixed-point objective, match bits) of the best configuration so far

    # -- LD graph and blocks
    def divide_snps_into_blocks(self, thr):
        graph = super().divide_snps_into_blocks(thr)
        snps = self.candidate_snps
        deg = {n: len(graph.adj[n]) for n in graph.nodes if graph.adj[n]}
        seen, depth = set(), 0
        for r in sorted(deg):                      # ld_components_wave: from the smallest node, the largest unvisited neighbour first
            if r in seen:
                continue
            seen.add(r)
            stack = [r]
            while stack:
                nxt = [y for y in graph.adj[stack[-1]] if y not in seen]
                if nxt:
                    seen.add(max(nxt))
                    stack.append(max(nxt))
                    depth = max(depth, len(stack) - 1)
                else:
                    stack.pop()

        def ok(s):
            one_ref = (s.alleles[0] == s.reference) != (s.alleles[1] == s.reference)
            return one_ref and s.allele_freqs[0] != 0.0 and s.allele_freqs[1] != 0.0
        self.c.update(degrees=deg, max_degree=max(deg.values(), default=0), min_degree=min(deg.values(), default=0), dfs_depth=depth,
                      blocks=[list(b) for b in self.ld_blocks], block_sizes=[len(b) for b in self.ld_blocks],
                      block_order=[min(b) for b in self.ld_blocks],
                      trans_edges=sum(1 for _, _, w in graph.all_edges() if w < 0), cis_edges=sum(1 for _, _, w in graph.all_edges() if w > 0),
                      eligible_without_edge=[i for i, s in enumerate(snps) if s.for_phasing and ok(s) and i not in deg],
                      phasing_not_eligible=[i for i, s in enumerate(snps) if s.for_phasing and not ok(s)],
                      not_phasing=[i for i, s in enumerate(snps) if not s.for_phasing])
        return graph

    # -- block flip
    def cross_optimize_by_block(self):
        snps = self.candidate_snps
        before = [s.haplotype for s in snps]
        last = set(self.ld_blocks[-1]) if self.ld_blocks else set()      # the block whose haplotags survive: device block 0
        of = {i: b for b, blk in enumerate(self.ld_blocks) for i in blk}
        kinds = dict(first_outside=0, ends_mid_row=0, wholly_inside=0, starts_in_another_block=0)
        runs = []
        for f in self.fragments:
            if not f.for_phasing or f.haplotag == 0 or not f.list:
                continue
            idx = [fe.snp_idx for fe in f.list]
            run = 0
            while run < len(idx) and idx[run] in last:
                run += 1
            runs.append(run)
            touches = any(i in last for i in idx)
            if run == len(idx):
                kinds["wholly_inside"] += 1
            elif run > 0:
                kinds["ends_mid_row"] += 1
            elif idx[0] not in of and touches:
                kinds["first_outside"] += 1
            elif idx[0] in of:
                kinds["starts_in_another_block"] += 1
        prob = super().cross_optimize_by_block()
        flipped = [snps[b[0]].haplotype != before[b[0]] for b in self.ld_blocks]
        self.c.update(flipped_blocks=flipped, block0_flips=bool(flipped[-1]) if flipped else None, flip_run_kinds=kinds,
                      flip_runs=runs, block_column_lengths=sorted({len(self.col_view(i)[0]) for i in last}))
        self._attempt(prob)
        return prob

    # -- cross_optimize on arrays
    def _matrix(self):
        if self._m is None:
            import math
            rows = [k for k, f in enumerate(self.fragments) if f.for_phasing and f.haplotag != 0 and any(fe.phase_site for fe in f.list)]
            ents = [[fe for fe in self.fragments[k].list if fe.phase_site] for k in rows]
            R, L = len(rows), max(len(e) for e in ents)
            m = dict(rows=rows, n=np.array([len(e) for e in ents]), valid=np.zeros((R, L), bool), col=np.zeros((R, L), np.int64),
                     p=np.zeros((R, L), np.int64), lm=np.zeros((R, L)), le=np.zeros((R, L)), fm=np.zeros((R, L), np.int64),
                     fe=np.zeros((R, L), np.int64))
            for r, es in enumerate(ents):
                for j, e in enumerate(es):
                    m["valid"][r, j], m["col"][r, j], m["p"][r, j] = True, e.snp_idx, e.p
                    m["lm"][r, j], m["le"][r, j] = math.log10(1.0 - e.prob), math.log10(e.prob)
                    m["fm"][r, j], m["fe"][r, j] = ec.FX_1E[e.baseq], ec.FX_E[e.baseq]
            m["cols"] = [np.argwhere(m["valid"] & (m["col"] == i)) for i in range(len(self.candidate_snps))]     # (row order)
            self._m = m
        return self._m

    def _attempt(self, prob):
        """phase()'s `prob > largest` beside the exact objective and the match bits of the configuration: an equal fixed-point objective is
        what liblcr sees as a tie of class 8, and other match bits send it to the ordered f64 sums"""
        m = self._matrix()
        delta = np.array([s.haplotype for s in self.candidate_snps])
        eta = np.array([s.genotype for s in self.candidate_snps])
        sigma = np.array([self.fragments[k].haplotag for k in m["rows"]])
        valid, col = m["valid"], m["col"]
        match = (m["p"] == np.where(eta[col] == 0, sigma[:, None] * delta[col], eta[col]))[valid]
        fx, bits = int(np.where(match, m["fm"][valid], m["fe"][valid]).sum()), np.packbits(match).tobytes()
        if self._best is not None and fx == self._best[1]:
            self.c["equal_objective_compares"] += 1
            self.c["f64_sum_compares"] += bits != self._best[2]
        if self._best is None or prob > self._best[0]:
            self._best = (prob, fx, bits)

    def cross_optimize(self, conserved, keep_conserved, with_genotype):   # noqa: C901
        import math
        self.n_cross += 1
        self.c["cross_calls"] += 1
        m, snps = self._matrix(), self.candidate_snps
        valid, col, p = m["valid"], m["col"], m["p"]
        delta = np.array([s.haplotype for s in snps])
        eta = np.array([s.genotype for s in snps])
        sigma = np.array([self.fragments[k].haplotag for k in m["rows"]])
        active = [i for i, s in enumerate(snps) if s.for_phasing and not (keep_conserved and i in conserved) and len(m["cols"][i])]
        hr, hv = math.log10(1 - 1.5 * 0.001), math.log10(0.5 * 0.001)
        hg_inc = h_inc = True
        iters = 0
        while hg_inc or h_inc:
            # ---- sigma step
            xp = np.where(eta == 0, delta, eta)[col]
            xm = np.where(eta == 0, -delta, eta)[col]
            lp = ec._seq_sum(np.where(valid, np.where(p == xp, m["lm"], m["le"]), 0.0), 1)
            ln = ec._seq_sum(np.where(valid, np.where(p == xm, m["lm"], m["le"]), 0.0), 1)
            den = lp + ln
            q = 1.0 - np.where(sigma == 1, lp, ln) / den
            qn = 1.0 - np.where(sigma == 1, ln, lp) / den
            flip = q < qn
            ap = np.where(valid, np.where(p == xp, m["fm"], m["fe"]), 0).sum(1)
            an = np.where(valid, np.where(p == xm, m["fm"], m["fe"]), 0).sum(1)
            d_fx = np.where(sigma == 1, ap - an, an - ap)
            tie = d_fx == 0
            self.c["sigma_ties"] += int(tie.sum())
            het_tie = tie & (valid & (eta[col] == 0)).any(1)
            self.c["max_tied_rows"] = max(self.c["max_tied_rows"], int(het_tie.sum()))
            if not np.any(d_fx < 0) and np.any(tie & flip):
                self.c["class4_steps"] += 1
            logp, pre = float(np.cumsum(np.where(flip, qn, q))[-1]), float(np.cumsum(q)[-1])
            sigma = np.where(flip, -sigma, sigma)
            if logp > pre:
                h_inc = hg_inc = True
            else:
                h_inc = False
            # ---- delta / eta step
            logp = pre = 0.0
            strict = tie_change = False
            new = []
            for i in active:
                at = m["cols"][i]
                r_, c_ = at[:, 0], at[:, 1]
                sg, pp, lm, le, fm, fe = sigma[r_], p[r_, c_], m["lm"][r_, c_], m["le"][r_, c_], m["fm"][r_, c_], m["fe"][r_, c_]
                match = [pp == sg * delta[i], pp == -sg * delta[i], pp == 1, pp == -1]
                Sd, Sn, Shr, Shv = (float(np.cumsum(np.where(k, lm, le))[-1]) for k in match)
                N = [int(np.where(k, fm, fe).sum()) for k in match]
                n = len(r_)
                het = math.log10(0.001) - n * math.log10(2.0)
                den_d = (Shv + hv) + (Sd + het) + (Shr + hr) + (Sn + het)
                den_n = (Shv + hv) + (Sn + het) + (Shr + hr) + (Sd + het)
                qs = [1.0 - (Sd + het) / den_d, 1.0 - (Sn + het) / den_n, 1.0 - (Shr + hr) / den_d, 1.0 - (Shv + hv) / den_d]
                N = [N[0] + ec.FX_HET0 - n * ec.FX_LOG2, N[1] + ec.FX_HET0 - n * ec.FX_LOG2, N[2] + ec.FX_HOMREF, N[3] + ec.FX_HOMVAR]
                if with_genotype:
                    mx = max(qs[0], max(qs[1], max(qs[2], qs[3])))
                    ch = 0 if qs[0] == mx else 1 if qs[1] == mx else 2 if qs[2] == mx else 3
                    self.c["class2_ties"] += sum(1 for t in range(4) if N[t] == max(N)) > 1
                elif eta[i] == 0:
                    ch = 0 if qs[0] == max(qs[0], qs[1]) else 1
                    self.c["class2_ties"] += N[0] == N[1]
                else:
                    ch = 2 if qs[2] == max(qs[2], qs[3]) else 3
                    self.c["class2_ties"] += N[2] == N[3]
                cur = {0: 0, 1: 2, -1: 3}[int(eta[i])]
                if N[ch] > N[cur]:
                    strict = True
                elif ch != cur:
                    tie_change = True
                logp += qs[ch]
                pre += qs[cur]
                new.append((i, [(delta[i], 0), (-delta[i], 0), (delta[i], 1), (delta[i], -1)][ch]))
            if not strict and tie_change:
                self.c["class4_steps"] += 1
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
        self._attempt(prob)
        return prob

    def report(self):
        return dict(self.c)


census_holds = ec.census_holds

"""Recipes for the fragment matrix (csrc/k3_fragments.hip and the site walker of lcr_dev.h that it shares with k2_hist): plain data and
builders, no tests.

A case is a small batch for helpers.mk_batch whose reads and CIGARs are written out, the preset it runs under, and the facts it was
designed for.  tests/test_fragment_cases.py runs the two CPU oracles against each other on every case and holds the case to its
facts; tests/test_fragment_cases_gpu.py puts the same cases in front of every path K3 can take.

Reads are error free: a read carries the reference base everywhere but at the sites of its recipe.  A het site carries its alt
allele (ALT_OF, never A>G / T>C) on the reads of haplotype A; every read is a '+' transcript, so only the sites made A>G on purpose
are RNA-editing sites (candidate.rs:379-407).  Every column without an alt base falls to low_frac in pass 1 of the candidate
filters: the survivors of a case -- the columns k2_hist keeps hits for -- are its design columns and nothing else.

Words used below
  hit      an aligned base (M / = / X) of a read on a survivor column: what k2_hist counts per read and lists up to LCR_HITS = 16
  entry    a hit at a candidate that is not dense, with the reference base or one of the site's two alleles (fragment.rs:127-152)
  row      a read of the region with pos <= the last candidate's pos (fragment.rs:51-54); its entries, in candidate order

Facts of a case (every key optional; test_fragment_cases.check_facts is the reader)
  kinds    column -> what oracle_np.candidates(trace=) must say of it: "het", "hom", "edit", "somatic", "baseq" (a survivor that is no
           candidate), or "dense" (a het or hom record with LCR_F_DENSE)
  n_rows   rows per region; n_cands: candidate records per region
  two_alt  column -> (reference base, allele1, allele2) of its record
  n_ops    read -> CIGAR ops
  hits     hits of every read, in batch order
  rows     entries of every row, in row order
  links    row_links of every row; for_phasing follows from the case's min_linkers
  marks    (read, column, what): "entry" -- the read's row holds the candidate at that column; "no_hit" -- the column is a candidate, the
           read spans it and has no aligned base there; "hit_only" -- a hit without an entry; "outside" -- the candidate is not in the
           read's span [pos, rend)
  vals     (read, column, val): the entry's whole value byte, q5 | p-bit << 5 | base code << 6
  dropped  reason -> number of hits that left no entry: "not_candidate", "dense", "other_base"
"""
import functools

import numpy as np

import helpers
from longcallr_amd import _abi

START0 = 5000
ALT_OF = {"A": "C", "C": "A", "G": "T", "T": "G"}
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def val_of(q, p, base):
    return min(q, 30) | (32 if p == 1 else 0) | (CODE[base] << 6)


def make_ref(length, seed, force=()):
    rng = np.random.default_rng(seed)
    ref = list(rng.choice(list("ACGT"), size=length))
    for x, b in force:
        ref[x] = b
    return "".join(ref)


def ops_of(cigar):
    import re
    return [(int(n), c) for n, c in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]


def read(ref, lo, cigar, hap, alts=(), over=None, qual=None, k=0, region=0, start0=START0):
    """one read that starts at region column lo (may be negative) with the given CIGAR: the reference base on every aligned column, but
    alts (column -> alt base) on the reads of haplotype "A" and over (column -> base) whatever the haplotype; qual: column -> quality
    (30 elsewhere).  Inserted bases are T, clipped bases G, bases outside the region follow their column number."""
    alts, over, qual = dict(alts), over or {}, qual or {}
    seq, q, p = [], [], lo
    for n, c in ops_of(cigar):
        if c in "M=X":
            for x in range(p, p + n):
                b = ref[x] if 0 <= x < len(ref) else "ACGT"[x % 4]
                if hap == "A" and x in alts:
                    b = alts[x]
                seq.append(over.get(x, b))
                q.append(qual.get(x, 30))
            p += n
        elif c in "DN":
            p += n
        elif c in "IS":
            seq += ["T" if c == "I" else "G"] * n
            q += [30] * n
    rev = k // 2 % 2         # both read strands under either haplotype; ts so that every read is a '+' transcript
    return dict(pos=start0 + lo, seq="".join(seq), qual=q, cigar=cigar, rev=rev, ts=1 + rev, region=region, hap=hap)


def reads_over(ref, spans, alts, first_hap=0, **kw):
    """a plain read (one M op) over every [lo, hi) of spans, haplotypes alternating A, B, ..."""
    return [read(ref, lo, "%dM" % (hi - lo), "AB"[(first_hap + k) % 2], alts, k=k, **kw) for k, (lo, hi) in enumerate(spans)]


def finish(reads, regions):
    """mk_batch of the reads in the order of (region, pos) -- stable, so reads of one start keep the order of the recipe"""
    order = sorted(range(len(reads)), key=lambda i: (reads[i]["region"], reads[i]["pos"]))
    return helpers.mk_batch([reads[i] for i in order], regions), order


def reorder(order, per_read):
    return [per_read[i] for i in order]


# ---- rows16: rows on both sides of LCR_HITS / K3_INLINE ------------------------------------------------------------------------------

def rows16(extras, n_het, spacing, cycle, n_full=24):
    """One region.  `extras` survivor columns that leave no entry in front of n_het het sites `spacing` columns apart:
      "baseq"  two columns whose alt bases have quality 5: they survive pass 1 and the base-quality rule drops them (no record)
      "dense"  five het sites 8 columns apart: records with LCR_F_DENSE, dropped from every row (fragment.rs:148-152)
    Reads, in batch order: two that start before the region and see the extras only / the extras and one het site; n_full reads over
    everything; 24 reads from column 0 that end 3 bases behind het site k for k in `cycle` in turn, so that every four consecutive rows
    hold one row of each length; a read behind the extras over exactly 16 and one over 17 het sites (16 hits, 16 entries: the longest row
    k3_hits builds); with 34 or more het sites a read over 32 and one over 33; a read over the last het site only; a read between
    the last two het sites (a row without entries); a read that starts ON the last het site (the last row) and one that starts one
    column behind it (no row)."""
    ex_cols = [40, 55] if extras == "baseq" else [40, 48, 56, 64, 72]
    het = [300 + spacing * k for k in range(n_het)]
    L = het[-1] + 60
    ref = make_ref(L, 16)
    alts = {x: ALT_OF[ref[x]] for x in het + ex_cols}
    qual = {x: 5 for x in ex_cols} if extras == "baseq" else {}
    ne = len(ex_cols)
    spans, hits, rows = [], [], []

    def add(lo, hi, n_hits, n_entries):
        spans.append((lo, hi)); hits.append(n_hits); rows.append(n_entries)
    add(-20, 90, ne, 0)
    add(-20, het[0] + 10, ne + 1, 1)
    for _ in range(n_full):
        add(0, L, ne + n_het, n_het)
    for j in range(24):
        k = cycle[j % len(cycle)]
        add(0, het[k] + 3, ne + k + 1, k + 1)
    add(100, het[15] + 3, 16, 16)
    add(100, het[16] + 3, 17, 17)
    if n_het >= 34:
        add(100, het[31] + 3, 32, 32)
        add(100, het[32] + 3, 33, 33)
    add(het[-1] - 40, L, 1, 1)
    add(het[-2] + 5, het[-1] - 5, 0, 0)
    add(het[-1], L, 1, 1)
    add(het[-1] + 1, L, 0, None)          # behind the last candidate: no row
    reads = [read(ref, lo, "%dM" % (hi - lo), "AB"[k % 2], alts, qual=qual, k=k) for k, (lo, hi) in enumerate(spans)]
    b, order = finish(reads, [(START0, ref)])
    hits, rows = reorder(order, hits), reorder(order, rows)
    kinds = {x: "het" for x in het}
    kinds.update({x: extras for x in ex_cols})
    dropped = sum(h - (r or 0) for h, r in zip(hits, rows))
    facts = dict(kinds=kinds, n_rows=[sum(r is not None for r in rows)], hits=hits, rows=[r for r in rows if r is not None],
                 dropped={"not_candidate" if extras == "baseq" else "dense": dropped})
    return b, facts


# ---- rules: the fragment rules of fragment.rs:127-152, 242-255 ---------------------------------------------------------------------

RULE_COLS = dict(h0=150, hq=300, hom=450, edit=600, som=750, h2=900, two=1050, h3=1200, h4=1350)
QUALS = [29, 30, 31, 93]


def rules():
    """One region of 1 500 columns, 40 long reads over all of it and short reads that cover chosen sites only.
      hq     a het site whose bases carry quality 29 / 30 / 31 / 93 in turn, under the reference base and under the alt base
      hom    the alt base on every read; edit: A>G with G on haplotype A; som: the alt on six long reads (below min_af)
      two    reference T; C on 17 long reads, G on 17, the reference base on 4 and A -- a fourth base -- on 2: a two-alt record
             (allele1 C, allele2 G) whose A reads are hits without an entry
      h2     two haplotype-B reads carry N there: hits without an entry
    Short reads, in batch order behind the long ones of their start: rows of 0, 1, 2 and 3 links.  A link is an entry at a
    LCR_F_FOR_PHASING site: het, hom and two-alt records carry the flag (candidate.rs:419-461), RNA-edit and somatic records do
    not -- their entries are no links."""
    C = RULE_COLS
    ref = make_ref(1500, 27, force=[(C["edit"], "A"), (C["two"], "T")])
    het = [C[k] for k in ("h0", "hq", "h2", "h3", "h4")]
    alts = {x: ALT_OF[ref[x]] for x in het}
    alts[C["edit"]] = "G"
    hom_alt, som_alt = ALT_OF[ref[C["hom"]]], ALT_OF[ref[C["som"]]]
    reads, links, rows, hits, vals, marks = [], [], [], [], [], []
    two_of = ["C"] * 17 + ["G"] * 17 + ["T"] * 4 + ["A"] * 2
    for k in range(40):
        hap = "AB"[k % 2]
        over = {C["hom"]: hom_alt, C["two"]: two_of[(k * 7) % 40]}      # (7 and 40 are coprime: a permutation that mixes the haplotypes)
        if k in (4, 8, 12, 20, 28, 36):
            over[C["som"]] = som_alt
        if k in (1, 3):
            over[C["h2"]] = "N"
        q = QUALS[k // 2 % 4]
        reads.append(read(ref, 0, "1500M", hap, alts, over=over, qual={C["hq"]: q}, k=k))
        base = alts[C["hq"]] if hap == "A" else ref[C["hq"]]
        vals.append((k, C["hq"], val_of(q, 1 if hap == "B" else -1, base)))
        n = 9 - (over[C["two"]] == "A") - (k in (1, 3))
        rows.append(n); hits.append(9); links.append(n - 2)         # (all but the edit and the somatic entry)
        marks.append((k, C["two"], "hit_only" if over[C["two"]] == "A" else "entry"))
        marks.append((k, C["h2"], "hit_only" if k in (1, 3) else "entry"))
        vals.append((k, C["two"], None if over[C["two"]] == "A" else val_of(30, 1 if over[C["two"]] == "T" else -1, over[C["two"]])))
    vals = [v for v in vals if v[2] is not None]
    short = [(400, 700, 2, 1), (400, 950, 4, 2), (250, 950, 5, 3), (550, 650, 1, 0), (700, 800, 1, 0), (1000, 1100, 1, 1), (1230, 1330, 0, 0),
             (1100, 1400, 2, 2)]
    for j, (lo, hi, n, ln) in enumerate(short):
        over = {C["hom"]: hom_alt, C["two"]: "C"}
        reads.append(read(ref, lo, "%dM" % (hi - lo), "AB"[j % 2], alts, over=over, k=j))
        rows.append(n); hits.append(n); links.append(ln)
    b, order = finish(reads, [(START0, ref)])
    back = {old: new for new, old in enumerate(order)}
    kinds = {x: "het" for x in het}
    kinds.update({C["hom"]: "hom", C["edit"]: "edit", C["som"]: "somatic", C["two"]: "hom"})
    facts = dict(kinds=kinds, n_rows=[len(reads)], rows=reorder(order, rows), hits=reorder(order, hits),
                 links=reorder(order, links), marks=[(back[k], x, w) for k, x, w in marks], vals=[(back[k], x, v) for k, x, v in vals],
                 dropped={"other_base": 4}, two_alt={C["two"]: ("T", "C", "G")})
    return b, facts


# ---- geometry: where a site can stand against a CIGAR ------------------------------------------------------------------------------

GEO_L = 2000
TRIPLE = ["8=", "1X", "2D"]          # 11 reference columns
QUAD = ["13=", "1X", "1I", "2D"]     # 16 reference columns


def pattern(parts, n_ops):
    return "".join(parts[i % len(parts)] for i in range(n_ops))


# (name, first column, CIGAR); the marks below name their sites by (read name, op index, where)
GEO_READS = [
    # a read that starts before the region behind a soft clip, and one behind a hard and a soft clip: column 0, the last aligned base
    # (column 49 = rend - 1) and the column behind it
    ("clip_s", -30, "5S80M"),
    ("clip_hs", -5, "3H4S55M2S3H"),
    # every op kind: 0 60M [100,160)  1 40D [160,200)  2 60= [200,260)  3 1X 260  4 59= [261,320)  5 45N [320,365)  6 60M [365,425)
    # 7 5I  8 60M [425,485)
    ("ops", 100, "60M40D60=1X59=45N60M5I60M"),
    # 210 ops of (8=, 1X, 2D) from column 520: op 15 = [575,583), op 16 X 583, op 63 = [751,759), op 64 X 759 (the first op of the second
    # round trip of 64 ops), op 65 D [760,762), op 66 = [762,770), op 127 X 990, op 128 D [991,993), op 130 X 1001
    ("ops210", 520, pattern(TRIPLE, 210)),
    ("ops66", 520, pattern(TRIPLE, 66)),        # ends at column 762: its last candidate (760, on a D) is in its second round trip
    ("ops65", 520, pattern(TRIPLE, 65)),        # ends at 760: the last candidate IS the first column of the second round trip
    ("ops64", 520, pattern(TRIPLE, 64)),        # ends at 759: one round trip, rend = the candidate's column
    # 508 ops over the whole region and beyond both ends: every candidate of the region against (13=, 1X, 1I, 2D) from column -10
    ("quads", -10, pattern(QUAD, 4 * 127)),
    # the region's end: a read that runs 10 columns past the last column, one that ends on it
    ("end_past", GEO_L - 60, "70M"),
    ("end_on", GEO_L - 40, "40M"),
]
GEO_MARKS = [
    ("clip_s", 0, "entry"), ("clip_s", 49, "entry"), ("clip_s", 50, "outside"),
    ("clip_hs", 0, "entry"), ("clip_hs", 49, "entry"), ("clip_hs", 50, "outside"),
    ("ops", 159, "entry"), ("ops", 180, "no_hit"), ("ops", 200, "entry"), ("ops", 260, "entry"), ("ops", 342, "no_hit"),
    ("ops", 365, "entry"), ("ops", 425, "entry"), ("ops", 484, "entry"), ("ops", 485, "outside"),
    ("ops210", 575, "entry"), ("ops210", 583, "entry"), ("ops210", 751, "entry"), ("ops210", 759, "entry"), ("ops210", 760, "no_hit"),
    ("ops210", 769, "entry"), ("ops210", 990, "entry"), ("ops210", 991, "no_hit"), ("ops210", 1001, "entry"),
    ("ops66", 751, "entry"), ("ops66", 759, "entry"), ("ops66", 760, "no_hit"), ("ops66", 769, "outside"),
    ("ops65", 751, "entry"), ("ops65", 759, "entry"), ("ops65", 760, "outside"),
    ("ops64", 751, "entry"), ("ops64", 759, "outside"),
    ("end_past", GEO_L - 1, "entry"), ("end_on", GEO_L - 1, "entry"),
]
GEO_SITES = sorted({x for _, x, _ in GEO_MARKS})


def geometry(n_bg):
    """One region of 2 000 columns.  n_bg plain reads that run past both ends of the region (from column -30 / -25: under an ONT preset
    column 0 is then outside their end zones) call the het sites GEO_SITES; the reads of GEO_READS meet them at the places GEO_MARKS names."""
    ref = make_ref(GEO_L, 33)
    alts = {x: ALT_OF[ref[x]] for x in GEO_SITES}
    reads = [read(ref, -30 + 5 * (k % 2), "%dM" % (GEO_L + 60 - 10 * (k % 2)), "AB"[k // 2 % 2], alts, k=k) for k in range(n_bg)]
    names = {}
    for j, (name, lo, cigar) in enumerate(GEO_READS):
        names[name] = len(reads)
        reads.append(read(ref, lo, cigar, "AB"[j % 2], alts, k=j))
    b, order = finish(reads, [(START0, ref)])
    back = {old: new for new, old in enumerate(order)}
    marks = [(back[names[n]], x, w) for n, x, w in GEO_MARKS]
    for x in GEO_SITES:        # "quads": column x is op 4 * ((x + 10) // 16) + {0: =, 1: X, 3: D} by (x + 10) % 16 of 0..12, 13, 14..15
        marks.append((back[names["quads"]], x, "entry" if (x + 10) % 16 < 14 else "no_hit"))
    facts = dict(kinds={x: "het" for x in GEO_SITES}, marks=marks, dropped={}, n_ops={back[names[n]]: len(ops_of(c)) for n, _, c in GEO_READS})
    return b, facts


def geometry_sites():
    """the import form of `geometry`: every column of these windows is a het site of the list -- sites no filter would call, side by side
    across each op boundary of the read "ops", at the region's first and last columns and around the round trips of "ops210" """
    win = [(0, 4), (47, 53), (155, 205), (255, 266), (316, 369), (421, 430), (480, 490), (572, 586), (748, 772), (988, 1003), (GEO_L - 4, GEO_L)]
    pos = np.array(sorted({START0 + x for lo, hi in win for x in range(lo, hi)}), np.int64)
    return pos, np.ones(pos.size, np.uint8), np.full(pos.size, 30.0, np.float32)


# ---- regions: row and region bookkeeping ----------------------------------------------------------------------------------------------

def many_regions(n_regions=1030, with_sites=(0, 1023, 1024, 1029)):
    """n_regions regions of 120 columns and six reads each (min_depth is 6); the regions `with_sites` have two het sites, all others
    none: k3_rows_offsets takes the regions 1 024 at a time, so the regions 1 024 .. 1 029 are its second turn and the rows of region
    1 023 are what it carries over"""
    reads, regions, n_rows = [], [], []
    for g in range(n_regions):
        ref = make_ref(120, 1000 + g)
        alts = {x: ALT_OF[ref[x]] for x in (30, 90)} if g in with_sites else {}
        s0 = START0 + 1000 * g
        reads += reads_over(ref, [(0, 120)] * 6, alts, region=g, start0=s0)
        regions.append((s0, ref))
        n_rows.append(6 if g in with_sites else 0)
    b, order = finish(reads, regions)
    return b, dict(n_rows=n_rows, n_cands=[2 if g in with_sites else 0 for g in range(n_regions)])


def mixed_regions():
    """Six regions of 400 columns: 0 het sites at 100 and 300 under 8 reads; 1 no reads; 2 reads and no site; 3 het sites at 100 and
    250 under 8 reads, a read that starts ON column 250 (the last row) and one that starts on 251 (no row) with two more behind it;
    4 no reads; 5 as region 0 with a read between the sites that starts behind the first"""
    reads, regions = [], []
    refs = [make_ref(400, 50 + g) for g in range(6)]

    def alts_of(g, cols):
        return {x: ALT_OF[refs[g][x]] for x in cols}
    s0 = [START0 + 1000 * g for g in range(6)]
    reads += reads_over(refs[0], [(0, 400)] * 8, alts_of(0, (100, 300)), region=0, start0=s0[0])
    reads += reads_over(refs[2], [(0, 400)] * 8, {}, region=2, start0=s0[2])
    reads += reads_over(refs[3], [(0, 400)] * 8 + [(250, 400), (251, 400), (300, 400), (320, 400)], alts_of(3, (100, 250)), region=3, start0=s0[3])
    reads += reads_over(refs[5], [(0, 400)] * 8 + [(150, 280)], alts_of(5, (100, 300)), region=5, start0=s0[5])
    b, order = finish(reads, [(s, r) for s, r in zip(s0, refs)])
    assert order == list(range(len(reads)))
    return b, dict(n_rows=[8, 0, 0, 9, 0, 9], n_cands=[2, 0, 0, 2, 0, 2], rows=[2] * 8 + [2] * 8 + [1] + [2] * 8 + [0],
                   hits=[2] * 8 + [0] * 8 + [2] * 8 + [1, 0, 0, 0] + [2] * 8 + [0])


def few_reads(n):
    """one region of n reads over three sites: n_reads on both sides of the four reads of a wave and the sixteen of a workgroup.  n = 1 runs
    under min_depth 1: the read's three mismatches survive pass 1 and fall to the base-quality rule, which asks for two alt bases -- three
    hits and no row; its site list (few_sites) gives the read a row in the import form"""
    ref = make_ref(300, 70 + n)
    alts = {x: ALT_OF[ref[x]] for x in (60, 150, 240)}
    reads = reads_over(ref, [(0, 300)] * n, alts)
    b, _ = finish(reads, [(START0, ref)])
    if n == 1:
        return b, dict(n_rows=[0], rows=[], hits=[3], kinds={x: "baseq" for x in alts}, dropped={})
    return b, dict(n_rows=[n], rows=[3] * n, hits=[3] * n, kinds={x: "het" for x in alts})


def few_sites():
    pos = np.array([START0 + x for x in (60, 150, 240)], np.int64)
    return pos, np.ones(3, np.uint8), np.full(3, 30.0, np.float32)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
# covers: the (boundary, side) pairs of test_fragment_cases.LEDGER the case stands for

def case(name, family, builder, preset="hifi-masseq", covers=(), sites=None, slow_np=False, **over):
    return dict(name=name, family=family, builder=builder, preset=preset, over=over, covers=list(covers), sites=sites, slow_np=slow_np)


CYCLE4 = [13, 14, 15, 16]                 # with the two baseq columns: (hits, entries) = (16, 14), (17, 15), (18, 16), (19, 17)
CYCLE7 = [10, 11, 12, 13, 14, 15, 16]     # with the five dense sites: (16, 11) .. (22, 17)
ROWS16_COVERS = [("row hits", "16"), ("row hits", "17 with at most 16 entries"), ("row entries", "16 beside 17 in one wave"),
                 ("row entries", "0"), ("row entries", "1"), ("hit", "survivor that is no candidate"), ("rows end", "read on the last candidate"),
                 ("rows end", "read one column behind it"), ("read start", "before the region")]
CASES = [
    case("rows16_baseq", "rows16", functools.partial(rows16, "baseq", 18, 70, CYCLE4), covers=ROWS16_COVERS),
    case("rows16_dense", "rows16", functools.partial(rows16, "dense", 34, 50, CYCLE7),
         covers=[("hit", "dense candidate"), ("row entries", "32"), ("row entries", "33"), ("site batch", "16"), ("site batch", "17"),
                 ("site batch", "32 and 33")]),
    case("rows16_baseq_ont", "rows16", functools.partial(rows16, "baseq", 18, 70, CYCLE4), preset="ont-drna", covers=[("preset", "ONT rows16")]),
    case("rows16_dense_ont", "rows16", functools.partial(rows16, "dense", 34, 50, CYCLE7), preset="ont-drna",
         covers=[("preset", "ONT rows16 with dense sites")]),
    case("rules_ml1", "rules", rules,
         covers=[("quality", "29"), ("quality", "30"), ("quality", "31"), ("quality", "93"), ("allele", "reference"), ("allele", "allele1"),
                 ("allele", "allele2"), ("allele", "a fourth base"), ("allele", "N"), ("link", "het site"), ("link", "hom site"),
                 ("link", "RNA-edit site"), ("link", "somatic site"), ("min_linkers 1", "0 links"), ("min_linkers 1", "1 link")]),
    case("rules_ml2", "rules", rules, covers=[("min_linkers 2", "1 link"), ("min_linkers 2", "2 links")], min_linkers=2),
    case("geometry", "geometry", functools.partial(geometry, 12), sites=geometry_sites,
         covers=[("op", "last base of M"), ("op", "first base of ="), ("op", "X"), ("op", "D column"), ("op", "N column"),
                 ("op", "first column behind D"), ("op", "first column behind N"), ("op", "first column behind I"),
                 ("read start", "column 0 under a read from before the region"), ("read end", "rend - 1"), ("read end", "rend"),
                 ("clip", "S"), ("clip", "H + S"), ("cigar scan", "op 15"), ("cigar scan", "op 16"), ("round trip", "op 63"),
                 ("round trip", "op 64"), ("round trip", "op 65"), ("round trip", "beyond op 128"), ("early exit", "last site in the group"),
                 ("early exit", "last site on the first column of the next group"), ("early exit", "last site in the next group"),
                 ("site probe", "first site behind the 16th"), ("site batch", "second batch walks the CIGAR again"),
                 ("region", "column 0"), ("region", "last column"), ("region", "last tile of the batch"), ("import", "site list")]),
    case("geometry_ont", "geometry", functools.partial(geometry, 20), preset="ont-drna", sites=geometry_sites, covers=[("preset", "ONT geometry")]),
    case("regions_1030", "regions", many_regions, slow_np=True,
         covers=[("k3_rows_offsets", "region 1023"), ("k3_rows_offsets", "region 1024"), ("k3_rows_offsets", "last region of the second turn")]),
    case("regions_mixed", "regions", mixed_regions,
         covers=[("region", "no reads"), ("region", "reads and no candidate"), ("rows end", "pos equal to the last candidate's"),
                 ("rows end", "pos one more")]),
    case("reads_1", "regions", functools.partial(few_reads, 1), covers=[("n_reads", "1")], sites=few_sites, min_depth=1),
    case("reads_15", "regions", functools.partial(few_reads, 15), covers=[("n_reads", "15")]),
    case("reads_16", "regions", functools.partial(few_reads, 16), covers=[("n_reads", "16")]),
    case("reads_17", "regions", functools.partial(few_reads, 17), covers=[("n_reads", "17")]),
]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]
FAMILIES = sorted({c["family"] for c in CASES})


@functools.lru_cache(maxsize=None)
def built(name):
    """(batch, facts) of a case"""
    return BY_NAME[name]["builder"]()


def batch(name):
    return built(name)[0]


def facts(name):
    return built(name)[1]


def params(name):
    c = BY_NAME[name]
    return _abi.make_params(c["preset"], **dict(dict(seed=6), **c["over"]))


# ---- the census: what a read meets, counted from its CIGAR alone -------------------------------------------------------------------------

def aligned(b, r):
    """region column -> offset into the read of the base an M / = / X op of read r puts there"""
    g = int(np.searchsorted(b.read_begin, r, side="right")) - 1
    p, q = int(b.pos[r]) - int(b.start0[g]), int(b.lead_clip[r])
    out = {}
    co = int(b.cig_off[r])
    for w in b.cigar[co:co + int(b.n_cig[r])]:
        op, n = int(w) & 15, int(w) >> 4
        if op in (0, 7, 8):
            for i in range(n):
                if 0 <= p + i < int(b.len[g]):
                    out[p + i] = q + i
            p += n; q += n
        elif op == 1:
            q += n
        elif op in (2, 3):
            p += n
    return out, p           # p: rend, the first column behind the read


def base_at(b, r, off):
    return chr(b.bases[int(b.seq_off[r]) + off]), int(b.quals[int(b.seq_off[r]) + off])


NOT_A_SURVIVOR = ("min_depth", "max_depth", "ref_base", "low_frac", "low_cnt", "deletion", "af_intron", "sor", "binomial", "one_strand")

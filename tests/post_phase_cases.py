"""Recipes for the post-phase steps (csrc/k4_post.h: post_run): plain data and builders, no tests.

A case is ONE region of at most 3 kb and ~130 reads, its parameters, and its census: what oracle_np_phase must have met on the way
for the case to count as a visit of the branch it was designed for.  tests/test_post_phase_cases.py runs the two CPU oracles against
each other and checks every census; tests/test_post_phase_gpu.py puts the same cases in front of the three scopes of post_run.

Reads come from read groups: `n` error-free reads over [lo, hi) of the region, alternating haplotype A, B, A, ... (or all of one
haplotype).  A het site carries its alt allele on haplotype A; the alt of a het site is never A>G / T>C (alt_of), so with every read
ts '+' only the sites made A>G on purpose are the RNA-editing class of candidate.rs:379-407.  Further sites put an allele on the
reads a rule picks: a seeded random half, a haplotype's reads, the reads of one group.

Branches no recipe reaches:
  * a het site kept with hap1 < 1 or hap2 < 1 (phase score 0.19940219, snpfrags.rs:536-545).  None was found, and none can be
    built from reads: with one haplotag in the whole column the het likelihood under either delta IS the hom-ref or the hom-var
    likelihood, term for term; the het prior log10(theta) - n log10(2) is below the hom-var prior log10(theta / 2) for n >= 2
    observations and equal to it for n = 1 -- and there hom-ref wins, because a base quality counts as 30 at most
    (fragment.rs:125): log10(1e-3) + log10(1 - 1.5 theta) = -3.0007 against log10(1 - 1e-3) + log10(theta / 2) = -3.3014.
    Rows without a haplotag (sigma 0, met at sites of variant type 0 / 2 / 3) are errors under het and cannot help it.
    The census reports such sites (het_without_both_haplotypes), so a case that meets the branch would show it;
  * rescue code 1 (a list member with an empty column): a site joins a list only with an alt count above its deletion count
    (candidate.rs:330), every read with the alt base leaves an entry (fragment.rs:120-200: p = -1) and the dense sweep that
    would strip the entries walks the het and hom lists only (candidate.rs:465-526) -- a list member always has a column;
  * rescue code 2 on the RNA-edit list: candidate.rs:379-407 puts a site there only with variant_type != 2, a variant_type 0
    needs the hom-ref likelihood on top, which leaves QUAL below any min_qual >= 1, and nothing changes the variant type of a
    site that is not FOR_PHASING before the list is walked.  The low-fraction list has no such test: `lowfrac_homvar` reaches it.
"""
import functools

import numpy as np

import helpers
from longcallr_amd import _abi
from oracle import oracle_np_phase as onp2

START0 = 5000
ALT_OF = {"A": "C", "C": "A", "G": "T", "T": "G"}


def layout(n_snps, span=2000):
    """the site offsets of helpers.two_haplotype_batch"""
    return [100 + (span - 200) * k // (n_snps - 1) for k in range(n_snps)]


def group(lo, hi, n, hap="AB"):
    """n reads over [lo, hi): hap "AB" alternates A, B, ...; "A" / "B" puts all of them on one haplotype"""
    return dict(lo=lo, hi=hi, n=n, hap=hap)


def build(length, seed, het, groups, edit=(), marks=()):
    """het: offsets of het sites (alt on haplotype A); edit: offsets whose reference base becomes A;
    marks: (offset, base or None for the site's alt_of, rule, qual or None) with rule(k, read) -> bool over the reads in group order
    (read: dict(group=index, hap="A" | "B", j=index in the group, rnd=a seeded draw per read and mark))."""
    rng = np.random.default_rng(seed)
    ref = list(rng.choice(list("ACGT"), size=length))
    for x in edit:
        ref[x] = "A"
    reads, k = [], 0
    for gi, g in enumerate(groups):
        for j in range(g["n"]):
            hap = g["hap"] if g["hap"] in ("A", "B") else "AB"[j % 2]
            s = ref[g["lo"]:g["hi"]]
            q = [30] * len(s)
            for x in het:
                if hap == "A" and g["lo"] <= x < g["hi"]:
                    s[x - g["lo"]] = ALT_OF[ref[x]]
            for x, base, rule, qual in marks:
                who = dict(group=gi, hap=hap, j=j, rnd=float(rng.random()))
                if g["lo"] <= x < g["hi"] and rule(k, who):
                    s[x - g["lo"]] = ref[x] if base == "ref" else base or ALT_OF[ref[x]]
                    if qual is not None:
                        q[x - g["lo"]] = qual
            rev = j // 2 % 2       # both read strands under either haplotype; ts so that every read is a '+' transcript
            reads.append(dict(pos=START0 + g["lo"], seq="".join(s), qual=q, cigar="%dM" % len(s), rev=rev, ts=1 + rev, region=0))
            k += 1
    reads.sort(key=lambda r: r["pos"])      # (stable: reads of one start keep their group order)
    return helpers.mk_batch(reads, [(START0, "".join(ref))])


# ---- the builders -----------------------------------------------------------------------------------------------------------------

def ps_chain(n_snps):
    """helpers.two_haplotype_batch: every read covers all n_snps sites, so every row has n_snps node entries"""
    return helpers.two_haplotype_batch(n_snps=n_snps, n_reads=12, seed=6)[0]


def ps_tail():
    """70 sites; 12 reads over all of them, 12 over the last six only: only the entries 65..70 of the long rows join the tail to the head"""
    at = layout(70)
    return build(2000, 6, at, [group(0, 2000, 12), group(at[64] - 10, 2000, 12)])


def ps_self_loop():
    """sites {300, 900} under 40 reads; site 2000 under 40 others: a one-node component, each of its rows a self loop"""
    return build(2400, 3, [300, 900, 2000], [group(100, 1200, 40), group(1800, 2300, 40)])


def ps_no_edge():
    """40 clean reads over two sites; 6 haplotype-A reads with B's allele (the reference base, q8) at the second site: whatever
    haplotypes the sites take, the alleles of such a row fall into different classes -- two node entries, no class of two, no edge"""
    return build(1600, 4, [400, 1100], [group(100, 1500, 40), group(100, 1500, 6, hap="A")],
                 marks=[(1100, "ref", lambda k, r: r["group"] == 1, 8)])


def hom_var_bridge():
    """het sites {300, 500} under 40 reads, {1700, 1900} under 40 others, and a middle site 1100, the only one both sets of reads
    cover, with its alt on three reads in four of EITHER haplotype: no haplotype explains it, hom-var (q4) scores best (with its alt on
    half the reads the two hom scores tie on the alleles and the prior makes it hom-ref, hom_ref_one_sided's branch) and the bridge falls"""
    return build(2400, 11, [300, 500, 1700, 1900], [group(100, 1300, 40), group(900, 2300, 40)],
                 marks=[(1100, None, lambda k, r: r["j"] % 8 < 6, None)])


def hom_ref_one_sided():
    """het sites {300, 700, 1100} under 30 long haplotype-A reads and 30 haplotype-B reads that end before site 1500, which has its
    alt on every second A read: one haplotag in the whole column, half the alleles each way -- hom-ref (q3) scores best"""
    return build(2000, 12, [300, 700, 1100], [group(100, 1800, 30, hap="A"), group(100, 1300, 30, hap="B")],
                 marks=[(1500, None, lambda k, r: r["hap"] == "A" and r["j"] % 2 == 0, None)])


EDIT_A, EDIT_HALF = (600, 700, 800, 900), (1100, 1200)


def edit_list_rounds():
    """60 long reads over six het sites; A>G sites 600..900 with G on haplotype A, 1100 / 1200 with G on a random half of all reads;
    12 short reads over [580, 980) that cover the four A>G sites and no het site: no phasing rows until the first rescue"""
    return build(2000, 21, [200, 400, 1000, 1400, 1600, 1800], [group(100, 1900, 60), group(580, 980, 12)], edit=EDIT_A + EDIT_HALF,
                 marks=[(x, "G", lambda k, r: r["hap"] == "A", None) for x in EDIT_A] +
                       [(x, "G", lambda k, r: r["rnd"] < 0.5, None) for x in EDIT_HALF])


def edit_single():
    """an A>G site with G on the 30 long haplotype-A reads; its reference base on 20 short reads that cover nothing else (no phasing
    rows), and the long haplotype-B reads end before it: hap2 = 0 < 2, the member is RNA_EDIT | SINGLE"""
    return build(2000, 22, [300, 700, 1100], [group(100, 1800, 30, hap="A"), group(100, 1300, 30, hap="B"), group(1400, 1700, 20, hap="B")],
                 edit=(1500,), marks=[(1500, "G", lambda k, r: r["group"] == 0, None)])


def _a_reads(num, den, short):
    """the alt of a low-fraction site: on `num` in `den` of the long haplotype-A reads (group 0), on `short` in 3 of the short ones"""
    return lambda k, r: r["hap"] == "A" and (r["j"] // 2 % den < num if r["group"] == 0 else r["j"] // 2 % 3 < short)


def lowfrac_list(homvar=False):
    """100 long reads over five het sites and 12 short reads over [450, 750), which holds no het site but
      * three low-fraction sites (the list of candidate.rs:410-417): 500 and 700 with their alt on 9 in 25 of haplotype A's reads,
        600 on 6 in 25.  Over the assigned rows the phase score is -10 log10((1 - f) / 2) for a fraction f: 4.95 and 4.20;
      * an A>G site 650 with G on haplotype A: the RNA-edit list runs first and its success makes the short rows phasing rows
        with drawn haplotags, so both lists draw from one counter.
    The short rows stay unassigned while the lists are walked: every success draws for them again, and the next member holds them.
    homvar: also site 1500, alt on one read in seven and its reference base at q2 everywhere else -- genotype likelihood hom-var,
    allele frequency below min_af: a low-fraction member with variant_type 2 (rescue code 2)."""
    marks = [(500, None, _a_reads(9, 25, 1), None), (600, None, _a_reads(6, 25, 1), None), (700, None, _a_reads(9, 25, 1), None),
             (650, "G", lambda k, r: r["hap"] == "A", None)]
    if homvar:      # (the second mark overwrites base and quality of the first)
        marks += [(1500, "ref", lambda k, r: True, 2), (1500, None, lambda k, r: r["j"] % 7 == 0, 30)]
    return build(2000, 31, [200, 400, 1000, 1600, 1800], [group(100, 1900, 100), group(450, 750, 12)], edit=(650,), marks=marks)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
# census: key -> value it must equal, or (">=", bound).  Keys: see Census.report().  n_sites is the number of candidate records.
# A case carries the preset and what it sets beside it (seed, min_phase_score, max_enum_snps; min_linkers stays the presets' 1).


def case(name, builder, census, preset="hifi-masseq", seed=6, **over):
    return dict(name=name, builder=builder, preset=preset, over=dict(over, seed=seed), census=census)


CASES = [
    case("ps_64", functools.partial(ps_chain, 64), dict(n_sites=64, max_node_entries=64, phase_sets=1, node_sites=64)),
    case("ps_65", functools.partial(ps_chain, 65), dict(n_sites=65, max_node_entries=65, phase_sets=1, node_sites=65)),
    case("ps_70", functools.partial(ps_chain, 70), dict(n_sites=70, max_node_entries=70, phase_sets=1, node_sites=70)),
    case("ps_tail", ps_tail, dict(n_sites=70, max_node_entries=70, phase_sets=1, node_sites=70, rows_on_tail_only=12)),
    case("ps_self_loop", ps_self_loop, dict(n_sites=3, phase_sets=2, one_node_components=1, single_node_rows=40)),
    case("ps_no_edge", ps_no_edge, dict(n_sites=2, node_sites=2, no_edge_rows=6, single_node_rows=0, phase_sets=1)),
    case("ps_no_edge_mps10", ps_no_edge, dict(n_sites=2, node_sites=2, no_edge_rows=6, single_node_rows=0), min_phase_score=10.0),
    case("ps_no_edge_mps20", ps_no_edge, dict(n_sites=2, node_sites=1, no_edge_rows=0, single_node_rows=46, one_node_components=1),
         min_phase_score=20.0),
    case("hom_var_bridge", hom_var_bridge, dict(n_sites=5, genotype_calls=[(START0 + 1100, -1, 2)], phase_sets=2)),
    case("hom_ref_one_sided", hom_ref_one_sided, dict(n_sites=4, genotype_calls=[(START0 + 1500, 1, 0)])),
    case("edit_list_rounds_mps8", edit_list_rounds, dict(n_sites=12, edit_codes=[4, 4, 4, 4, 5, 5], edit_shared=(">=", 3), edit_rounds=(">=", 2),
                                                         rows_made_phasing=12, unassigned_rows=0), seed=4, min_phase_score=8.0),
    case("edit_list_rounds_mps60", edit_list_rounds, dict(n_sites=12, edit_codes=[5, 5, 5, 5, 5, 5], edit_shared=0, edit_rounds=1,
                                                          rows_made_phasing=0, unassigned_rows=12), seed=4, min_phase_score=60.0),
    case("edit_single", edit_single, dict(n_sites=4, edit_codes=[3]), seed=4),
    case("lowfrac_list", functools.partial(lowfrac_list, False), dict(n_sites=9, edit_codes=[4], lowfrac_codes=[4, 5, 4], lowfrac_shared=2, lowfrac_rounds=2,
                                                                      rows_made_phasing=12, unassigned_rows=0),
         preset="ont-cdna", seed=3, min_phase_score=7.6, max_enum_snps=4),
    case("lowfrac_homvar", functools.partial(lowfrac_list, True), dict(n_sites=10, edit_codes=[4], lowfrac_codes=[4, 5, 4, 2]),
         preset="ont-cdna", seed=3, min_phase_score=7.6, max_enum_snps=4),
]
BY_NAME = {c["name"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def batch(name):
    return BY_NAME[name]["builder"]()


def params(name, lowered=False):
    """lowered: max_enum_snps below the case's number of sites (2, or 1 for a case of two sites), which makes it a chain region --
    k4_gpost takes chain regions only.  Every census holds under either value (test_post_phase_cases.py)."""
    c = BY_NAME[name]
    more = dict(max_enum_snps=min(2, c["census"]["n_sites"] - 1)) if lowered else {}
    return _abi.make_params(c["preset"], **dict(c["over"], **more))


def is_enumerated(name):
    """the case's region has no more sites than its max_enum_snps: it is phased by enumeration and needs `lowered` for k4_gpost"""
    return BY_NAME[name]["census"]["n_sites"] <= params(name).max_enum_snps


VARIANTS = [(c["name"], False) for c in CASES] + [(c["name"], True) for c in CASES if is_enumerated(c["name"])]
VARIANT_IDS = [n + ("-chain" if low else "") for n, low in VARIANTS]


# ---- the census -------------------------------------------------------------------------------------------------------------------

class Census(onp2.SNPFrag):
    """oracle_np_phase.SNPFrag that counts, beside its unchanged steps, the branches they take"""

    def __init__(self, *a):
        super().__init__(*a)
        self.codes = {False: [], True: []}        # low_frac -> outcome code of every list member (k4_post.h: 1 .. 5)
        self.shared = {False: 0, True: 0}         # members whose column holds a row that an earlier success of the list changed
        self.rounds = {False: 1, True: 1}         # rounds of the serial rule: a member that sees a row changed in its round starts the next
        self.made_phasing = 0                     # rows a rescue made phasing rows
        self.calls = []                           # per assign_snp_haplotype_genotype: (pos, genotype, variant_type) of the sites it leaves +-1
        self.ps = {}

    def _eval_rescue(self, lst, min_phase_score, low_frac):
        snps = self.candidate_snps
        changed, in_round = set(), set()
        for ti in lst:
            s = snps[ti]
            code = 1 if not s.snp_cover_fragments else 2 if s.variant_type != 1 else 0
            cover = set(s.snp_cover_fragments)
            if code == 0 and cover & changed:
                self.shared[low_frac] += 1
            if code == 0 and cover & in_round:
                self.rounds[low_frac] += 1
                in_round = set()
            would = {k for k in cover if not self.fragments[k].for_phasing or self.fragments[k].haplotag == 0 or self.fragments[k].assignment == 0}
            new_rows = sum(1 for k in cover if not self.fragments[k].for_phasing)
            super()._eval_rescue([ti], min_phase_score, low_frac)
            if code == 0:
                code = 3 if s.single else 4 if s.for_phasing and not s.non_selected else 5
            if code == 4:
                changed |= would
                in_round |= would
                self.made_phasing += new_rows
            self.codes[low_frac].append(code)

    def assign_snp_haplotype_genotype(self):
        super().assign_snp_haplotype_genotype()
        self.calls.append([(s.pos, s.genotype, s.variant_type) for s in self.candidate_snps
                           if s.for_phasing and s.snp_cover_fragments and s.genotype != 0])

    def assign_phase_set(self, min_phase_score):
        read_ps = super().assign_phase_set(min_phase_score)
        snps = self.candidate_snps
        node = [s.phase_set != 0 for s in snps]           # (every node, and only a node, receives pos + 1 of some node)
        root = list(range(len(snps)))

        def find(x):
            while root[x] != x:
                x = root[x]
            return x
        ps = dict(max_node_entries=0, single_node_rows=0, no_edge_rows=0, rows_on_tail_only=0)
        for f in self.fragments:
            if not f.for_phasing or f.assignment == 0:
                continue
            ents = [fe for fe in f.list if node[fe.snp_idx]]
            ps["max_node_entries"] = max(ps["max_node_entries"], len(ents))
            ps["single_node_rows"] += len(ents) == 1
            edges = [(a.snp_idx, b.snp_idx) for i, a in enumerate(ents) for b in ents[i + 1:]
                     if snps[a.snp_idx].haplotype * snps[b.snp_idx].haplotype == a.p * b.p]
            ps["no_edge_rows"] += len(ents) >= 2 and not edges
            ps["rows_on_tail_only"] += bool(ents) and min(fe.snp_idx for fe in ents) >= 64
            for a, b in edges:
                root[find(a)] = find(b)
        comps = {}
        for i in range(len(snps)):
            if node[i]:
                comps.setdefault(find(i), []).append(i)
        ps["one_node_components"] = sum(1 for c in comps.values() if len(c) == 1)
        ps["phase_sets"] = len({snps[i].phase_set for i in range(len(snps)) if node[i]})
        assert ps["phase_sets"] == len(comps)
        ps["node_sites"] = sum(node)
        self.ps = ps
        return read_ps

    def report(self):
        snps = self.candidate_snps
        out = dict(self.ps, n_sites=len(snps), edit_codes=self.codes[False], lowfrac_codes=self.codes[True],
                   edit_shared=self.shared[False], lowfrac_shared=self.shared[True], edit_rounds=self.rounds[False],
                   lowfrac_rounds=self.rounds[True], rows_made_phasing=self.made_phasing, lowfrac_members=len(self.codes[True]),
                   genotype_calls=self.calls[-1], unassigned_rows=sum(1 for f in self.fragments if f.assignment == 0),
                   het_without_both_haplotypes=[s.pos for s in snps if s.for_phasing and s.genotype == 0 and s.phase_score == 0.19940219])
        return out


def census_holds(want, got):
    """the entries of `want` that `got` does not meet (empty: the census holds)"""
    bad = {}
    for k, v in want.items():
        if isinstance(v, tuple) and v and v[0] == ">=":
            ok = got[k] >= v[1]
        else:
            ok = got[k] == v
        if not ok:
            bad[k] = (v, got[k])
    return bad

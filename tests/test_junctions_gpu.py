"""K6 lcr_junctions on the GPU against the plain-Python restatement of its contract (tests/asj_ref.py), fed with the GPU's own phasing
results: a hand-checkable allele-specific instance, the edges of every rule of the contract, more than one workgroup per kernel,
synthetic ONT cDNA and demo.bam, and the call's order and re-entry on one context."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import asj_ref
import helpers
from longcallr_amd import _abi, asj, synth

pytestmark = pytest.mark.gpu

ALT = {"A": "C", "C": "A", "G": "T", "T": "G"}
FIELDS = ("region", "motif", "start0", "len", "n_reads", "phase_set", "n_phase_sets", "h1_absent", "h1_present", "h2_absent", "h2_present")


def tuples(rec):
    return [tuple(int(rec[f][i]) for f in FIELDS) for i in range(len(rec))]


def build_region(start0, length, sites, reads, seed, patches=()):
    """A region's reference (random, `patches` = [(column, text)] written into it) and its error-free reads.  reads: [(column, CIGAR,
    hap_a)], columns relative to the region; haplotype A carries the alternate base at every het site of `sites`."""
    rng = np.random.default_rng(seed)
    ref = list(rng.choice(list("ACGT"), size=length))
    for col, text in patches:
        ref[col:col + len(text)] = text
    sites = set(sites)
    out = []
    for k, (col, cigar, hap_a) in enumerate(reads):
        seq, c = [], col
        for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar):
            n = int(n)
            if op in "M=X":
                seq += [ALT[ref[x].upper()] if hap_a and x in sites else ref[x].upper() for x in range(c, c + n)]
                c += n
            elif op in "DN":
                c += n
            elif op in "IS":
                seq += ["A"] * n
        assert c <= length
        out.append(dict(pos=start0 + col, seq="".join(seq), qual=30, cigar=cigar, rev=k // 2 % 2, ts=1 + (k // 2 % 2)))
    out.sort(key=lambda r: r["pos"])
    return "".join(ref), out


def batch_of(regions):
    """regions: [(start0, ref, reads)] -> ReadBatch"""
    reads = []
    for g, (_, _, rs) in enumerate(regions):
        reads += [dict(r, region=g) for r in rs]
    return helpers.mk_batch(reads, [(s, ref) for s, ref, _ in regions])


def run_table(E, batch, min_count, min_junctions, rerun=True):
    """the engine's table and the restatement's on the engine's own phasing results"""
    if rerun:
        E.load_batch(batch).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    got, off = E.junctions(min_count, min_junctions)
    want, woff = asj_ref.junctions(batch, fm["row_region_off"], fm["row_read"], pr["assignment"], pr["phase_set"], min_count, min_junctions)
    return got, off, want, woff, fm, pr


def check(E, batch, min_count, min_junctions, rerun=True):
    got, off, want, woff, fm, pr = run_table(E, batch, min_count, min_junctions, rerun)
    assert off.tolist() == woff.tolist()
    assert tuples(got) == tuples(want)
    assert not got["pad_"].any()
    return got, off, fm, pr


# ---- 1. the allele-specific instance ---------------------------------------------------------------------------------------------
def allele_specific_region(start0=5000, seed=3):
    """Three exons [0, 800) [1100, 1400) [1900, 2700); 20 reads of haplotype A carry the middle exon, 20 of B skip it; four het sites
    in each outer exon.  Intron bounds: (800, 300) GT..AG, (1400, 500) ct..ac, so the skipping junction (800, 1100) is GT..ac = 0."""
    sites = [150, 300, 450, 600, 2050, 2200, 2350, 2500]
    reads = [(0, "800M300N300M500N800M", True) if k % 2 == 0 else (0, "800M1100N800M", False) for k in range(40)]
    ref, rs = build_region(start0, 2700, sites, reads, seed, patches=[(800, "GT"), (1098, "AG"), (1400, "ct"), (1898, "ac")])
    return (start0, ref, rs)


def test_allele_specific_instance(engine_cls):
    b = batch_of([allele_specific_region()])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=7))
    got, off, fm, pr = check(E, b, 10, 0)
    E.close()
    assert (pr["assignment"] != 0).all() and len(set(pr["phase_set"].tolist())) == 1     # the reads phase, in one set
    assert [(int(r["start0"]), int(r["len"]), int(r["motif"]), int(r["n_reads"])) for r in got] == [(5800, 300, 1, 20), (5800, 1100, 0, 20), (6400, 500, 2, 20)]
    skip = got[1]
    cells = (int(skip["h1_absent"]), int(skip["h1_present"]), int(skip["h2_absent"]), int(skip["h2_present"]))
    assert cells in ((20, 0, 0, 20), (0, 20, 20, 0)) and int(skip["n_phase_sets"]) == 1
    p = asj.fisher_two_sided([[cells[0], cells[2]], [cells[1], cells[3]]])
    assert p == pytest.approx(2.0 / math.comb(40, 20), rel=1e-9)
    for r in (got[0], got[2]):   # the middle exon's own junctions: present on A's reads, absent on B's
        assert sorted((int(r["h1_absent"]) + int(r["h2_absent"]), int(r["h1_present"]) + int(r["h2_present"]))) == [20, 20]


# ---- 2. edges ----------------------------------------------------------------------------------------------------------------------
ANCHOR = [100, 200, 300, 400, 500]


def haps(reads):
    """alternate the haplotypes over a list of (column, CIGAR)"""
    return [(c, cig, k % 2 == 0) for k, (c, cig) in enumerate(reads)]


def edge_regions():
    """Params (min_count 4, min_junctions 1).  Every region has an anchor exon [0, 600) with five het sites, so its reads phase."""
    # E0: thresholds, overlap ends, same s / same end, the op classes.  A second anchor [2000, 2600) lets reads start behind the junctions.
    e0 = ([(0, "600M100N50M100N50M")] * 4            # P: (600, 100) (750, 100)
          + [(0, "600M100N50M200N50M")] * 3          # Q: (750, 200) has min_count - 1 rows: dropped
          + [(0, "600M100N50M")] * 2                 # S: exactly min_junctions junctions: takes no part
          + [(0, "600M150N50M50N50M")] * 4           # T: (600, 150) same s as (600, 100); (800, 50) same end as (750, 100)
          + [(0, "300M5N295M100N51M")]               # U1: rend = 751: one base inside (750, 100): absent
          + [(0, "300M5N295M100N50M")]               # U2: rend = 750: adjacent, no overlap
          + [(0, "600M1400N600M")] * 6               # one junction: no part, but they link the two anchors for the phasing
          + [(849, "1M1100N350M5N295M")]             # V1: pos = 849: one base inside (750, 100): absent
          + [(850, "1M1099N350M5N295M")]             # V2: pos = 850 = s + l: no overlap
          + [(0, "2H3S300=10D5I290M100N50X20N30M2S")] * 4   # W: D = X advance, I S H do not: (600, 100) (750, 20)
          + [(50, "10M2650N10M2N10M")]               # a row without an entry: assignment 0
          + [(2600, "50M5N50M5N50M")])               # behind the last candidate: no row
    r0 = build_region(10000, 2800, ANCHOR + [2050, 2150, 2250, 2400, 2500], haps(e0), 11)
    # E1: 17 and 70 ops: the carry across rounds of 16 lanes
    e1 = [(0, "600M" + "10N10M" * 8)] * 4 + [(0, "600M" + "5N5M" * 34 + "4S")] * 4 + [(0, "600M")] * 6
    r1 = build_region(20000, 1000, ANCHOR, haps(e1), 12)
    # E2 / E3: two site clusters no read links; the long intron of group 1 spans group 2's reads.  E2: 8 against 10 rows, E3: 8 against 8
    def two_sets(n1, n2):
        return [(0, "600M2000N50M10N50M")] * n1 + [(1000, "600M10N50M10N50M")] * n2
    r2 = build_region(30000, 2800, ANCHOR + [1100, 1200, 1300, 1400, 1500], haps(two_sets(8, 10)), 13)
    r3 = build_region(40000, 2800, ANCHOR + [1100, 1200, 1300, 1400, 1500], haps(two_sets(8, 8)), 14)
    # E4: no participating row
    r4 = build_region(50000, 700, ANCHOR, haps([(0, "600M")] * 8), 15)
    return [(10000,) + r0, (20000,) + r1, (30000,) + r2, (40000,) + r3, (50000,) + r4]


def test_edges(engine_cls):
    regs = edge_regions()
    assert [len(re.findall(r"\d+[MIDNSHP=X]", c)) for c in ("600M" + "10N10M" * 8, "600M" + "5N5M" * 34 + "4S")] == [17, 70]
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    b = batch_of(regs)
    got, off, fm, pr = check(E, b, 4, 1)
    all_t = tuples(got)
    for g, reg in enumerate(regs):    # every region alone: the same records
        one, off1, _, _ = check(E, batch_of([reg]), 4, 1)
        assert [(0,) + t[1:] for t in all_t[off[g]:off[g + 1]]] == tuples(one), g
    # a batch (and a region) without a participating row
    assert off[5] - off[4] == 0
    none, off0 = E.junctions(4, 1)          # (the bound batch is E4 alone)
    assert none.size == 0 and off0.tolist() == [0, 0]
    E.close()
    asg, ps, rread = pr["assignment"], pr["phase_set"], fm["row_read"]
    rb = b.read_begin
    # E0 by hand.  Rows: every read but the one at 2600; the read at 50 has no entry and stays unassigned; all others are assigned, in one set
    rows0 = rread[fm["row_region_off"][0]:fm["row_region_off"][1]]
    assert rows0.size == rb[1] - rb[0] - 1 and int(b.pos[rb[1] - 1]) == 12600 and rb[1] - 1 not in rows0
    r50 = int(np.flatnonzero(b.pos[:rb[1]] == 10050)[0])
    assert asg[r50] == 0 and (np.delete(asg[:rows0.size], r50) != 0).all()
    assert len(set(np.delete(ps[:rows0.size], r50).tolist())) == 1
    j0 = {(t[2] - 10000, t[3]): t for t in all_t[off[0]:off[1]]}
    assert sorted(j0) == [(600, 100), (600, 150), (750, 20), (750, 100), (800, 50)]
    assert (750, 200) not in j0 and (300, 5) not in j0                       # min_count - 1 rows; two rows
    assert j0[(600, 100)][4] == 13                                            # P 4 + Q 3 + U 2 + W 4: the S reads take no part
    assert j0[(750, 100)][4] == 4 and j0[(600, 150)][4] == 4 and j0[(800, 50)][4] == 4 and j0[(750, 20)][4] == 4
    assert (600, 1400) not in j0                                              # its six reads have one junction each
    t = j0[(750, 100)]
    assert t[6] == 1 and t[8] + t[10] == 4 and t[7] + t[9] == 13             # absent: Q 3 + T 4 + U1 + W 4 + V1; U2 and V2 touch it only
    # E1: the 8 junctions of the 17-op reads and the 34 of the 70-op reads, all with 4 rows
    j1 = {(t[2] - 20000, t[3]): t[4] for t in all_t[off[1]:off[2]]}
    assert j1 == dict([((600 + 20 * k, 10), 4) for k in range(8)] + [((600 + 10 * k, 5), 4) for k in range(34)])
    # E2 / E3: two phase sets; the larger one wins, the smaller VALUE at equal sizes
    for g, base, bigger in ((2, 30000, 2), (3, 40000, 1)):
        r0, r1 = fm["row_region_off"][g], fm["row_region_off"][g + 1]
        grp1 = [r for r in range(r0, r1) if int(b.pos[rread[r]]) == base]
        grp2 = [r for r in range(r0, r1) if int(b.pos[rread[r]]) == base + 1000]
        ps1, ps2 = set(ps[grp1].tolist()), set(ps[grp2].tolist())
        assert len(ps1) == 1 and len(ps2) == 1 and ps1 != ps2 and 0 not in ps1 | ps2 and (asg[grp1 + grp2] != 0).all()
        (p1,), (p2,) = ps1, ps2
        long_intron = [t for t in all_t[off[g]:off[g + 1]] if (t[2] - base, t[3]) == (600, 2000)][0]
        assert long_intron[6] == 2
        assert long_intron[5] == (p2 if bigger == 2 else min(p1, p2))
        if bigger == 2:
            assert long_intron[8] + long_intron[10] == 0 and long_intron[7] + long_intron[9] == 10    # group 2's rows: absent
        else:
            assert long_intron[7] + long_intron[8] + long_intron[9] + long_intron[10] == 8


# ---- 3. more than one workgroup per kernel -----------------------------------------------------------------------------------------
def test_many_rows(engine_cls):
    iso = ["600M50N40M50N40M50N40M50N40M50N40M",      # all five exons behind the anchor
           "600M50N40M140N40M50N40M50N40M30N40M",     # skips one, another acceptor at the end
           "600M70N20M50N40M140N40M50N40M50N20M"]     # another donor at the start
    reads = []
    for k in range(600):       # isoform 0: 300 reads, 70 % on haplotype A; 1: 200 reads, 30 %; 2: 100 reads, half
        i = 0 if k < 300 else 1 if k < 500 else 2
        reads.append((0, iso[i], (k * 7 % 10) < (7, 3, 5)[i]))
    ref, rs = build_region(8000, 1300, ANCHOR, reads, 21)
    b = batch_of([(8000, ref, rs)])
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=5))
    got, off, fm, pr = check(E, b, 10, 2)
    E.close()
    assert (pr["assignment"] != 0).all()
    first = [t for t in tuples(got) if (t[2], t[3]) == (8600, 50)][0]
    assert first[4] == 500 and sum(first[7:]) == 600 and first[8] + first[10] == 500     # 600 participating rows, isoform 2 absent


# ---- 4. synthetic ONT cDNA, demo.bam -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ont-cdna", "demo"])
def test_synth_and_demo(engine_cls, which):
    """Kept junctions on demo.bam (1 697 filtered reads; 26 distinct junctions over all reads, 8 with >= 10 reads): the figures over the
    phased rows are printed and recorded in DESIGN.md section 1b (demo.bam: 8 kept at (10, 2), 11 at (2, 0), 1 067 of 1 697 rows assigned)."""
    if which == "demo":
        b, prm = helpers.demo_batch(), _abi.make_params("hifi-masseq")
    else:
        b, prm = synth.make_batch("ont-cdna", n_genes=4), _abi.make_params("ont-cdna")
    E = engine_cls(0, prm)
    E.load_batch(b).run_all()
    n = {}
    for mc, mj in ((10, 2), (2, 0)):
        got, off, fm, pr = check(E, b, mc, mj, rerun=False)
        n[(mc, mj)] = got.size
    print("%s: rows %d, assigned %d, kept junctions %r" % (which, pr["assignment"].size, int((pr["assignment"] != 0).sum()), n))
    E.close()
    assert n[(2, 0)] >= 1


# ---- 5. call order and re-entry ----------------------------------------------------------------------------------------------------
def test_call_order_and_reentry(engine_cls):
    b1, b2 = batch_of([allele_specific_region()]), batch_of(edge_regions()[:2])
    prm = _abi.make_params("hifi-masseq", seed=7)
    E = engine_cls(0, prm)
    lib, jp, jl = E.lib, _abi.LcrJunctionParams(10, 0), _abi.LcrJunctionList()
    E.load_batch(b1).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
    assert lib.lcr_junctions(E.h, C.byref(jp)) == -4 and lib.lcr_get_junctions(E.h, C.byref(jl)) == -4      # LCR_E_STATE
    E.phase()
    assert lib.lcr_get_junctions(E.h, C.byref(jl)) == -4                                                      # no table yet
    assert lib.lcr_junctions(E.h, None) == -1                                                                 # LCR_E_ARG
    before = (E.phase_result(), E.candidates())
    t1 = check(E, b1, 10, 0, rerun=False)[0]
    t2 = check(E, b1, 21, 0, rerun=False)[0]
    t3 = check(E, b1, 10, 1, rerun=False)[0]
    assert (t1.size, t2.size, t3.size) == (3, 0, 2)       # 20 rows each; above 20 none; B's reads have one junction
    after = (E.phase_result(), E.candidates())
    for k in before[0]:
        assert before[0][k].tobytes() == after[0][k].tobytes(), k
    assert before[1][0].tobytes() == after[1][0].tobytes() and before[1][1].tobytes() == after[1][1].tobytes()
    # the asynchronous phase stage: the same table, and lcr_collect_phase still delivers afterwards
    A = engine_cls(0, prm)
    A.set_async_phase(True)
    A.load_batch(b1).run_all()
    ta, offa = A.junctions(10, 0)
    assert tuples(ta) == tuples(t1)
    res = A.collect_phase(copy=True)
    assert res["assignment"].tobytes() == after[0]["assignment"].tobytes() and res["phase_set"].tobytes() == after[0]["phase_set"].tobytes()
    assert res["cand"].tobytes() == after[1][0].tobytes()
    A.close()
    # the next batch: the table is gone when it is bound, and its own carries nothing stale
    E.load_batch(b2)
    assert lib.lcr_get_junctions(E.h, C.byref(jl)) == -4
    E.run_all()
    assert lib.lcr_get_junctions(E.h, C.byref(jl)) == -4
    t4 = check(E, b2, 4, 1, rerun=False)[0]
    assert t4.size > 40 and int(t4["start0"].min()) >= 10000
    E.get_candidate_snps()                                  # a new candidate stage drops the phase stage's results, and the table with them
    assert lib.lcr_get_junctions(E.h, C.byref(jl)) == -4
    E.close()

"""The host side of lcr_indels without a GPU: the restatement of the contract (tests/indels_ref.py) against brute force -- an event applied
at its raw and at its normalised placement spells the same sequence, and s_left / s_right are the smallest / largest equivalent placement
inside the window, by exhaustive enumeration on low-complexity windows of at most 60 columns --, the restatement's CIGAR arms (the P op
among them, which no batch carries as far as the GPU call), every boundary of indels.genotype, and the VCF text."""
import types

import numpy as np
import pytest

import helpers
import indels_ref as ref
from longcallr_amd import _abi, indels


def spell(refseq, w0, typ, s, L, q):
    """the window's sequence with the event applied"""
    i = s - w0
    return refseq[:i] + refseq[i + L:] if typ == 0 else refseq[:i] + q + refseq[i:]


def placements(refseq, w0, w1, typ, L, target):
    """every placement inside the window that spells `target`: DEL s in [w0 + 1, w1 - L], INS s in [w0 + 1, w1] with the bases the target
    holds there"""
    out = []
    for s in range(w0 + 1, (w1 - L if typ == 0 else w1) + 1):
        q = target[s - w0:s - w0 + L] if typ else ""
        if spell(refseq, w0, typ, s, L, q) == target:
            out.append((s, q))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_normalisation_against_enumeration(seed):
    rng = np.random.default_rng(seed)
    moved = 0
    for _ in range(60):
        n = int(rng.integers(8, 61))
        w0 = int(rng.integers(0, 1000))
        w1 = w0 + n
        refseq = "".join(rng.choice(list("ACGT")[:int(rng.integers(2, 4))], size=n))
        for typ in (0, 1):
            L = int(rng.integers(1, 5))
            if typ == 0:
                s, q = int(rng.integers(w0 + 1, w1 - L + 1)), None
            else:
                s, q = int(rng.integers(w0 + 1, w1 + 1)), "".join(rng.choice(list(set(refseq)), size=L))
            target = spell(refseq, w0, typ, s, L, q)
            sl, ql = ref.left_shift(refseq, w0, typ, s, L, q)
            sr = ref.right_shift(refseq, w0, w1, typ, sl, L, ql)
            assert spell(refseq, w0, typ, sl, L, ql) == target                     # the normalised placement spells the same sequence
            want = placements(refseq, w0, w1, typ, L, target)
            assert (s, q or "") in want
            assert sl == want[0][0] and sr == want[-1][0] and (typ == 0 or ql == want[0][1])
            assert [p[0] for p in want] == list(range(sl, sr + 1))                # the equivalent placements are one interval
            # every equivalent raw placement gives the same key
            for s2, q2 in want:
                assert ref.left_shift(refseq, w0, typ, s2, L, q2 or None) == (sl, ql)
            moved += sr > sl
    assert moved > 20


def test_shift_stops():
    assert ref.left_shift("TTTTTTTTAC", 100, 0, 105, 1, None)[0] == 101                      # w0 + 1, though column w0 holds a T too
    assert ref.left_shift("ACNAAAAC", 0, 0, 6, 1, None)[0] == 3                              # the N stops it
    assert ref.left_shift("ACNNNNAC", 0, 0, 4, 1, None)[0] == 4                              # equal letters outside ACGT do not shift
    assert ref.right_shift("ACAAAAAC", 0, 8, 0, 2, 1, None) == 6 and ref.right_shift("CAAAA", 0, 5, 0, 1, 1, None) == 4      # s + L < w1
    assert ref.right_shift("CAAAA", 0, 5, 1, 1, 1, "A") == 5                                 # an insertion can stand in front of column w1
    long = "C" + "A" * 1100 + "C"
    assert ref.left_shift(long, 0, 0, 1100, 1, None)[0] == 76 and ref.right_shift(long, 0, 1102, 0, 1, 1, None) == 1025      # 1024 steps each
    assert ref.left_shift(long, 0, 1, 1100, 2, "AA") == (76, "AA")
    assert ref.pack("A") == 0 and ref.pack("CA") == 1 and ref.pack("AC") == 4 and ref.pack("ACGT") == 0b11100100


def one_read_batch(cigar, seq, pos=100):
    return helpers.mk_batch([dict(pos=pos, seq=seq, qual=30, cigar=cigar, region=0)], [(90, "ACGT" * 30)])


def test_restatement_cigar_arms():
    b = one_read_batch("2H3S5M2I4M1P3M2D0D0I0N6M10N5=2X1I", "CCC" + "ACGTA" + "TT" + "CGTA" + "CGT" + "ACGTAC" + "ACGTA" + "CG" + "T")
    pos, rend, gaps, blocks = ref.read_gaps(b, 0)
    assert (pos, rend) == (100, 137)
    assert gaps == [(1, 105, 2, "TT"), (2, 112, 2, None), (3, 120, 10, None)]     # P and the zero-length ops are nothing; the trailing I is dropped
    assert blocks == [(100, 120), (130, 137)]
    assert ref.read_gaps(one_read_batch("2I5M3D5M", "GG" + "A" * 10), 0)[2] == [(2, 105, 3, None)]      # a leading I: s <= pos
    assert ref.read_gaps(one_read_batch("3D5M", "A" * 5), 0)[2] == []                                   # a leading D
    assert ref.read_gaps(one_read_batch("5M3D", "A" * 5), 0)[2] == []                                   # a trailing D: s + Lr >= rend
    assert ref.read_gaps(one_read_batch("5N5M", "A" * 5), 0)[2] == [(3, 100, 5, None)]                  # every N is a gap
    w = ("ACGT" * 30)
    ev = lambda g, **kw: ref.event_of(g, w, 90, 210, kw.get("max_ins", 12), kw.get("max_del", 50))
    assert ev((1, 105, 2, "TN")) is None and ev((1, 105, 2, "tt"))[0] == (105, 1, (2 << 24) | 15)       # another letter; either case
    assert ev((2, 91, 2, None)) is not None and ev((2, 90, 2, None)) is None                            # s >= w0 + 1
    assert ev((2, 208, 2, None)) is not None and ev((2, 209, 2, None)) is None                          # s + L <= w1
    assert ev((1, 210, 1, "G")) is not None and ev((1, 211, 1, "G")) is None
    assert ev((2, 100, 51, None)) is None and ev((1, 100, 3, "GGG"), max_ins=2) is None and ev((3, 100, 5, None)) is None
    with pytest.raises(ValueError):
        ref.indels(b, [0, 1], [0], [1], [0], max_ins=13)


def rec_of(**kw):
    r = np.zeros(1, _abi.INDEL_DTYPE)[0]
    for k, v in kw.items():
        r[k] = v
    return r


def het(h1p, h1a, h2p, h2a, ps=7, **kw):
    return rec_of(phase_set=ps, h1_present=h1p, h1_absent=h1a, h2_present=h2p, h2_absent=h2a, n_present=h1p + h2p, n_absent=h1a + h2a, **kw)


def test_genotype_boundaries():
    g = indels.genotype
    assert g(rec_of(n_other=5)) is None                                           # no PRESENT or ABSENT row: not written
    assert g(het(20, 0, 0, 20))[:3] == ("1|0", "PASS", 7) and g(het(0, 20, 20, 0))[:3] == ("0|1", "PASS", 7)
    assert g(het(20, 0, 0, 20, ps=0))[:2] == ("0/1", "LowQual")                   # phase_set 0: never phased
    assert g(het(6, 4, 2, 8))[0] == "0/1" and g(het(6, 4, 2, 8), alpha=1.0)[0] == "1|0"              # 0.6 and 0.2 are inside
    assert g(het(59, 41, 2, 8), alpha=1.0)[0] == "0/1" and g(het(6, 4, 21, 79), alpha=1.0)[0] == "0/1"      # 0.59; 0.21
    assert g(het(3, 0, 0, 3), alpha=1.0)[0] == "1|0" and g(het(2, 0, 0, 3), alpha=1.0)[0] == "0/1"   # min_hap_reads on either side
    assert g(het(3, 0, 0, 2), alpha=1.0)[0] == "0/1" and g(het(2, 0, 0, 3), alpha=1.0, min_hap_reads=2)[0] == "1|0"
    p = indels.fisher(het(5, 0, 0, 5))
    assert g(het(5, 0, 0, 5), alpha=p)[0] == "1|0" and g(het(5, 0, 0, 5), alpha=p * 0.999)[0] == "0/1"      # p <= alpha
    assert g(het(5, 0, 0, 5), alpha=p, p_adj=p * 1.001)[0] == "0/1" and g(het(5, 0, 0, 5), p_adj=0.05)[0] == "1|0"
    assert g(het(8, 2, 8, 2))[:3] == ("1/1", "PASS", None) and g(het(79, 21, 79, 21))[:2] == ("0/1", "LowQual")      # hom_frac 0.8 is inside
    assert g(rec_of(n_present=4, n_absent=1))[0] == "1/1" and g(rec_of(n_present=4, n_absent=1), hom_frac=0.81)[0] == "0/1"
    assert g(het(20, 0, 0, 20), het_high=1.0, het_low=0.0)[0] == "1|0" and g(het(19, 1, 0, 20), het_high=1.0)[0] == "0/1"
    assert g(rec_of(n_present=1, n_absent=0, phase_set=3))[:3] == ("1/1", "PASS", None)       # untagged rows only: no cell, no phasing


def test_vcf_text():
    #            0         1
    #            0123456789012345
    refa = np.frombuffer(b"acgtACGTTTGGccaa", np.uint8)
    start0, col_off = [1000, 5000], [0, 8, 16]
    d = het(12, 0, 0, 10, region=0, type=0, start0=1003, len=2, hrun=1, shift=0, depth=25, n_other=3)          # deletes columns 1003-1004: tA
    i = het(0, 9, 11, 0, region=1, type=1, start0=5002, len=3, seq=ref.pack("GCA"), hrun=2, shift=4, depth=21)
    h = rec_of(region=1, type=1, start0=5002, len=3, seq=ref.pack("CCA"), n_present=9, n_absent=1, depth=11)
    e = rec_of(region=1, type=0, start0=5001, len=1, n_other=4)                                                   # not written
    assert indels.unpack(ref.pack("GCA"), 3) == "GCA" and indels.unpack(0b1101, 2) == "CT"                        # the first base in the lowest bits
    al = [indels.alleles(r, start0, col_off, refa) for r in (d, i, h, e)]
    assert al[:3] == [("GTA", "G"), ("T", "TGCA"), ("T", "TCCA")]
    # tables in another order than the contigs', records in another order than their positions
    text, n_pass = indels.format_vcf([("chrB", np.array([h, i, e]), [al[2], al[1], al[3]]), ("chrA", np.array([d]), [al[0]])], ["chrA", "chrB"])
    lines = [ln.split("\t") for ln in text.splitlines()]
    assert [(ln[0], ln[1], ln[3], ln[4]) for ln in lines] == [("chrA", "1003", "GTA", "G"), ("chrB", "5002", "T", "TCCA"), ("chrB", "5002", "T", "TGCA")]
    assert n_pass == 3 and [ln[6] for ln in lines] == ["PASS"] * 3 and all(ln[5] == "." and ln[8] == "GT:DP:AD:AF:PS:HC:PV" for ln in lines)
    assert lines[0][7] == "HRUN=1;SHIFT=0" and lines[2][7] == "HRUN=2;SHIFT=4"
    f0, f1, f2 = [ln[9].split(":") for ln in lines]
    assert f0[:6] == ["1|0", "25", "10,12", "0.5455", "7", "12,0,0,10"] and f2[:6] == ["0|1", "21", "9,11", "0.5500", "7", "0,9,11,0"]
    assert f1[:6] == ["1/1", "11", "1,9", "0.9000", ".", "0,0,0,0"]
    # the p-values are adjusted over the written records: three of them here
    from longcallr_amd.asj import bh_adjust
    want = bh_adjust([indels.fisher(h), indels.fisher(i), indels.fisher(d)])
    assert [f1[6], f2[6], f0[6]] == ["%.3g" % float(x) for x in want]
    assert indels.format_vcf([("chrB", np.array([i]), [al[1]])], het_high=1.1)[1] == 0                            # the thresholds reach genotype()

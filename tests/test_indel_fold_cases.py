"""The recipes of tests/indel_fold_cases.py on the CPU: the two restatements of the pileup (oracle/lcr_oracle.cpp, oracle_np.pileup) agree on
every case and meet its hand-written facts; the model of the fold rule folds and keeps what each case says it does; and the long read's
M / indel pairs really fall on the thread, wave and block borders its recipe names -- read off the op indices."""
import numpy as np
import pytest

import indel_fold_cases as fc
import pileup_cases as pc
from test_pileup_cases import check_facts, np_planes
from longcallr_amd import _abi

T = fc.T
PLANES = _abi.PLANE_NAMES
CASE_PLATFORMS = [(n, pl) for n in fc.NAMES for pl in fc.PLATFORMS]


@pytest.mark.parametrize("name,platform", CASE_PLATFORMS)
def test_both_restatements_agree_and_meet_the_facts(orc, name, platform):
    b, prm = fc.batch(name), fc.params(name, platform)
    facts = fc.facts(name, platform)
    for label, g in fc.built(name)[2].items():
        want = orc.Region(b, g, prm).pileup().planes()
        got = np_planes(b, g, prm)
        assert want.shape == got.shape == (len(PLANES), int(b.len[g]))
        for k, plane in enumerate(PLANES):
            assert np.array_equal(want[k], got[k]), "%s %s: plane %s" % (name, label, plane)
        assert facts[label], label
        check_facts(want, facts[label], "%s %s (%s)" % (name, label, platform))


@pytest.mark.parametrize("name", fc.NAMES)
def test_the_model_folds_and_keeps_what_the_case_says(name):
    c = fc.BY_NAME[name]
    b, prm = fc.batch(name), fc.params(name, "ont")
    items, records, folded = fc.model(name, "ont")
    assert bool(folded) == c["folds"], (name, folded)
    assert bool(fc.kept_indels(b, prm)) == c["keeps"], name
    assert records == fc.unfolded_records(b, prm) - len(folded) and items <= fc.unfolded_records(b, prm)
    # a folded op is an I, or a D of length 1, right behind an M-class op of the same read
    for j, kind, jm in folded:
        w, wm = int(b.cigar[int(b.cig_off[0]) + j]), int(b.cigar[int(b.cig_off[0]) + jm])
        assert jm == j - 1 and (wm & 15) in (0, 7, 8)
        assert (w & 15, kind) in ((1, "I"), (2, "D")) and (kind == "I" or w >> 4 == 1)
        r = int(np.searchsorted(b.cig_off, int(b.cig_off[0]) + j, side="right")) - 1
        assert int(b.cig_off[r]) <= int(b.cig_off[0]) + jm, "a fold across two reads"


def test_literal_counts():
    """a few of the model's figures, written out"""
    assert T == 256 and fc.K0_OPT == 4 and fc.WOPS == 256 and fc.K0_OPB == 1024 and fc.K0_WIN == 256
    assert [k for _, k, _ in fc.model("mid", "ont")[2]] == ["I", "I", "D", "D"] + ["D", "I"] * 12
    assert [k for _, k, _ in fc.model("tile_end", "ont")[2]] == ["I", "D", "I"]          # (the D on column T stays)
    assert [k for _, k, _ in fc.model("region_end", "ont")[2]] == ["D", "I", "D"]
    assert [k for _, k, _ in fc.model("region_start", "ont")[2]] == ["I", "I", "D"]
    assert [k for _, k, _ in fc.model("neighbours", "ont")[2]] == ["I", "D", "D"]
    assert fc.model("read_border", "ont")[2] == [] and fc.model("read_border", "hifi")[2] == []
    # the end trim: one fold at dist_to_end 20, all five at 0 and under the HiFi preset
    assert [len(fc.model(n, pl)[2]) for n, pl in (("trim_20", "ont"), ("trim_0", "ont"), ("trim_20", "hifi"))] == [1, 5, 5]
    # items do not move with the fold, whatever the trim leaves
    assert fc.model("trim_0", "ont")[0] == 15 and fc.model("trim_0", "ont")[1] == 10
    assert fc.model("trim_20", "ont")[0] == 11 and fc.model("trim_20", "ont")[1] == 10      # (four M ops of 10 bases are trimmed away; one fold)
    n = fc.OVF_READS
    assert fc.model("overflow", "ont")[:2] == (n * (1 + 1 + 40), n * (2 + 2 + 20))      # (100M over [500, 600) crosses 2 T; the intron's two ends; twenty M)


def test_the_long_read_meets_every_border():
    """over the four shifts: a folded pair across a thread border (the M is its thread's last op) for I and for D, an unfolded pair across a
    wave border and across the block border for I and for D, and pairs inside a thread"""
    seen = set()
    for s in range(4):
        name = "long_%d" % s
        b, prm = fc.batch(name), fc.params(name, "ont")
        assert int(b.n_cig.max()) > fc.K0_OPB and int(b.cig_off[0]) == 0
        g = fc.region_of(name, "long")
        r = int(b.read_begin[g])
        c0 = int(b.cig_off[r])
        assert c0 == s and int(b.cigar[c0]) & 15 == 4                      # `shift` ops in front, then the soft clip
        folded = {jm: kind for _, kind, jm in fc.model(name, "ont")[2]}
        for i in range(int(b.n_cig[r]) - 1):
            j, w, w2 = c0 + i, int(b.cigar[c0 + i]), int(b.cigar[c0 + i + 1])
            if (w & 15) != 0 or (w2 & 15) not in (1, 2):
                continue
            kind = "ID"[(w2 & 15) - 1]
            col_end = fc.LONG_LO + 5 * ((i - 1) // 4) + (2 if kind == "D" else 5)
            on_next_tile = kind == "D" and col_end % T == 0
            where = "block" if j % fc.K0_OPB == fc.K0_OPB - 1 else "wave" if j % fc.WOPS == fc.WOPS - 1 else "thread" if j % fc.K0_OPT == fc.K0_OPT - 1 else "inside"
            if where in ("block", "wave"):
                assert j not in folded, (name, j)
            elif not on_next_tile:
                assert folded.get(j) == kind, (name, j)
            else:
                assert j not in folded
            seen.add((where, kind))
    assert seen == {(w, k) for w in ("block", "wave", "thread", "inside") for k in "ID"}


def test_the_overflow_case_leaves_the_window():
    b, prm = fc.batch("overflow"), fc.params("overflow", "ont")
    tiles, _, first = pc.records(b, prm)
    behind = [t for t in range(len(tiles)) if tiles[t] and t >= fc.K0_WIN + fc.OVF_S // T]
    assert behind and sum(len(tiles[t]) for t in behind) == fc.OVF_READS * (1 + 20 + 20)          # the intron's last tile, the tail's M, D and I
    assert all(j > 1 for j, _, _ in fc.model("overflow", "ont")[2])                                 # every fold lies behind the intron

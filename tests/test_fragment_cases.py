"""The recipes of tests/fragment_cases.py on the CPU.  For every case the two restatements of SNPFrag::get_fragments -- oracle/lcr_oracle.cpp
(what the GPU tests compare with) and oracle_np_phase.fragment_rows -- leave the same rows: read, candidate indices, all eight bits of every
value (quality, p-bit and the base code in bits 6-7), row_links and row_for_phasing.  Then the case is held to the facts it was designed
for (fragment_cases' docstring lists the keys): hits are counted here from the reads' CIGARs and the survivor columns of
oracle_np.candidates' trace, by neither restatement.  LEDGER names every (boundary, side) pair the cases stand for."""
import functools

import numpy as np
import pytest

import fragment_cases as fc
from longcallr_amd import _abi
from oracle import oracle_np as onp
from oracle import oracle_np_phase as onp2

F = _abi

LEDGER = [
    # rows against LCR_HITS = K3_INLINE = 16 (k3_hits / k3_walk_list / k3_place)
    ("row hits", "16"), ("row hits", "17 with at most 16 entries"), ("row entries", "16 beside 17 in one wave"), ("row entries", "0"),
    ("row entries", "1"), ("row entries", "32"), ("row entries", "33"), ("hit", "survivor that is no candidate"), ("hit", "dense candidate"),
    # fragment.rs:127-152, 242-255
    ("quality", "29"), ("quality", "30"), ("quality", "31"), ("quality", "93"), ("allele", "reference"), ("allele", "allele1"),
    ("allele", "allele2"), ("allele", "a fourth base"), ("allele", "N"), ("link", "het site"), ("link", "hom site"), ("link", "RNA-edit site"),
    ("link", "somatic site"), ("min_linkers 1", "0 links"), ("min_linkers 1", "1 link"), ("min_linkers 2", "1 link"), ("min_linkers 2", "2 links"),
    # row16_find_sites / row16_walk_range
    ("op", "last base of M"), ("op", "first base of ="), ("op", "X"), ("op", "D column"), ("op", "N column"), ("op", "first column behind D"),
    ("op", "first column behind N"), ("op", "first column behind I"), ("read start", "before the region"),
    ("read start", "column 0 under a read from before the region"), ("read end", "rend - 1"), ("read end", "rend"), ("clip", "S"), ("clip", "H + S"),
    ("cigar scan", "op 15"), ("cigar scan", "op 16"), ("round trip", "op 63"), ("round trip", "op 64"), ("round trip", "op 65"),
    ("round trip", "beyond op 128"), ("early exit", "last site in the group"), ("early exit", "last site on the first column of the next group"),
    ("early exit", "last site in the next group"), ("site probe", "first site behind the 16th"), ("site batch", "16"), ("site batch", "17"),
    ("site batch", "32 and 33"), ("site batch", "second batch walks the CIGAR again"),
    # rows and regions
    ("rows end", "read on the last candidate"), ("rows end", "read one column behind it"), ("rows end", "pos equal to the last candidate's"),
    ("rows end", "pos one more"), ("region", "column 0"), ("region", "last column"), ("region", "last tile of the batch"), ("region", "no reads"),
    ("region", "reads and no candidate"), ("k3_rows_offsets", "region 1023"), ("k3_rows_offsets", "region 1024"),
    ("k3_rows_offsets", "last region of the second turn"), ("n_reads", "1"), ("n_reads", "15"), ("n_reads", "16"), ("n_reads", "17"),
    ("preset", "ONT rows16"), ("preset", "ONT rows16 with dense sites"), ("preset", "ONT geometry"), ("import", "site list"),
]


def np_rows(b, g, prm, cands):
    """oracle_np_phase's rows of region g as (read, [candidate], [value byte], links, for_phasing)"""
    sf = onp2.fragment_rows(b, g, prm, cands)
    return [(read, [e[0] for e in ents], [(e[2] & 31) | (32 if e[3] == 1 else 0) | (fc.CODE[e[1]] << 6) for e in ents], links, int(fp))
            for read, ents, links, fp in sf.fragmat_snapshot]


def rows_of(fm):
    """the same tuples from a fragmat() dict of one region"""
    return [(int(fm["row_read"][k]), fm["col"][fm["row_ptr"][k]:fm["row_ptr"][k + 1]].tolist(), fm["val"][fm["row_ptr"][k]:fm["row_ptr"][k + 1]].tolist(),
             int(fm["row_links"][k]), int(fm["row_for_phasing"][k])) for k in range(len(fm["row_read"]))]


def trace_of(b, g, prm):
    tr = {}
    onp.candidates(onp.pileup(b, g, prm), int(b.start0[g]), prm, trace=tr)
    return tr


@functools.lru_cache(maxsize=None)
def oracle_state(name):
    """per region of the case: the C++ oracle's candidates and rows"""
    from oracle import orc
    orc.build()
    b, prm = fc.batch(name), fc.params(name)
    out = []
    for g in range(b.n_regions):
        R = orc.Region(b, g, prm).pileup().candidates().fragments()
        out.append((R.cands(), R.fragmat()))
    return out


def np_regions(name):
    """the regions oracle_np walks: all of them, but in a case marked slow_np the regions with candidates, their neighbours and every 64th"""
    b = fc.batch(name)
    if not fc.BY_NAME[name]["slow_np"]:
        return list(range(b.n_regions))
    st = oracle_state(name)
    has = {g for g in range(b.n_regions) if len(st[g][0])}
    return sorted({x for g in has for x in (g - 1, g, g + 1) if 0 <= x < b.n_regions} | set(range(0, b.n_regions, 64)))


@pytest.mark.parametrize("name", fc.NAMES)
def test_both_restatements_leave_the_same_rows(orc, name):
    b, prm = fc.batch(name), fc.params(name)
    assert b.n_reads <= 6200 and int(max(b.seq_len)) <= 2100
    st = oracle_state(name)
    for g in np_regions(name):
        cands, fm = st[g]
        assert rows_of(fm) == np_rows(b, g, prm, cands), "%s region %d" % (name, g)


def check_facts(name, b, prm, st, traces):     # noqa: C901
    """st: per region (candidate records, fragmat dict); traces: region -> oracle_np.candidates' trace (the regions np_regions names)"""
    want = fc.facts(name)
    ng = b.n_regions
    cand_at = [{int(c["pos"]) - int(b.start0[g]): i for i, c in enumerate(st[g][0])} for g in range(ng)]
    rows = [rows_of(st[g][1]) for g in range(ng)]
    row_of_read = {r[0]: (g, r) for g in range(ng) for r in rows[g]}
    if "n_rows" in want:
        assert [len(r) for r in rows] == want["n_rows"]
    if "n_cands" in want:
        assert [len(st[g][0]) for g in range(ng)] == want["n_cands"]
    for x, kind in want.get("kinds", {}).items():
        why = traces[0].get(x, "")
        if kind == "dense":
            assert why.startswith(("het", "hom")) and int(st[0][0]["flags"][cand_at[0][x]]) & F.F_DENSE, (x, why)
        else:
            assert why.startswith(kind), (x, kind, why)
            assert (x in cand_at[0]) == (kind != "baseq")
            if kind != "baseq":
                fl = int(st[0][0]["flags"][cand_at[0][x]])
                assert not fl & F.F_DENSE and bool(fl & F.F_FOR_PHASING) == (kind in ("het", "hom")), (x, kind, fl)
    for x, (ref, a1, a2) in want.get("two_alt", {}).items():
        c = st[0][0][cand_at[0][x]]
        assert (chr(c["ref_base"]), chr(c["allele1"]), chr(c["allele2"])) == (ref, a1, a2)
    survivors = {g: {x for x, why in tr.items() if why not in fc.NOT_A_SURVIVOR} for g, tr in traces.items()}
    hits, dropped, n_entries, n_row_hits = [], {}, 0, 0
    for r in range(b.n_reads):
        g = int(np.searchsorted(b.read_begin, r, side="right")) - 1
        if g not in survivors:
            hits.append(None)
            continue
        al, rend = fc.aligned(b, r)
        mine = sorted(x for x in al if x in survivors[g])
        hits.append(len(mine))
        if r not in row_of_read:
            continue
        cols = row_of_read[r][1][1]
        n_entries += len(cols)
        n_row_hits += len(mine)
        for x in mine:
            i = cand_at[g].get(x)
            base, _ = fc.base_at(b, r, al[x])
            c = st[g][0][i] if i is not None else None
            why = ("not_candidate" if c is None else "dense" if int(c["flags"]) & F.F_DENSE else
                   "other_base" if base not in (chr(c["ref_base"]), chr(c["allele1"]), chr(c["allele2"])) else None)
            assert (why is None) == (i in cols), (r, x, why)
            if why:
                dropped[why] = dropped.get(why, 0) + 1
    assert n_entries == n_row_hits - sum(dropped.values())          # every entry is a hit, every other hit has its reason
    if "hits" in want:
        assert hits == want["hits"]
    if "rows" in want:
        assert [len(r[1]) for g in range(ng) for r in rows[g]] == want["rows"]
    if "links" in want:
        assert [r[3] for r in rows[0]] == want["links"]
        assert [r[4] for r in rows[0]] == [int(n >= prm.min_linkers) for n in want["links"]]
    if "dropped" in want:
        assert dropped == {k: v for k, v in want["dropped"].items() if v}
    for r, x, what in want.get("marks", []):
        al, rend = fc.aligned(b, r)
        i = cand_at[0][x]                     # (every mark stands on a candidate)
        cols = row_of_read[r][1][1]
        lo = int(b.pos[r]) - int(b.start0[0])
        if what == "entry":
            assert x in al and i in cols, (r, x, what)
        elif what == "no_hit":
            assert lo <= x < rend and x not in al and i not in cols, (r, x, what)
        elif what == "hit_only":
            assert x in al and x in survivors[0] and i not in cols, (r, x, what)
        else:
            assert what == "outside" and not (lo <= x < rend) and i not in cols, (r, x, what)
    for r, x, v in want.get("vals", []):
        _, (_, cols, vals, _, _) = row_of_read[r]
        assert vals[cols.index(cand_at[0][x])] == v, (r, x, v)
    for r, n in want.get("n_ops", {}).items():
        assert int(b.n_cig[r]) == n
    return hits


@pytest.mark.parametrize("name", fc.NAMES)
def test_the_case_meets_its_facts(orc, name):
    b, prm = fc.batch(name), fc.params(name)
    traces = {g: trace_of(b, g, prm) for g in np_regions(name)}
    check_facts(name, b, prm, oracle_state(name), traces)


@pytest.mark.parametrize("name", [c["name"] for c in fc.CASES if c["sites"]])
def test_site_list_rows(orc, name):
    """the import form of a case with a site list: every site is a record, none is dense and every read base is the reference base or an
    allele, so a row is exactly the read's aligned bases on the listed columns -- sites side by side across every op boundary"""
    from test_import_candidates_gpu import expected_import
    b, prm = fc.batch(name), fc.params(name)
    pos0, gt, qual = fc.BY_NAME[name]["sites"]()
    recs = expected_import(orc, b, prm, pos0, gt, qual)
    assert len(recs) == pos0.size and (pos0.size > 100 or not name.startswith("geometry"))
    rows = np_rows(b, 0, prm, recs)
    assert [r[0] for r in rows] == list(range(b.n_reads))
    at = {int(p) - fc.START0: i for i, p in enumerate(pos0)}
    for r, cols, vals, links, fp in rows:
        al, _ = fc.aligned(b, r)
        assert cols == [at[x] for x in sorted(al) if x in at], r
        assert links == len(cols) and fp == int(links >= 1)
    assert max(len(r[1]) for r in rows) == pos0.size


def test_the_ledger_is_complete():
    """every (boundary, side) pair has a case, every case has a pair, and the pairs that name a number find it in their case's facts"""
    covered = {}
    for c in fc.CASES:
        for pair in c["covers"]:
            assert pair not in covered, "%s: %s is %s's" % (c["name"], pair, covered.get(pair))
            covered[pair] = c["name"]
    assert set(covered) == set(LEDGER) and len(set(LEDGER)) == len(LEDGER)
    assert all(c["covers"] for c in fc.CASES)
    f = fc.facts("rows16_baseq")
    pairs = list(zip(f["hits"], f["rows"] + [None]))       # (the last read has no row)
    for want in ((16, 14), (17, 15), (18, 16), (19, 17), (16, 16), (17, 17), (2, 0), (3, 1), (0, 0), (1, 1)):
        assert want in pairs, want
    at = pairs.index((16, 14))
    at += -at % 4                                           # the next wave of four reads
    assert sorted(pairs[at:at + 4]) == [(16, 14), (17, 15), (18, 16), (19, 17)]
    f = fc.facts("rows16_dense")
    pairs = list(zip(f["hits"], f["rows"] + [None]))
    assert {(16 + k, 11 + k) for k in range(7)} | {(16, 16), (32, 32), (33, 33), (39, 34)} <= set(pairs)
    f = fc.facts("rules_ml1")
    assert {0, 1, 2, 3} <= set(f["links"]) and f["dropped"] == {"other_base": 4}
    assert (1, 0) in zip(f["rows"], f["links"])             # an entry that is no link
    assert {v & 31 for _, x, v in f["vals"] if x == fc.RULE_COLS["hq"]} == {29, 30}
    assert fc.params("rules_ml2").min_linkers == 2 and fc.params("rules_ml1").min_linkers == 1
    f = fc.facts("geometry")
    assert sorted(f["n_ops"].values()) == [1, 1, 2, 5, 9, 64, 65, 66, 210, 508]
    assert len(fc.GEO_SITES) > 16 and {w for _, _, w in f["marks"]} == {"entry", "no_hit", "outside"}
    f = fc.facts("regions_1030")
    assert len(f["n_rows"]) >= 1030 and [g for g, n in enumerate(f["n_rows"]) if n] == [0, 1023, 1024, len(f["n_rows"]) - 1]

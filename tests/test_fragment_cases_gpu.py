"""The recipes of tests/fragment_cases.py in front of the kernels: every case through load_batch -> pileup -> candidates -> get_fragments ->
fragmat(), byte for byte against the C++ oracle on row_region_off, row_ptr, col, val, row_links, row_for_phasing and row_read, in every
form K3 can take.  tests/test_fragment_cases.py shows on the CPU that each case meets the boundary it names.

  hits      the default: k3_hits builds the rows from k2_hist's hit lists, k3_walk_list<count | fill> walks the reads beyond them
  walk      debug_set("k3_hits", 0): k3_walk<count | fill> walks every read's CIGAR (the path of batches without hit lists)
  tiles     debug_set("hist_tiles", 1), ONT presets: the tile histograms leave no hit lists either
  import    import_external_candidates with the case's own records as sites (and with the case's site list, where it has one): no
            survivors, no dense flags -- against oracle_np_phase.fragment_rows over the expected import records
No test here goes beyond fragmat() but test_phase_of_a_family."""
import functools

import numpy as np
import pytest

import fragment_cases as fc
import test_gpu_parity as par
from test_fragment_cases import np_rows
from test_import_candidates_gpu import check_records, expected_import, sites_of

pytestmark = pytest.mark.gpu

FIELDS = ("row_region_off", "row_ptr", "col", "val", "row_links", "row_for_phasing", "row_read")
ONT = [c["name"] for c in fc.CASES if c["preset"].startswith("ont")]
WITH_SITES = [c["name"] for c in fc.CASES if c["sites"]]


@functools.lru_cache(maxsize=None)
def oracle_fragmat(name):
    """the C++ oracle's fragment matrix of the whole batch in fragmat()'s layout (col batch-wide), and its candidate offsets"""
    from oracle import orc
    orc.build()
    b = fc.batch(name)
    O = orc.Batch(b, fc.params(name), mode=orc.MODE_EXACT_ONLY, upto="frag", keep_planes=False)
    fm, off = O.fragmat(), O.cand_off.copy()
    O.close()
    row_region = np.repeat(np.arange(b.n_regions), np.diff(fm["row_region_off"]))
    fm["col"] = fm["col"] + np.repeat(off[:-1][row_region], np.diff(fm["row_ptr"]))
    return {k: np.ascontiguousarray(fm[k]) for k in FIELDS}, off


def same(got, want, what):
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), "%s: %s" % (what, k)


def fragmat_of(E, b):
    E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
    return {k: v.copy() for k, v in E.fragmat().items()}


def run(engine_cls, name, switch=None):
    E = engine_cls(0, fc.params(name))
    if switch:
        E.debug_set(*switch)
    fm = fragmat_of(E, fc.batch(name))
    off = E.candidates()[1].copy()
    E.close()
    return fm, off


@pytest.mark.parametrize("name", fc.NAMES)
def test_hit_lists(engine_cls, orc, name):
    want, want_off = oracle_fragmat(name)
    fm, off = run(engine_cls, name)
    assert np.array_equal(off, want_off)
    if name.startswith("rows16"):
        # the case's precondition on the kernels' own output: rows on both sides of K3_INLINE among the four reads of one wave
        n = np.diff(fm["row_ptr"])
        waves = {}
        for k, r in zip(n.tolist(), fm["row_read"].tolist()):
            waves.setdefault(r // 4, []).append(k)
        if "baseq" in name:
            assert [14, 15, 16, 17] in [sorted(w) for w in waves.values()]
        assert any(16 in w and 17 in w for w in waves.values())
        fm0, _ = run(engine_cls, name, ("k3_hits", 0))
        same(fm0, fm, "%s, k3_hits 0 against 1" % name)
    same(fm, want, name)


@pytest.mark.parametrize("name", fc.NAMES)
def test_walk_of_every_read(engine_cls, orc, name):
    same(run(engine_cls, name, ("k3_hits", 0))[0], oracle_fragmat(name)[0], name)


@pytest.mark.parametrize("name", ONT)
def test_tile_histograms(engine_cls, orc, name):
    same(run(engine_cls, name, ("hist_tiles", 1))[0], oracle_fragmat(name)[0], name)


def check_import(engine_cls, orc, name, sites):
    b, prm = fc.batch(name), fc.params(name)
    pos0, gt, qual = sites
    recs = expected_import(orc, b, prm, pos0, gt, qual)
    E = engine_cls(0, prm)
    E.load_batch(b).fill_data_into_freq_vec().import_external_candidates(pos0, gt, qual)
    cands, off = E.candidates()
    check_records(cands, off, recs, b.n_regions)
    off = off.copy()
    E.get_fragments()
    fm = {k: v.copy() for k, v in E.fragmat().items()}
    E.close()
    want = {k: [] for k in FIELDS}
    want["row_region_off"], want["row_ptr"] = [0], [0]
    for g in range(b.n_regions):
        rows = np_rows(b, g, prm, recs[int(off[g]):int(off[g + 1])]) if off[g + 1] > off[g] else []
        for read, cols, vals, links, fp in rows:
            want["row_read"].append(read); want["col"] += [c + int(off[g]) for c in cols]; want["val"] += vals
            want["row_links"].append(links); want["row_for_phasing"].append(fp); want["row_ptr"].append(len(want["col"]))
        want["row_region_off"].append(len(want["row_read"]))
    same(fm, {k: np.array(want[k], fm[k].dtype) for k in FIELDS}, "%s, import of %d sites" % (name, pos0.size))
    return fm


@pytest.mark.parametrize("name", fc.NAMES)
def test_import_of_the_case_s_own_candidates(engine_cls, orc, name):
    b, prm = fc.batch(name), fc.params(name)
    E = engine_cls(0, prm)
    E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps()
    sites = sites_of(E.candidates()[0])
    E.close()
    fm = check_import(engine_cls, orc, name, sites)
    if name == "rows16_dense":          # no dense flags on imported records: the five sites of the cluster are entries now
        assert np.diff(fm["row_ptr"]).max() == 34 + 5


@pytest.mark.parametrize("name", WITH_SITES)
def test_import_of_the_case_s_site_list(engine_cls, orc, name):
    sites = fc.BY_NAME[name]["sites"]()
    fm = check_import(engine_cls, orc, name, sites)
    assert np.diff(fm["row_ptr"]).max() == sites[0].size


@pytest.mark.parametrize("switch", [None, ("k3_hits", 0)], ids=["hits", "walk"])
def test_rows16_as_a_second_batch(engine_cls, orc, switch):
    """behind a batch with a hundred times the reads (regions_1030: 6 180): the hit slots, the overflow list and the provisional row slots of the first batch are
    still in the context's buffers, and nothing of them may be read"""
    E = engine_cls(0, fc.params("regions_1030"))
    if switch:
        E.debug_set(*switch)
    same(fragmat_of(E, fc.batch("regions_1030")), oracle_fragmat("regions_1030")[0], "regions_1030")
    for name in ("rows16_baseq", "rows16_dense", "reads_17"):
        E.params = fc.params(name)
        assert fc.batch(name).n_reads * 100 < fc.batch("regions_1030").n_reads + 100
        same(fragmat_of(E, fc.batch(name)), oracle_fragmat(name)[0], "%s behind regions_1030" % name)
    E.close()


@pytest.mark.parametrize("name", ["rows16_baseq", "rules_ml2", "geometry", "regions_mixed"])
def test_phase_of_a_family(engine_cls, orc, name):
    """one case of each family through phase() under test_gpu_parity.full_check's bars"""
    par.full_check(engine_cls, orc, fc.batch(name), fc.params(name))

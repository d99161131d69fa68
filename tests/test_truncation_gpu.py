"""lcr_discover_regions_truncated on the GPU against the loop restatement of util.rs:236-332 (tests/truncation_ref.py): regions and
the count of columns above the cap, at the smallest shapes at which the kernels can go wrong.  (The prefix scan under them has size
limits of its own, at windows of hundreds of thousands and of millions of columns: tests/test_scan_regime_cases_gpu.py.  The depth
builders of this file live in tests/scan_regime_cases.py, where the CPU test of the windowed reference shares them.)"""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import truncation_ref as tr
from longcallr_amd import _abi, bamio
from scan_regime_cases import HAND_BUILT, TRUNC_CAP as CAP, depth_to_spans, hand_built, random_case, tiny_islands

pytestmark = pytest.mark.gpu

DEMO_LEN = 64444167


def arrays(spans):
    return (np.array([s for s, _ in spans], dtype=np.int32), np.array([e for _, e in spans], dtype=np.int32))


def region_list(o):
    def view(ptr, dtype):
        return np.frombuffer((C.c_char * (np.dtype(dtype).itemsize * o.n_regions)).from_address(ptr), dtype=dtype).tolist()
    return list(zip(view(o.start0, np.int64), view(o.len, np.int32), view(o.max_cov, np.uint32))) if o.n_regions else []


def plain(E, spans, contig_len):
    """lcr_discover_regions itself (the entry without the cap)"""
    rs, re_ = arrays(spans)
    o = _abi.LcrRegionList()
    assert E.lib.lcr_discover_regions(E.h, _abi.LCR_MEM_HOST, int(rs.size), rs.ctypes.data, re_.ctypes.data, contig_len, C.byref(o)) == 0
    return region_list(o)


def check(E, spans, contig_len, cap):
    """the truncated call == the restatement, regions and count; returns both"""
    rs, re_ = arrays(spans)
    want, want_n = tr.discover(spans, contig_len, True, cap)
    got = E.discover_regions(rs, re_, contig_len, truncation=True, truncation_coverage=cap)
    assert got == want, cap
    assert E.last_truncated_columns == want_n, cap
    return want, want_n


def check_off(E, spans, contig_len, max_depth):
    """truncation off at any cap, and a cap no column exceeds: lcr_discover_regions"""
    rs, re_ = arrays(spans)
    base = plain(E, spans, contig_len)
    assert base == tr.discover(spans, contig_len)[0]
    for cap in (0, 1, CAP, 200000):
        assert E.discover_regions(rs, re_, contig_len, truncation=False, truncation_coverage=cap) == base
        assert E.last_truncated_columns == 0
    for cap in (max_depth, max_depth + 1, (1 << 32) - 1):
        assert E.discover_regions(rs, re_, contig_len, truncation=True, truncation_coverage=cap) == base
        assert E.last_truncated_columns == 0
    assert E.discover_regions(rs, re_, contig_len) == base


@pytest.mark.parametrize("variant,tail", HAND_BUILT)
def test_hand_built_spans(engine_cls, variant, tail):
    d, L = hand_built(variant, tail)
    assert 3200 - 1100 >= 2049
    spans = depth_to_spans(d)
    E = engine_cls(0, _abi.make_params())
    want, n = check(E, spans, L, CAP)
    assert n == int((d > CAP).sum()) > 2049
    assert want[0] == (10, 10, 5) and want[1] == (22, 28, 6)      # the stretch in front; the pending column + three maxima in one region
    assert (3207, 100, 8) in want                                  # the maximum of the middle block of the stretch in front
    assert (want[-1] == (4000, 96, 4)) == (tail == "island") and (want[-1] == (3900, 100, 6)) == (tail == "deep")
    check_off(E, spans, L, int(d.max()))
    E.close()


def test_degenerate_cases(engine_cls):
    d, L = hand_built(0, "deep")
    spans = depth_to_spans(d)
    rs, re_ = arrays(spans)
    E = engine_cls(0, _abi.make_params())
    assert E.discover_regions(rs, re_, L, truncation=True, truncation_coverage=0) == [] == tr.discover(spans, L, True, 0)[0]
    assert E.last_truncated_columns == int((d > 0).sum())          # every covered column
    for on in (False, True):
        assert E.discover_regions([], [], 1000, truncation=on, truncation_coverage=CAP) == [] and E.last_truncated_columns == 0
        assert E.discover_regions([0], [10], 0, truncation=on, truncation_coverage=CAP) == [] and E.last_truncated_columns == 0
    assert E.discover_regions([0], [10], 10, truncation=True, truncation_coverage=1) == [(0, 10, 1)]
    with pytest.raises(ValueError):
        E.discover_regions([0], [10], 10, truncation=True, truncation_coverage=1 << 32)
    E.close()


def test_many_tiny_islands(engine_cls):
    """depth alternating around the cap every one or two columns over 6000 columns: more islands than a block has threads, islands of
    one column next to each other, every thread's four columns holding several runs"""
    d, L, n_isl = tiny_islands()
    assert n_isl > 1024
    spans = depth_to_spans(d)
    E = engine_cls(0, _abi.make_params())
    want, n = check(E, spans, L, CAP)
    assert len(want) > 256 and n > 1024
    check(E, spans, L, CAP + 1)
    check_off(E, spans, L, int(d.max()))
    E.close()


def covered_depths(spans, L):
    diff = np.zeros(L + 1, dtype=np.int64)
    for s, e in spans:
        diff[s] += 1
        diff[min(e, L)] -= 1
    depth = np.cumsum(diff[:-1])
    return depth[depth > 0]


def test_random_spans(engine_cls):
    spans, L = random_case()
    cd = covered_depths(spans, L)
    E = engine_cls(0, _abi.make_params())
    results = [check(E, spans, L, cap) for cap in (1, 2, int(np.median(cd)), int(cd.max()) - 1)]
    assert results[0][1] > 0 and results[-1][1] > 0 and results[0][0] != results[-1][0]
    check_off(E, spans, L, int(cd.max()))
    E.close()


def test_device_spans(engine_cls):
    """the spans as LCR_MEM_DEVICE pointers give the answer of the host-pointer call"""
    import torch
    d, L = hand_built(1, "island")
    spans = depth_to_spans(d)
    rs, re_ = arrays(spans)
    E = engine_cls(0, _abi.make_params())
    want, want_n = check(E, spans, L, CAP)
    t_s, t_e = torch.from_numpy(rs).to("cuda:0"), torch.from_numpy(re_).to("cuda:0")
    torch.cuda.synchronize()
    for on, cap, w, wn in ((1, CAP, want, want_n), (0, CAP, plain(E, spans, L), 0)):
        o, nt = _abi.LcrRegionList(), C.c_int64(-1)
        rc = E.lib.lcr_discover_regions_truncated(E.h, _abi.LCR_MEM_DEVICE, int(rs.size), t_s.data_ptr(), t_e.data_ptr(), L, on, cap,
                                                  C.byref(o), C.byref(nt))
        assert rc == 0
        assert region_list(o) == w and nt.value == wn
    o = _abi.LcrRegionList()     # n_truncated may be NULL
    assert E.lib.lcr_discover_regions_truncated(E.h, _abi.LCR_MEM_DEVICE, int(rs.size), t_s.data_ptr(), t_e.data_ptr(), L, 1, CAP, C.byref(o), None) == 0
    assert region_list(o) == want
    E.close()


def test_demo_bam(engine_cls):
    nb = bamio.NativeBam(os.path.join(helpers.GOLDEN, "demo.bam"), 4)
    rid = [n for n, _ in nb.refs].index("chr20")
    rs, re_ = nb.spans(rid, **_abi.READ_FILTER)
    spans = list(zip(rs.tolist(), re_.tolist()))
    E = engine_cls(0, _abi.make_params())
    for cap, want in ((1648, [(16729960, 6413, 1649), (16736485, 6731, 1649)]), (1200, [(16729960, 81, 1296), (16741210, 2006, 1649)])):
        assert E.discover_regions(rs, re_, DEMO_LEN, truncation=True, truncation_coverage=cap) == want
        assert E.last_truncated_columns == tr.discover(spans, DEMO_LEN, True, cap)[1] > 0
    assert E.discover_regions(rs, re_, DEMO_LEN, truncation=False, truncation_coverage=1200) == [(16729960, 13256, 1649)]
    E.close()
    nb.close()

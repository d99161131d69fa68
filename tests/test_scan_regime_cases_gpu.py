"""Region discovery on windows large enough to leave the depth scan's first size regime (launch_scan_i32, csrc/k2_candidates.hip):
fused with one stride of the block-sum loop, fused with several, and the three-phase path with its rounds of 1024 block sums.
The cases and their reference are tests/scan_regime_cases.py and truncation_ref.discover_np; tests/test_scan_regime_cases.py checks
both on the CPU, and that a block carry lost at any of the cases' borders would change the expected regions."""
import ctypes as C

import numpy as np
import pytest

import helpers
import scan_regime_cases as sc
from longcallr_amd import _abi

pytestmark = pytest.mark.gpu


def arrays(name):
    spans, contig_len, _ = sc.built(name)
    a = np.asarray(spans, dtype=np.int64)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), contig_len


def region_list(o):
    def view(ptr, dtype):
        return np.frombuffer((C.c_char * (np.dtype(dtype).itemsize * o.n_regions)).from_address(ptr), dtype=dtype).tolist()
    return list(zip(view(o.start0, np.int64), view(o.len, np.int32), view(o.max_cov, np.uint32))) if o.n_regions else []


def capped(E, name, cap):
    """the truncated call == the windowed reference, regions and count; returns the regions"""
    rs, re_, contig_len = arrays(name)
    want, want_n = sc.expected(name, cap)
    got = E.discover_regions(rs, re_, contig_len, truncation=True, truncation_coverage=cap)
    assert got == want, (name, cap)
    assert E.last_truncated_columns == want_n, (name, cap)
    return got


def check(E, name):
    """cap 2, the cap no column exceeds, truncation off and the entry without a cap; returns what the calls gave"""
    rs, re_, contig_len = arrays(name)
    want = sc.expected(name)[0]
    cut = capped(E, name, sc.CAP)
    assert capped(E, name, sc.max_depth(name)) == want
    o = _abi.LcrRegionList()
    assert E.lib.lcr_discover_regions(E.h, _abi.LCR_MEM_HOST, int(rs.size), rs.ctypes.data, re_.ctypes.data, contig_len, C.byref(o)) == 0
    assert region_list(o) == want, name
    for cap in (0, 1, sc.CAP, 200000):
        assert E.discover_regions(rs, re_, contig_len, truncation=False, truncation_coverage=cap) == want, (name, cap)
        assert E.last_truncated_columns == 0
    return cut, want


@pytest.mark.parametrize("name", sc.NAMES)
def test_regime(engine_cls, name):
    E = engine_cls(0, _abi.make_params())
    cut, off = check(E, name)
    assert cut != off
    E.close()


@pytest.mark.parametrize("name", ["three_first", "fused_257"])
def test_device_spans(engine_cls, name):
    """the spans as LCR_MEM_DEVICE pointers (the window comes from a reduction on the device) give the same lists"""
    import torch
    rs, re_, contig_len = arrays(name)
    E = engine_cls(0, _abi.make_params())
    t_s, t_e = torch.from_numpy(rs).to("cuda:0"), torch.from_numpy(re_).to("cuda:0")
    torch.cuda.synchronize()
    for on, cap in ((1, sc.CAP), (1, sc.max_depth(name)), (0, sc.CAP)):
        want, want_n = sc.expected(name, cap if on and cap == sc.CAP else None)
        o, nt = _abi.LcrRegionList(), C.c_int64(-1)
        rc = E.lib.lcr_discover_regions_truncated(E.h, _abi.LCR_MEM_DEVICE, int(rs.size), t_s.data_ptr(), t_e.data_ptr(), contig_len, on, cap,
                                                  C.byref(o), C.byref(nt))
        assert rc == 0
        assert region_list(o) == want and nt.value == want_n, (name, on, cap)
        if on:
            assert E.discover_regions(rs, re_, contig_len, truncation=True, truncation_coverage=cap) == want
    E.close()


def stage_bytes(E):
    c, off = E.candidates()
    pr = E.phase_result()
    fm = E.fragmat()
    return (c.tobytes(), off.tobytes()) + tuple(pr[k].tobytes() for k in ("haplotag", "assignment", "phase_set", "objective")) \
        + tuple(fm[k].tobytes() for k in sorted(fm))


def test_reentry_across_regimes(engine_cls):
    """one context: the scan's block sums are a buffer that grows and is reused, and the regimes leave different things in it.  Then the
    stages on the demo batch: a chromosome-sized discovery in front of them changes none of their bytes."""
    prm = _abi.make_params("hifi-masseq")
    E = engine_cls(0, prm)
    seen = [check(E, name) for name in ("three_3073", "tile_exact", "fused_last", "three_3073")]
    assert seen[0] == seen[3] and seen[0] != seen[2]
    b = helpers.demo_batch()
    E.load_batch(b).run_all()
    got = stage_bytes(E)
    E.close()
    F = engine_cls(0, prm)
    F.load_batch(b).run_all()
    want = stage_bytes(F)
    F.close()
    assert len(want[0]) > 0 and got == want


def test_contig_length_limit(engine_cls):
    """0x7FFFFFF0 is the largest contig_len the entry takes (the cases three_first_high and three_first_end run at it); one more is
    LCR_E_ARG in front of any work: the output is not written and the context answers the next call as if nothing had been asked"""
    rs, re_, contig_len = arrays("tile_plus1")
    assert sc.built("three_first_end")[1] == sc.MAX_CONTIG == 0x7FFFFFF0
    E = engine_cls(0, _abi.make_params())
    for on in (0, 1):
        o, nt = _abi.LcrRegionList(), C.c_int64(-7)
        rc = E.lib.lcr_discover_regions_truncated(E.h, _abi.LCR_MEM_HOST, int(rs.size), rs.ctypes.data, re_.ctypes.data, sc.MAX_CONTIG + 1, on, sc.CAP,
                                                  C.byref(o), C.byref(nt))
        assert rc == -1                                            # LCR_E_ARG
        assert o.n_regions == 0 and not o.start0 and not o.len and not o.max_cov and nt.value == -7
    o = _abi.LcrRegionList()
    assert E.lib.lcr_discover_regions(E.h, _abi.LCR_MEM_HOST, int(rs.size), rs.ctypes.data, re_.ctypes.data, sc.MAX_CONTIG + 1, C.byref(o)) == -1
    assert o.n_regions == 0 and not o.start0
    # the same spans on a contig of the largest length: only contig_len differs, and the answer is tile_plus1's
    assert E.discover_regions(rs, re_, sc.MAX_CONTIG, truncation=True, truncation_coverage=sc.CAP) == sc.expected("tile_plus1", sc.CAP)[0]
    E.close()

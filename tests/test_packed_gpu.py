"""Packed batches on the GPU (-m gpu): the unpack kernel alone through Engine.unpack_bases against a base-by-base numpy expansion, with a
sentinel everywhere it must not write -- lane, round and loop boundaries, every output / source alignment, all 16 codes, permuted
layouts, the guard --; then the three packed load paths against load_batch of the plain batch on a second context, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import helpers
import packed_ref as pr
from longcallr_amd import _abi, _lib, bamio, synth
from longcallr_amd._lib import LcrError

pytestmark = pytest.mark.gpu

SENTINEL = 0xEE


# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def unpack_on_gpu(E, seq_len, seq_off, pack_off, seq4, n_bases):
    """(LcrError or None, the output array) of Engine.unpack_bases over a sentinel-filled output"""
    import torch
    out = torch.full((n_bases,), SENTINEL, dtype=torch.uint8, device="cuda")
    ts = (dev(np.asarray(seq_len, np.int32)), dev(np.asarray(seq_off, np.int64)), dev(np.asarray(pack_off, np.int64)), dev(np.asarray(seq4, np.uint8)))
    assert all(t.data_ptr() % 16 == 0 for t in ts + (out,))       # offsets' residues are the addresses' residues
    err = None
    try:
        E.unpack_bases(*ts, out)
    except LcrError as e:
        err = e
    torch.cuda.synchronize()
    return err, out.cpu().numpy()


def check(E, lengths, seq_off, pack_off, n_bases, n_pack, seed=0, fill=0x5A):
    """random codes of the given lengths at the given offsets: the kernel's output is the numpy expansion, the sentinel everywhere else"""
    rng = np.random.default_rng(seed)
    codes = [rng.integers(0, 16, size=l, dtype=np.uint8) for l in lengths]
    seq4 = pr.pack_into(codes, pack_off, n_pack, fill)
    lengths, seq_off, pack_off = np.asarray(lengths, np.int32), np.asarray(seq_off, np.int64), np.asarray(pack_off, np.int64)
    want = pr.expand(seq4, pack_off, seq_off, lengths, np.full(n_bases, SENTINEL, np.uint8))
    err, got = unpack_on_gpu(E, lengths, seq_off, pack_off, seq4, n_bases)
    assert err is None, err
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    inside = np.zeros(n_bases, bool)
    for so, l in zip(seq_off.tolist(), lengths.tolist()):
        inside[so:so + l] = True
    assert np.all(got[~inside] == SENTINEL)       # (implied by got == want; said once more on its own)
    return got


def lay_out(lengths, gap_b=lambda k: 1 + k % 17, gap_p=lambda k: 1 + (5 * k) % 17):
    """offsets with 1- to 17-byte gaps in both arrays -> seq_off, pack_off, n_bases, n_pack"""
    so, po, seq_off, pack_off = 3, 1, [], []
    for k, l in enumerate(lengths):
        seq_off.append(so); pack_off.append(po)
        so += l + gap_b(k); po += (l + 1) // 2 + gap_p(k)
    return seq_off, pack_off, so + 5, po + 2


def test_lengths_across_lane_round_and_loop_boundaries(engine_cls):
    E = engine_cls(0)
    lengths = [0, 1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 1023, 1024, 1025, 2049]
    check(E, lengths, *lay_out(lengths), seed=1)
    # the same reads back to back from offset 0 of both arrays, up to the arrays' last bytes (the kernel's dword window at both edges of seq4)
    seq_off = np.cumsum([0] + lengths[:-1]); pack_off = np.cumsum([0] + [(l + 1) // 2 for l in lengths[:-1]])
    check(E, lengths, seq_off, pack_off, int(sum(lengths)), int(sum((l + 1) // 2 for l in lengths)), seed=2)
    E.close()


def test_every_output_and_source_alignment(engine_cls):
    """16 residues of seq_off mod 16 x 4 residues of pack_off mod 4 x both length parities at length 40: 128 reads in one launch"""
    E = engine_cls(0)
    lengths, seq_off, pack_off, so, po, k = [], [], [], 1, 1, 0
    for par in (0, 1):
        for rb in range(16):
            for rp in range(4):
                l = 40 + par
                so += 1 + (k % 2)
                so += (rb - so) % 16
                po += 1 + (k % 3) + 4 * (k % 3)
                po += (rp - po) % 4
                assert so % 16 == rb and po % 4 == rp
                lengths.append(l); seq_off.append(so); pack_off.append(po)
                so += l; po += (l + 1) // 2
                k += 1
    gaps_b = np.diff(seq_off) - np.array(lengths[:-1]); gaps_p = np.diff(pack_off) - (np.array(lengths[:-1]) + 1) // 2
    assert len(lengths) == 128 and 1 <= gaps_b.min() and gaps_b.max() <= 17 and 1 <= gaps_p.min() and gaps_p.max() <= 17
    check(E, lengths, seq_off, pack_off, so + 3, po + 1, seed=3)
    E.close()


def test_all_sixteen_codes_and_a_dangling_nibble(engine_cls):
    E = engine_cls(0)
    codes = [np.arange(16, dtype=np.uint8), np.arange(15, -1, -1, dtype=np.uint8)[:15], np.tile(np.arange(16, dtype=np.uint8), 5)[3:]]   # 16, 15 (odd), 77 bases
    seq_off, pack_off, n_bases, n_pack = lay_out([c.size for c in codes])
    for fill in (0xFF, 0x07):
        seq4 = pr.pack_into(codes, pack_off, n_pack, fill)
        assert seq4[pack_off[1] + 7] & 15 == fill & 15 != 0                 # the low nibble behind the odd-length read is not zero
        err, got = unpack_on_gpu(E, [c.size for c in codes], seq_off, pack_off, seq4, n_bases)
        assert err is None
        want = np.full(n_bases, SENTINEL, np.uint8)
        for c, so in zip(codes, seq_off):
            want[so:so + c.size] = pr.NT16[c]
        assert np.array_equal(got, want)
        assert bytes(got[seq_off[0]:seq_off[0] + 16]) == b"=ACMGRSVTWYHKDBN"
    E.close()


def test_permuted_layouts_and_no_reads(engine_cls):
    E = engine_cls(0)
    lengths = [5, 130, 17, 64, 33, 1, 250, 16, 48, 9, 1100, 31]
    rng = np.random.default_rng(4)
    order_b, order_p = rng.permutation(len(lengths)), rng.permutation(len(lengths))      # the reads lie in one order in bases, in another in seq4
    seq_off, pack_off, so, po = [0] * len(lengths), [0] * len(lengths), 2, 3
    for k in range(len(lengths)):
        i, j = int(order_b[k]), int(order_p[k])
        seq_off[i], pack_off[j] = so, po
        so += lengths[i] + 1 + k % 17
        po += (lengths[j] + 1) // 2 + 1 + (7 * k) % 17
    assert seq_off != sorted(seq_off) and pack_off != sorted(pack_off) and list(np.argsort(seq_off)) != list(np.argsort(pack_off))
    check(E, lengths, seq_off, pack_off, so + 4, po + 1, seed=5)
    err, got = unpack_on_gpu(E, [], [], [], np.zeros(7, np.uint8), 64)      # n_reads == 0: no launch
    assert err is None and np.all(got == SENTINEL)
    E.close()


@pytest.mark.parametrize("what", ["output range", "source range", "negative length", "offset beyond 2^63"])
def test_the_guard_skips_a_violating_read(engine_cls, what):
    """one bad read in ten: LCR_E_ARG, that read untouched, nothing outside the other nine reads' ranges written"""
    E = engine_cls(0)
    lengths = [40, 17, 64, 33, 5, 100, 16, 1, 250, 31]
    seq_off, pack_off, n_bases, n_pack = lay_out(lengths)
    rng = np.random.default_rng(6)
    seq4 = pr.pack_into([rng.integers(0, 16, size=l, dtype=np.uint8) for l in lengths], pack_off, n_pack, 0x5A)
    L, so, po = np.array(lengths, np.int64), np.array(seq_off, np.int64), np.array(pack_off, np.int64)
    good = np.arange(10) != 5
    want = pr.expand(seq4, po[good], so[good], L[good], np.full(n_bases, SENTINEL, np.uint8))
    if what == "output range":
        so[5] = n_bases - L[5] + 1
    elif what == "source range":
        po[5] = n_pack - (L[5] + 1) // 2 + 1
    elif what == "negative length":
        L[5] = -3
    else:
        po[5] = -1          # 2^64 - 1 as the kernel reads it: the sums must not wrap
    err, got = unpack_on_gpu(E, L, so, po, seq4, n_bases)
    assert err is not None and "(-1)" in str(err) and "lcr_unpack_bases" in str(err)
    assert np.array_equal(got, want)
    assert np.all(got[seq_off[5]:seq_off[5] + lengths[5]] == SENTINEL)
    err, got = unpack_on_gpu(E, lengths, seq_off, pack_off, seq4, n_bases)      # the context is as good as before: the same reads, intact
    assert err is None and np.array_equal(got, pr.expand(seq4, np.array(pack_off), np.array(seq_off), np.array(lengths), np.full(n_bases, SENTINEL, np.uint8)))
    E.close()


def test_unpack_time_is_reported_only_with_timing(engine_cls):
    E = engine_cls(0)
    ms = C.c_float()
    assert E.lib.lcr_unpack_ms(E.h, C.byref(ms)) == -4
    E.close()
    E = engine_cls(0, timing=True)
    assert E.lib.lcr_unpack_ms(E.h, C.byref(ms)) == -4
    lengths = [100, 33]
    check(E, lengths, *lay_out(lengths))
    assert 0 < E.unpack_ms() < 1000
    E.close()


# ---- 2. the load paths ----------------------------------------------------------------------------------------------------------------------
def snapshot(E):
    """everything the stages leave, as bytes: planes, candidates, fragment matrix, phase results, read records"""
    E.run_all()
    out = dict(planes=E.columns().tobytes())
    c, off = E.candidates()
    out.update(cand=c.tobytes(), cand_off=off.tobytes())
    out.update({"fm_" + k: v.tobytes() for k, v in E.fragmat().items()})
    out.update({"ph_" + k: v.tobytes() for k, v in E.phase_result().items()})
    ptr, n = E.read_records_device()
    rec = np.zeros(n, dtype=_abi.READ_REC_DTYPE)
    E.sync()
    if n:
        hip = _lib.load()       # (the HIP runtime is among the library's dependencies: its symbols resolve through the handle)
        assert hip.hipMemcpy(C.c_void_p(rec.ctypes.data), C.c_void_p(ptr), C.c_size_t(rec.nbytes), 2) == 0
    out["read_rec"] = rec.tobytes()
    assert n == len(out["ph_haplotag"]) and len(out["cand"]) > 0
    return out


def demo_native():
    b = helpers.demo_batch()
    refs, recs = bamio.read_bam(helpers.GOLDEN + "/demo.bam")
    rid = next(r["ref_id"] for r in recs if bamio.passes_filter(r, **_abi.READ_FILTER))
    nb = bamio.NativeBam(helpers.GOLDEN + "/demo.bam", 2)
    regions = [(int(b.start0[0]), int(b.len[0]))]
    plain = nb.batch(rid, regions, [b.ref], **_abi.READ_FILTER)
    packed = nb.batch(rid, regions, [b.ref], packed=True, **_abi.READ_FILTER)
    nb.close()
    return plain, packed


BATCHES = {}


def batch_of(name):
    """(preset, plain batch, packed batch, snapshot of load_batch(plain) on a context of its own) -- computed once per module"""
    if name not in BATCHES:
        from longcallr_amd import api
        if name == "demo":
            preset, (plain, packed) = "hifi-masseq", demo_native()
        else:
            preset = "ont-cdna" if name == "ont-cdna" else "hifi-masseq"
            plain = synth.make_batch(name, n_genes=2)
            packed = plain.pack()
        E = api.Engine(0, _abi.make_params(preset))
        E.load_batch(plain)
        BATCHES[name] = (preset, plain, packed, snapshot(E))
        E.close()
    return BATCHES[name]


def same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], k


def to_device_packed(p):
    """a PackedReadBatch as torch tensors -> the (LcrReadsPacked, LcrRegions, keepalive) triple of Engine.load_batch"""
    import torch
    t = {f: dev(getattr(p, f)) for f in p.FIELDS + ["start0", "len", "col_off", "read_begin", "ref"]}
    torch.cuda.synchronize()
    reads, regions = p.c_reads(), p.c_regions()
    reads.mem = regions.mem = _abi.LCR_MEM_DEVICE
    for f in p.FIELDS:
        setattr(reads, f, C.c_void_p(t[f].data_ptr()))
    for f in ["start0", "len", "col_off", "read_begin", "ref"]:
        setattr(regions, f, C.c_void_p(t[f].data_ptr()))
    return reads, regions, t


@pytest.mark.parametrize("form", ["host", "device", "async"])
@pytest.mark.parametrize("name", ["ont-cdna", "masseq", "demo"])
def test_packed_load_is_the_plain_load(engine_cls, name, form):
    preset, plain, packed, want = batch_of(name)
    assert packed.n_bases == plain.bases.size and packed.n_pack < plain.bases.size
    E = engine_cls(0, _abi.make_params(preset))
    if form == "host":
        E.load_batch(packed)
    elif form == "device":
        E.load_batch(to_device_packed(packed))
    else:
        E.load_batch_async(packed, 1).bind_batch(1)
    same(snapshot(E), want)
    if form != "async":      # and once more on the same context: the second load writes the buffers the first one's stages read
        E.load_batch(packed if form == "host" else to_device_packed(packed))
        same(snapshot(E), want)
    E.close()


def test_plain_and_packed_batches_alternate_on_the_two_slots(engine_cls):
    pa, plain_a, packed_a, want_a = batch_of("ont-cdna")
    E = engine_cls(0, _abi.make_params(pa))
    plain_b = synth.make_batch("ont-cdna", n_genes=1, seed=9)
    Eb = engine_cls(0, _abi.make_params(pa))
    Eb.load_batch(plain_b)
    want_b = snapshot(Eb)
    Eb.close()
    steps = [(packed_a, want_a), (plain_b, want_b), (plain_a, want_a), (plain_b.pack(), want_b)]
    E.load_batch_async(steps[0][0], 0)
    for k, (_, want) in enumerate(steps):
        E.bind_batch(k & 1)
        if k + 1 < len(steps):
            E.load_batch_async(steps[k + 1][0], (k + 1) & 1)
        same(snapshot(E), want)
    E.close()


def test_packed_load_beside_an_asynchronous_phase_stage(engine_cls):
    pa, plain_a, packed_a, want_a = batch_of("ont-cdna")
    E = engine_cls(0, _abi.make_params(pa)).set_async_phase(True)
    E.load_batch_async(plain_a, 0).bind_batch(0).run_all()                # batch 1's phase stage is in flight ...
    E.load_batch_async(packed_a, 1).bind_batch(1)                          # ... while the packed batch is uploaded, unpacked and bound
    E.fill_data_into_freq_vec()
    res = E.collect_phase(copy=True)                                       # batch 1's results, collected behind batch 2's pileup
    assert res["cand"].tobytes() == want_a["cand"] and res["haplotag"].tobytes() == want_a["ph_haplotag"]
    assert res["assignment"].tobytes() == want_a["ph_assignment"] and res["phase_set"].tobytes() == want_a["ph_phase_set"]
    E.get_candidate_snps().get_fragments().phase()
    res = E.collect_phase(copy=True)
    assert res["cand"].tobytes() == want_a["cand"] and res["haplotag"].tobytes() == want_a["ph_haplotag"]
    E.load_batch_async(packed_a, 1)                                        # into the slot whose batch is bound, its stage possibly in flight
    E.bind_batch(1)
    same(snapshot(E), want_a)
    dv = to_device_packed(packed_a)                                        # the device form has ONE buffer for the unpacked bases: the second load
    E.load_batch(dv).run_all()                                             # waits for the first one's stage before it unpacks over them
    E.load_batch(dv)
    res = E.collect_phase(copy=True)
    assert res["cand"].tobytes() == want_a["cand"] and res["phase_set"].tobytes() == want_a["ph_phase_set"]
    same(snapshot(E), want_a)
    E.close()


def test_a_refused_host_batch_leaves_the_bound_batch_alone(engine_cls):
    pa, plain_a, packed_a, want_a = batch_of("ont-cdna")
    E = engine_cls(0, _abi.make_params(pa))
    E.load_batch(packed_a)
    got = snapshot(E)
    bad = packed_a.pack_off.copy()
    bad[3] = packed_a.n_pack - 1                                            # read 3 would read past seq4's end
    kw = {f: getattr(packed_a, f) for f in packed_a.FIELDS if f != "pack_off"}
    refused = _abi.PackedReadBatch(pack_off=bad, start0=packed_a.start0, len=packed_a.len, read_begin=packed_a.read_begin, ref=packed_a.ref, **kw)
    for call in (lambda: E.load_batch(refused), lambda: E.load_batch_async(refused, 0)):
        with pytest.raises(LcrError, match=r"\(-1\).*read 3 "):
            call()
        c, off = E.candidates()                                            # the getters of the batch bound before still answer
        assert c.tobytes() == want_a["cand"] and E.columns().tobytes() == want_a["planes"]
        assert E.phase_result()["haplotag"].tobytes() == want_a["ph_haplotag"]
    neg = packed_a.c_reads()
    neg.n_pack = -1
    assert E.lib.lcr_load_batch_packed(E.h, C.byref(neg), C.byref(packed_a.c_regions())) == -1
    assert E.candidates()[0].tobytes() == want_a["cand"]
    same(got, want_a)
    E.close()

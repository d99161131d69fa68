"""Packed batches on the host (no GPU): lcr_bam_batch_packed against lcr_bam_batch on demo.bam and on a hand-built file, ReadBatch.pack /
PackedReadBatch.unpack, the decoder pair once more in a stand-alone program under the host sanitizers, and the struct's layout."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers
import packed_ref as pr
from longcallr_amd import _abi, _lib, bamio, build, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(helpers.GOLDEN, "demo.bam")


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build()
    return _lib.load()


def demo_regions():
    """demo.bam's coverage islands under the presets' read filter: (ref_id, [(start0, len)])"""
    refs, recs = bamio.read_bam(DEMO)
    keep = [r for r in recs if bamio.passes_filter(r, **_abi.READ_FILTER)]
    rid = keep[0]["ref_id"]
    return rid, [(s, l) for s, l, _ in bamio.discover_regions(keep, rid, refs[rid][1])]


def same_batch(plain, packed, name_format):
    """every array the two forms share is equal; the packed one's nibbles are the plain one's bases"""
    assert isinstance(packed, _abi.PackedReadBatch) and isinstance(plain, _abi.ReadBatch)
    for f in ("pos", "seq_len", "lead_clip", "trail_clip", "flags", "seq_off", "cig_off", "n_cig", "quals", "cigar", "read_begin", "start0", "len", "ref"):
        assert np.array_equal(getattr(plain, f), getattr(packed, f)), f
        assert getattr(plain, f).dtype == getattr(packed, f).dtype, f
    if name_format == "list":
        assert plain.names == packed.names and len(plain.names) == plain.n_reads
    else:
        assert np.array_equal(plain.name_off, packed.name_off) and np.array_equal(plain.name_blob, packed.name_blob)
    half = (plain.seq_len.astype(np.int64) + 1) // 2
    assert packed.n_pack == int(half.sum()) == packed.seq4.size
    assert np.array_equal(packed.pack_off.astype(np.int64), np.cumsum(half) - half)      # back to back
    assert packed.n_bases == plain.bases.size
    assert np.array_equal(packed.unpack().bases, plain.bases)
    assert np.array_equal(pr.expand(packed.seq4, packed.pack_off, packed.seq_off, packed.seq_len, np.zeros(packed.n_bases, np.uint8)), plain.bases)
    assert packed.upload_bytes_saved() == plain.bases.size - packed.n_pack - 8 * plain.n_reads


@pytest.mark.parametrize("name_format,copy", [("list", True), ("blob", False)])
def test_decoder_agreement_on_demo_bam(name_format, copy):
    rid, regions = demo_regions()
    assert regions
    wins = [np.full(l, ord("N"), np.uint8) for _, l in regions]
    nb = bamio.NativeBam(DEMO, 2)
    plain = nb.batch(rid, regions, wins, name_format=name_format, **_abi.READ_FILTER)       # (copies: the handle reuses its buffers)
    packed = nb.batch(rid, regions, wins, name_format=name_format, copy=copy, packed=True, **_abi.READ_FILTER)
    assert plain.n_reads > 100
    same_batch(plain, packed, name_format)
    nb.close()


def test_decoder_agreement_on_a_hand_built_file(tmp_path):
    path = tmp_path / "hand.bam"
    src = pr.write_hand_bam(path)
    wins = [src.ref[s:s + l] for s, l in pr.HAND_REGIONS]
    nb = bamio.NativeBam(str(path), 2)
    plain = nb.batch(0, pr.HAND_REGIONS, wins, **pr.HAND_FILTER)
    packed = nb.batch(0, pr.HAND_REGIONS, wins, packed=True, **pr.HAND_FILTER)
    nb.close()
    same_batch(plain, packed, "list")
    assert sorted(set(plain.seq_len.tolist())) == pr.HAND_LENGTHS
    assert set(plain.bases.tolist()) == set(pr.NT16.tolist())                               # all 16 letters came through the file
    rb = plain.read_begin
    twice = set(plain.names[rb[0]:rb[1]]) & set(plain.names[rb[1]:rb[2]])
    assert twice and plain.n_reads == len(pr.HAND_LENGTHS) + len(twice)                      # a read of both regions is listed in both
    first = {n: i for i, n in reversed(list(enumerate(plain.names)))}
    for i, n in enumerate(plain.names):                                                      # ... with the same bases both times, and the writer's
        j, k = first[n], int(n[1:])
        assert np.array_equal(plain.bases[int(plain.seq_off[i]):][:plain.seq_len[i]], plain.bases[int(plain.seq_off[j]):][:plain.seq_len[j]])
        assert np.array_equal(plain.bases[int(plain.seq_off[i]):][:plain.seq_len[i]], src.bases[int(src.seq_off[k]):][:src.seq_len[k]])


def test_pack_unpack_round_trip():
    b = synth.make_batch("ont-cdna", n_genes=1)
    p = b.pack()
    half = (b.seq_len.astype(np.int64) + 1) // 2
    assert p.n_pack == int(half.sum()) and np.array_equal(p.pack_off.astype(np.int64), np.cumsum(half) - half)
    assert np.array_equal(pr.expand(p.seq4, p.pack_off, p.seq_off, p.seq_len, np.zeros(p.n_bases, np.uint8)), b.bases)
    u = p.unpack()
    for f in _abi.ReadBatch.FIELDS + ["start0", "len", "read_begin", "ref", "col_off"]:
        assert np.array_equal(getattr(u, f), getattr(b, f)), f
    odd = np.flatnonzero(b.seq_len % 2 == 1)
    assert odd.size and not np.any(p.seq4[(p.pack_off[odd] + half[odd].astype(np.uint64) - np.uint64(1)).astype(np.int64)] & 15)   # the dangling nibble is 0
    r, c = p.c_reads(), p.c_regions()
    assert (r.mem, r.n_reads, r.n_bases, r.n_cigar, r.n_pack) == (_abi.LCR_MEM_HOST, b.n_reads, b.bases.size, b.cigar.size, p.seq4.size)
    assert r.seq4 == p.seq4.ctypes.data and r.pack_off == p.pack_off.ctypes.data and c.n_regions == b.n_regions
    # a hand-built batch with every letter and a gap in front of the second read
    h = pr.hand_batch()
    h2 = _abi.ReadBatch(**dict({f: getattr(h, f) for f in _abi.ReadBatch.FIELDS}, seq_off=h.seq_off + np.uint64(5), bases=np.concatenate([np.full(5, ord("A"), np.uint8), h.bases]),
                               quals=np.concatenate([np.zeros(5, np.uint8), h.quals]), start0=h.start0, len=h.len, read_begin=h.read_begin, ref=h.ref))
    u2 = h2.pack().unpack()
    assert np.array_equal(u2.bases[5:], h.bases) and not u2.bases[:5].any() and u2.bases.size == h2.bases.size


def test_pack_refuses_a_base_outside_the_sixteen_letters():
    b = helpers.mk_batch([dict(pos=0, seq="ACGTacgt", cigar="8M")], [(0, "ACGTACGTAC")])
    with pytest.raises(ValueError, match="=ACMGRSVTWYHKDBN"):
        b.pack()


def test_the_decoder_pair_stand_alone_under_sanitizers(tmp_path):
    """tests/packed_main.cpp + csrc/lcr_bam.cpp as one host program under ASan / UBSan: both calls on demo.bam and on the hand-built file"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "packed_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "packed_main.cpp"), os.path.join(ROOT, "longcallr_amd", "csrc", "lcr_bam.cpp"), "-o", exe, "-lz", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rid, regions = demo_regions()
    hand = tmp_path / "hand.bam"
    pr.write_hand_bam(hand)
    runs = [(DEMO, _abi.READ_FILTER["min_mapq"], _abi.READ_FILTER["min_read_length"], regions),
            (str(hand), 0, 0, pr.HAND_REGIONS)]
    for path, mapq, min_len, regs in runs:
        args = [exe, path, str(mapq), str(min_len), str(len(regs))] + [str(v) for s, l in regs for v in (s, l)]
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr


def test_packed_struct_layout_matches_the_header(tmp_path):
    fields = [f for f, _ in _abi.LcrReadsPacked._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include "lcr.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu\\n", sizeof(lcr_reads_packed));\n'
                   + "".join('printf("%%zu\\n", offsetof(lcr_reads_packed, %s));\n' % f for f in fields) + "return 0;}")
    exe = tmp_path / "sz"
    assert os.system("gcc -I%s %s -o %s" % (os.path.join(ROOT, "include"), src, exe)) == 0
    got = [int(x) for x in os.popen(str(exe)).read().split()]
    assert got == [C.sizeof(_abi.LcrReadsPacked)] + [getattr(_abi.LcrReadsPacked, f).offset for f in fields]
    assert {"lcr_load_batch_packed", "lcr_load_batch_packed_async", "lcr_unpack_bases", "lcr_bam_batch_packed"} <= set(_lib.SYMBOLS)
    lib = _lib.load()
    assert lib.lcr_load_batch_packed(None, None, None) == -1 and lib.lcr_load_batch_packed_async(None, None, None, 0) == -1      # LCR_E_ARG in front of anything
    assert lib.lcr_unpack_bases(None, 0, None, None, None, None, 0, None, 0) == -1 and lib.lcr_bam_batch_packed(None, 0, None, 0, None, None, None, None, None, None) == -1

"""Shared by the packed-batch tests: a base-by-base numpy expansion of BAM nibbles (the reference of the unpack kernel and of the host
producers), packing into arbitrary layouts, and the small hand-built BAM of the decoder tests."""
import numpy as np

from longcallr_amd import bamio
import helpers

NT16 = np.frombuffer(b"=ACMGRSVTWYHKDBN", dtype=np.uint8)
HAND_LENGTHS = [1, 2, 3, 15, 16, 17, 31, 32, 33]


def expand(seq4, pack_off, seq_off, seq_len, out):
    """write every read's bases into `out` (a copy is returned), one read and one base at a time: base i of a read is the high (even i)
    or low (odd i) nibble of seq4[pack_off + i // 2]"""
    out = out.copy()
    for po, so, ln in zip(pack_off.tolist(), seq_off.tolist(), seq_len.tolist()):
        i = np.arange(ln)
        b = seq4[po + i // 2]
        out[so:so + ln] = NT16[np.where(i % 2 == 0, b >> 4, b & 15)]
    return out


def pack_into(codes, pack_off, n_pack, fill=0):
    """seq4 of n_pack bytes (prefilled with `fill`, so the dangling low nibble of an odd read and the gaps are not zero) holding the
    reads' nibble codes (a list of arrays, values 0..15) at pack_off"""
    seq4 = np.full(n_pack, fill, dtype=np.uint8)
    for c, po in zip(codes, pack_off):
        c = np.asarray(c, dtype=np.uint8)
        n = (c.size + 1) // 2
        hi = c[0::2].astype(np.uint8)
        lo = np.full(n, fill & 15, dtype=np.uint8)
        lo[:c.size // 2] = c[1::2]
        seq4[po:po + n] = (hi << 4) | lo
    return seq4


def hand_batch():
    """reads of the lengths HAND_LENGTHS over one 200-column reference, every one of the 16 base letters present, sorted by position;
    regions (0, 100) and (50, 150) share the reads that cross column 50..100"""
    rng = np.random.default_rng(7)
    ref = "".join(rng.choice(list("ACGT"), size=200))
    reads = []
    for k, ln in enumerate(HAND_LENGTHS):
        seq = "".join(chr(NT16[(k + j) % 16]) for j in range(ln))
        reads.append(dict(pos=10 + 9 * k, seq=seq, qual=[(3 * k + j) % 41 for j in range(ln)], cigar="%dM" % ln, rev=k & 1, ts=k % 3, region=0))
    b = helpers.mk_batch(reads, [(0, ref)])
    assert set(b.bases.tolist()) == set(NT16.tolist())
    return b


HAND_REGIONS = [(0, 100), (50, 150)]
HAND_FILTER = dict(min_mapq=0, min_read_length=0, divergence=2.0)


def write_hand_bam(path):
    b = hand_batch()
    bamio.write_reads_bam(str(path), b, contig="chrH", contig_len=200)
    return b

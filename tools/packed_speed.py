#!/usr/bin/env python
"""What the packed input path costs and saves on the C3 batch: 400 synthetic ONT-cDNA genes written to a BAM and
read back, as bench.py's end_to_end_from_bam stage does.  Three measurements, all on the GPU (there is no fallback):

  1. the unpack kernel (k0_unpack) by HIP events, warm, three calls: ms, (n_pack + n_bases) / t, share of the 8 TB/s HBM peak;
  2. bench.py's host_fed asynchronous loop -- bind_batch(k & 1); load_batch_async(next, (k + 1) & 1); run_all() over page-locked arrays,
     eight steps -- with the plain and with the packed batch, interleaved in one process, three runs each: ms and bytes per step;
  3. host time of NativeBam.batch plain against packed on the same file.

  python tools/packed_speed.py [--genes 400] [--out profiles/packed_upload.txt]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longcallr_amd import _abi, api, bamio, synth  # noqa: E402

HBM_PEAK = 8.0e12     # bytes / s


def upload_bytes(b):
    """bytes a batch sends over the link: every array of its header"""
    arrays = [getattr(b, f) for f in b.FIELDS] + [b.start0, b.len, b.col_off, b.read_begin, b.ref]
    return int(sum(a.nbytes for a in arrays))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--genes", type=int, default=400)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workers", type=int, default=0, help="processes of the generator (0: one per CPU, at most 16)")
    ap.add_argument("--out", default=os.path.join("profiles", "packed_upload.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    params = _abi.make_params("ont-cdna")
    src = synth.make_genes("ont-cdna", n_genes=a.genes, workers=a.workers or min(16, os.cpu_count() or 1))
    tmp = tempfile.mkdtemp(prefix="lcr_packed_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        path = os.path.join(tmp, "c3.bam")
        bamio.write_reads_bam(path, src, "chrS", level=1, threads=0)
        flt = dict(min_mapq=0, min_read_length=0, divergence=2.0)
        regions = list(zip(src.start0.tolist(), src.len.tolist()))
        wins = [src.ref[int(src.col_off[g]):int(src.col_off[g + 1])] for g in range(src.n_regions)]
        nb = bamio.NativeBam(path, 0)
        # ---- 3. the host producers, interleaved, views of the decoder's buffers as the pipeline takes them
        t_plain, t_packed = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter(); nb.batch(0, regions, wins, name_format="blob", copy=False, **flt); t_plain.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); nb.batch(0, regions, wins, name_format="blob", copy=False, packed=True, **flt); t_packed.append(time.perf_counter() - t0)
        plain = nb.batch(0, regions, wins, name_format="blob", **flt)
        pk = nb.batch(0, regions, wins, name_format="blob", packed=True, **flt)
        nb.close()
        assert np.array_equal(plain.bases, src.bases) and np.array_equal(pk.quals, plain.quals)
        # the packed batch over the plain one's arrays: one set of page-locked pages serves both loops
        packed = _abi.PackedReadBatch(seq4=pk.seq4, pack_off=pk.pack_off, start0=plain.start0, len=plain.len, read_begin=plain.read_begin, ref=plain.ref,
                                      **{f: getattr(plain, f) for f in _abi.PackedReadBatch.FIELDS if f not in ("seq4", "pack_off")})
        n_bases, n_pack, nr = packed.n_bases, packed.n_pack, packed.n_reads
        say("batch: %d genes, %d reads, n_bases %d, n_pack %d, %d columns" % (a.genes, nr, n_bases, n_pack, int(plain.col_off[-1])))
        say("upload bytes per step: plain %d, packed %d, saved %d = n_bases - n_pack - 8 n_reads = %d (%.1f %% of plain)" % (
            upload_bytes(plain), upload_bytes(packed), upload_bytes(plain) - upload_bytes(packed), packed.upload_bytes_saved(),
            100.0 * packed.upload_bytes_saved() / upload_bytes(plain)))
        say("NativeBam.batch host time, s (views, %d runs interleaved): plain %s  packed %s" % (
            a.runs, " ".join("%.3f" % t for t in t_plain), " ".join("%.3f" % t for t in t_packed)))

        # ---- 1. the unpack kernel alone
        E = api.Engine(0, params, timing=True)
        ms = []
        for _ in range(4):      # the first call allocates and loads the code object: not reported
            E.load_batch(packed)
            ms.append(E.unpack_ms())
        E.run_all()
        want = E.candidates()[0].tobytes()
        E.close()
        for t in ms[1:]:
            say("k0_unpack: %.4f ms  %.1f GB/s of (n_pack + n_bases) = %d bytes  %.1f %% of the 8 TB/s peak" % (
                t, (n_pack + n_bases) / (t * 1e-3) / 1e9, n_pack + n_bases, 100.0 * (n_pack + n_bases) / (t * 1e-3) / HBM_PEAK))

        # ---- 2. the host-fed asynchronous loop, plain against packed
        pinned = api.host_register(*([getattr(plain, f) for f in plain.FIELDS] + [plain.ref, packed.seq4, packed.pack_off]))
        E = api.Engine(0, params)
        try:
            def loop(batch, steps):
                E.load_batch_async(batch, 0)
                for k in range(2):          # warm: both slots hold this form's buffers
                    E.bind_batch(k & 1); E.load_batch_async(batch, (k + 1) & 1); E.run_all()
                E.sync()
                t0 = time.perf_counter()
                for k in range(steps):
                    E.bind_batch(k & 1); E.load_batch_async(batch, (k + 1) & 1); E.run_all()
                E.sync()
                return (time.perf_counter() - t0) / steps * 1e3
            res = {"plain": [], "packed": []}
            for _ in range(a.runs):
                res["plain"].append(loop(plain, a.steps))
                assert E.candidates()[0].tobytes() == want
                res["packed"].append(loop(packed, a.steps))
                assert E.candidates()[0].tobytes() == want
        finally:
            E.close()
            api.host_unregister(pinned)
        for k in ("plain", "packed"):
            say("async host-fed loop, %s: ms per step over %d steps, %d runs: %s  (best %.2f)" % (
                k, a.steps, a.runs, " ".join("%.2f" % t for t in res[k]), min(res[k])))
        say("packed / plain: time %.3f (best over best), bytes %.3f" % (min(res["packed"]) / min(res["plain"]), upload_bytes(packed) / upload_bytes(plain)))
        say("outputs: the candidates of every timed loop's last step equal those of load_batch(packed) byte for byte")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

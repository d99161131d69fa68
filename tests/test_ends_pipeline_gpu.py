"""pipeline.run(ends_out=...) on a synthetic ONT cDNA BAM: the TSV against ends.format_tsv over the restatement (tests/ends_ref.py) on the
batch the pipeline cuts, the two stats, every other output untouched by the option, and the command line's flags reaching the same file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ends_ref as ref
from longcallr_amd import _abi, bamio, ends, pipeline, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT = dict(min_mapq=0, min_read_length=0, divergence=2.0)
STATS = ("end_sites", "end_reads")


def test_pipeline_ends_out(engine_cls, tmp_path):
    src = synth.make_batch("ont-cdna", n_genes=4, seed=5)
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "ref.fa")
    clen = bamio.write_reads_bam(bam, src, "chrS")
    seq = np.full(clen, ord("N"), np.uint8)
    for g in range(src.n_regions):
        seq[int(src.start0[g]):int(src.start0[g]) + int(src.len[g])] = src.ref[int(src.col_off[g]):int(src.col_off[g + 1])]
    with open(fa, "wb") as f, open(fa + ".fai", "w") as fi:
        f.write(b">chrS\n" + seq.tobytes() + b"\n")
        fi.write("chrS\t%d\t6\t%d\t%d\n" % (clen, clen, clen + 1))

    def run(tag, **kw):
        v, bm, aj = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".bam")), str(tmp_path / (tag + ".asj.tsv"))
        st = pipeline.run(bam, fa, v, bm, preset="ont-cdna", threads=4, asj_out=aj, **kw)
        return st, open(v, "rb").read(), bamio.bgzf_decompress(bm), open(aj, "rb").read()
    tsv = str(tmp_path / "out.ends.tsv")
    st_on, vcf_on, bam_on, asj_on = run("on", read_filter=FLT, ends_out=tsv, ends_min_count=3, ends_window=10)
    st_off, vcf_off, bam_off, asj_off = run("off", read_filter=FLT)
    st_none, vcf_none, bam_none, asj_none = run("none", read_filter=FLT, ends_out=None)
    assert vcf_on == vcf_off == vcf_none and bam_on == bam_off == bam_none and asj_on == asj_off == asj_none and vcf_on.count(b"\n") > 30
    assert not any(k in st_off for k in STATS) and {k: v for k, v in st_on.items() if k not in STATS} == st_off == st_none

    # the batch the pipeline cut (one chunk), phased once more here; the file against the restatement on the engine's phasing results
    nb = bamio.NativeBam(bam, 2)
    rs, re_ = nb.spans(0, **FLT)
    E = engine_cls(0, _abi.make_params("ont-cdna", seed=2025))
    regions = E.discover_regions(rs, re_, clen)
    batch = nb.batch(0, [(s, l) for s, l, _ in regions], [seq[s:s + l] for s, l, _ in regions], **FLT)
    nb.close()
    E.load_batch(batch).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    rec, off, row_site, tot = E.transcript_ends(3, 10)
    E.close()
    want = ref.transcript_ends(batch, fm["row_region_off"], fm["row_read"], pr["assignment"], pr["phase_set"], 3, 10)
    assert [x.tobytes() for x in (rec, off, row_site)] == [x.tobytes() for x in want[:3]] and tot == want[3]
    got = open(tsv).read()
    assert got.split("\n") == ends.format_tsv([("chrS", want[0], batch.start0, batch.len)], 3).split("\n")
    assert st_on["end_sites"] == rec.size and st_on["end_reads"] == tot["n_assigned"] == int((row_site >= 0).sum()) and st_on["regions"] == len(regions)
    print("ont-cdna n_genes=4: %d kept sites at (3, 10), %d ends assigned, %d rows written" % (rec.size, st_on["end_reads"], got.count("\n") - 1))

    # the command line (its own read filter): the flags reach the same file as the keywords
    st_kw = pipeline.run(bam, fa, str(tmp_path / "kw.vcf"), None, preset="ont-cdna", threads=4, ends_out=str(tmp_path / "kw.tsv"), ends_min_count=1,
                         ends_window=0, ends_strand="read")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_pipeline.py"), "-b", bam, "-f", fa, "-o", str(tmp_path / "cli.vcf"),
                        "-p", "ont-cdna", "-t", "4", "--ends-out", str(tmp_path / "cli.tsv"), "--ends-min-count", "1", "--ends-window", "0",
                        "--ends-strand", "read"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "cli.tsv")).read() == open(str(tmp_path / "kw.tsv")).read()
    st_cli = json.loads(r.stdout.strip().splitlines()[-1])
    assert st_cli["end_sites"] == st_kw["end_sites"] > 0 and st_cli["end_reads"] == st_kw["end_reads"] > 0

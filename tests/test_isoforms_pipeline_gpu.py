"""pipeline.run(isoforms_out=...) on a synthetic ONT cDNA BAM: the TSV against isoforms.format_tsv of Engine.isoforms on the batch the
pipeline cuts (checked there against the restatement, tests/isoforms_ref.py), the two stats, VCF and phased BAM untouched by the option,
and the command line's flags reaching the same file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import isoforms_ref as ref
from longcallr_amd import _abi, bamio, isoforms, pipeline, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT = dict(min_mapq=0, min_read_length=0, divergence=2.0)
STATS = ("isoforms", "isoform_reads")


def test_pipeline_isoforms_out(engine_cls, tmp_path):
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
        v, bm = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".bam"))
        st = pipeline.run(bam, fa, v, bm, preset="ont-cdna", threads=4, **kw)
        return st, open(v, "rb").read(), bamio.bgzf_decompress(bm)
    tsv = str(tmp_path / "out.isoforms.tsv")
    st_on, vcf_on, bam_on = run("on", read_filter=FLT, isoforms_out=tsv, isoform_min_count=2, isoform_min_junctions=1)
    st_off, vcf_off, bam_off = run("off", read_filter=FLT)
    assert vcf_on == vcf_off and bam_on == bam_off and vcf_on.count(b"\n") > 30
    assert not any(k in st_off for k in STATS) and {k: v for k, v in st_on.items() if k not in STATS} == st_off

    # the batch the pipeline cut (one chunk), phased once more here; its records by the engine, checked against the restatement
    nb = bamio.NativeBam(bam, 2)
    rs, re_ = nb.spans(0, **FLT)
    E = engine_cls(0, _abi.make_params("ont-cdna", seed=2025))
    regions = E.discover_regions(rs, re_, clen)
    batch = nb.batch(0, [(s, l) for s, l, _ in regions], [seq[s:s + l] for s, l, _ in regions], **FLT)
    nb.close()
    E.load_batch(batch).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    rec, off, pool, row_iso = E.isoforms(2, 1)
    E.close()
    want = ref.isoforms(batch, fm["row_region_off"], fm["row_read"], pr["assignment"], pr["phase_set"], 2, 1)
    assert [x.tobytes() for x in (rec, off, pool, row_iso)] == [x.tobytes() for x in want]
    got = open(tsv).read()
    assert got.split("\n") == isoforms.format_tsv([("chrS", rec, pool, batch.start0, batch.len)], 2).split("\n")
    assert st_on["isoforms"] == rec.size > 0 and st_on["isoform_reads"] == int((row_iso >= 0).sum()) > 0 and st_on["regions"] == len(regions)
    assert got.count("\n") > 1          # at least one chain's table reaches min_count
    print("ont-cdna n_genes=4: %d kept chains at (2, 1), %d rows hold one, %d rows written" % (rec.size, st_on["isoform_reads"], got.count("\n") - 1))

    # the command line (its own read filter): the flags reach the same file as the keywords
    st_kw, _, _ = run("kw", isoforms_out=str(tmp_path / "kw.tsv"), isoform_min_count=2, isoform_min_junctions=2)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_pipeline.py"), "-b", bam, "-f", fa, "-o", str(tmp_path / "cli.vcf"),
                        "-p", "ont-cdna", "-t", "4", "--isoforms-out", str(tmp_path / "cli.tsv"), "--isoform-min-count", "2",
                        "--isoform-min-junctions", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "cli.tsv")).read() == open(str(tmp_path / "kw.tsv")).read()
    st_cli = json.loads(r.stdout.strip().splitlines()[-1])
    assert st_cli["isoforms"] == st_kw["isoforms"] and st_cli["isoform_reads"] == st_kw["isoform_reads"]

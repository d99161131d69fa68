"""pipeline.run(asj_out=...) on a synthetic ONT cDNA BAM: the TSV against asj.format_tsv of the restatement's records (tests/asj_ref.py)
on the batch the pipeline cuts, the junction count in the stats, and VCF / phased BAM untouched by the option."""
import numpy as np
import pytest

import asj_ref
from longcallr_amd import _abi, asj, bamio, pipeline, synth

pytestmark = pytest.mark.gpu

FLT = dict(min_mapq=0, min_read_length=0, divergence=2.0)


def test_pipeline_asj_out(engine_cls, tmp_path):
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
        st = pipeline.run(bam, fa, v, bm, preset="ont-cdna", threads=4, read_filter=FLT, **kw)
        return st, open(v, "rb").read(), bamio.bgzf_decompress(bm)
    tsv = str(tmp_path / "out.asj.tsv")
    st_on, vcf_on, bam_on = run("on", asj_out=tsv, asj_min_count=4, asj_min_junctions=1)
    st_off, vcf_off, bam_off = run("off")
    assert vcf_on == vcf_off and bam_on == bam_off and vcf_on.count(b"\n") > 30
    assert "junctions" not in st_off and {k: v for k, v in st_on.items() if k != "junctions"} == st_off

    # the batch the pipeline cut, phased once more here; its table by the restatement
    prm = _abi.make_params("ont-cdna", seed=2025)
    nb = bamio.NativeBam(bam, 2)
    rs, re_ = nb.spans(0, **FLT)
    E = engine_cls(0, prm)
    regions = E.discover_regions(rs, re_, clen)
    batch = nb.batch(0, [(s, l) for s, l, _ in regions], [seq[s:s + l] for s, l, _ in regions], **FLT)
    nb.close()
    E.load_batch(batch).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    E.close()
    rec, off = asj_ref.junctions(batch, fm["row_region_off"], fm["row_read"], pr["assignment"], pr["phase_set"], 4, 1)
    want = asj.format_tsv([("chrS", rec, batch.start0, batch.len)], 4)
    got = open(tsv).read()
    assert got.split("\n") == want.split("\n")
    assert st_on["junctions"] == rec.size > 0 and st_on["regions"] == len(regions)
    assert got.count("\n") > 1          # at least one junction's table reaches min_count

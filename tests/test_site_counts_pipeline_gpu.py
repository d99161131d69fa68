"""pipeline.run(ase_sites_out=...) on tests/golden/demo.bam: the table against ase.format_sites_tsv over direct Engine calls and the
restatement's records (tests/site_counts_ref.py), VCF and phased BAM untouched by the option, the row count in the stats -- behind
lcr_phase, and once more behind lcr_haplotag with the run's own VCF fed back."""
import os

import numpy as np
import pytest

import helpers
import site_counts_ref as ref
import test_downsample_pipeline_gpu as dp
import test_haplotag_gpu as hg
from longcallr_amd import _abi, ase, bamio, pipeline, vcf

pytestmark = pytest.mark.gpu


def test_pipeline_ase_sites_out(engine_cls, tmp_path):
    src = os.path.join(helpers.GOLDEN, "demo.bam")
    fa = dp.demo_fasta(tmp_path)
    b = helpers.demo_batch()
    p = lambda name: str(tmp_path / name)

    def run(tag, **kw):
        st = pipeline.run(src, fa, p(tag + ".vcf"), p(tag + ".bam"), preset="hifi-masseq", threads=4, **kw)
        assert st["regions"] == 1 and st["reads"] == b.n_reads
        return st, open(p(tag + ".vcf"), "rb").read(), bamio.bgzf_decompress(p(tag + ".bam"))
    st_off, vcf_off, bam_off = run("off")
    st_on, vcf_on, bam_on = run("on", ase_sites_out=p("on.tsv"))
    st_q, vcf_q, bam_q = run("q", ase_sites_out=p("q.tsv"), ase_sites_min_baseq=30, ase_min_support=4, ase_overdispersion=0.01, ase_out=p("q.ase.tsv"))
    assert vcf_on == vcf_off and bam_on == bam_off and vcf_q == vcf_off and bam_q == bam_off
    assert "ase_sites" not in st_off and {k: x for k, x in st_on.items() if k != "ase_sites"} == st_off
    assert {k: x for k, x in st_q.items() if k not in ("ase_sites", "ase_regions")} == st_off
    for bad in (31, -1, 12.5, True):
        with pytest.raises(ValueError):
            pipeline.run(src, fa, p("x.vcf"), ase_sites_out=p("x.tsv"), ase_sites_min_baseq=bad)

    # the batch the pipeline cut, phased once more here; its records by the restatement
    prm = _abi.make_params("hifi-masseq", seed=2025)
    E = engine_cls(0, prm)
    E.load_batch(b).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    cands, _ = E.candidates()
    got13, got30 = E.site_counts(13), E.site_counts(30)
    E.close()
    want13, want30 = ref.of_engine(fm, pr, cands, 13), ref.of_engine(fm, pr, cands, 30)
    assert got13.tobytes() == want13.tobytes() and got30.tobytes() == want30.tobytes() and got13.tobytes() != got30.tobytes()
    mps = float(prm.min_phase_score)
    text = open(p("on.tsv")).read()
    assert text == ase.format_sites_tsv([("chr20", cands, want13)], 10, 0.001, mps) == ref.format_rows([("chr20", cands, want13)], 10, 0.001, mps)
    assert open(p("q.tsv")).read() == ase.format_sites_tsv([("chr20", cands, want30)], 4, 0.01, mps)
    assert st_on["ase_sites"] == text.count("\n") - 1 > 0 and st_q["ase_sites"] == open(p("q.tsv")).read().count("\n") - 1
    rows = [l.split("\t") for l in text.split("\n")[1:-1]]
    body = [l.split("\t") for l in dp.body_of(p("on.vcf")).split("\n") if l]
    by_pos = {f[1]: f for f in body}
    assert all(r[1] in by_pos and by_pos[r[1]][6] == r[4] and by_pos[r[1]][9].split(":")[0] == r[5] for r in rows)      # a row per VCF record, its own fields
    print("demo.bam --ase-sites-out: %d VCF records, %d rows at min_support 10, filters %r" % (len(body), len(rows), sorted({r[4] for r in rows})))

    # once more behind lcr_haplotag: the run's own VCF fed back, the input's phase kept, min_phase_score 0.0
    st_h, vcf_h, bam_h = run("hap", input_vcf=p("off.vcf"), haplotag=True)
    st_hs, vcf_hs, bam_hs = run("haps", input_vcf=p("off.vcf"), haplotag=True, ase_sites_out=p("haps.tsv"))
    assert vcf_hs == vcf_h and bam_hs == bam_h and {k: x for k, x in st_hs.items() if k != "ase_sites"} == st_h
    arrays = vcf.read_sites(p("off.vcf"), alleles=True, phase_sets=True)["chr20"]
    lo, hi = np.searchsorted(arrays[0], [int(b.start0[0]), int(b.start0[0]) + int(b.len[0])])
    hsites = vcf.haplotag_sites(arrays)
    hlo, hhi = np.searchsorted(hsites[0], [int(b.start0[0]), int(b.start0[0]) + int(b.len[0])])
    hsites = tuple(a[hlo:hhi] for a in hsites)
    E = engine_cls(0, prm)
    fm, _, _ = hg.staged(E, b, tuple(a[lo:hi] for a in arrays[:3]))
    E.haplotag(hsites)
    pr = E.phase_result()
    cands, _ = E.candidates()
    got = E.site_counts(13)
    E.close()
    want = ref.of_engine(fm, pr, cands, 13)
    assert got.tobytes() == want.tobytes() and pr["assignment"].any()
    text_h = open(p("haps.tsv")).read()
    assert text_h == ase.format_sites_tsv([("chr20", cands, want)], 10, 0.001, 0.0) and st_hs["ase_sites"] == text_h.count("\n") - 1 > 0

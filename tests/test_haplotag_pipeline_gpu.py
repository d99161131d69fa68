"""pipeline.run(input_vcf=..., haplotag=True) on tests/golden/demo.bam: the run's own phased VCF is fed back, and the second run's VCF
body and every read's HP / PS equal what direct Engine calls and the restatement (tests/haplotag_ref.py) give for the same chunk; the
new stats, and the junction / expression tables behind it.  Prints the share of reads that keep their HP between the two runs."""
import os
import struct

import numpy as np
import pytest

import haplotag_ref as ref
import helpers
import test_downsample_pipeline_gpu as dp
import test_haplotag_gpu as hg
from longcallr_amd import _abi, bamio, pipeline, vcf

pytestmark = pytest.mark.gpu


def tags_by_name(bam_path):
    _, recs = bamio.read_bam(bam_path, keep_raw=True)
    out = {}
    for r in recs:
        out.setdefault(r["name"], r["raw"][r["aux_off"]:])
    return out


def hp_of(aux):
    return 1 if b"HPi" + struct.pack("<i", 1) in aux else 2 if b"HPi" + struct.pack("<i", 2) in aux else 0


def test_pipeline_haplotag_on_demo_bam(engine_cls, tmp_path):
    src = os.path.join(helpers.GOLDEN, "demo.bam")
    fa = dp.demo_fasta(tmp_path)
    b = helpers.demo_batch()
    p = lambda name: str(tmp_path / name)
    st1 = pipeline.run(src, fa, p("one.vcf"), p("one.bam"), preset="hifi-masseq", threads=4)
    assert "haplotag_sites" not in st1 and st1["regions"] == 1
    st2 = pipeline.run(src, fa, p("two.vcf"), p("two.bam"), preset="hifi-masseq", threads=4, input_vcf=p("one.vcf"), haplotag=True,
                       asj_out=p("two.asj.tsv"), asj_min_count=2, asj_min_junctions=0, ase_out=p("two.ase.tsv"))
    # the same chunk by direct calls: the demo window is one region, one chunk
    prm = _abi.make_params("hifi-masseq", seed=2025)
    arrays = vcf.read_sites(p("one.vcf"), alleles=True, phase_sets=True)["chr20"]
    lo, hi = np.searchsorted(arrays[0], [int(b.start0[0]), int(b.start0[0]) + int(b.len[0])])
    hsites = vcf.haplotag_sites(arrays)
    hlo, hhi = np.searchsorted(hsites[0], [int(b.start0[0]), int(b.start0[0]) + int(b.len[0])])
    hsites = tuple(a[hlo:hhi] for a in hsites)
    assert hsites[0].size >= 5 and (hsites[3] != 0).all()
    E = engine_cls(0, prm)
    fm, cands0, _ = hg.staged(E, b, tuple(a[lo:hi] for a in arrays[:3]))
    E.haplotag(hsites)
    want, pr, got, _ = hg.compare(E, fm, cands0, hsites)
    E.close()
    assert dp.body_of(p("two.vcf")) == vcf.format_records(got, "chr20", 0.0)
    body = dp.body_of(p("two.vcf"))
    assert body.count("|") == int(want["usable"].sum()) > 0           # every tagged site is printed phased, whatever its PQ
    assert st2["input_sites"] == arrays[0].size and st2["imported_sites"] == hi - lo
    assert st2["haplotag_sites"] == int(want["usable"].sum()) and st2["haplotag_reads"] == int((want["assignment"] != 0).sum()) > 0
    assert st2["candidates"] == cands0.size and st2["regions"] == 1
    # every fragment row's HP / PS in the phased BAM
    _, recs = bamio.read_bam(src)
    keep = [r for r in recs if bamio.passes_filter(r, **_abi.READ_FILTER)]
    two, one = tags_by_name(p("two.bam")), tags_by_name(p("one.bam"))
    same = both = 0
    for row in range(len(want["assignment"])):
        name = keep[int(fm["row_read"][row])]["name"]
        aux = two[name]
        a, ps = int(want["assignment"][row]), int(want["phase_set"][row])
        assert (b"HPi" + struct.pack("<i", a) in aux) == (a in (1, 2)), row
        assert (b"PSI" + struct.pack("<I", ps) in aux) == (ps != 0), row
        h1 = hp_of(one.get(name, b""))
        if a and h1:
            both += 1
            same += a == h1
    assert both > 0
    print("demo.bam: %d rows, %d assigned by lcr_phase's run and by the haplotag run, %d of them with the same HP (%.4f)" % (
        len(want["assignment"]), both, same, same / both))
    # the tables behind it are written
    assert open(p("two.asj.tsv")).read().count("\n") >= 1 and open(p("two.ase.tsv")).read().count("\n") >= 1
    assert "junctions" in st2 and "ase_regions" in st2

"""pipeline.run(annotation=..., exon_only=True) on tests/golden/demo.bam (-m gpu): the coverage island of chr20 clipped to annotated
genes, candidates called at CDS columns only.  The record set is the oracle's on the clipped regions' batch with 'N' at the columns
outside CDS (exon_cases.py)."""
import os

import numpy as np
import pytest

import exon_cases as ex
import helpers
import test_truncation_pipeline_gpu as tp
from longcallr_amd import _abi, annotation, bamio, pipeline

pytestmark = pytest.mark.gpu

W = 16729960        # first column of demo.bam's coverage island on chr20 (0-based); 13 256 columns
# genes as (id, span, CDS list), 0-based half-open offsets from W.  The unmasked run has records at 185, 756, 3052, 5469, 6038, 6439, 6687,
# 6774, 7657, 7786, 7892, 8178, 8424, 9148, 10196, 11286, 12319, 12766 and 13124 (asserted below through the oracle).
GENES = [("G1", (100, 6500), [(150, 800), (5400, 5500)]),          # overlaps G2: one cluster [100, 9500)
         ("G2", (6000, 9500), [(7700, 7900), (6600, 6800)]),
         ("G3", (10000, 10500), []),                               # no CDS: its region is dropped
         ("G5", (11000, 13000), [(11200, 11300)]),
         ("G4", (20000, 21000), [(20100, 20200)])]                 # outside the coverage
CLIPPED = [(W + 100, 9400), (W + 11000, 2000)]
IN_CDS = [185, 756, 5469, 6687, 6774, 7786, 7892, 11286]
IN_KEPT_REGIONS = [185, 756, 3052, 5469, 6038, 6439, 6687, 6774, 7657, 7786, 7892, 8178, 8424, 9148, 11286, 12319, 12766]


def write_annotation(tmp_path):
    rows = ["##gff-version 3"]
    for gid, (a, z), cds in GENES:
        attrs = "ID=%s;gene_id=%s;gene_type=protein_coding" % (gid, gid)
        rows.append("\t".join(["chr20", "t", "gene", str(W + a + 1), str(W + z), ".", "+", ".", attrs]))
        rows.append("\t".join(["chr20", "t", "exon", str(W + a + 1), str(W + z), ".", "+", ".", attrs]))
        rows += ["\t".join(["chr20", "t", "CDS", str(W + x + 1), str(W + y), ".", "+", "0", attrs]) for x, y in cds]
    path = str(tmp_path / "genes.gff3")
    open(path, "w").write("\n".join(rows) + "\n")
    return path


@pytest.fixture(scope="module")
def demo():
    src = os.path.join(helpers.GOLDEN, "demo.bam")
    _, recs = bamio.read_bam(src, keep_raw=True)
    keep = [r for r in recs if bamio.passes_filter(r, **_abi.READ_FILTER)]
    full = helpers.load_pseudo_ref()
    assert int(helpers.demo_batch().start0[0]) == W
    batch = bamio.build_batch(keep, CLIPPED, [full[s - W:s - W + l] for s, l in CLIPPED])
    lists = [[(W + x, W + y) for gid, _, cds in GENES if gid in ids for x, y in cds] for ids in (("G1", "G2"), ("G5",))]
    return dict(src=src, recs=recs, keep=keep, batch=batch, lists=lists)


def oracle_text(orc, batch, prm):
    out = ""
    for g in range(batch.n_regions):
        R = orc.Region(batch, g, prm).set_fast(1).pileup()
        R.candidates()
        R.fragments()
        R.set_tie_mask(orc.TIE_MASK_LIBLCR).phase(orc.MODE_TIE).post_phase()
        out += R.vcf_text("chr20")
    return out


def test_pipeline_exon_only_on_demo_bam(engine_cls, orc, demo, tmp_path):
    fa, gff = tp.demo_fasta(tmp_path), write_annotation(tmp_path)
    prm = _abi.make_params("hifi-masseq", seed=2025)
    batch, lists = demo["batch"], demo["lists"]
    clusters, cds = annotation.calling_annotation(gff)
    assert [(s, e) for s, e, _ in clusters["chr20"]] == [(W + 100, W + 9500), (W + 10000, W + 10500), (W + 11000, W + 13000), (W + 20000, W + 21000)]
    keep = ex.mask_of_lists(batch, lists)
    want = oracle_text(orc, ex.n_substituted(batch, keep), prm)
    unmasked = tp.positions(oracle_text(orc, batch, prm))
    assert [x - W for x in unmasked] == IN_KEPT_REGIONS and [x - W for x in tp.positions(want)] == IN_CDS

    def run(tag, out_bam=True, **kw):
        o_vcf, o_bam = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".bam"))
        st = pipeline.run(demo["src"], fa, o_vcf, o_bam if out_bam else None, preset="hifi-masseq", threads=4, **kw)
        return st, o_vcf, o_bam

    st, on_vcf, on_bam = run("on", annotation=gff, exon_only=True)
    assert st["regions"] == 1 and st["exon_regions"] == 2 and st["exon_skipped_regions"] == 1
    assert st["reads"] == batch.n_reads and st["chunks"] == 1
    body = tp.body_of(on_vcf)
    assert body == want
    pos = tp.positions(body)
    assert all(any(s <= x < s + l for s, l in CLIPPED) for x in pos)                                   # in a clipped region ...
    assert all(any(a <= x < z for v in lists for a, z in v) for x in pos)                              # ... and in a CDS
    assert len(pos) == len(IN_CDS)

    # phased BAM: only reads contained in a clipped region are written, and some of them carry the tags
    _, got = bamio.read_bam(on_bam, keep_raw=True)
    assert len(got) > 0 and any(tp.bamio_has(g, b"HP") for g in got) and any(tp.bamio_has(g, b"PS") for g in got)
    for g in got:
        end = g["pos"] + (g["ref_len"] if g["ref_len"] > 0 else 1)
        assert any(s <= g["pos"] and end <= s + l for s, l in CLIPPED), g["name"]
    contained = [r for r in demo["recs"] if any(s <= r["pos"] and r["pos"] + (r["ref_len"] if r["ref_len"] > 0 else 1) <= s + l for s, l in CLIPPED)]
    assert 0 < len(got) <= len(contained) < len(demo["recs"])

    # the same files from every configuration
    stream = bamio.bgzf_decompress(on_bam)
    for tag, kw in (("three", dict(devices=[0, 0, 0])), ("chunks", dict(chunk_cost=1.0)), ("sync", dict(async_phase=False))):
        st2, v, bm = run(tag, annotation=gff, exon_only=True, **kw)
        assert st2["exon_regions"] == 2 and st2["exon_skipped_regions"] == 1 and st2["chunks"] == (2 if tag == "chunks" else 1)
        assert open(v, "rb").read() == open(on_vcf, "rb").read(), tag
        assert bamio.bgzf_decompress(bm) == stream, tag

    # annotation alone: parsed, and nothing else
    st_off, off_vcf, off_bam = run("off")
    st_a, a_vcf, a_bam = run("anno", annotation=gff)
    assert st_a == st_off and "exon_regions" not in st_a
    assert open(a_vcf, "rb").read() == open(off_vcf, "rb").read() and tp.body_of(off_vcf) != body
    assert open(a_bam, "rb").read() == open(off_bam, "rb").read()
    bad = str(tmp_path / "bad.gtf")
    open(bad, "w").write("chr20\tt\tgene\t200\t300\t.\t+\t.\tgene_id \"A\";\nchr20\tt\tgene\t100\t300\t.\t+\t.\tgene_id \"B\";\n")
    with pytest.raises(ValueError, match="not sorted"):
        run("bad", out_bam=False, annotation=bad)
    with pytest.raises(ValueError, match="annotation file is not provided"):
        run("alone", out_bam=False, exon_only=True)


def test_pipeline_exon_only_with_input_vcf(engine_cls, orc, demo, tmp_path):
    """-v with --exon-only: the regions are clipped and the CDS-less one is dropped, but a site outside CDS inside a kept region is phased"""
    fa, gff = tp.demo_fasta(tmp_path), write_annotation(tmp_path)
    prm = _abi.make_params("hifi-masseq", seed=2025)
    batch = demo["batch"]
    p = np.array([W + x for x in IN_KEPT_REGIONS], np.int64)
    E = engine_cls(0, prm)
    E.load_batch(batch).fill_data_into_freq_vec().import_external_candidates(p, np.ones(p.size, np.uint8), np.full(p.size, 30.0, np.float32))
    E.get_fragments().phase()
    from longcallr_amd import vcf
    want = vcf.format_records(E.candidates()[0], "chr20", prm.min_phase_score)
    E.close()
    sites = sorted(p.tolist() + [W + 50, W + 10196, W + 13124])        # in front of every gene, in the dropped region, behind every gene
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"]
    lines += ["chr20\t%d\t.\tA\tG\t30.0\tPASS\t.\tGT\t0/1" % (x + 1) for x in sites]
    path = str(tmp_path / "sites.vcf")
    open(path, "w").write("\n".join(lines) + "\n")
    out_vcf = str(tmp_path / "v.vcf")
    st = pipeline.run(demo["src"], fa, out_vcf, None, preset="hifi-masseq", threads=4, input_vcf=path, annotation=gff, exon_only=True)
    assert st["exon_regions"] == 2 and st["exon_skipped_regions"] == 1 and st["input_sites"] == len(sites)
    body = tp.body_of(out_vcf)
    assert body == want
    pos = [x - W for x in tp.positions(body)]
    assert pos and set(pos) <= set(IN_KEPT_REGIONS) and any(x not in IN_CDS for x in pos)

"""pipeline.run(asj_cluster_with_exons / asj_dna_vcf / asj_gene_coverage) on tests/golden/demo.bam with the small GTF of
test_genes_pipeline_gpu: with the three options off every output is the annotated run's; with them on the VCF and the phased BAM stay,
the table is asj.format_tsv_genes' text over the restatement's records (tests/asj_modes_ref.py) and the coverage file lists every `gene`
feature in file order.  On a synthetic ONT cDNA BAM of four regions: the same outputs from one chunk and from one chunk per region."""
import os

import numpy as np
import pytest

import ase_ref
import asj_modes_ref
import helpers
import test_asj_genes_gpu as tg
import test_downsample_pipeline_gpu as dp
import test_genes_pipeline_gpu as gp
from longcallr_amd import _abi, annotation, asj, bamio, pipeline

pytestmark = pytest.mark.gpu


def restate(engine_cls, prm, b, genes, mc, mj, dna):
    E = engine_cls(0, prm)
    E.load_batch(b).assign_genes(genes).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    gene, _ = E.read_genes()
    cands, coff = E.candidates()
    E.close()
    mps = float(prm.min_phase_score)
    want = asj_modes_ref.asj_genes(b, fm["row_region_off"], fm["row_read"], pr["assignment"], pr["phase_set"], gene, genes, cands, coff, mc, mj,
                                   True, dna, True, mps)
    sites = sorted({int(cands["pos"][i]) for i in range(len(cands)) if int(cands["phase_set"][i]) and ase_ref.pass_phased_het(cands[i:i + 1], mps)})
    return want, sites, cands


def write_dna_vcf(path, contig, cands, positions):
    at = {int(cands["pos"][i]): i for i in range(len(cands))}
    lines = []
    for p in positions:
        i = at[p]
        ref = chr(cands["ref_base"][i]).upper()
        alt = [chr(cands[a][i]) for a in ("allele1", "allele2") if chr(cands[a][i]).upper() != ref][0]
        lines.append("%s\t%d\t.\t%s\t%s\t50\tPASS\t.\tGT\t0/1\n" % (contig, p + 1, ref, alt.upper()))
    open(path, "w").write(gp.VCF_HEAD.replace("chr20", contig) + "".join(lines))


def test_pipeline_asj_modes_demo(engine_cls, tmp_path):
    src = os.path.join(helpers.GOLDEN, "demo.bam")
    fa = dp.demo_fasta(tmp_path)
    b = helpers.demo_batch()
    gtf = str(tmp_path / "genes.gtf.gz")
    gp.write_gtf(gtf, int(b.start0[0]), int(b.len[0]))
    genes = annotation.load(gtf)["chr20"]
    prm = _abi.make_params("hifi-masseq", seed=2025)
    _, sites, cands = restate(engine_cls, prm, b, genes, 2, 0, None)
    dna = sites[::2]
    assert len(dna) >= 2
    dvcf = str(tmp_path / "dna.vcf")
    write_dna_vcf(dvcf, "chr20", cands, dna)
    want, _, _ = restate(engine_cls, prm, b, genes, 2, 0, dna)
    p = lambda name: str(tmp_path / name)

    def run(tag, **kw):
        v, bm = p(tag + ".vcf"), p(tag + ".bam")
        st = pipeline.run(src, fa, v, bm, preset="hifi-masseq", threads=4, asj_out=p(tag + ".asj.tsv"), asj_annotation=gtf, asj_min_count=2,
                          asj_min_junctions=0, **kw)
        return st, open(v, "rb").read(), bamio.bgzf_decompress(bm), open(p(tag + ".asj.tsv")).read(), open(p(tag + ".asj_gene.tsv")).read()
    off = run("off")
    off2 = run("off2", asj_cluster_with_exons=False, asj_dna_vcf=None, asj_gene_coverage=False)
    assert off[0] == off2[0] and off[1:] == off2[1:] and not os.path.exists(p("off2.gene_coverage.tsv")) and "asj_exons" not in off2[0]
    on = run("on", asj_cluster_with_exons=True, asj_dna_vcf=dvcf, asj_gene_coverage=True)
    assert on[1] == off[1] and on[2] == off[2]                                   # VCF and phased BAM do not depend on the options
    table = [("chr20", want["junc"], genes, want["exon"])]
    assert on[3].split("\n") == asj.format_tsv_genes(table, 2).split("\n") and on[4] == asj.format_gene_tsv(table, 2)
    assert on[0]["asj_exons"] == want["exon"].size and on[0]["junctions"] == want["junc"].size
    # Junction_set from the restatement's own graph walk
    comp = asj_modes_ref.cluster(want["junc"], want["exon"])
    assert comp.tolist() == asj.cluster(want["junc"], want["exon"]).tolist()
    cov = open(p("on.gene_coverage.tsv")).read()
    print(on[3] + cov)
    feats = annotation.gene_features(gtf)
    assert [f[1] for f in feats] == ["g.left", "g.right", "g.noname", "g.far"]
    n = {gid: int(want["gene_reads"][k]) for k, gid in enumerate(genes.gene_id)}
    assert cov == asj.format_gene_coverage([(f[2], f[0], f[3], f[4], n.get(f[1], 0) if f[0] == "chr20" else 0) for f in feats])
    assert on[0]["asj_coverage_genes"] == 4 and sum(want["gene_reads"]) > 0 and cov.split("\n")[4].endswith("\t0")
    # another output name
    st = pipeline.run(src, fa, p("x.vcf"), preset="hifi-masseq", threads=4, asj_out=p("x.tsv"), asj_annotation=gtf, asj_min_count=2, asj_min_junctions=0,
                      asj_gene_coverage=True, chunk_cost=1.0)
    assert open(p("x.tsv.gene_coverage.tsv")).read() == cov and st["asj_exons"] == 0


def test_pipeline_asj_modes_over_several_chunks(engine_cls, tmp_path):
    from longcallr_amd import synth
    FLT = dict(min_mapq=0, min_read_length=0, divergence=2.0)
    src = synth.make_batch("ont-cdna", n_genes=4, seed=5)
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "ref.fa")
    clen = bamio.write_reads_bam(bam, src, "chrS")
    seq = np.full(clen, ord("N"), np.uint8)
    for g in range(src.n_regions):
        seq[int(src.start0[g]):int(src.start0[g]) + int(src.len[g])] = src.ref[int(src.col_off[g]):int(src.col_off[g + 1])]
    with open(fa, "wb") as f, open(fa + ".fai", "w") as fi:
        f.write(b">chrS\n" + seq.tobytes() + b"\n")
        fi.write("chrS\t%d\t6\t%d\t%d\n" % (clen, clen, clen + 1))
    prm = _abi.make_params("ont-cdna", seed=2025)
    nb = bamio.NativeBam(bam, 2)
    rs, re_ = nb.spans(0, **FLT)
    E = engine_cls(0, prm)
    regions = E.discover_regions(rs, re_, clen)
    E.close()
    b = nb.batch(0, [(s, l) for s, l, _ in regions], [seq[s:s + l] for s, l, _ in regions], **FLT)
    nb.close()
    assert b.n_regions == 4
    ex = [tg.region_exons(b, g) for g in range(4)]
    gtf = str(tmp_path / "genes.gtf")
    with open(gtf, "w") as f:
        for gid, exons in (("I0", ex[0][0::2]), ("I1", ex[0][1::2]), ("SPLIT", ex[1] + ex[2]), ("MAIN3", ex[3])):
            attrs = 'gene_id "%s"; gene_type "protein_coding"; gene_name "%s"; transcript_id "%s.t";' % (gid, gid.lower(), gid)
            f.write("\t".join(["chrS", "t", "gene", str(exons[0][0] + 1), str(exons[-1][1]), ".", "+", ".", attrs]) + "\n")
            for x, y in exons:
                f.write("\t".join(["chrS", "t", "exon", str(x + 1), str(y), ".", "+", ".", attrs]) + "\n")
    genes = annotation.load(gtf)["chrS"]
    _, sites, cands = restate(engine_cls, prm, b, genes, 10, 2, None)
    dna = sites[::2]
    dvcf = str(tmp_path / "dna.vcf")
    write_dna_vcf(dvcf, "chrS", cands, dna)
    want, _, _ = restate(engine_cls, prm, b, genes, 10, 2, dna)

    def run(tag, **kw):
        v, t = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".asj.tsv"))
        st = pipeline.run(bam, fa, v, preset="ont-cdna", threads=4, read_filter=FLT, asj_out=t, asj_annotation=gtf, asj_cluster_with_exons=True,
                          asj_dna_vcf=dvcf, asj_gene_coverage=True, **kw)
        return st, open(v, "rb").read(), open(t).read(), open(str(tmp_path / (tag + ".asj_gene.tsv"))).read(), open(str(tmp_path / (tag + ".gene_coverage.tsv"))).read()
    one, many = run("one"), run("many", chunk_cost=1.0)
    assert one[0]["chunks"] == 1 and many[0]["chunks"] == 4 and one[1:] == many[1:]
    assert {k: v for k, v in one[0].items() if k != "chunks"} == {k: v for k, v in many[0].items() if k != "chunks"}
    table = [("chrS", want["junc"], genes, want["exon"])]
    assert many[2] == asj.format_tsv_genes(table, 10) and many[3] == asj.format_gene_tsv(table, 10)
    n = {gid: int(want["gene_reads"][k]) for k, gid in enumerate(genes.gene_id)}
    assert many[4] == asj.format_gene_coverage([(f[2], f[0], f[3], f[4], n[f[1]]) for f in annotation.gene_features(gtf)])
    assert many[0]["asj_exons"] == want["exon"].size and want["exon"].size > 0 and sum(n.values()) > 0

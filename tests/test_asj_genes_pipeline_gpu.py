"""pipeline.run(asj_out=..., asj_annotation=...) on tests/golden/demo.bam with a small GTF: the per-gene junction table and the gene
file against the texts asj.format_tsv_genes / format_gene_tsv give for the restatement's records (tests/asj_genes_ref.py) on the batch
the pipeline cuts; the gene file once more from the table's own rows; VCF, phased BAM and the table without asj_annotation untouched by
the option; both per-gene tables out of one gene assignment per chunk."""
import os

import pytest

import asj_genes_ref
import asj_ref
import helpers
import test_downsample_pipeline_gpu as dp
import test_genes_pipeline_gpu as gp
from longcallr_amd import _abi, annotation, asj, bamio, pipeline

pytestmark = pytest.mark.gpu


def gene_file_from_table(text):
    """the .asj_gene.tsv that follows from a .asj.tsv: per Gene_name the first row with the smallest P_value among those with GT_AG True"""
    best = {}
    for line in text.split("\n")[1:-1]:
        f = line.split("\t")
        if f[11] != "True":
            continue
        if f[12] not in best or float(f[8]) < float(best[f[12]][1]):
            best[f[12]] = (f[0].split(":")[0], f[8], f[9])
    return "#Gene_name\tChr\tP_value\tSOR\n" + "".join("%s\t%s\t%s\t%s\n" % ((n,) + v) for n, v in best.items())


def test_pipeline_asj_annotation(engine_cls, tmp_path):
    src = os.path.join(helpers.GOLDEN, "demo.bam")
    fa = dp.demo_fasta(tmp_path)
    b = helpers.demo_batch()
    gtf = str(tmp_path / "genes.gtf.gz")
    gp.write_gtf(gtf, int(b.start0[0]), int(b.len[0]))
    genes = annotation.load(gtf)["chr20"]
    assert genes.gene_id == ["g.left", "g.noname", "g.right", "g.exononly"]

    def run(tag, **kw):
        v, bm = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".bam"))
        st = pipeline.run(src, fa, v, bm, preset="hifi-masseq", threads=4, **kw)
        return st, open(v, "rb").read(), bamio.bgzf_decompress(bm)
    p = lambda name: str(tmp_path / name)
    st_reg, vcf_reg, bam_reg = run("region", asj_out=p("region.asj.tsv"), asj_min_count=2, asj_min_junctions=0)
    st_gen, vcf_gen, bam_gen = run("genes", asj_out=p("genes.asj.tsv"), asj_annotation=gtf, asj_min_count=2, asj_min_junctions=0)
    st_ase, _, _ = run("ase", ase_out=p("ase.tsv"), ase_annotation=gtf)
    st_both, vcf_both, bam_both = run("both", asj_out=p("both.tsv"), asj_annotation=gtf, ase_out=p("both.ase.tsv"), ase_annotation=gtf)
    assert vcf_gen == vcf_reg == vcf_both and bam_gen == bam_reg == bam_both              # VCF and phased BAM do not depend on the option
    assert not os.path.exists(p("region.asj_gene.tsv")) and "asj_genes" not in st_reg

    # the batch the pipeline cut, phased once more here with its reads assigned
    prm = _abi.make_params("hifi-masseq", seed=2025)
    E = engine_cls(0, prm)
    E.load_batch(b).assign_genes(genes).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    gene, _ = E.read_genes()
    plain = E.junctions(2, 0)[0]
    E.close()
    args = (b, fm["row_region_off"], fm["row_read"], pr["assignment"], pr["phase_set"])
    # without asj_annotation: the table of regions, as before
    reg_text = open(p("region.asj.tsv")).read()
    assert reg_text == asj.format_tsv([("chr20", plain, b.start0, b.len)], 2)
    assert reg_text == asj.format_tsv([("chr20", asj_ref.junctions(*args, 2, 0)[0], b.start0, b.len)], 2) and st_reg["junctions"] == plain.size
    # with it: every row of the table from the restatement's records; the gene file beside it
    want, _ = asj_genes_ref.junctions_genes(*args, gene, genes, 2, 0)
    text, gene_text = open(p("genes.asj.tsv")).read(), open(p("genes.asj_gene.tsv")).read()
    print(text + gene_text)
    assert text.split("\n") == asj.format_tsv_genes([("chr20", want, genes)], 2).split("\n")
    assert gene_text == asj.format_gene_tsv([("chr20", want, genes)], 2) == gene_file_from_table(text)
    rows = [l.split("\t") for l in text.split("\n")[1:-1]]
    assert len(rows) >= 1 and st_gen["junctions"] == want.size and st_gen["asj_genes"] == gene_text.count("\n") - 1
    assert {r[12] for r in rows} <= {"LEFT", "RIGHT", "."} and all(r[1] == "+" and r[10] == "True" for r in rows)     # no exon-only gene; no annotated intron
    assert {k: v for k, v in st_gen.items() if k != "asj_genes"} == st_reg | {"junctions": int(want.size)}
    # both annotations: one assignment per chunk feeds both tables; another output name gets ".gene.tsv"
    want10, _ = asj_genes_ref.junctions_genes(*args, gene, genes, 10, 2)
    assert open(p("both.tsv")).read() == asj.format_tsv_genes([("chr20", want10, genes)], 10)
    assert open(p("both.tsv.gene.tsv")).read() == asj.format_gene_tsv([("chr20", want10, genes)], 10)
    assert open(p("both.ase.tsv")).read() == open(p("ase.tsv")).read() and st_both["ase_genes"] == st_ase["ase_genes"]
    assert st_both["junctions"] == want10.size

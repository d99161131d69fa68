"""pipeline.run(ase_out=..., ase_annotation=...) on tests/golden/demo.bam with a small GTF: the per-gene table in its three modes against
the text ase.format_tsv gives for the restatement's records (tests/genes_ref.py) on the batch the pipeline cuts; VCF and phased BAM
untouched by the option; a run without ase_annotation writes what Engine.ase gives, as before."""
import gzip
import os

import numpy as np
import pytest

import ase_ref
import genes_ref
import helpers
import test_downsample_pipeline_gpu as dp
from longcallr_amd import _abi, annotation, ase, bamio, pipeline

pytestmark = pytest.mark.gpu

VCF_HEAD = "##fileformat=VCFv4.2\n##contig=<ID=chr20>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"


def write_gtf(path, start0, length):
    """Genes over demo.bam's island [start0, start0 + length), 1-based inclusive in the file: LEFT over its first 60 %, RIGHT over its last
    60 % (they overlap in the middle fifth), NONAME inside LEFT, an exon-only gene (takes reads, never printed), a pseudogene and a
    readthrough gene over everything (both dropped), a gene on a contig without reads."""
    a, n = start0 + 1, length

    def row(contig, feature, s, e, gid, gtype="protein_coding", name=None, extra=""):
        attrs = 'gene_id "%s"; gene_type "%s"; transcript_id "%s.t";%s%s' % (gid, gtype, gid, ' gene_name "%s";' % name if name else "", extra)
        return "\t".join([contig, "t", feature, str(s), str(e), ".", "+", ".", attrs]) + "\n"
    text = "# demo annotation\n"
    text += row("chr20", "gene", a, a + 6 * n // 10, "g.left", name="LEFT") + row("chr20", "exon", a, a + 3 * n // 10, "g.left") + row("chr20", "exon", a + 4 * n // 10, a + 6 * n // 10, "g.left")
    text += row("chr20", "gene", a + 4 * n // 10, a + n - 1, "g.right", "lncRNA", name="RIGHT") + row("chr20", "exon", a + 4 * n // 10, a + n - 1, "g.right", "lncRNA")
    text += row("chr20", "gene", a + n // 10, a + 2 * n // 10, "g.noname") + row("chr20", "exon", a + n // 10, a + 2 * n // 10, "g.noname")
    text += row("chr20", "exon", a + 7 * n // 10, a + 8 * n // 10, "g.exononly")
    text += row("chr20", "gene", a, a + n - 1, "g.pseudo", "pseudogene", name="PSEUDO") + row("chr20", "exon", a, a + n - 1, "g.pseudo", "pseudogene")
    text += row("chr20", "gene", a, a + n - 1, "g.rt", name="RT", extra=' tag "readthrough_gene";') + row("chr20", "exon", a, a + n - 1, "g.rt", extra=' tag "readthrough_gene";')
    text += row("chr19", "gene", 1000, 2000, "g.far", name="FAR") + row("chr19", "exon", 1000, 2000, "g.far")
    with gzip.open(path, "wt") as f:
        f.write(text)


def test_pipeline_ase_annotation(engine_cls, tmp_path):
    src = os.path.join(helpers.GOLDEN, "demo.bam")
    fa = dp.demo_fasta(tmp_path)
    b = helpers.demo_batch()
    gtf = str(tmp_path / "genes.gtf.gz")
    write_gtf(gtf, int(b.start0[0]), int(b.len[0]))
    genes = annotation.load(gtf)["chr20"]
    assert genes.gene_id == ["g.left", "g.noname", "g.right", "g.exononly"] and genes.reported.tolist() == [True, True, True, False]

    def run(tag, **kw):
        v, bm = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".bam"))
        st = pipeline.run(src, fa, v, bm, preset="hifi-masseq", threads=4, **kw)
        return st, open(v, "rb").read(), bamio.bgzf_decompress(bm)
    tsv = {m: str(tmp_path / (m + ".tsv")) for m in ("region", "plain", "patmat", "filter")}
    st_reg, vcf_reg, bam_reg = run("region", ase_out=tsv["region"])

    # the batch the pipeline cut, phased once more here
    prm = _abi.make_params("hifi-masseq", seed=2025)
    E = engine_cls(0, prm)
    E.load_batch(b).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    cands, coff = E.candidates()
    region_rec = E.ase()
    E.close()
    mps = float(prm.min_phase_score)
    # without ase_annotation: the table of regions, as before
    assert open(tsv["region"]).read() == ase.format_tsv([("chr20", region_rec, b.start0, b.len)], 10, 0.001)
    assert open(tsv["region"]).read() == ase.format_tsv([("chr20", ase_ref.regions(fm, pr["assignment"], pr["phase_set"], cands, coff, None, 13, mps), b.start0, b.len)], 10, 0.001)
    assert st_reg["ase_regions"] == 1 and "ase_genes" not in st_reg

    # the PASS phased records of the run's VCF as the script reads them; a parental and a DNA VCF from them
    rna = []
    for line in vcf_reg.decode().split("\n"):
        f = line.split("\t")
        if line.startswith("#") or len(f) < 10 or f[6] != "PASS" or len(f[3]) != 1 or len(f[4]) != 1:
            continue
        s = dict(zip(f[8].split(":"), f[9].split(":")))
        if s["GT"] in ("0|1", "1|0") and s.get("PS", ".") != ".":
            rna.append((int(f[1]) - 1, f[3], f[4], int(s["PS"]), int(s["DP"]), float(s["AF"])))
    assert len(rna) > 5
    parental = {pos: ((alt, ref) if k % 2 == 0 else (ref, alt)) for k, (pos, ref, alt, _, _, _) in enumerate(rna)}
    pvcf, dvcf = str(tmp_path / "parental.vcf"), str(tmp_path / "dna.vcf")
    open(pvcf, "w").write(VCF_HEAD + "".join("chr20\t%d\t.\t%s\t%s\t50\tPASS\t.\tGT\t%s\n" % (p + 1, r, a, "0|1" if k % 2 == 0 else "1|0")
                                              for k, (p, r, a, _, _, _) in enumerate(rna)))
    open(dvcf, "w").write(VCF_HEAD + "".join("chr20\t%d\t.\t%s\t%s\t50\tPASS\t.\tGT\t0/1\n" % (p + 1, r, a) for p, r, a, _, _, _ in rna[::2]))

    st = {"plain": run("plain", ase_out=tsv["plain"], ase_annotation=gtf),
          "patmat": run("patmat", ase_out=tsv["patmat"], ase_annotation=gtf, ase_parental_vcf=pvcf),
          "filter": run("filter", ase_out=tsv["filter"], ase_annotation=gtf, ase_dna_vcf=dvcf, ase_gene_types=("protein_coding", "lncRNA", "pseudogene"))}
    for m, (s, v, bm) in st.items():
        assert v == vcf_reg and bm == bam_reg, m                      # VCF and phased BAM do not depend on the option
        assert {k: x for k, x in s.items() if k != "ase_genes"} == {k: x for k, x in st_reg.items() if k != "ase_regions"}, m
    with pytest.raises(ValueError):
        pipeline.run(src, fa, str(tmp_path / "x.vcf"), ase_annotation=gtf)

    # the restatement: read -> gene, the pairs, one record per gene
    def table(genes, par, keep_fn=None):
        gene, _ = genes_ref.assign(b, genes)
        pairs, _ = genes_ref.pairs(fm, pr["assignment"], pr["phase_set"], cands, coff, gene, par, 13, mps)
        merged = genes_ref.genes_of(pairs)
        rec = np.array(merged, dtype=_abi.AGENE_DTYPE)
        if keep_fn is None:
            return [("chr20", rec, genes)]
        return [("chr20", rec, genes, np.array([keep_fn(int(r["phase_set"])) for r in rec], dtype=bool))]
    plain_t = table(genes, None)
    text = open(tsv["plain"]).read()
    print(text)
    assert text == ase.format_tsv(plain_t, 10, 0.001)
    names = [l.split("\t")[0] for l in text.split("\n")[1:-1]]
    assert "LEFT" in names and "RIGHT" in names and "PSEUDO" not in names and "RT" not in names and st["plain"][0]["ase_genes"] == len(names)
    pm = open(tsv["patmat"]).read()
    assert pm == ase.format_tsv(table(genes, parental), 10, 0.001, patmat=True) and pm.startswith(ase.HEADER_PATMAT)
    assert any(int(x) for l in pm.split("\n")[1:-1] for x in l.split("\t")[6:])

    # the filter mode by the script's route (DP and AF read off the VCF text), with the pseudogene kept by ase_gene_types
    dna = {r[0] for r in rna[::2]}
    kept = lambda chosen: any(ps == chosen and pos in dna and d >= 10 and ase.betabinom_two_sided(int(d * af), d, 0.5, 0.001) < 0.05
                              for pos, _, _, ps, d, af in rna if d != 0 and af == af)
    genes3 = annotation.load(gtf, ("protein_coding", "lncRNA", "pseudogene"))["chr20"]
    assert "g.pseudo" in genes3.gene_id
    flt = open(tsv["filter"]).read()
    assert flt == ase.format_tsv(table(genes3, None, kept), 10, 0.001)
    print(flt)


def test_pipeline_ase_annotation_over_several_chunks(engine_cls, tmp_path):
    """A synthetic ONT cDNA BAM of four regions cut into one chunk per region (chunk_cost=1): every chunk assigns its reads after
    binding and the pair records of the chunks are merged per gene -- one gene lies over regions 1 and 2, i.e. in two chunks.  The
    table equals the one-chunk run's and the text of the restatement's records on the whole batch, in the plain and the parental mode."""
    from longcallr_amd import synth
    import test_genes_gpu as tg
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
    # the batch the pipeline cuts, phased here in one piece
    prm = _abi.make_params("ont-cdna", seed=2025)
    nb = bamio.NativeBam(bam, 2)
    rs, re_ = nb.spans(0, **FLT)
    E = engine_cls(0, prm)
    regions = E.discover_regions(rs, re_, clen)
    b = nb.batch(0, [(s, l) for s, l, _ in regions], [seq[s:s + l] for s, l, _ in regions], **FLT)
    nb.close()
    assert b.n_regions == 4
    E.load_batch(b).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    cands, coff = E.candidates()
    E.close()
    mps = float(prm.min_phase_score)
    ex = [tg.region_exons(b, g) for g in range(4)]
    gtf = str(tmp_path / "genes.gtf")
    with open(gtf, "w") as f:
        for gid, exons in (("I0", ex[0][0::2]), ("I1", ex[0][1::2]), ("SPLIT", ex[1] + ex[2]), ("MAIN3", ex[3])):
            attrs = 'gene_id "%s"; gene_type "protein_coding"; gene_name "%s"; transcript_id "%s.t";' % (gid, gid.lower(), gid)
            f.write("\t".join(["chrS", "t", "gene", str(exons[0][0] + 1), str(exons[-1][1]), ".", "+", ".", attrs]) + "\n")
            for x, y in exons:
                f.write("\t".join(["chrS", "t", "exon", str(x + 1), str(y), ".", "+", ".", attrs]) + "\n")
    genes = annotation.load(gtf)["chrS"]
    assert sorted(genes.gene_id) == ["I0", "I1", "MAIN3", "SPLIT"]
    elig = [i for i in range(len(cands)) if ase_ref.pass_phased_het(cands[i:i + 1], mps) and int(cands["phase_set"][i]) != 0]
    parental, lines = {}, []
    for k, i in enumerate(elig):
        ref = chr(cands["ref_base"][i]).upper()
        alt = [chr(cands[a][i]) for a in ("allele1", "allele2") if chr(cands[a][i]) != ref][0]
        if ref not in "ACGT" or alt not in "ACGT":
            continue
        parental[int(cands["pos"][i])] = (alt, ref) if k % 2 == 0 else (ref, alt)
        lines.append("chrS\t%d\t.\t%s\t%s\t50\tPASS\t.\tGT\t%s\n" % (int(cands["pos"][i]) + 1, ref, alt, "0|1" if k % 2 == 0 else "1|0"))
    pvcf = str(tmp_path / "parental.vcf")
    open(pvcf, "w").write(VCF_HEAD.replace("chr20", "chrS") + "".join(lines))

    def run(tag, **kw):
        v, t = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".tsv"))
        st = pipeline.run(bam, fa, v, preset="ont-cdna", threads=4, read_filter=FLT, ase_out=t, ase_annotation=gtf, **kw)
        return st, open(v, "rb").read(), open(t).read()
    one = run("one")
    many = run("many", chunk_cost=1.0)
    many_pm = run("many_pm", chunk_cost=1.0, ase_parental_vcf=pvcf, devices=[0, 0])
    assert one[0]["chunks"] == 1 and many[0]["chunks"] == 4 == many_pm[0]["chunks"]
    assert many[1] == one[1] == many_pm[1] and many[2] == one[2]

    def text(par):
        gene, _ = genes_ref.assign(b, genes)
        pairs, _ = genes_ref.pairs(fm, pr["assignment"], pr["phase_set"], cands, coff, gene, par, 13, mps)
        assert sorted(int(r["region"]) for r in pairs if genes.gene_id[int(r["gene"])] == "SPLIT") == [1, 2]
        return ase.format_tsv([("chrS", np.array(genes_ref.genes_of(pairs), dtype=_abi.AGENE_DTYPE), genes)], 10, 0.001, patmat=par is not None)
    assert many[2] == text(None) and many[2].count("\n") == 5 and many[0]["ase_genes"] == 4
    assert many_pm[2] == text(parental)
    assert any(int(x) for l in many_pm[2].split("\n")[1:-1] for x in l.split("\t")[6:])

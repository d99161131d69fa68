"""pipeline.run(ase_out=...) on tests/golden/demo.bam in its three modes -- alone, with a parental VCF written from the run's own output
VCF, with a DNA VCF --: each table against ase.format_tsv of the restatement's records (tests/ase_ref.py) on the batch the pipeline
cuts, the row count in the stats, and VCF / phased BAM untouched by the option."""
import os

import numpy as np
import pytest

import ase_ref
import helpers
import test_downsample_pipeline_gpu as dp
from longcallr_amd import _abi, ase, bamio, pipeline

pytestmark = pytest.mark.gpu

VCF_HEAD = "##fileformat=VCFv4.2\n##contig=<ID=chr20>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"


def test_pipeline_ase_out(engine_cls, tmp_path):
    src = os.path.join(helpers.GOLDEN, "demo.bam")
    fa = dp.demo_fasta(tmp_path)
    b = helpers.demo_batch()

    def run(tag, **kw):
        v, bm = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".bam"))
        st = pipeline.run(src, fa, v, bm, preset="hifi-masseq", threads=4, **kw)
        assert st["regions"] == 1 and st["reads"] == b.n_reads
        return st, open(v, "rb").read(), bamio.bgzf_decompress(bm)
    st_off, vcf_off, bam_off = run("off")

    # the PASS phased records of the run's own VCF, as the script's load_longcallR_phased_vcf reads them
    rna = []     # (pos0, REF, ALT, PS, DP, AF)
    for line in vcf_off.decode().split("\n"):
        f = line.split("\t")
        if line.startswith("#") or len(f) < 10 or f[6] != "PASS" or len(f[3]) != 1 or len(f[4]) != 1:
            continue
        s = dict(zip(f[8].split(":"), f[9].split(":")))
        if s["GT"] in ("0|1", "1|0") and s.get("PS", ".") != ".":
            rna.append((int(f[1]) - 1, f[3], f[4], int(s["PS"]), int(s["DP"]), float(s["AF"])))
    assert len(rna) > 5
    # a parental VCF: every second record 1|0, one record unphased, one homozygous, an indel, a position the run does not call
    parental, lines = {}, []
    for k, (pos, ref, alt, _, _, _) in enumerate(rna):
        gt = ("0|1", "1|0", "0|1", "1|0", "0/1", "1|1")[k % 6]
        lines.append((pos, "chr20\t%d\t.\t%s\t%s\t50\tPASS\t.\tGT\t%s\n" % (pos + 1, ref, alt, gt)))
        if gt in ("0|1", "1|0"):
            parental[pos] = (alt, ref) if gt == "0|1" else (ref, alt)
    free = [p for p in range(rna[0][0] + 1, rna[0][0] + 200) if p not in {r[0] for r in rna}][:2]
    lines.append((free[0], "chr20\t%d\t.\tA\tC\t50\tPASS\t.\tGT\t0|1\n" % (free[0] + 1)))
    parental[free[0]] = ("C", "A")
    lines.append((free[1], "chr20\t%d\t.\tAT\tA\t50\tPASS\t.\tGT\t0|1\n" % (free[1] + 1)))
    pvcf, dvcf, dvcf2 = str(tmp_path / "parental.vcf"), str(tmp_path / "dna.vcf"), str(tmp_path / "dna2.vcf")
    open(pvcf, "w").write(VCF_HEAD + "".join(t for _, t in sorted(lines)))
    open(dvcf, "w").write(VCF_HEAD + "".join("chr20\t%d\t.\t%s\t%s\t50\tPASS\t.\tGT\t0/1\n" % (p + 1, r, a) for p, r, a, _, _, _ in rna))
    open(dvcf2, "w").write(VCF_HEAD + "chr20\t%d\t.\tA\tC\t50\tPASS\t.\tGT\t0/1\n" % (free[0] + 1))

    tsv = {m: str(tmp_path / (m + ".tsv")) for m in ("plain", "patmat", "filter", "filter2")}
    st = {"plain": run("plain", ase_out=tsv["plain"]),
          "patmat": run("patmat", ase_out=tsv["patmat"], ase_parental_vcf=pvcf),
          "filter": run("filter", ase_out=tsv["filter"], ase_dna_vcf=dvcf, asj_out=str(tmp_path / "j.tsv")),
          "filter2": run("filter2", ase_out=tsv["filter2"], ase_dna_vcf=dvcf2, ase_min_support=20, ase_overdispersion=0.01)}
    for m, (s, v, bm) in st.items():
        assert v == vcf_off and bm == bam_off, m
        assert {k: x for k, x in s.items() if k not in ("ase_regions", "junctions")} == st_off and "ase_regions" not in st_off, m
    with pytest.raises(ValueError):
        pipeline.run(src, fa, str(tmp_path / "x.vcf"), ase_out=tsv["plain"], ase_parental_vcf=pvcf, ase_dna_vcf=dvcf)
    with pytest.raises(ValueError):
        pipeline.run(src, fa, str(tmp_path / "x.vcf"), ase_parental_vcf=pvcf)

    # the batch the pipeline cut, phased once more here; its records by the restatement
    prm = _abi.make_params("hifi-masseq", seed=2025)
    E = engine_cls(0, prm)
    E.load_batch(b).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    cands, coff = E.candidates()
    E.close()
    mps = float(prm.min_phase_score)
    plain = ase_ref.regions(fm, pr["assignment"], pr["phase_set"], cands, coff, None, 13, mps)
    patmat = ase_ref.regions(fm, pr["assignment"], pr["phase_set"], cands, coff, parental, 13, mps)
    assert patmat["n_sites"][0] > 0 and any(int(patmat[f][0]) for f in ("h1_pat", "h1_mat", "h2_pat", "h2_mat"))
    tab = lambda rec, *keep: [("chr20", rec, b.start0, b.len) + keep]
    assert open(tsv["plain"]).read() == ase.format_tsv(tab(plain), 10, 0.001)
    assert open(tsv["patmat"]).read() == ase.format_tsv(tab(patmat), 10, 0.001, patmat=True)
    assert st["plain"][0]["ase_regions"] == st["patmat"][0]["ase_regions"] == 1 and open(tsv["plain"]).read().count("\n") == 2

    # the filter mode by the script's route: DP and AF read off the VCF text
    def kept(dna, min_support, rho):
        chosen = int(plain["phase_set"][0])
        return any(ps == chosen and pos in dna and d >= min_support and ase.betabinom_two_sided(int(d * af), d, 0.5, rho) < 0.05
                   for pos, _, _, ps, d, af in rna if d != 0 and af == af)
    k1, k2 = kept({r[0] for r in rna}, 10, 0.001), kept({free[0]}, 20, 0.01)
    print("demo.bam filter mode: kept %r / %r; plain %r; patmat %r" % (k1, k2, plain.tolist(), patmat.tolist()))
    assert not k2
    assert open(tsv["filter"]).read() == ase.format_tsv(tab(plain, np.array([k1])), 10, 0.001)
    assert open(tsv["filter2"]).read() == ase.HEADER + "\n" and st["filter2"][0]["ase_regions"] == 0
    assert st["filter"][0]["ase_regions"] == int(k1) and st["filter"][0]["junctions"] >= 0

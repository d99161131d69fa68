"""pipeline.run(downsample=...) on tests/golden/demo.bam: the VCF text and every read's HP / PS against records built from the CPU
reference (tests/downsample_ref.py), the engines' wiring (one context, two contexts, synchronous and asynchronous phase stage), and the
default arguments: files identical to a run that never names them."""
import os
import struct

import numpy as np
import pytest

import downsample_ref as dsr
import helpers
from longcallr_amd import _abi, bamio, pipeline, vcf

F = _abi
CUT = 1e-6
DEPTH = 500


def reference_records(cands0, sf):
    """the candidate records as the phase stage leaves them, from the reference's SNPs: every field lcr_phase writes"""
    out = cands0.copy()
    for c, s in zip(out, sf.candidate_snps):
        c["haplotype"], c["genotype"], c["variant_type"], c["phase_set"], c["phase_score"] = s.haplotype, s.genotype, s.variant_type, s.phase_set, s.phase_score
        fl = int(c["flags"]) & F.F_HET
        for bit, on in ((F.F_RNA_EDIT, s.rna_editing), (F.F_DENSE, s.dense), (F.F_FOR_PHASING, s.for_phasing), (F.F_HOM, s.hom_var),
                        (F.F_SINGLE, s.single), (F.F_NON_SELECTED, s.non_selected), (F.F_CAND_SOMATIC, s.cand_somatic)):
            fl |= bit if on else 0
        c["flags"] = fl
    return out


def demo_fasta(tmp_path):
    """chr19 / chr20 of demo.bam's header, N everywhere but the demo window (the pseudo-reference), with its .fai"""
    refs, _ = bamio.read_bam(os.path.join(helpers.GOLDEN, "demo.bam"))
    b = helpers.demo_batch()
    start0, length = int(b.start0[0]), int(b.len[0])
    fa = str(tmp_path / "pseudo.fa")
    with open(fa, "wb") as f, open(fa + ".fai", "w") as fi:
        for name, ln in refs:
            if name not in ("chr19", "chr20"):
                continue
            seq = np.full(ln, ord("N"), np.uint8)
            if name == "chr20":
                seq[start0:start0 + length] = helpers.load_pseudo_ref()
            f.write(b">" + name.encode() + b" pseudo\n" + seq.tobytes() + b"\n")
            fi.write("%s\t%d\t0\t%d\t%d\n" % (name, ln, ln, ln + 1))
    return fa


def body_of(path):
    return open(path).read().split("#CHROM")[1].split("\n", 1)[1]


@pytest.mark.gpu
def test_pipeline_downsample_on_demo_bam(engine_cls, tmp_path):
    src = os.path.join(helpers.GOLDEN, "demo.bam")
    fa = demo_fasta(tmp_path)
    b = helpers.demo_batch()
    prm = _abi.make_params("hifi-masseq", seed=2025, read_assign_cutoff=CUT)
    E = engine_cls(0, prm)
    E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps()
    cands0 = E.candidates()[0].copy()           # (the candidate stage is pinned by its own tests)
    E.get_fragments().set_downsample(DEPTH, 2025).phase()
    tc = E.tie_census()
    assert tc["delta_unresolved"] == tc["step_unresolved"] == tc["best_unresolved"] == tc["sigma_unresolved"] == 0, tc
    E.close()
    # the reference with the sample, and without it: the sample changes haplotypes, assignments and phase scores of this region
    sf, read_ps, app = dsr.run_region(b, 0, prm, cands0, depth=DEPTH, seed=2025)
    off, off_ps, _ = dsr.run_region(b, 0, prm, cands0)
    assert app and len(sf.fragments) > 3 * DEPTH and int(sf.sampled.sum()) == DEPTH
    assert [s.haplotype for s in sf.candidate_snps] != [s.haplotype for s in off.candidate_snps]
    assert [f.assignment for f in sf.fragments] != [f.assignment for f in off.fragments]
    want_on = vcf.format_records(reference_records(cands0, sf), "chr20", prm.min_phase_score)
    want_off = vcf.format_records(reference_records(cands0, off), "chr20", prm.min_phase_score)
    assert want_on != want_off and want_on.count("\n") > 5

    def run(tag, out_bam=True, **kw):
        o_vcf, o_bam = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".bam"))
        st = pipeline.run(src, fa, o_vcf, o_bam if out_bam else None, preset="hifi-masseq", threads=4, **kw)
        assert st["regions"] == 1 and st["reads"] == b.n_reads
        return o_vcf, o_bam

    on_vcf, on_bam = run("on", downsample=True, downsample_depth=DEPTH, read_assign_cutoff=CUT)
    assert body_of(on_vcf) == want_on
    # every engine of the list gets the setting, in both forms of the phase stage
    v, _ = run("on2", out_bam=False, downsample=True, downsample_depth=DEPTH, read_assign_cutoff=CUT, devices=[0, 0], async_phase=False)
    assert open(v).read() == open(on_vcf).read()
    # phased BAM: HP / PS of every fragment row as the reference assigns them (thread.rs:204-214, 307-361)
    _, recs = bamio.read_bam(src)
    keep = [r for r in recs if bamio.passes_filter(r, **_abi.READ_FILTER)]
    _, out_recs = bamio.read_bam(on_bam, keep_raw=True)
    by_name = {}
    for r in out_recs:
        by_name.setdefault(r["name"], r)
    n_tagged = n_unsampled_tagged = 0
    for row, f in enumerate(sf.fragments):
        r = by_name[keep[int(f.read)]["name"]]
        aux = r["raw"][r["aux_off"]:]
        a, ps = int(f.assignment), int(read_ps.get(row, 0))
        assert (b"HPi" + struct.pack("<i", a) in aux) == (a in (1, 2)), row
        assert (b"PSI" + struct.pack("<I", ps) in aux) == (ps != 0), row
        n_tagged += a in (1, 2)
        n_unsampled_tagged += a in (1, 2) and not f.downsampled
    assert n_tagged > DEPTH and n_unsampled_tagged > 0      # the last round assigns the reads outside the sample too

    # off: the arguments at their defaults, and a depth no region reaches, give the files of a run that never names them
    base_vcf, base_bam = run("base", read_assign_cutoff=CUT)
    assert body_of(base_vcf) == want_off
    for tag, kw in (("dflt", dict(downsample=False, downsample_depth=10000, downsample_seed=2025)),
                    ("deep", dict(downsample=True))):                    # (10 000 fragments: more than the region has)
        v, bm = run(tag, read_assign_cutoff=CUT, **kw)
        assert open(v, "rb").read() == open(base_vcf, "rb").read()
        assert bamio.bgzf_decompress(bm) == bamio.bgzf_decompress(base_bam)


def test_pipeline_refuses_downsample_without_a_positive_cutoff(tmp_path):
    """the presets' read_assign_cutoff is 0.0, which lcr_phase refuses while down-sampling is on: pipeline.run says so before it opens
    a file or a device, and names the argument"""
    nowhere = str(tmp_path / "missing")
    with pytest.raises(ValueError, match="read_assign_cutoff"):
        pipeline.run(nowhere + ".bam", nowhere + ".fa", nowhere + ".vcf", downsample=True)
    with pytest.raises(ValueError, match="read_assign_cutoff"):
        pipeline.run(nowhere + ".bam", nowhere + ".fa", nowhere + ".vcf", downsample=True, downsample_depth=5, read_assign_cutoff=0.0)
    for kw in (dict(), dict(downsample=True, downsample_depth=0), dict(downsample=True, read_assign_cutoff=CUT)):
        with pytest.raises(FileNotFoundError):           # (past the check: the missing .fai)
            pipeline.run(nowhere + ".bam", nowhere + ".fa", nowhere + ".vcf", **kw)

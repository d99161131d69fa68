"""pipeline.run(pairs_out=..., mnv_out=...): on tests/golden/demo.bam the pair table against pairs.format_pairs_tsv over direct Engine
calls and against the restatement's text (tests/site_pairs_ref.py), VCF and phased BAM untouched by the options, the new stats; on a
synthetic BAM of two haplotypes (written through lcr_bam_write_reads) with an adjacent het pair in cis, one in trans, an adjacent 1/1 pair
and a cis pair two apart: the MNV file holds exactly the three merged records, the trans pair shows in the pair table only, and no phase is
contradicted.  pairs.callable_gt is pinned against the main VCF's own lines on both."""
import os

import numpy as np
import pytest

import helpers
import site_pairs_ref as ref
import test_downsample_pipeline_gpu as dp
import test_junctions_gpu as tj
import test_site_counts_gpu as ts
from longcallr_amd import _abi, bamio, pairs, pipeline

pytestmark = pytest.mark.gpu

FLT = dict(min_mapq=0, min_read_length=0, divergence=2.0)
NEW = ("site_pairs", "phase_disagreements", "mnv_records")


def callable_matches_the_vcf(cands, chrom, mps):
    got = [pairs.callable_gt(s, mps) for s in cands]
    want = [ref.vcf_callable(s, chrom, mps) for s in cands]
    assert got == want, [(int(cands["pos"][i]), got[i], want[i]) for i in range(len(cands)) if got[i] != want[i]]
    return got


def test_pipeline_pairs_out_on_demo(engine_cls, tmp_path):
    src = os.path.join(helpers.GOLDEN, "demo.bam")
    fa = dp.demo_fasta(tmp_path)
    b = helpers.demo_batch()
    p = lambda name: str(tmp_path / name)

    def run(tag, **kw):
        st = pipeline.run(src, fa, p(tag + ".vcf"), p(tag + ".bam"), preset="hifi-masseq", threads=4, **kw)
        assert st["regions"] == 1 and st["reads"] == b.n_reads
        return st, open(p(tag + ".vcf"), "rb").read(), bamio.bgzf_decompress(p(tag + ".bam"))
    st_off, vcf_off, bam_off = run("off")
    st_on, vcf_on, bam_on = run("on", pairs_out=p("on.pairs.tsv"), mnv_out=p("on.mnv.vcf"))
    st_q, vcf_q, bam_q = run("q", pairs_out=p("q.pairs.tsv"), pairs_partners=1, pairs_min_count=3, pairs_min_baseq=30)
    assert vcf_on == vcf_off and bam_on == bam_off and vcf_q == vcf_off and bam_q == bam_off
    assert not any(k in st_off for k in NEW) and {k: x for k, x in st_on.items() if k not in NEW} == st_off
    assert {k: x for k, x in st_q.items() if k not in NEW} == st_off and "mnv_records" not in st_q

    # the batch the pipeline cut, phased once more here
    prm = _abi.make_params("hifi-masseq", seed=2025)
    mps = float(prm.min_phase_score)
    E = engine_cls(0, prm)
    E.load_batch(b).run_all()
    fm = E.fragmat()
    cands, _ = E.candidates()
    got = E.site_pairs("phased", 2, 0, 13)
    got_q = E.site_pairs("phased", 1, 0, 30)
    got_m = E.site_pairs("all", 2, 2, 13)
    E.close()
    want, want_q, want_m = ref.of_engine(fm, cands, "phased", 2, 0, 13), ref.of_engine(fm, cands, "phased", 1, 0, 30), ref.of_engine(fm, cands, "all", 2, 2, 13)
    for g, w in ((got, want), (got_q, want_q), (got_m, want_m)):
        assert g[0].tobytes() == w[0].tobytes() and g[1].tobytes() == w[1].tobytes() and g[2] == w[2]
    text = open(p("on.pairs.tsv")).read()
    assert text == pairs.format_pairs_tsv([("chr20", cands, want[0])], 10, mps) == ref.format_pairs_tsv([("chr20", cands, want[0])], 10, mps)
    text_q = open(p("q.pairs.tsv")).read()
    assert text_q == pairs.format_pairs_tsv([("chr20", cands, want_q[0])], 3, mps) == ref.format_pairs_tsv([("chr20", cands, want_q[0])], 3, mps)
    rows = [l.split("\t") for l in text.splitlines()[1:]]
    assert st_on["site_pairs"] == want[0].size > 0 and st_q["site_pairs"] == want_q[0].size
    assert st_on["phase_disagreements"] == sum(r[18] == "disagree" for r in rows)
    print("demo.bam --pairs-out: %d pairs, %d rows at min_count 10: %r; at partners 1, min_count 3, min_baseq 30: %d rows" % (
        want[0].size, len(rows), {k: sum(r[18] == k for r in rows) for k in ("agree", "disagree", ".")}, text_q.count("\n") - 1))
    # a site may be part of an MNV exactly where the main VCF prints a PASS line with GT 0|1, 1|0 or 1/1 and one ALT
    gts = callable_matches_the_vcf(cands, "chr20", mps)
    body = {int(f[1]): f for f in (l.split("\t") for l in dp.body_of(p("on.vcf")).split("\n") if l)}
    for s, gt in zip(cands, gts):
        f = body.get(int(s["pos"]) + 1)
        assert (gt is not None) == (f is not None and f[6] == "PASS" and "," not in f[4] and f[9].split(":")[0] in ("0|1", "1|0", "1/1"))
        assert gt is None or f[9].split(":")[0] == gt
    # the MNV file against both forms of the host arithmetic
    refseq = np.asarray(b.ref, np.uint8)
    recs = pairs.mnv_records(cands, want_m[0], want_m[1], refseq, int(b.start0[0]), mps, 2, 3, 0.8, 2)
    assert [(m["pos0"], m["ref"], m["alt"], m["qual"], m["gt"], m["ps"], m["dp"], m["sites"], m["rb"]) for m in recs] == \
        ref.mnv_records(cands, want_m[0], want_m[1], refseq, int(b.start0[0]), mps, 2, 3, 0.8, 2)
    mnv = open(p("on.mnv.vcf")).read()
    assert "".join(l + "\n" for l in mnv.splitlines() if not l.startswith("#")) == pairs.format_mnv_vcf([("chr20", recs)], ["chr20"])[0]
    assert st_on["mnv_records"] == len(recs) and "ID=SITES" in mnv and "ID=RB" in mnv
    print("demo.bam --mnv-out: %d records of %d callable sites" % (len(recs), sum(g is not None for g in gts)))


S0, LEN = 5000, 1500
ANCHORS = (150, 300, 450, 600, 850, 1150, 1300, 1400)
CIS, TRANS, HOM, CIS2 = (700, 701), (900, 901), (1000, 1001), (1210, 1212)


def planted_batch():
    """40 reads over [S0, S0 + LEN), alternating haplotypes: haplotype 2 carries the alternate base at the anchors, at both sites of CIS and
    CIS2 and at the first site of TRANS; haplotype 1 at the second site of TRANS; every read at both sites of HOM"""
    probe = ts.region(S0, LEN, {}, [], 71)[1]
    alt = lambda cols: {c: tj.ALT[probe[c]] for c in cols}
    h2 = {**alt(ANCHORS + CIS + CIS2 + TRANS[:1] + HOM)}
    h1 = {**alt(TRANS[1:] + HOM)}
    reads = [([(0, LEN)], h2 if k % 2 else h1, {}) for k in range(40)]
    reg = ts.region(S0, LEN, {}, reads, 71)
    return tj.batch_of([reg]), reg[1]


def test_pipeline_mnv_out_on_planted_pairs(engine_cls, tmp_path):
    src, refseq = planted_batch()
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "ref.fa")
    clen = bamio.write_reads_bam(bam, src, "chrS")
    seq = np.full(clen, ord("N"), np.uint8)
    seq[S0:S0 + LEN] = src.ref
    with open(fa, "wb") as f, open(fa + ".fai", "w") as fi:
        f.write(b">chrS\n" + seq.tobytes() + b"\n")
        fi.write("chrS\t%d\t6\t%d\t%d\n" % (clen, clen, clen + 1))

    def run(tag, **kw):
        v, bm = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".bam"))
        st = pipeline.run(bam, fa, v, bm, preset="hifi-masseq", threads=4, read_filter=FLT, **kw)
        return st, open(v, "rb").read(), bamio.bgzf_decompress(bm)
    out, tsv = str(tmp_path / "out.mnv.vcf"), str(tmp_path / "out.pairs.tsv")
    st_on, vcf_on, bam_on = run("on", mnv_out=out, pairs_out=tsv)
    st_off, vcf_off, bam_off = run("off")
    assert vcf_on == vcf_off and bam_on == bam_off and {k: v for k, v in st_on.items() if k not in NEW} == st_off
    main = {int(f[1]) - 1 - S0: f for f in (ln.split("\t") for ln in vcf_on.decode().splitlines() if not ln.startswith("#"))}
    fmt = lambda f: dict(zip(f[8].split(":"), f[9].split(":")))
    planted = CIS + TRANS + HOM + CIS2
    assert all(c in main and main[c][6] == "PASS" for c in planted), {c: main.get(c) for c in planted}
    main_ps = {fmt(main[c])["PS"] for c in CIS + TRANS + CIS2}
    assert len(main_ps) == 1 and all(fmt(main[c])["GT"] == "1/1" for c in HOM)
    assert fmt(main[CIS[0]])["GT"] == fmt(main[CIS[1]])["GT"] == fmt(main[CIS2[0]])["GT"] == fmt(main[CIS2[1]])["GT"] == fmt(main[TRANS[0]])["GT"] != fmt(main[TRANS[1]])["GT"]

    # exactly the three merged records; the constituent sites stay in the main VCF (above)
    body = [ln.split("\t") for ln in open(out).read().splitlines() if not ln.startswith("#")]
    alt_of = lambda cols, lo, hi: "".join(tj.ALT[refseq[c]] if c in cols else refseq[c] for c in range(lo, hi + 1))
    assert [int(r[1]) - 1 - S0 for r in body] == [CIS[0], HOM[0], CIS2[0]]
    for r, cols in zip(body, (CIS, HOM, CIS2)):
        f = fmt(r)
        assert (r[3], r[4], r[6]) == (refseq[cols[0]:cols[-1] + 1], alt_of(cols, cols[0], cols[-1]), "PASS"), r
        assert f["GT"] == fmt(main[cols[0]])["GT"] and f["PS"] == ("." if cols == HOM else next(iter(main_ps))) and int(f["DP"]) == min(int(fmt(main[c])["DP"]) for c in cols)
        assert r[7] == "RDS=mnv;SITES=%s;RB=%s" % (",".join(str(S0 + c + 1) for c in cols), "40,0,0,0" if cols == HOM else "20,0,0,20")
        assert int(r[5]) == min(int(main[c][5]) for c in cols)
    assert st_on["mnv_records"] == 3

    # the trans pair: in no MNV record, "trans" in the pair table, in agreement with the phase -- like every other row
    rows = {(int(l[1]) - 1 - S0, int(l[2]) - 1 - S0): l for l in (ln.split("\t") for ln in open(tsv).read().splitlines()[1:])}
    assert rows[TRANS][11:19] == ["0", "20", "20", "0", "0", "0", "trans", "agree"]
    assert rows[CIS][11:19] == ["20", "0", "0", "20", "0", "0", "cis", "agree"] and rows[CIS2][17:19] == ["cis", "agree"]
    assert all(l[18] == "agree" for l in rows.values()) and st_on["phase_disagreements"] == 0 and st_on["site_pairs"] >= len(rows) > 0
    assert not any(c in HOM for k in rows for c in k)         # (the table pairs phased hets only)

    # the batch the pipeline cut (one chunk), phased once more here: both files against the restatement
    nb = bamio.NativeBam(bam, 2)
    rs, re_ = nb.spans(0, **FLT)
    prm = _abi.make_params("hifi-masseq", seed=2025)
    mps = float(prm.min_phase_score)
    E = engine_cls(0, prm)
    regions = E.discover_regions(rs, re_, clen)
    batch = nb.batch(0, [(s_, l_) for s_, l_, _ in regions], [seq[s_:s_ + l_] for s_, l_, _ in regions], **FLT)
    nb.close()
    E.load_batch(batch).run_all()
    fm = E.fragmat()
    cands, _ = E.candidates()
    got_p, got_m = E.site_pairs("phased", 2, 0, 13), E.site_pairs("all", 2, 2, 13)
    E.close()
    want_p, want_m = ref.of_engine(fm, cands, "phased", 2, 0, 13), ref.of_engine(fm, cands, "all", 2, 2, 13)
    assert got_p[0].tobytes() == want_p[0].tobytes() and got_m[0].tobytes() == want_m[0].tobytes() and got_m[1].tobytes() == want_m[1].tobytes()
    assert open(tsv).read() == ref.format_pairs_tsv([("chrS", cands, want_p[0])], 10, mps)
    want_recs = ref.mnv_records(cands, want_m[0], want_m[1], seq, 0, mps, 2, 3, 0.8, 2)
    assert [(int(r[1]) - 1, r[3], r[4], int(r[5]), fmt(r)["GT"]) for r in body] == [m[:5] for m in want_recs]
    callable_matches_the_vcf(cands, "chrS", mps)
    for bad in (dict(pairs_partners=9), dict(mnv_max_dist=0), dict(mnv_min_frac=2.0)):
        with pytest.raises(ValueError):
            pipeline.run(bam, fa, str(tmp_path / "bad.vcf"), None, preset="hifi-masseq", mnv_out=out, **bad)

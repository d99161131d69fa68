"""pipeline.run(truncation=...) on tests/golden/demo.bam at a cap of 1648: the two flanks of the over-deep stretch as regions of their
own -- VCF text and phased BAM against an engine run on the batch the Python restatements build from the restated regions
(tests/truncation_ref.py), the engines' wiring, user-provided sites, and the default arguments."""
import os

import numpy as np
import pytest

import helpers
import truncation_ref as tr
from longcallr_amd import _abi, bamio, pipeline, vcf
from oracle import oracle_np

pytestmark = pytest.mark.gpu

CAP = 1648
DEMO_LEN = 64444167


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


def positions(body):
    return [int(line.split("\t")[1]) - 1 for line in body.splitlines()]


@pytest.fixture(scope="module")
def demo():
    """demo.bam's filtered records, the restated regions at CAP and the batch the Python restatements build on them"""
    src = os.path.join(helpers.GOLDEN, "demo.bam")
    _, recs = bamio.read_bam(src, keep_raw=True)
    keep = [r for r in recs if bamio.passes_filter(r, **_abi.READ_FILTER)]
    rid = keep[0]["ref_id"]
    spans = [(r["pos"], r["pos"] + max(r["ref_len"], 1)) for r in keep]
    regions, n_trunc = tr.discover(spans, DEMO_LEN, True, CAP)
    assert len(regions) == 2 and n_trunc > 0
    b = helpers.demo_batch()
    w0, full = int(b.start0[0]), helpers.load_pseudo_ref()
    wins = [full[s - w0:s - w0 + l] for s, l, _ in regions]
    batch = bamio.build_batch(keep, [(s, l) for s, l, _ in regions], wins)
    stretch = (regions[0][0] + regions[0][1], regions[1][0])        # [first column above the cap, first column of the second region)
    return dict(src=src, recs=recs, keep=keep, rid=rid, spans=spans, regions=regions, n_trunc=n_trunc, batch=batch, stretch=stretch)


def test_pipeline_truncation_on_demo_bam(engine_cls, orc, demo, tmp_path):
    fa = demo_fasta(tmp_path)
    regions, batch, (t_lo, t_hi) = demo["regions"], demo["batch"], demo["stretch"]
    prm = _abi.make_params("hifi-masseq", seed=2025)
    # a read that spans the stretch is fetched for both regions
    rb = batch.read_begin
    names0, names1 = set(batch.names[rb[0]:rb[1]]), set(batch.names[rb[1]:rb[2]])
    both = names0 & names1
    assert len(both) > 0
    E = engine_cls(0, prm)
    E.load_batch(batch).run_all()
    cands, off = E.candidates()
    cands, off = cands.copy(), off.copy()
    fm, pr = E.fragmat(), E.phase_result()
    row_names = [batch.names[r] for r in fm["row_read"]]
    asg, ps = pr["assignment"].astype(np.int32), pr["phase_set"].copy()
    hp = np.where((fm["row_for_phasing"] != 0) | (asg != 0), asg, -1)
    E.close()
    want = "".join(vcf.format_records(cands[off[g]:off[g + 1]], "chr20", prm.min_phase_score) for g in range(2))
    for g in range(2):      # the candidates of both flanks against the CPU oracle
        R = orc.Region(batch, g, prm).set_fast(1).pileup()
        R.candidates()
        R.fragments()
        R.set_tie_mask(orc.TIE_MASK_LIBLCR).phase(orc.MODE_TIE).post_phase()
        text = vcf.format_records(cands[off[g]:off[g + 1]], "chr20", prm.min_phase_score)
        assert text == R.vcf_text("chr20"), g
        assert text.count("\n") >= 1                               # both regions yield records

    def run(tag, out_bam=True, **kw):
        o_vcf, o_bam = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".bam"))
        st = pipeline.run(demo["src"], fa, o_vcf, o_bam if out_bam else None, preset="hifi-masseq", threads=4, **kw)
        return st, o_vcf, o_bam

    st, on_vcf, on_bam = run("on", truncation=True, truncation_coverage=CAP)
    assert st["regions"] == 2 and st["truncated_columns"] == demo["n_trunc"] == t_hi - t_lo
    assert st["reads"] == batch.n_reads and st["candidates"] == cands.size
    body = body_of(on_vcf)
    assert body == want
    pos = positions(body)
    assert all(regions[0][0] <= p < t_lo or t_hi <= p < regions[1][0] + regions[1][1] for p in pos)    # none in the stretch
    assert any(p < t_lo for p in pos) and any(p >= t_hi for p in pos)
    st_off, off_vcf, off_bam = run("off")
    assert "truncated_columns" not in st_off and st_off["regions"] == 1
    assert body_of(off_vcf) != body

    # phased BAM (thread.rs:307-361): the records contained in a region, HP / PS from the first entry of a name
    reg3 = [(demo["rid"], s, l) for s, l, _ in regions]
    stream = bamio.bgzf_decompress(on_bam)
    assert stream == bamio.phased_stream(demo["recs"], reg3, row_names, hp, ps)
    assert stream != bamio.bgzf_decompress(off_bam)
    recs = demo["recs"]
    tup = [(r["ref_id"], r["pos"], r["pos"] + (r["ref_len"] if r["ref_len"] > 0 else 1), r["flag"], r["name"],
            bamio_has(r, b"HP"), bamio_has(r, b"PS")) for r in recs]
    want_recs = oracle_np.phased_bam_records(tup, [(rid, s + 1, s + l + 1) for rid, s, l in reg3],
                                             [(n, int(h)) for n, h in zip(row_names, hp) if h >= 0], [(n, int(p)) for n, p in zip(row_names, ps) if p != 0])
    _, got = bamio.read_bam(on_bam, keep_raw=True)
    assert len(got) == len(want_recs) > 0
    first_hp, first_ps = {}, {}
    for n, h, p in zip(row_names, hp, ps):
        if h >= 0:
            first_hp.setdefault(n, int(h))
        if p != 0:
            first_ps.setdefault(n, int(p))
    for g, (idx, h, p) in zip(got, want_recs):
        assert (g["name"], g["pos"]) == (recs[idx]["name"], recs[idx]["pos"])
        extra = (b"" if h is None else b"HPi" + np.int32(h).tobytes()) + (b"" if p is None else b"PSI" + np.uint32(p).tobytes())
        assert g["raw"] == recs[idx]["raw"] + extra, g["name"]
        assert h in (None, first_hp.get(g["name"])) and p in (None, first_ps.get(g["name"]))
    # a read that crosses the stretch is contained in neither region (thread.rs:340-345): it is not written, although it has rows (and
    # so entries in the name maps) in both; the disjoint regions leave no record that is listed twice AND written, so the first-entry
    # rule reaches the file only through the maps compared above
    written = {g["name"] for g in got}
    crossing = {r["name"] for r in demo["keep"] if r["pos"] < t_lo and r["pos"] + max(r["ref_len"], 1) > t_hi}
    assert crossing and (crossing & both) and not (crossing & written) and not (both & written)
    assert sum(n in both for n in row_names) > len(set(n for n in row_names if n in both))     # listed twice in the maps' input

    # the same files from every configuration
    for tag, kw in (("two", dict(devices=[0, 0])), ("chunks", dict(chunk_cost=1.0)), ("sync", dict(async_phase=False)),
                    ("all", dict(devices=[0, 0], chunk_cost=1.0, async_phase=False))):
        st2, v, bm = run(tag, truncation=True, truncation_coverage=CAP, **kw)
        assert st2["regions"] == 2 and st2["truncated_columns"] == demo["n_trunc"]
        assert open(v, "rb").read() == open(on_vcf, "rb").read(), tag
        assert bamio.bgzf_decompress(bm) == stream, tag

    # defaults: the switch off at any cap writes the files of a run that names neither argument, with the same stats
    st3, v, bm = run("dflt", truncation=False, truncation_coverage=5)
    assert st3 == st_off
    assert open(v, "rb").read() == open(off_vcf, "rb").read()
    assert bamio.bgzf_decompress(bm) == bamio.bgzf_decompress(off_bam)


def bamio_has(r, tag):
    """whether the record's aux block carries the tag (the types demo.bam and the writer use)"""
    raw, q = r["raw"], r["aux_off"]
    size = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while q + 3 <= len(raw):
        if raw[q:q + 2] == tag:
            return True
        typ = chr(raw[q + 2])
        q += 3
        if typ in size:
            q += size[typ]
        elif typ in "ZH":
            q = raw.index(b"\0", q) + 1
        elif typ == "B":
            q += 5 + int.from_bytes(raw[q + 1:q + 5], "little") * size[chr(raw[q])]
        else:
            raise ValueError(typ)
    return False


def test_pipeline_truncation_with_input_vcf(engine_cls, demo, tmp_path):
    """user-provided sites: one inside the truncated stretch gives no record, the ones in the flanks do"""
    fa = demo_fasta(tmp_path)
    regions, batch, (t_lo, t_hi) = demo["regions"], demo["batch"], demo["stretch"]
    prm = _abi.make_params("hifi-masseq", seed=2025)
    E = engine_cls(0, prm)
    E.load_batch(batch).fill_data_into_freq_vec().get_candidate_snps()
    p = E.candidates()[0]["pos"].astype(np.int64)
    assert (p < t_lo).any() and (p >= t_hi).any()
    g, q = np.ones(p.size, np.uint8), np.full(p.size, 30.0, np.float32)
    E.fill_data_into_freq_vec().import_external_candidates(p, g, q).get_fragments().phase()
    want = vcf.format_records(E.candidates()[0], "chr20", prm.min_phase_score)
    E.close()
    inside = (t_lo + t_hi) // 2
    sites = sorted(p.tolist() + [inside])
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"]
    lines += ["chr20\t%d\t.\tA\tG\t30.0\tPASS\t.\tGT\t0/1" % (x + 1) for x in sites]
    path = str(tmp_path / "sites.vcf")
    open(path, "w").write("\n".join(lines) + "\n")
    for tag, kw in (("one", dict()), ("chunks", dict(chunk_cost=1.0))):
        out_vcf = str(tmp_path / (tag + ".vcf"))
        st = pipeline.run(demo["src"], fa, out_vcf, None, preset="hifi-masseq", threads=4, input_vcf=path, truncation=True, truncation_coverage=CAP, **kw)
        assert st["regions"] == 2 and st["input_sites"] == len(sites)
        body = body_of(out_vcf)
        assert body == want
        pos = positions(body)
        assert inside not in pos and not any(t_lo <= x < t_hi for x in pos)
        assert any(x < t_lo for x in pos) and any(x >= t_hi for x in pos)

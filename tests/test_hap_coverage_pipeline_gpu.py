"""pipeline.run(hap_coverage_out=...) on tests/golden/demo.bam: VCF, phased BAM and the shared stats untouched by the option; the three
bedGraph files parse, are sorted and non-overlapping and add up to the stats; in a plain run and behind lcr_haplotag the tracks equal the
depth the restatement (tests/hap_coverage_ref.py) computes from the reads bamio's pure-Python decoder yields under the same read filter,
classed by the HP tags of the phased BAM the same run wrote; with truncation a read that spans the cut is counted in each flank inside
that flank's window only.

In the truncation run a read that spans the cut is listed in both flanks and classed in each by that flank's own row, while the BAM
writer gives a name the tag of its FIRST entry (first-name-wins, thread.rs:307-361): there the reads are classed from Engine results on
the batch the restated regions give, not from the tags."""
import os

import numpy as np
import pytest

import hap_coverage_ref as ref
import helpers
import test_downsample_pipeline_gpu as dp
import truncation_ref as tr
from longcallr_amd import _abi, bamio, pipeline

pytestmark = pytest.mark.gpu

CAP = 1648                  # test_truncation_pipeline_gpu's cap: it cuts demo.bam's region in two
DEMO_LEN = 64444167
FILES = ((0, "unassigned"), (1, "h1"), (2, "h2"))


def parse(prefix, k, name):
    """one track -> [(start, end, value)]; the lines are the contig's, sorted and non-overlapping, values positive"""
    rows = []
    for line in open("%s.%s.bedgraph" % (prefix, name)).read().splitlines():
        c, s, e, v = line.split("\t")
        assert c == "chr20" and not line.startswith(("track", "#"))
        rows.append((int(s), int(e), int(v)))
    assert all(s < e and v > 0 for s, e, v in rows)
    assert all(a[1] <= b[0] for a, b in zip(rows, rows[1:]))
    assert all(not (a[1] == b[0] and a[2] == b[2]) for a, b in zip(rows, rows[1:]))      # abutting equal values are merged
    return rows


def dense_of(rows, start0, length):
    d = np.zeros(length, np.int64)
    for s, e, v in rows:
        assert start0 <= s and e <= start0 + length
        d[s - start0:e - start0] = v
    return d


def hp_tags(bam_path):
    """name -> HP of the phased BAM (the writer appends HP:i and PS:I to a record's bytes); a record without the tag is absent"""
    out = {}
    for r in bamio.read_bam(bam_path, keep_raw=True)[1]:
        raw = r["raw"]
        if raw[-7:-4] == b"PSI":
            raw = raw[:-7]
        if raw[-7:-4] == b"HPi":
            out.setdefault(r["name"], int(np.frombuffer(raw[-4:], "<i4")[0]))
    return out


def reads_of(recs):
    return [(int(r["pos"]), [(int(w) >> 4, int(w) & 15) for w in r["cigar"]]) for r in recs]


def test_pipeline_hap_coverage_out(engine_cls, tmp_path):
    src = os.path.join(helpers.GOLDEN, "demo.bam")
    fa = dp.demo_fasta(tmp_path)
    b = helpers.demo_batch()
    start0, length = int(b.start0[0]), int(b.len[0])
    _, recs = bamio.read_bam(src)
    keep = [r for r in recs if bamio.passes_filter(r, **_abi.READ_FILTER)]
    assert len({r["name"] for r in keep}) == len(keep) == b.n_reads
    p = lambda name: str(tmp_path / name)

    def run(tag, **kw):
        st = pipeline.run(src, fa, p(tag + ".vcf"), p(tag + ".bam"), preset="hifi-masseq", threads=4, **kw)
        return st, open(p(tag + ".vcf"), "rb").read(), bamio.bgzf_decompress(p(tag + ".bam"))

    def against_tags(tag, st):
        """the three tracks of run `tag` against the restatement over the decoded reads, classed by the run's own HP tags"""
        hp = hp_tags(p(tag + ".bam"))
        cls = [hp.get(r["name"], 0) if hp.get(r["name"], 0) in (1, 2) else 0 for r in keep]
        want, nr = ref.dense(start0, length, reads_of(keep), cls)
        print("%s: %d records with an HP tag, reads per class by the tags %r" % (tag, len(hp), nr))
        assert nr[1] > 0 and nr[2] > 0 and nr[0] > 0
        total = []
        for k, name in FILES:
            rows = parse(p(tag + ".cov"), k, name)
            assert (dense_of(rows, start0, length) == want[k].astype(np.int64)).all(), name
            total.append(sum((e - s) * v for s, e, v in rows))
        assert tuple(total) == st["hap_coverage_bases"] == tuple(int(want[k].sum()) for k in range(3))
        assert st["hap_coverage_segments"] == len(ref.encode(0, start0, want))
        return nr, total

    st_off, vcf_off, bam_off = run("off")
    st_on, vcf_on, bam_on = run("on", hap_coverage_out=p("on.cov"))
    assert vcf_on == vcf_off and bam_on == bam_off
    assert "hap_coverage_segments" not in st_off and "hap_coverage_bases" not in st_off
    assert {k: x for k, x in st_on.items() if k not in ("hap_coverage_segments", "hap_coverage_bases")} == st_off
    assert st_on["regions"] == 1 and st_on["reads"] == b.n_reads
    nr, total = against_tags("on", st_on)
    print("demo.bam --hap-coverage-out: reads per class %r, bases per class %r, segments %d" % (nr, total, st_on["hap_coverage_segments"]))

    # once more behind lcr_haplotag: the run's own VCF fed back, the labels are the input's
    st_h, vcf_h, bam_h = run("hap", input_vcf=p("off.vcf"), haplotag=True)
    st_hc, vcf_hc, bam_hc = run("hapc", input_vcf=p("off.vcf"), haplotag=True, hap_coverage_out=p("hapc.cov"))
    assert vcf_hc == vcf_h and bam_hc == bam_h
    assert {k: x for k, x in st_hc.items() if k not in ("hap_coverage_segments", "hap_coverage_bases")} == st_h
    against_tags("hapc", st_hc)

    # truncation at a cap that cuts the region: the flanks' windows, every read classed by its flank's own row
    spans = [(r["pos"], r["pos"] + max(r["ref_len"], 1)) for r in keep]
    regions, n_trunc = tr.discover(spans, DEMO_LEN, True, CAP)
    assert len(regions) == 2 and n_trunc > 0
    full = helpers.load_pseudo_ref()
    batch = bamio.build_batch(keep, [(s, l) for s, l, _ in regions], [full[s - start0:s - start0 + l] for s, l, _ in regions])
    rb = batch.read_begin
    both = set(batch.names[rb[0]:rb[1]]) & set(batch.names[rb[1]:rb[2]])
    assert len(both) > 0                                              # reads that span the cut are listed in both flanks
    st_t, vcf_t, bam_t = run("trunc", truncation=True, truncation_coverage=CAP, hap_coverage_out=p("trunc.cov"))
    st_t0, vcf_t0, bam_t0 = run("trunc0", truncation=True, truncation_coverage=CAP)
    assert vcf_t == vcf_t0 and bam_t == bam_t0 and st_t["regions"] == 2 and st_t["reads"] == batch.n_reads
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=2025))
    E.load_batch(batch).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    E.close()
    cls = ref.classes(batch.n_reads, [int(x) for x in rb], fm["row_region_off"], fm["row_read"], pr["assignment"])
    reads = ref.batch_reads(batch)
    t_lo, t_hi = regions[0][0] + regions[0][1], regions[1][0]        # the stretch between the flanks
    total = [0, 0, 0]
    tracks = {k: parse(p("trunc.cov"), k, name) for k, name in FILES}
    for g, (s, l, _) in enumerate(regions):
        want, _ = ref.dense(s, l, reads[rb[g]:rb[g + 1]], cls[rb[g]:rb[g + 1]])
        for k, name in FILES:
            rows = [r for r in tracks[k] if s <= r[0] < s + l]
            assert (dense_of(rows, s, l) == want[k].astype(np.int64)).all(), (g, name)
            total[k] += int(want[k].sum())
    for k, _ in FILES:
        assert all(e <= t_lo or s >= t_hi for s, e, _ in tracks[k])  # nothing in the stretch: a spanning read stops at its flank's window
        assert sum((e - s) * v for s, e, v in tracks[k]) == total[k] == st_t["hap_coverage_bases"][k]
    assert st_t["hap_coverage_bases"] != st_on["hap_coverage_bases"]

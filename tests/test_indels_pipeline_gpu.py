"""pipeline.run(indels_out=...) on a synthetic BAM (written through lcr_bam_write_reads) of two haplotypes over one region: a 2-base
deletion planted on one haplotype's reads only, a 2-base insertion on all reads, and a 1-base deletion at a column of its own in every read
(single-read noise).  The indel VCF holds a phased record with the run's PS at the deletion, a 1/1 record at the insertion and no PASS
record at the noise; its text equals indels.format_vcf over the restatement (tests/indels_ref.py) on the batch the pipeline cuts; the two
stats match; every other output is untouched by the option; the command line's flags reach the same file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import indels_ref as ref
import test_indels_gpu as tg
from longcallr_amd import _abi, bamio, indels, pipeline

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT = dict(min_mapq=0, min_read_length=0, divergence=2.0)
STATS = ("indel_events", "indel_calls")
S0, LEN = 5000, 1500
SITES = (150, 300, 450, 600, 850, 1150, 1300, 1400)
DEL_COL, INS_COL = 700, 1000


def planted_batch():
    """40 reads over [S0, S0 + LEN): reads 2k carry the alternate base at every het site and the deletion of columns 700-701, reads 2k + 1
    neither; all carry GG in front of column 1000 and one 1-base deletion at a column of their own near 200 + 7 i (i < 20) or 1050 + 7
    (i - 20).  The reference is ACGT repeated, in which none of these events shifts: column 699 is T, 700-701 AC, 999 T, 1000 A."""
    refseq = tg.bg(LEN)
    reads = []
    for i in range(40):
        noise = 200 + 7 * i if i < 20 else 1050 + 7 * (i - 20)
        while noise in SITES or noise + 1 in SITES or noise - 1 in SITES:
            noise += 2
        cuts = sorted([(noise, "D", 1), (INS_COL, "I", 2)] + ([(DEL_COL, "D", 2)] if i % 2 == 0 else []))
        cigar, cur = "", 0
        for c, op, n in cuts:
            cigar += "%dM%d%s" % (c - cur, n, op)
            cur = c + (n if op == "D" else 0)
        cigar += "%dM" % (LEN - cur)
        reads.append((0, cigar, 2 if i % 2 == 0 else 1, "GG"))
    return tg.tj.batch_of([tg.region(S0, refseq, SITES, reads)]), refseq


def test_pipeline_indels_out(engine_cls, tmp_path):
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
    out = str(tmp_path / "out.indels.vcf")
    knobs = dict(indel_min_count=1, indel_min_permille=0, indel_flank=5, indel_max_ins=12, indel_max_del=50)
    st_on, vcf_on, bam_on = run("on", indels_out=out, **knobs)
    st_off, vcf_off, bam_off = run("off")
    st_none, vcf_none, bam_none = run("none", indels_out=None)
    assert vcf_on == vcf_off == vcf_none and bam_on == bam_off == bam_none
    assert not any(k in st_off for k in STATS) and {k: v for k, v in st_on.items() if k not in STATS} == st_off == st_none
    main_ps = {ln.split("\t")[9].split(":")[ln.split("\t")[8].split(":").index("PS")] for ln in vcf_on.decode().splitlines()
               if not ln.startswith("#") and "|" in ln.split("\t")[9].split(":")[0]}
    assert len(main_ps) == 1                                  # the run phases the region into one set

    body = [ln.split("\t") for ln in open(out).read().splitlines() if not ln.startswith("#")]
    head = [ln for ln in open(out).read().splitlines() if ln.startswith("##")]
    assert any("ID=HRUN" in ln for ln in head) and any("ID=PV" in ln for ln in head)
    by_pos = {int(r[1]): r for r in body}
    assert len(by_pos) == len(body) and [int(r[1]) for r in body] == sorted(by_pos)
    d = by_pos[S0 + DEL_COL]                                 # POS is s_left, 1-based: the anchor base
    fmt = dict(zip(d[8].split(":"), d[9].split(":")))
    assert (d[3], d[4], d[6]) == ("TAC", "T", "PASS") and fmt["GT"] in ("1|0", "0|1") and fmt["PS"] in main_ps and fmt["AD"] == "20,20"
    assert sorted(fmt["HC"].split(",")) == ["0", "0", "20", "20"] and float(fmt["PV"]) <= 0.05
    i = by_pos[S0 + INS_COL]
    fmt = dict(zip(i[8].split(":"), i[9].split(":")))
    assert (i[3], i[4], i[6]) == ("T", "TGG", "PASS") and fmt["GT"] == "1/1" and fmt["AD"] == "0,40" and fmt["PS"] == "."
    noise = [r for p, r in by_pos.items() if p not in (S0 + DEL_COL, S0 + INS_COL)]
    assert len(noise) == 40 and all(r[6] == "LowQual" and r[9].startswith("0/1:") for r in noise)
    assert st_on["indel_events"] == 42 and st_on["indel_calls"] == 2

    # the batch the pipeline cut (one chunk), phased once more here; the file against the restatement on the engine's phasing results
    nb = bamio.NativeBam(bam, 2)
    rs, re_ = nb.spans(0, **FLT)
    E = engine_cls(0, _abi.make_params("hifi-masseq", seed=2025))
    regions = E.discover_regions(rs, re_, clen)
    batch = nb.batch(0, [(s_, l_) for s_, l_, _ in regions], [seq[s_:s_ + l_] for s_, l_, _ in regions], **FLT)
    nb.close()
    E.load_batch(batch).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    rec, off, rows, tot = E.indels(1, 0, 5, 12, 50)
    E.close()
    want = ref.indels(batch, fm["row_region_off"], fm["row_read"], pr["assignment"], pr["phase_set"], 1, 0, 5, 12, 50)
    assert [x.tobytes() for x in (rec, off, rows)] == [x.tobytes() for x in want[:3]] and tot == want[3]
    text, n_pass = indels.format_vcf([("chrS", want[0], [indels.alleles(r, batch.start0, batch.col_off, batch.ref) for r in want[0]])], ["chrS"])
    assert ["\t".join(r) for r in body] == text.splitlines() and n_pass == 2

    # the command line: the flags reach the same file as the keywords
    kw_out, cli_out = str(tmp_path / "kw.indels.vcf"), str(tmp_path / "cli.indels.vcf")
    st_kw = pipeline.run(bam, fa, str(tmp_path / "kw.vcf"), None, preset="hifi-masseq", threads=4, indels_out=kw_out, indel_min_count=5,
                         indel_min_permille=100, indel_flank=3, indel_max_ins=4, indel_max_del=10)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_pipeline.py"), "-b", bam, "-f", fa, "-o", str(tmp_path / "cli.vcf"),
                        "-p", "hifi-masseq", "-t", "4", "--indels-out", cli_out, "--indel-min-count", "5", "--indel-min-permille", "100",
                        "--indel-flank", "3", "--indel-max-ins", "4", "--indel-max-del", "10"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(cli_out).read() == open(kw_out).read()
    st_cli = json.loads(r.stdout.strip().splitlines()[-1])
    assert st_cli["indel_events"] == st_kw["indel_events"] == 2 and st_cli["indel_calls"] == st_kw["indel_calls"] == 2
    with pytest.raises(ValueError):
        pipeline.run(bam, fa, str(tmp_path / "bad.vcf"), None, preset="hifi-masseq", indels_out=kw_out, indel_max_ins=13)

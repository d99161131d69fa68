"""pipeline.run(retention_out=...) on a synthetic ONT cDNA BAM in which some reads of one gene keep an intron: the TSV against
retention.format_tsv over the restatement (tests/retention_ref.py) on the batch the pipeline cuts, the two stats, every other output
untouched by the option, and the command line's flags reaching the same file.  The synthetic generator never retains an intron, so
`retain` below rewrites chosen reads: one N op becomes an = op over the reference bases it skipped."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import retention_ref as ref
from longcallr_amd import _abi, bamio, pipeline, retention, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT = dict(min_mapq=0, min_read_length=0, divergence=2.0)
STATS = ("retention_introns", "retention_reads")
QUERY = (0, 1, 4, 7, 8)     # M I S = X consume the read's sequence


def junctions_of(b, i):
    """[(op index, s, l)] of read i"""
    out, cur, c0 = [], int(b.pos[i]), int(b.cig_off[i])
    for k in range(int(b.n_cig[i])):
        w = int(b.cigar[c0 + k])
        op, n = w & 15, w >> 4
        if op == 3 and n >= 1:
            out.append((k, cur, n))
        if op in (0, 2, 3, 7, 8):
            cur += n
    return out


def retain(b, g, every=3):
    """The batch with every `every`-th read that splices region g's most frequent junction rewritten to keep that intron: its N op becomes an
    = op of the same length, the window's reference bases and quality 30 go into the read at that query offset, seq_len and the offsets
    follow.  -> (batch, (s, l), rewritten reads)"""
    reads = range(int(b.read_begin[g]), int(b.read_begin[g + 1]))
    count = {}
    for i in reads:
        for _, s, l in junctions_of(b, i):
            if s >= int(b.start0[g]) and s + l <= int(b.start0[g]) + int(b.len[g]):
                count[(s, l)] = count.get((s, l), 0) + 1
    s, l = max(sorted(count), key=lambda j: count[j])
    window = b.ref[int(b.col_off[g]):int(b.col_off[g + 1])]
    fill = window[s - int(b.start0[g]):s - int(b.start0[g]) + l]
    cigar, bases, quals, seq_len = b.cigar.copy(), [], [], b.seq_len.copy()
    chosen, n_hold = [], 0
    for i in range(b.n_reads):
        q0, q1 = int(b.seq_off[i]), int(b.seq_off[i]) + int(b.seq_len[i])
        hit = [k for k, js, jl in junctions_of(b, i) if (js, jl) == (s, l)] if i in reads else []
        if hit:
            n_hold += 1
        if not hit or n_hold % every:
            bases.append(b.bases[q0:q1]); quals.append(b.quals[q0:q1])
            continue
        k, c0 = hit[0], int(b.cig_off[i])
        at = q0 + sum(int(w) >> 4 for w in b.cigar[c0:c0 + k] if (int(w) & 15) in QUERY)
        cigar[c0 + k] = (l << 4) | 7
        bases += [b.bases[q0:at], fill, b.bases[at:q1]]
        quals += [b.quals[q0:at], np.full(l, 30, np.uint8), b.quals[at:q1]]
        seq_len[i] += l
        chosen.append(i)
    sl = seq_len.astype(np.int64)
    out = _abi.ReadBatch(pos=b.pos, seq_len=seq_len, lead_clip=b.lead_clip, trail_clip=b.trail_clip, flags=b.flags,
                         seq_off=(np.cumsum(sl) - sl).astype(np.uint64), cig_off=b.cig_off, n_cig=b.n_cig, bases=np.concatenate(bases),
                         quals=np.concatenate(quals), cigar=cigar, start0=b.start0, len=b.len, read_begin=b.read_begin, ref=b.ref)
    assert int(out.bases.size) == int(b.bases.size) + l * len(chosen) == int(out.quals.size) and len(chosen) >= 3
    return out, (s, l), chosen


def test_pipeline_retention_out(engine_cls, tmp_path):
    src, (s, l), chosen = retain(synth.make_batch("ont-cdna", n_genes=4, seed=5), 0)
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "ref.fa")
    clen = bamio.write_reads_bam(bam, src, "chrS")
    seq = np.full(clen, ord("N"), np.uint8)
    for g in range(src.n_regions):
        seq[int(src.start0[g]):int(src.start0[g]) + int(src.len[g])] = src.ref[int(src.col_off[g]):int(src.col_off[g + 1])]
    with open(fa, "wb") as f, open(fa + ".fai", "w") as fi:
        f.write(b">chrS\n" + seq.tobytes() + b"\n")
        fi.write("chrS\t%d\t6\t%d\t%d\n" % (clen, clen, clen + 1))

    def run(tag, **kw):
        v, bm, aj = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".bam")), str(tmp_path / (tag + ".asj.tsv"))
        st = pipeline.run(bam, fa, v, bm, preset="ont-cdna", threads=4, asj_out=aj, **kw)
        return st, open(v, "rb").read(), bamio.bgzf_decompress(bm), open(aj, "rb").read()
    tsv = str(tmp_path / "out.retention.tsv")
    st_on, vcf_on, bam_on, asj_on = run("on", read_filter=FLT, retention_out=tsv, retention_min_count=3, retention_anchor=10)
    st_off, vcf_off, bam_off, asj_off = run("off", read_filter=FLT)
    st_none, vcf_none, bam_none, asj_none = run("none", read_filter=FLT, retention_out=None)
    assert vcf_on == vcf_off == vcf_none and bam_on == bam_off == bam_none and asj_on == asj_off == asj_none and vcf_on.count(b"\n") > 30
    assert not any(k in st_off for k in STATS) and {k: v for k, v in st_on.items() if k not in STATS} == st_off == st_none

    # the batch the pipeline cut (one chunk), phased once more here; the file against the restatement on the engine's phasing results
    nb = bamio.NativeBam(bam, 2)
    rs, re_ = nb.spans(0, **FLT)
    E = engine_cls(0, _abi.make_params("ont-cdna", seed=2025))
    regions = E.discover_regions(rs, re_, clen)
    batch = nb.batch(0, [(s_, l_) for s_, l_, _ in regions], [seq[s_:s_ + l_] for s_, l_, _ in regions], **FLT)
    nb.close()
    E.load_batch(batch).run_all()
    fm, pr = E.fragmat(), E.phase_result()
    rec, off, row_ret, tot = E.intron_retention(3, 10)
    E.close()
    want = ref.intron_retention(batch, fm["row_region_off"], fm["row_read"], pr["assignment"], pr["phase_set"], 3, 10)
    assert [x.tobytes() for x in (rec, off, row_ret)] == [x.tobytes() for x in want[:3]] and tot == want[3]
    got = open(tsv).read()
    assert got.split("\n") == retention.format_tsv([("chrS", want[0], batch.start0, batch.len)], 3, 1).split("\n")
    assert st_on["retention_introns"] == rec.size and st_on["retention_reads"] == int((row_ret > 0).sum()) > 0 and st_on["regions"] == len(regions)
    rows = [ln.split("\t") for ln in got.splitlines()[1:]]
    assert any(int(r[8]) + int(r[10]) > 0 for r in rows) and "chrS:%d-%d" % (s + 1, s + l) in [r[0] for r in rows]     # the intron the test retained
    print("ont-cdna n_genes=4, %d reads rewritten at (%d, %d): %d kept introns at (3, 10), %d rows retain one, %d retained in all, %d rows written"
          % (len(chosen), s, l, rec.size, st_on["retention_reads"], tot["n_retained"], len(rows)))

    # the command line (its own read filter): the flags reach the same file as the keywords
    st_kw = pipeline.run(bam, fa, str(tmp_path / "kw.vcf"), None, preset="ont-cdna", threads=4, retention_out=str(tmp_path / "kw.tsv"),
                         retention_min_count=2, retention_anchor=5, retention_min_retained=0)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_pipeline.py"), "-b", bam, "-f", fa, "-o", str(tmp_path / "cli.vcf"),
                        "-p", "ont-cdna", "-t", "4", "--retention-out", str(tmp_path / "cli.tsv"), "--retention-min-count", "2",
                        "--retention-anchor", "5", "--retention-min-retained", "0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "cli.tsv")).read() == open(str(tmp_path / "kw.tsv")).read()
    st_cli = json.loads(r.stdout.strip().splitlines()[-1])
    assert st_cli["retention_introns"] == st_kw["retention_introns"] > 0 and st_cli["retention_reads"] == st_kw["retention_reads"] > 0

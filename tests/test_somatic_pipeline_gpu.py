"""pipeline.run(somatic_out=...) on a small two-contig BAM -- a synthetic preset contig and, on the second contig, the low-fraction reads
of tests/test_gpu_parity.py: the somatic VCF against somatic.format_vcf_records over direct Engine.somatic calls on the batches the
pipeline cuts (checked against the restatement, tests/somatic_ref.py), its header, the stats, the main VCF and the phased BAM untouched
by the option -- in one chunk per contig, with chunk_cost forcing a chunk per region, on two engines of one device, and behind
lcr_haplotag with the run's own VCF fed back."""
import struct
import zlib

import numpy as np
import pytest

import somatic_ref as ref
import test_gpu_parity as tp
import test_haplotag_gpu as hg
from longcallr_amd import _abi, bamio, pipeline, somatic, synth, vcf

pytestmark = pytest.mark.gpu

FLT = dict(min_mapq=0, min_read_length=0, divergence=2.0)
OVER = dict(min_phase_score=13.0)       # (the low-fraction sites are not rescued at it: tests/test_gpu_parity.py)


def bam_parts(path):
    """a one-contig BAM of bamio.write_reads_bam -> (header text, [(name, length)], the record stream)"""
    raw = bamio.bgzf_decompress(path)
    assert raw[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", raw, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", raw, p)[0]
        refs.append((raw[p + 4:p + 4 + l_name - 1].decode(), struct.unpack_from("<i", raw, p + 4 + l_name)[0]))
        p += 8 + l_name
    return raw[8:8 + l_text], refs, raw[p:]


def bgzf_block(data):
    z = zlib.compressobj(1, zlib.DEFLATED, -15)
    c = z.compress(data) + z.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(c) + 25) + c
            + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


def write_two_contig_bam(path, part_a, part_b):
    """two one-contig BAMs as one: the second's records get reference id 1; BGZF blocks end at record boundaries"""
    (_, refs_a, rec_a), (_, refs_b, rec_b) = part_a, part_b
    refs = refs_a + refs_b
    text = b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode(), l) for n, l in refs)
    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for n, l in refs:
        head += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    blocks, cur = [bgzf_block(head)], []
    size = 0
    for rid, stream in ((0, rec_a), (1, rec_b)):
        p = 0
        while p < len(stream):
            n = 4 + struct.unpack_from("<i", stream, p)[0]
            r = bytearray(stream[p:p + n])
            struct.pack_into("<i", r, 4, rid)
            if size + n > 60000:
                blocks.append(bgzf_block(b"".join(cur)))
                cur, size = [], 0
            cur.append(bytes(r)); size += n
            p += n
    if cur:
        blocks.append(bgzf_block(b"".join(cur)))
    with open(path, "wb") as f:
        f.write(b"".join(blocks) + bgzf_block(b""))


def contig_sequence(batch, clen):
    seq = np.full(clen, ord("N"), np.uint8)
    for g in range(batch.n_regions):
        seq[int(batch.start0[g]):int(batch.start0[g]) + int(batch.len[g])] = batch.ref[int(batch.col_off[g]):int(batch.col_off[g + 1])]
    return seq


def body_of(path):
    return open(path).read().split("#CHROM")[1].split("\n", 1)[1]


def test_pipeline_somatic_out(engine_cls, tmp_path):
    p = lambda name: str(tmp_path / name)
    src = {"chrS": synth.make_batch("ont-cdna", n_genes=3, seed=5), "chrL": tp._low_fraction_batch(seed=1)}
    seqs, parts = {}, []
    for name, b in src.items():
        clen = bamio.write_reads_bam(p(name + ".bam"), b, name)
        seqs[name] = contig_sequence(b, clen)
        parts.append(bam_parts(p(name + ".bam")))
    bam, fa = p("in.bam"), p("ref.fa")
    write_two_contig_bam(bam, *parts)
    with open(fa, "wb") as f, open(fa + ".fai", "w") as fi:
        at = 0
        for name, seq in seqs.items():
            f.write(b">" + name.encode() + b"\n" + seq.tobytes() + b"\n")
            fi.write("%s\t%d\t%d\t%d\t%d\n" % (name, seq.size, at + len(name) + 2, seq.size, seq.size + 1))
            at += len(name) + 2 + seq.size + 1

    def run(tag, **kw):
        st = pipeline.run(bam, fa, p(tag + ".vcf"), p(tag + ".bam"), preset="ont-cdna", threads=4, seed=3, read_filter=FLT, **OVER, **kw)
        return st, open(p(tag + ".vcf"), "rb").read(), bamio.bgzf_decompress(p(tag + ".bam"))
    som_keys = ("somatic_sites", "somatic_calls")
    without = lambda st: {k: x for k, x in st.items() if k not in som_keys}
    st_off, vcf_off, bam_off = run("off")
    st_on, vcf_on, bam_on = run("on", somatic_out=p("on.som.vcf"))
    assert st_off["contigs"] == 2 and st_off["reads"] == sum(b.n_reads for b in src.values()) and st_off["chunks"] == 2
    assert vcf_on == vcf_off and bam_on == bam_off and without(st_on) == st_off and not set(som_keys) & set(st_off)
    for bad in (dict(somatic_purity=0.0), dict(somatic_purity=1.5), dict(somatic_min_baseq=31), dict(somatic_min_baseq=-1), dict(somatic_min_baseq=2.5)):
        with pytest.raises(ValueError):
            pipeline.run(bam, fa, p("x.vcf"), somatic_out=p("x.som.vcf"), **bad)

    # the batches the pipeline cut (one per contig), phased once more here; their records by the restatement
    prm = _abi.make_params("ont-cdna", seed=3, **OVER)

    def direct(min_score=0.0, input_vcf=None, **kw):
        nb = bamio.NativeBam(bam, 2)
        text, n_sites, n_calls = "", 0, 0
        arrays = vcf.read_sites(input_vcf, alleles=True, phase_sets=True) if input_vcf else None
        for rid, name in enumerate(src):
            rs, re_ = nb.spans(rid, **FLT)
            E = engine_cls(0, prm)
            regions = E.discover_regions(rs, re_, seqs[name].size)
            batch = nb.batch(rid, [(s, l) for s, l, _ in regions], [seqs[name][s:s + l] for s, l, _ in regions], **FLT)
            if arrays is None:
                E.load_batch(batch).run_all()
                fm = E.fragmat()
            else:       # behind lcr_haplotag: the contig's sites inside the batch's span, as the pipeline cuts them
                a = arrays[name]
                span = [int(batch.start0[0]), int(batch.start0[-1]) + int(batch.len[-1])]
                lo, hi = np.searchsorted(a[0], span)
                hs = vcf.haplotag_sites(a)
                hlo, hhi = np.searchsorted(hs[0], span)
                fm, _, _ = hg.staged(E, batch, tuple(x[lo:hi] for x in a[:3]))
                E.haplotag(tuple(x[hlo:hhi] for x in hs))
            pr = E.phase_result()
            cands, _ = E.candidates()
            got = E.somatic(**kw)
            want = ref.of_engine(fm, pr, cands, **kw)
            E.close()
            assert got.tobytes() == want.tobytes(), name
            text += somatic.format_vcf_records(cands, got, name, min_score)
            n_sites += int(np.count_nonzero(((cands["flags"] & _abi.F_CAND_SOMATIC) != 0) & (got["status"] == somatic.SOM_OK)))
            n_calls += int(np.count_nonzero(got["call"]))
        nb.close()
        return text, n_sites, n_calls
    text, n_sites, n_calls = direct()
    assert body_of(p("on.som.vcf")) == text and (st_on["somatic_sites"], st_on["somatic_calls"]) == (n_sites, n_calls)
    print("somatic_out: %d flagged sites evaluated, %d calls\n%s" % (n_sites, n_calls, text))
    assert n_calls >= 1 and n_sites >= n_calls and text.count("\n") == n_calls
    rows = [l.split("\t") for l in text.split("\n")[:-1]]
    assert all(r[0] == "chrL" and r[6] == "PASS" and r[7].startswith("RDS=somatic;SHP=") and r[8] == "GT:DP:AF:PS:SQ" and r[9].startswith("0/1:") for r in rows)
    assert [int(r[1]) for r in rows] == sorted(int(r[1]) for r in rows)
    main = {l.split("\t")[1]: l.split("\t") for l in vcf_off.decode().split("\n") if l.startswith("chrL\t")}
    assert all(main[r[1]][7] == "RDS=noselect" and main[r[1]][5] == r[5] for r in rows)      # what the user saw of them before
    # the header: the run's own plus the three INFO lines in front of the column line
    head_main = open(p("on.vcf")).read().split("#CHROM")[0]
    assert open(p("on.som.vcf")).read().split("#CHROM")[0] == head_main + somatic.INFO_LINES

    # a score threshold, another purity and base-quality threshold
    st_q, vcf_q, bam_q = run("q", somatic_out=p("q.som.vcf"), somatic_purity=0.2, somatic_min_baseq=13, somatic_min_score=1000.0)
    tq, sq, cq = direct(1000.0, purity=0.2, min_baseq=13)
    assert body_of(p("q.som.vcf")) == tq and (st_q["somatic_sites"], st_q["somatic_calls"]) == (sq, cq) and vcf_q == vcf_off and bam_q == bam_off
    assert all(l.split("\t")[6] == "LowQual" for l in tq.split("\n")[:-1])

    # a chunk per region; two engines on one device
    st_c, vcf_c, bam_c = run("c", somatic_out=p("c.som.vcf"), chunk_cost=1.0)
    assert st_c["chunks"] == st_off["regions"] > 2 and body_of(p("c.som.vcf")) == text and vcf_c == vcf_off and bam_c == bam_off
    assert {k: x for k, x in st_c.items() if k != "chunks"} == {k: x for k, x in st_on.items() if k != "chunks"}
    st_d, vcf_d, bam_d = run("d", somatic_out=p("d.som.vcf"), chunk_cost=1.0, devices=[0, 0])
    assert body_of(p("d.som.vcf")) == text and vcf_d == vcf_off and bam_d == bam_off and st_d == st_c

    # behind lcr_haplotag, the run's own VCF fed back: the low-fraction sites come back as imported sites, so nothing is flagged
    st_h, vcf_h, bam_h = run("hap", input_vcf=p("off.vcf"), haplotag=True)
    st_hs, vcf_hs, bam_hs = run("haps", input_vcf=p("off.vcf"), haplotag=True, somatic_out=p("haps.som.vcf"))
    assert vcf_hs == vcf_h and bam_hs == bam_h and without(st_hs) == st_h and st_h["haplotag_reads"] > 0
    th_, sh, ch = direct(input_vcf=p("off.vcf"))
    assert body_of(p("haps.som.vcf")) == th_ and (st_hs["somatic_sites"], st_hs["somatic_calls"]) == (sh, ch)

"""User-provided candidates, host half: liblcr's VCF reader (lcr_vcf_*) against a restatement of
get_genotype_quality_phase_from_vcf (reference src/vcf.rs:400-462) written here, on constructed files in plain and
multi-member gzip form, its refusals, and the VCF writer's NaN allele frequency.  No GPU needed."""
import gzip
import re

import numpy as np
import pytest

from longcallr_amd import _abi, _lib, build, vcf

HEADER = ("##fileformat=VCFv4.2\n##contig=<ID=chr1>\n##contig=<ID=chr2>\n##contig=<ID=chr3>\n"
          '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
          "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\n")
BODY = [
    "chr2\t100\t.\tA\tG\t50\tPASS\t.\tGT\t0|1\t1/0",          # several contigs, not in header order
    "chr2\t120\t.\tC\tT,G\t12.5\tPASS\t.\tGT:DP\t1/2:7\t0/0:3",  # multi-sample: the second sample overwrites the first
    "chr2\t130\t.\tC\tT\t.\tPASS\t.\tGT\t1|1\t1",             # missing QUAL; haploid second sample skipped
    "chr1\t5\t.\tG\tA\t-3\tPASS\t.\tGT\t0/1\t.",              # negative QUAL; lone '.' skipped
    "chr1\t9\t.\tACGT\tA\t40\tPASS\t.\tGT\t0/1\t./.",         # indel: a site at POS; ./. -> 4 overwrites the 0/1
    "chr1\t12\t.\tT\tC\t41\tPASS\t.\tDP:GT\t9:0/.\t8:2/1",    # GT not the first key; 0/. -> 4, then 2/1 -> 3
    "chr1\t20\t.\tT\tC\t7\tPASS\t.\tGT\t1/1\t0/2",            # 0/2 -> 4
    "chr2\t100\t.\tA\tC\t60\tPASS\t.\tGT\t1/1\t1|1",          # duplicate position in a later record: overwrites
    "chr3\t1\t.\tA\tC\t1e1\tPASS\t.\tGT\t1/0\t3/3",
    "chr1\t15\t.\tT\tC\t8\tPASS\t.\tGT:AD\t1/1:3,4",          # one sample only
    "chr1\t16\t.\tT\tC\t8\tPASS\t.\tGT:AD\t.:3,4\t1",         # no sample with two alleles: no site
    "chr2\t150\t.\tA\tG\t33\tPASS\t.",                       # sites-only record: no samples
]
GT_CODE = {(0, 0): 0, (0, 1): 1, (1, 0): 1, (1, 1): 2, (1, 2): 3, (2, 1): 3}


def read_sites_reference(text):
    """vcf.rs:400-462 in Python: contig -> 0-based POS -> (genotype code, f32 QUAL); later values overwrite earlier ones."""
    m = {}
    for line in text.split("\n"):
        if not line or line.startswith("#"):
            continue
        f = line.split("\t")
        qual = np.float32(np.nan) if f[5] == "." else np.float32(float(f[5]))
        if len(f) < 10:
            continue                                   # sample_count = 0: the loop body never runs
        k = f[8].split(":").index("GT")
        for smp in f[9:]:
            sub = smp.split(":")
            gt = re.split(r"[/|]", sub[k]) if k < len(sub) else ["."]
            if len(gt) != 2:                            # gt.len() != 2 (vcf.rs:421)
                continue
            a = tuple(3 if x == "." else int(x) for x in gt)
            m.setdefault(f[0], {})[int(f[1]) - 1] = (GT_CODE.get(a, 4), qual)
    out = {}
    for c, d in m.items():
        ks = sorted(d)
        out[c] = (np.array(ks, np.int64), np.array([d[p][0] for p in ks], np.uint8), np.array([d[p][1] for p in ks], np.float32))
    return out


@pytest.fixture(scope="module")
def lib():
    build.build()  # hipcc cross-compiles gfx950 without a GPU; the reader itself is host code
    return _lib.load()


def _same(got, want):
    assert sorted(got) == sorted(want)
    for c in want:
        gp, gg, gq = got[c]
        wp, wg, wq = want[c]
        assert gp.dtype == np.int64 and gg.dtype == np.uint8 and gq.dtype == np.float32
        assert np.array_equal(gp, wp), c
        assert np.array_equal(gg, wg), c
        assert np.array_equal(gq, wq, equal_nan=True), c


def _members(text, n):
    """text as n gzip members back to back plus BGZF's empty end-of-file member"""
    lines = text.splitlines(keepends=True)
    cut = [len(lines) * i // n for i in range(n + 1)]
    return b"".join(gzip.compress("".join(lines[cut[i]:cut[i + 1]]).encode()) for i in range(n)) + gzip.compress(b"")


def test_reader_matches_the_reference_rules(lib, tmp_path):
    text = HEADER + "\n".join(BODY) + "\n"
    want = read_sites_reference(text)
    # the rules the restatement encodes, spelled out on a few sites
    assert want["chr2"][0].tolist() == [99, 119, 129] and want["chr2"][1].tolist() == [2, 0, 2]
    assert want["chr1"][0].tolist() == [4, 8, 11, 14, 19] and want["chr1"][1].tolist() == [1, 4, 3, 2, 4]
    assert np.isnan(want["chr2"][2][2]) and want["chr1"][2][0] == np.float32(-3)
    plain = tmp_path / "sites.vcf"
    plain.write_text(text)
    _same(vcf.read_sites(str(plain)), want)
    for n in (1, 3, len(BODY) + 6):
        gz = tmp_path / ("sites%d.vcf.gz" % n)
        gz.write_bytes(_members(text, n))
        _same(vcf.read_sites(str(gz)), want)


def test_crlf_and_sites_only_files(lib, tmp_path):
    p = tmp_path / "crlf.vcf"
    text = HEADER + "\n".join(BODY) + "\n"
    p.write_bytes(text.replace("\n", "\r\n").encode())
    _same(vcf.read_sites(str(p)), read_sites_reference(text))
    p = tmp_path / "sites_only.vcf"
    p.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nchr1\t5\t.\tA\tG\t30\tPASS\t.\n")
    assert vcf.read_sites(str(p)) == {}


def test_reader_refuses_what_it_cannot_read(lib, tmp_path):
    with pytest.raises(_lib.LcrError, match="cannot open"):
        vcf.read_sites(str(tmp_path / "missing.vcf"))
    bcf = tmp_path / "x.bcf"
    bcf.write_bytes(gzip.compress(b"BCF\x02\x02" + b"\0" * 32))
    with pytest.raises(_lib.LcrError, match="BCF"):
        vcf.read_sites(str(bcf))
    bcf.write_bytes(b"BCF\x02\x02" + b"\0" * 32)
    with pytest.raises(_lib.LcrError, match="BCF"):
        vcf.read_sites(str(bcf))
    nogt = tmp_path / "nogt.vcf"
    nogt.write_text(HEADER + "chr1\t5\t.\tA\tG\t30\tPASS\t.\tDP\t7\t8\n")
    with pytest.raises(_lib.LcrError, match="GT"):
        vcf.read_sites(str(nogt))


def test_nan_allele_frequency_prints_like_rust():
    """An imported site at a column without A/C/G/T counts has af = 0 / 0 = NaN (f32); Rust's {:.2} prints it as NaN."""
    c = np.zeros(2, dtype=_abi.CAND_DTYPE)
    for s, vt in zip(c, (1, 3)):
        s["pos"], s["ref_base"], s["allele1"], s["allele2"] = 41, ord("A"), ord("A"), ord("C")
        s["af1"] = s["af2"] = np.float32(np.nan)
        s["variant_type"], s["genotype"], s["flags"], s["qual"] = vt, 0 if vt == 1 else -1, _abi.F_HET | _abi.F_FOR_PHASING, np.nan
    c[1]["allele1"], c[1]["flags"] = ord("G"), _abi.F_HOM
    text = vcf.format_records(c, "chr1", 8.0)
    assert text == ("chr1\t42\t.\tA\tC\t0\tLowQual\tRDS=select\tGT:GQ:PS:DP:AF:PQ\t0/1:0:.:0:NaN:0.00\n"
                    "chr1\t42\t.\tA\tG\t0\tPASS\tRDS=select\tGT:GQ:PS:DP:AF:PQ\t1/1:0:.:0:NaN:0.00\n")


def test_reader_streams_files_larger_than_its_buffers(lib, tmp_path):
    """Lines cut by the reader's 1 MiB input / 256 KiB output chunks; a truncated gzip stream is an error, not a short result."""
    rng = np.random.default_rng(4)
    gts = ["0/0", "0/1", "1|0", "1/1", "1/2", "./.", "0/.", "1", "2/2"]
    body = []
    for i in range(60000):
        q = "." if i % 97 == 0 else "%.1f" % rng.uniform(-5, 60)
        smp = "\t".join("%s:%d" % (gts[int(rng.integers(0, len(gts)))], int(rng.integers(0, 99))) for _ in range(3))
        body.append("chr%d\t%d\t.\tA\tG\t%s\tPASS\tDP=%d\tGT:DP\t%s" % (1 + i % 3, 1 + int(rng.integers(0, 40000)), q, i, smp))
    text = HEADER.replace("\tS1\tS2", "\tS1\tS2\tS3") + "\n".join(body)     # (no newline after the last line)
    assert len(text) > 3 << 20
    want = read_sites_reference(text)
    plain = tmp_path / "big.vcf"
    plain.write_text(text)
    _same(vcf.read_sites(str(plain)), want)
    gz = tmp_path / "big.vcf.gz"
    data = gzip.compress(text.encode(), compresslevel=1)
    gz.write_bytes(data)
    _same(vcf.read_sites(str(gz)), want)
    gz.write_bytes(data[:len(data) // 2])
    with pytest.raises(_lib.LcrError, match="truncated"):
        vcf.read_sites(str(gz))

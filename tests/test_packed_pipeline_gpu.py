"""pipeline.run(packed_upload=True) on tests/golden/demo.bam (-m gpu): VCF text and the inflated phased-BAM stream byte for byte those
of the run without the option, the same stats, and upload_bytes_saved recomputed from the chunks' batches."""
import os

import numpy as np
import pytest

import helpers
from longcallr_amd import _abi, bamio, pipeline

pytestmark = pytest.mark.gpu


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


def test_packed_upload_reproduces_the_plain_run(engine_cls, tmp_path):
    src = os.path.join(helpers.GOLDEN, "demo.bam")
    fa = demo_fasta(tmp_path)

    def run(tag, **kw):
        o_vcf, o_bam = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".bam"))
        st = pipeline.run(src, fa, o_vcf, o_bam, preset="hifi-masseq", threads=4, **kw)
        return st, open(o_vcf).read(), bamio.bgzf_decompress(o_bam)

    st_plain, vcf_plain, bam_plain = run("plain")
    st_packed, vcf_packed, bam_packed = run("packed", packed_upload=True)
    assert st_plain["vcf_records"] > 0 and st_plain["reads"] > 100 and "upload_bytes_saved" not in st_plain
    assert vcf_packed == vcf_plain
    assert bam_packed == bam_plain and len(bam_plain) > 100000
    saved = st_packed.pop("upload_bytes_saved")
    assert st_packed == st_plain
    # the figure once more from the batches the run cut: the same spans, regions and chunks
    nb = bamio.NativeBam(src, 4)
    E = engine_cls(0, _abi.make_params("hifi-masseq"))
    want, reads = 0, 0
    for rid, (name, length) in enumerate(nb.refs):
        rs, re_ = nb.spans(rid, **_abi.READ_FILTER)
        if name not in ("chr19", "chr20") or rs.size == 0:
            continue
        for chunk in pipeline.chunk_regions(E.discover_regions(rs, re_, length)):
            wins = [np.zeros(l, np.uint8) for _, l, _ in chunk]
            b = nb.batch(rid, [(s, l) for s, l, _ in chunk], wins, packed=True, **_abi.READ_FILTER)
            want += b.n_bases - b.n_pack - 8 * b.n_reads
            reads += b.n_reads
    E.close(); nb.close()
    assert reads == st_plain["reads"] and saved == want > 0

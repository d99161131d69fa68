"""Record-free tiles stay implicit (-m gpu): lcr_pileup writes the planes of the tiles that hold K0 records only; the constant
planes of the others (0, intron plane = introns that cover the whole tile) are stored when lcr_get_columns asks for them.
What lies in a record-free tile before that is an earlier batch's data, so every reader has to leave it alone: checked against
the oracle, with the plane buffer poisoned in front of the pileup (lcr_debug_set("poison_planes")), across batches on one
context, through the import path at sites inside such tiles, and in the stage's byte accounting."""
import os
import re

import numpy as np
import pytest

import helpers
import test_gpu_parity as par
import test_import_candidates_gpu as imp
from longcallr_amd import _abi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "longcallr_amd", "csrc", "lcr_dev.h")) as _f:
    TILE = int(re.search(r"#define LCR_TILE (\d+)", _f.read()).group(1))

# spliced batches (exons are a quarter of a gene: most tiles hold no record); masseq takes the HiFi path (no fused filter, k1_zonefix)
PROFILES = {"ont-cdna": dict(n_genes=24, gene_len=25000, depth=30, seed=5), "masseq": dict(n_genes=16, gene_len=25000, depth=30, seed=6)}
_BATCH, _ORACLE, _TILES = {}, {}, {}


def batch_of(profile, **over):
    kw = dict(PROFILES[profile], **over)
    key = (profile,) + tuple(sorted(kw.items()))
    if key not in _BATCH:
        _BATCH[key] = synth.make_genes(profile, workers=1, **kw)
    return _BATCH[key]


def params_of(profile, **over):
    return _abi.make_params(synth.preset_for(profile), seed=PROFILES[profile]["seed"], **over)


def oracle_of(orc, profile, upto):
    if (profile, upto) not in _ORACLE:
        _ORACLE[profile, upto] = par.oracle_all(orc, batch_of(profile), params_of(profile), upto=upto)
    return _ORACLE[profile, upto]


def tiles_with_records(b, prm):
    """K0's rule (k0_ops.hip), restated: per region, which tiles receive at least one record.  M blocks (clipped to the region and,
    on ONT, to the read offsets [lead + D, reb - D + 1) the end trim keeps) and D runs leave one in every tile they touch, an
    insertion in the tile of the column in front of it (columns 1 .. len - 1), an intron in its first and its last tile."""
    ont, D = int(prm.platform) == _abi.LCR_PLATFORM_ONT, int(prm.dist_to_end)
    key = (id(b), ont, D)
    if key in _TILES:
        return _TILES[key][1]
    out = []
    for g in range(b.n_regions):
        vec, s0 = int(b.len[g]), int(b.start0[g])
        has = np.zeros((vec + TILE - 1) // TILE, bool)
        for r in range(int(b.read_begin[g]), int(b.read_begin[g + 1])):
            lead, reb = int(b.lead_clip[r]), int(b.seq_len[r]) - int(b.trail_clip[r])
            p, q = int(b.pos[r]) - s0, max(lead, 0)
            c0 = int(b.cig_off[r])
            for w in b.cigar[c0:c0 + int(b.n_cig[r])].tolist():
                op, n = w & 15, w >> 4
                m = op in (0, 7, 8)
                if m or op in (2, 3):
                    a, e = max(p, 0), min(p + n, vec)
                    if m and ont:
                        a, e = max(a, p + (lead + D - q)), min(e, p + (reb - D + 1 - q))
                    if n > 0 and e > a:
                        if op == 3:
                            has[a // TILE] = has[(e - 1) // TILE] = True
                        else:
                            has[a // TILE:(e - 1) // TILE + 1] = True
                    p += n
                elif op == 1 and n > 0 and 1 <= p < vec:
                    has[(p - 1) // TILE] = True
                if m or op == 1:
                    q += n
        out.append(has)
    _TILES[key] = (b, out)   # (the batch is kept with its entry: its id stays its own)
    return out


def record_free_fraction(b, prm):
    has = np.concatenate(tiles_with_records(b, prm))
    return 1.0 - has.mean()


def results(E):
    """every stage's host results as bytes, the planes last (the getter that stores the record-free tiles)"""
    c, off = E.candidates()
    pr, fm = E.phase_result(), E.fragmat()
    out = {"cand": c.tobytes(), "cand_off": off.tobytes()}
    out.update({"phase." + k: pr[k].tobytes() for k in ("haplotag", "assignment", "phase_set", "objective")})
    out.update({"fm." + k: fm[k].tobytes() for k in sorted(fm)})
    out["columns"] = E.columns().tobytes()
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], "%s: %s differs" % (what, k)


@pytest.mark.parametrize("poison", [0, 1])
@pytest.mark.parametrize("profile", ["ont-cdna", "masseq"])
def test_planes_whenever_they_are_asked_for(engine_cls, orc, profile, poison):
    """lcr_get_columns == the oracle's planes, bit for bit: right after lcr_pileup, only after the three stages behind it, and twice;
    with and without the poison in front of the pileup."""
    b, p = batch_of(profile), params_of(profile)
    assert record_free_fraction(b, p) > 0.5
    regs = oracle_of(orc, profile, "pileup")
    E = engine_cls(0, p)
    E.debug_set("poison_planes", poison)
    E.load_batch(b).fill_data_into_freq_vec()
    par.check_pileup(E, regs, b)                                  # right after the pileup
    par.check_pileup(E, regs, b)                                  # a second call
    first = E.columns().copy()
    E.get_candidate_snps().get_fragments().phase()
    par.check_pileup(E, regs, b)                                  # stored before the other stages, read after them
    E.load_batch(b).run_all()
    E.phase_result()
    par.check_pileup(E, regs, b)                                  # asked for only after the other three stages
    assert np.array_equal(E.columns(), first)
    E.fill_data_into_freq_vec().get_candidate_snps()              # a second pileup on the same batch, the getter between two stages
    par.check_pileup(E, regs, b)
    E.close()


@pytest.mark.parametrize("profile", ["ont-cdna", "masseq"])
def test_poison_changes_nothing(engine_cls, orc, profile):
    """poison_planes = 1 against 0 on one context: candidates, fragment matrix, phase results and planes identical -- and the oracle's"""
    b, p = batch_of(profile), params_of(profile)
    regs = oracle_of(orc, profile, "post")
    E = engine_cls(0, p)
    got = {}
    for poison in (0, 1, 0):
        E.debug_set("poison_planes", poison)
        E.load_batch(b).fill_data_into_freq_vec().get_candidate_snps().get_fragments()
        fm = par.check_fragmat(E, regs)
        E.phase()
        par.check_cands(E, regs, phased=True)
        par.check_phase(E, regs, fm)
        r = results(E)
        if got:
            assert_same(got, r, "poison_planes = %d" % poison)
        got = r
    par.check_pileup(E, regs, b)
    E.close()


@pytest.mark.parametrize("profile", ["ont-cdna", "masseq"])
def test_batches_follow_each_other_on_one_context(engine_cls, profile):
    """A, then B -- other genes over the same columns: its record-free tiles lie where A had coverage --, then A again on one context;
    every stage's results are those of a fresh context per batch.  Once with the planes fetched after every batch, once with the
    planes of the last batch only (nothing stored in between)."""
    p = params_of(profile)
    A, B = batch_of(profile), batch_of(profile, seed=PROFILES[profile]["seed"] + 100)
    ta, tb = np.concatenate(tiles_with_records(A, p)), np.concatenate(tiles_with_records(B, p))
    n = min(ta.size, tb.size)
    assert (ta[:n] & ~tb[:n]).sum() > 20 and (tb[:n] & ~ta[:n]).sum() > 20
    fresh = {}
    for name, b in (("A", A), ("B", B)):
        F = engine_cls(0, p)
        F.load_batch(b).run_all()
        fresh[name] = results(F)
        F.close()
    E = engine_cls(0, p)
    for name, b in (("A", A), ("B", B), ("A", A)):
        E.load_batch(b).run_all()
        assert_same(fresh[name], results(E), "batch %s behind another" % name)
    E.close()
    E = engine_cls(0, p)
    for name, b in (("A", A), ("B", B), ("A", A), ("B", B)):
        E.load_batch(b).run_all()
        c, off = E.candidates()
        assert c.tobytes() == fresh[name]["cand"] and off.tobytes() == fresh[name]["cand_off"]
        assert E.phase_result()["haplotag"].tobytes() == fresh[name]["phase.haplotag"]
    assert_same(fresh["B"], results(E), "the last batch")
    E.close()


def _gapped_batch():
    """one region of 8 000 columns: 40 reads over columns 100-560, nothing until 2 000, 40 spliced reads (200M 2000N 200M) from
    2 000-2 060 on, nothing behind 4 460: tiles that no read touches, tiles inside the introns only, two het sites per group"""
    rng = np.random.default_rng(17)
    L = 8000
    ref = "".join(rng.choice(list("ACGT"), size=L))
    alt = lambda x: "G" if ref[x] != "G" else "T"
    reads = []
    for i in range(40):
        s = 100 + 4 * i
        a = list(ref[s:s + 300])
        if i % 2:
            for x in (300, 380):
                a[x - s] = alt(x)
        reads.append(dict(pos=s, seq="".join(a), qual=30, cigar="300M", rev=(i // 2) % 2, ts=1 + (i // 2) % 2))
    for i in range(40):
        s = 2000 + (3 * i) // 2
        a, c = list(ref[s:s + 200]), list(ref[s + 2200:s + 2400])
        if i % 2:
            a[2150 - s] = alt(2150)
            c[4300 - (s + 2200)] = alt(4300)
        reads.append(dict(pos=s, seq="".join(a + c), qual=30, cigar="200M2000N200M", rev=(i // 2) % 2, ts=1 + (i // 2) % 2))
    return helpers.mk_batch(reads, [(0, ref)])


@pytest.mark.parametrize("case", ["gapped-ont", "gapped-hifi", "ont-cdna", "masseq"])
def test_import_at_sites_inside_record_free_tiles(engine_cls, orc, case):
    """lcr_import_candidates with sites in tiles that no read touches and in tiles that lie inside introns only (poisoned planes:
    a load from such a tile would show), beside sites on covered columns: the oracle's import, and its phasing."""
    if case.startswith("gapped"):
        b = _gapped_batch()
        prm = _abi.make_params("ont-cdna" if case == "gapped-ont" else "hifi-masseq", seed=4, max_enum_snps=6, min_depth=3)
    else:
        b = batch_of(case, n_genes=6)
        prm = params_of(case, max_enum_snps=6)
    has = tiles_with_records(b, prm)
    rng = np.random.default_rng(3)
    ni = _abi.PLANE_NAMES.index("n")
    pos, n_unc, n_intr = [], 0, 0
    for g in range(b.n_regions):
        s0, L = int(b.start0[g]), int(b.len[g])
        pl = orc.Region(b, g, prm).pileup().planes()
        depth = pl[:4].sum(axis=0)
        free = np.flatnonzero(~has[g])
        assert free.size
        for t in rng.choice(free, size=min(12, free.size), replace=False).tolist():
            col = min(t * TILE + int(rng.integers(0, TILE)), L - 1)
            assert depth[col] == 0
            n_intr += int(pl[ni, col] > 0)
            n_unc += int(pl[ni, col] == 0)
            pos.append(s0 + col)
        cov = np.flatnonzero(depth >= 8)
        pos += (s0 + rng.choice(cov, size=min(5, cov.size), replace=False)).tolist()
        if case.startswith("gapped"):
            pos += [300, 380, 2150, 4300]
    assert n_intr >= 3 and (n_unc >= 3 or not case.startswith("gapped")), (n_unc, n_intr)
    pos = np.unique(np.array(pos, np.int64))
    gt = np.where(np.arange(pos.size) % 5 == 4, 2, 1).astype(np.uint8)
    qual = np.full(pos.size, 30.0, np.float32)
    E = engine_cls(0, prm)
    E.debug_set("poison_planes", 1)
    E.load_batch(b).fill_data_into_freq_vec().import_external_candidates(pos, gt, qual)
    cands, off = E.candidates()
    imp.check_records(cands, off, imp.expected_import(orc, b, prm, pos, gt, qual), b.n_regions)
    assert (cands["depth"] == 0).sum() >= n_unc + n_intr
    E.get_fragments().phase()
    imp.check_downstream(E, b, prm, cands, off)
    regs = par.oracle_all(orc, b, prm, upto="pileup")
    par.check_pileup(E, regs, b)
    E.close()


@pytest.mark.parametrize("profile", ["ont-cdna", "masseq"])
def test_stage_bytes_count_the_planes_that_are_written(engine_cls, profile):
    """lcr_pileup_stage_bytes = B + 4 C + 37 R + L + 52 L' (DESIGN.md section 4): bases, CIGAR words, read headers, one reference
    byte per column and 13 u32 planes per column of a tile WITH records -- the others' planes are not written by the stage."""
    b, p = batch_of(profile, n_genes=8), params_of(profile)
    has = tiles_with_records(b, p)
    cols_written = sum(int(np.minimum(TILE, int(b.len[g]) - np.flatnonzero(h) * TILE).sum()) for g, h in enumerate(has))
    n_cols = int(np.sum(b.len))
    assert 0 < cols_written < n_cols // 2
    want = int(b.bases.size) + 4 * int(b.cigar.size) + 37 * int(b.n_reads) + n_cols + 4 * _abi.NPLANES * cols_written
    E = engine_cls(0, p)
    for _ in range(2):
        E.load_batch(b).fill_data_into_freq_vec()
        assert E.pileup_stage_bytes() == want
    E.columns()
    assert E.pileup_stage_bytes() == want            # (storing the record-free tiles for the getter is not the stage's traffic)
    E.close()

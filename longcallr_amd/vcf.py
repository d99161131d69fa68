"""VCF body text of the phased candidates — the parity diff surface — and the reader of user-provided sites.

Host formatting only; mirrors SNPFrag::output_phased_vcf (reference src/vcf.rs:27-306) and the
record writer of src/thread.rs:266-303 (records without an ALT allele are silently skipped).
read_sites wraps liblcr's VCF reader (lcr_vcf_*, include/lcr.h: get_genotype_quality_phase_from_vcf, vcf.rs:400-462).
"""
import ctypes as C
import os

import numpy as np

from . import _abi


def read_sites(path, alleles=False, phase_sets=False):
    """A VCF / .vcf.gz -> {contig: (pos0 int64, genotype uint8, qual float32)}, every array sorted by position: the sites
    lcr_import_candidates takes (genotype codes 0-4 and the overwrite rules of vcf.rs:400-462, see include/lcr.h).
    alleles=True: three more uint8 arrays per contig, (..., ref, alt, phase) of lcr_vcf_contig_alleles.
    phase_sets=True: one more uint32 array behind them, the FORMAT PS of lcr_vcf_contig_phase_sets (0 = none)."""
    from . import _lib
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.lcr_vcf_open(os.fsencode(path), 0, C.byref(h))
    try:
        if rc:
            raise _lib.LcrError("lcr_vcf_open(%s): %s" % (path, lib.lcr_vcf_last_error(h).decode() if h else "out of memory"))
        n, names = C.c_int32(), C.POINTER(C.c_char_p)()
        if lib.lcr_vcf_contigs(h, C.byref(n), C.byref(names)):
            raise _lib.LcrError(lib.lcr_vcf_last_error(h).decode())
        out = {}
        for name in [names[i] for i in range(n.value)]:
            m, pos, gt, q = C.c_int32(), C.c_void_p(), C.c_void_p(), C.c_void_p()
            if lib.lcr_vcf_contig(h, name, C.byref(m), C.byref(pos), C.byref(gt), C.byref(q)):
                raise _lib.LcrError(lib.lcr_vcf_last_error(h).decode())
            k = m.value

            def arr(ptr, dt):
                if k == 0:
                    return np.zeros(0, dt)
                return np.frombuffer((C.c_char * (k * np.dtype(dt).itemsize)).from_address(ptr.value), dtype=dt).copy()
            out[name.decode()] = (arr(pos, np.int64), arr(gt, np.uint8), arr(q, np.float32))
            if alleles:
                ref, alt, ph = C.c_void_p(), C.c_void_p(), C.c_void_p()
                if lib.lcr_vcf_contig_alleles(h, name, C.byref(m), C.byref(ref), C.byref(alt), C.byref(ph)) or m.value != k:
                    raise _lib.LcrError(lib.lcr_vcf_last_error(h).decode())
                out[name.decode()] += (arr(ref, np.uint8), arr(alt, np.uint8), arr(ph, np.uint8))
            if phase_sets:
                ps = C.c_void_p()
                if lib.lcr_vcf_contig_phase_sets(h, name, C.byref(m), C.byref(ps)) or m.value != k:
                    raise _lib.LcrError(lib.lcr_vcf_last_error(h).decode())
                out[name.decode()] += (arr(ps, np.uint32),)
        return out
    finally:
        if h:
            lib.lcr_vcf_close(h)


def haplotag_sites(contig_arrays):
    """One contig's read_sites(path, alleles=True, phase_sets=True) tuple -> (pos0 int64, h1 uint8, h2 uint8, ps uint32): the sites
    Engine.haplotag takes.  Kept are the phased heterozygous SNVs: genotype code 1, phase 1 (`0|1`) or 2 (`1|0`), REF and ALT one base
    each and both in ACGT after upper-casing.  `0|1` puts REF on haplotype 1 and ALT on haplotype 2, `1|0` the reverse.  ps is the
    file's PS; a site without one (0) gets the 1-based position of the contig's first kept site -- one contig-wide set, named the way
    the project names its own sets (after the first site's position)."""
    pos0, gt, _q, ref, alt, phase, ps = contig_arrays
    up = lambda a: np.where((a >= ord("a")) & (a <= ord("z")), a - 32, a).astype(np.uint8)
    r, a = up(np.asarray(ref, np.uint8)), up(np.asarray(alt, np.uint8))
    acgt = np.frombuffer(b"ACGT", np.uint8)
    keep = (np.asarray(gt) == 1) & ((np.asarray(phase) == 1) | (np.asarray(phase) == 2)) & np.isin(r, acgt) & np.isin(a, acgt)
    p, r, a, ph = np.asarray(pos0, np.int64)[keep], r[keep], a[keep], np.asarray(phase)[keep]
    out_ps = np.asarray(ps, np.uint32)[keep].copy()
    if p.size:
        out_ps[out_ps == 0] = np.uint32(int(p[0]) + 1)
    return p, np.where(ph == 1, r, a).astype(np.uint8), np.where(ph == 1, a, r).astype(np.uint8), out_ps


def _f2(x):  # Rust `{:.2}` of an f32: NaN prints as "NaN" (an imported site at a column without A/C/G/T counts)
    return "NaN" if x != x else "%.2f" % x


def _as_i32(x):  # Rust `f64 as i32`: saturating, NaN -> 0
    if x != x:
        return 0
    if x >= 2147483647.0:
        return 2147483647
    if x <= -2147483648.0:
        return -2147483648
    return int(x)


def format_records(cands, chrom, min_phase_score):
    out = []
    for s in cands:
        ref, a1, a2 = chr(s["ref_base"]), chr(s["allele1"]), chr(s["allele2"])
        fl, vt, gtp = int(s["flags"]), int(s["variant_type"]), int(s["genotype"])
        alt, af = [], [0.0, 0.0]

        def one_alt():
            if a1 != ref:
                alt[:] = [a1]; af[0] = float(s["af1"])
            elif a2 != ref:
                alt[:] = [a2]; af[0] = float(s["af2"])

        def two_alt():
            alt[:] = [a1, a2]; af[0] = float(s["af1"]); af[1] = float(s["af2"])

        def by_genotype():
            nonlocal gt, filt
            if gtp in (-1, 1):
                one_alt()
                gt, filt = ("1/1", "PASS") if gtp == -1 else ("0/0", "HomRef")
            elif gtp == 0:
                two_alt()
                gt, filt = "1/2", "Multiallelic"

        gt, filt = "0/0", ""
        gq, dp, qual = _as_i32(float(s["gq"])), int(s["depth"]), _as_i32(float(s["qual"]))
        if fl & _abi.F_DENSE:  # vcf.rs:31-78
            if vt in (1, 2):
                one_alt()
            elif vt == 3:
                two_alt()
            if vt not in (1, 2, 3):
                continue
            gt = {1: "0/1", 2: "1/1", 3: "1/2"}[vt]
            filt, info, fmt = "dn", "RDS=dense_snp", "GT:GQ:DP:AF"
            sample = ("%s:%d:%d:%s,%s" % (gt, gq, dp, _f2(af[0]), _f2(af[1])) if vt == 3
                      else "%s:%d:%d:%s" % (gt, gq, dp, _f2(af[0])))
        elif fl & _abi.F_NON_SELECTED:  # vcf.rs:80-174
            info, fmt = "RDS=noselect", "GT:GQ:DP:AF"
            if fl & _abi.F_RNA_EDIT:
                if vt not in (1, 2):
                    continue
                one_alt()
                filt = "RnaEdit"
                gt = "0/1" if vt == 1 else "1/1"
                sample = "%s:%d:%d:%s" % (gt, gq, dp, _f2(af[0]))
            else:
                if vt in (0, 1, 2):
                    one_alt()
                    gt, filt = {0: ("0/0", "HomRef"), 1: ("0/1", "LowQual"), 2: ("1/1", "PASS")}[vt]
                else:
                    by_genotype()
                sample = ("%s:%d:%d:%s" % (gt, gq, dp, _f2(af[0])) if gt in ("0/0", "0/1", "1/1")
                          else "%s:%d:%d:%s,%s" % (gt, gq, dp, _f2(af[0]), _f2(af[1])))
        else:  # vcf.rs:175-303
            info, fmt = "RDS=select", "GT:GQ:PS:DP:AF:PQ"
            if float(s["phase_score"]) >= float(min_phase_score):
                if vt == 1:
                    one_alt()
                    gt, filt = ("0|1" if int(s["haplotype"]) == 1 else "1|0"), "PASS"
            else:
                if vt in (0, 1, 2):
                    one_alt()
                    gt, filt = {0: ("0/0", "HomRef"), 1: ("0/1", "LowQual"), 2: ("1/1", "PASS")}[vt]
                else:
                    by_genotype()
            ps = str(int(s["phase_set"])) if int(s["phase_set"]) != 0 else "."
            pq = float(s["phase_score"])
            sample = ("%s:%d:%s:%d:%s:%.2f" % (gt, gq, ps, dp, _f2(af[0]), pq) if gt in ("0/0", "0/1", "1/1", "0|1", "1|0")
                      else "%s:%d:%s:%d:%s,%s:%.2f" % (gt, gq, ps, dp, _f2(af[0]), _f2(af[1]), pq))
        if len(alt) not in (1, 2):
            continue
        out.append("%s\t%d\t.\t%s\t%s\t%d\t%s\t%s\t%s\t%s\n" % (
            chrom, int(s["pos"]) + 1, ref, ",".join(alt), qual, filt, info, fmt, sample))
    return "".join(out)

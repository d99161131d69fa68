"""Host-side mirror of the reference's per-region call sequence (src/thread.rs:93-201) on top of
the C ABI.  Names follow the reference methods they replace:

    Engine.fill_data_into_freq_vec  -> Profile::fill_data_into_freq_vec   (util.rs:621)
    Engine.get_candidate_snps       -> SNPFrag::get_candidate_snps        (candidate.rs:54)
    Engine.import_external_candidates -> SNPFrag::import_external_candidates (candidate.rs:530)
    Engine.get_fragments            -> SNPFrag::get_fragments             (fragment.rs:10)
    Engine.phase                    -> SNPFrag::phase + post-phase steps  (phase.rs:1087, snpfrags.rs)

All compute happens in liblcr.so (HIP); this module only marshals numpy / device pointers.
"""
import ctypes as C

import numpy as np

from . import _abi, _lib
from ._lib import LcrError


def _view(ptr, dtype, n):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (np.dtype(dtype).itemsize * n)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=n).copy()


def _view_nocopy(ptr, dtype, n):
    """the context's own buffer as an array (no copy): valid until the call that rewrites it"""
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (np.dtype(dtype).itemsize * n)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=n)


_DEBUG_ENV = {"LCR_PHASE_PROF": "phase_prof", "LCR_GRID_MIN_ENTRIES": "grid_min_entries",
              "LCR_GRID_GENERIC": "grid_generic", "LCR_GRID_SPEC_LANES": "grid_spec_lanes", "LCR_GRID_SPEC_BATCH": "grid_spec_batch", "LCR_POST_HALF": "post_half", "LCR_ENUM_FORCE_BIG": "enum_force_big",
              "LCR_ENUM_FORCE_STREAM": "enum_force_stream", "LCR_ENUM_ELIDE": "enum_elide", "LCR_HIST_TILES": "hist_tiles", "LCR_TIE_ARITH": "tie_arith", "LCR_CHAIN_TIES": "chain_ties", "LCR_K3_HITS": "k3_hits", "LCR_K3_LIST_BLOCKS": "k3_list_blocks", "LCR_FUSE_FILTER": "fuse_filter", "LCR_ASYNC_PHASE": "async_phase", "LCR_HOST_TRACE": "host_trace", "LCR_OWN_FILL": "own_fill", "LCR_REDO_LDS": "redo_lds", "LCR_SPEC_COMPACT": "spec_compact", "LCR_LEAN_PLANES": "lean_planes", "LCR_FOLD_INDELS": "fold_indels"}


class Engine:
    def __init__(self, device=0, params=None, timing=False):
        self.lib = _lib.load()
        h = C.c_void_p()
        rc = self.lib.lcr_ctx_create(device, C.byref(h))
        if rc != 0:
            raise LcrError("lcr_ctx_create(device=%d) failed with %d: no usable HIP device; "
                           "liblcr has no CPU fallback" % (device, rc))
        self.h = h
        self.device = device
        self.params = params if params is not None else _abi.make_params()
        self._sites = None   # device tensors of the last import_external_candidates: its kernels read them after the call returns
        self._keep = None
        self._n_regions = None   # regions of the bound batch (set_exon_mask sizes iv_off by it)
        self._mask_keep = None
        self.last_truncated_columns = 0   # columns above the cap of the last discover_regions(truncation=True)
        if timing:
            self.lib.lcr_enable_timing(self.h, 1)
            if timing is not True:   # an iterable of _abi.K_* : only these kernel groups get their two event records per call
                self.debug_set("timing_mask", sum(1 << int(k) for k in timing))
        # developer / test hooks: the library reads no environment variable; this mirror hands LCR_* switches on (tests, tools)
        import os
        for env, key in _DEBUG_ENV.items():
            v = os.environ.get(env)
            if v is not None:
                self.debug_set(key, int(v) if v.lstrip("-").isdigit() else 1)
        if os.environ.get("LCR_LOCK_DIR"):
            self._chk(self.lib.lcr_ctx_set_lock_dir(self.h, os.fsencode(os.environ["LCR_LOCK_DIR"])), "lcr_ctx_set_lock_dir")

    def debug_set(self, key, value):
        self._chk(self.lib.lcr_debug_set(self.h, key.encode(), int(value)), "lcr_debug_set")
        return self

    def close(self):
        if getattr(self, "h", None):
            self.lib.lcr_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc, what):
        if rc != 0:
            raise LcrError("%s failed (%d): %s" % (what, rc, self.lib.lcr_last_error(self.h).decode()))

    def set_stream(self, hip_stream_ptr):
        self._chk(self.lib.lcr_ctx_set_stream(self.h, C.c_void_p(hip_stream_ptr)), "lcr_ctx_set_stream")

    def sync(self):
        self._chk(self.lib.lcr_ctx_sync(self.h), "lcr_ctx_sync")
        self._sites = None
        self._mask_keep = None   # (device intervals of the last set_exon_mask: the builder has read them)

    def set_async_phase(self, on=True):
        """lcr_ctx_set_async_phase: phase() returns with its kernels in flight; getters / sync() collect the results (include/lcr.h)"""
        rc = self.lib.lcr_ctx_set_async_phase(self.h, 1 if on else 0)
        self.async_warning = self.lib.lcr_last_error(self.h).decode() if rc > 0 else None   # (LCR_W_HW_QUEUES: on, but GPU_MAX_HW_QUEUES < 8)
        if rc < 0:
            self._chk(rc, "lcr_ctx_set_async_phase")
        return self

    # ---- batch binding -------------------------------------------------------------------------
    def load_batch(self, batch):
        """batch: _abi.ReadBatch or _abi.PackedReadBatch (host numpy), or a (LcrReads | LcrReadsPacked, LcrRegions, keepalive) device
        triple.  A packed batch (bases as BAM nibbles) goes through lcr_load_batch_packed: the engine unpacks it on the GPU and is
        afterwards in the state the unpacked batch would leave."""
        if isinstance(batch, (_abi.ReadBatch, _abi.PackedReadBatch)):
            reads, regions = batch.c_reads(), batch.c_regions()
            self._keep = (batch, reads, regions)
        else:
            reads, regions, keep = batch
            self._keep = (keep, reads, regions)
        if isinstance(reads, _abi.LcrReadsPacked):
            self._chk(self.lib.lcr_load_batch_packed(self.h, C.byref(reads), C.byref(regions)), "lcr_load_batch_packed")
        else:
            self._chk(self.lib.lcr_load_batch(self.h, C.byref(reads), C.byref(regions)), "lcr_load_batch")
        self._n_regions = int(regions.n_regions)
        return self

    def load_batch_async(self, batch, slot):
        """Enqueue the upload of a host batch (_abi.ReadBatch or _abi.PackedReadBatch) into staging slot 0 / 1 and return; bind_batch(slot)
        makes it the current batch.  The batch's arrays should be page-locked (host_register) for the copy to run beside the kernels.
        A packed batch crosses the link as nibbles and is unpacked on the upload stream (lcr_load_batch_packed_async)."""
        reads, regions = batch.c_reads(), batch.c_regions()
        if not hasattr(self, "_keep_slot"):
            self._keep_slot = {}
        if isinstance(reads, _abi.LcrReadsPacked):
            self._chk(self.lib.lcr_load_batch_packed_async(self.h, C.byref(reads), C.byref(regions), int(slot)), "lcr_load_batch_packed_async")
        else:
            self._chk(self.lib.lcr_load_batch_async(self.h, C.byref(reads), C.byref(regions), int(slot)), "lcr_load_batch_async")
        self._keep_slot[int(slot)] = (batch, reads, regions)
        return self

    def unpack_bases(self, seq_len, seq_off, pack_off, seq4, bases_out):
        """lcr_unpack_bases: the unpack kernel by itself, over contiguous 1-d tensors on this engine's device -- seq_len int32, seq_off
        and pack_off uint64 or int64 (n_reads each), seq4 and bases_out uint8.  Writes read i's bases to bases_out[seq_off[i] :
        seq_off[i] + seq_len[i]] and no other byte; returns after the kernel's verdict (LcrError for a read that leaves either array:
        that read is skipped whole)."""
        import torch
        want = (("seq_len", seq_len, (torch.int32,)), ("seq_off", seq_off, (torch.int64, torch.uint64)), ("pack_off", pack_off, (torch.int64, torch.uint64)),
                ("seq4", seq4, (torch.uint8,)), ("bases_out", bases_out, (torch.uint8,)))
        for name, t, dts in want:
            if not getattr(t, "is_cuda", False) or t.dtype not in dts or t.device.index != self.device or t.dim() != 1 or not t.is_contiguous():
                raise ValueError("unpack_bases: %s must be a contiguous 1-d %s tensor on device %d" % (name, dts[0], self.device))
        if not (seq_len.numel() == seq_off.numel() == pack_off.numel()):
            raise ValueError("seq_len, seq_off and pack_off must have the same length")
        torch.cuda.current_stream(self.device).synchronize()   # (the tensors may still be being written on torch's stream)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
        self._chk(self.lib.lcr_unpack_bases(self.h, int(seq_len.numel()), ptr(seq_len), ptr(seq_off), ptr(pack_off), ptr(seq4), int(seq4.numel()),
                                            ptr(bases_out), int(bases_out.numel())), "lcr_unpack_bases")
        return self

    def unpack_ms(self):
        """lcr_unpack_ms: HIP-event time of the last unpack kernel (timing on)"""
        ms = C.c_float()
        self._chk(self.lib.lcr_unpack_ms(self.h, C.byref(ms)), "lcr_unpack_ms")
        return float(ms.value)

    def bind_batch(self, slot):
        self._chk(self.lib.lcr_bind_batch(self.h, int(slot)), "lcr_bind_batch")
        self._n_regions = int(self._keep_slot[int(slot)][2].n_regions)
        return self

    def discover_regions(self, ref_start, ref_end, contig_len, truncation=False, truncation_coverage=200000):
        """find_isolated_regions_with_depth (util.rs:236-332) for one contig -> [(start0, len, max_cov)].
        truncation / truncation_coverage: longcallR --truncation / --truncation-coverage -- a column deeper than the cap ends a
        region like an uncovered one (include/lcr.h).  last_truncated_columns holds the number of such columns of the last call
        (0 with truncation off)."""
        if not 0 <= int(truncation_coverage) < 1 << 32:
            raise ValueError("truncation_coverage must be in [0, 2^32), got %r" % (truncation_coverage,))
        rs = np.ascontiguousarray(ref_start, dtype=np.int32)
        re_ = np.ascontiguousarray(ref_end, dtype=np.int32)
        o = _abi.LcrRegionList()
        nt = C.c_int64(0)
        self._chk(self.lib.lcr_discover_regions_truncated(self.h, _abi.LCR_MEM_HOST, int(rs.size), rs.ctypes.data, re_.ctypes.data,
                                                          int(contig_len), 1 if truncation else 0, int(truncation_coverage), C.byref(o),
                                                          C.byref(nt)), "lcr_discover_regions_truncated")
        self.last_truncated_columns = int(nt.value)
        return list(zip(_view(o.start0, np.int64, o.n_regions).tolist(), _view(o.len, np.int32, o.n_regions).tolist(),
                        _view(o.max_cov, np.uint32, o.n_regions).tolist()))

    # ---- stages ----------------------------------------------------------------------------------
    def fill_data_into_freq_vec(self):
        self._chk(self.lib.lcr_pileup(self.h, C.byref(self.params)), "lcr_pileup")
        return self

    def get_candidate_snps(self):
        self._chk(self.lib.lcr_candidates(self.h, C.byref(self.params)), "lcr_candidates")
        return self

    def import_external_candidates(self, pos0, genotype, qual):
        """SNPFrag::import_external_candidates (candidate.rs:530-613): the candidate stage from user-provided sites instead of
        get_candidate_snps -- pos0 ascending and unique, genotype codes 0-4, qual f32 (vcf.read_sites gives them per contig).
        numpy arrays (converted), or contiguous int64 / uint8 / float32 tensors on this engine's device, used in place
        (LCR_MEM_DEVICE): they are made ready on the context's stream (the current torch stream is waited for) and held by the
        engine until the stage's kernels have read them (get_fragments, candidates, sync or the next import)."""
        if any(getattr(t, "is_cuda", False) for t in (pos0, genotype, qual)):
            import torch
            ts = (pos0, genotype, qual)
            want = (torch.int64, torch.uint8, torch.float32)
            if not all(getattr(t, "is_cuda", False) for t in ts):
                raise ValueError("device sites: pos0, genotype and qual must all be device tensors")
            for name, t, dt in zip(("pos0", "genotype", "qual"), ts, want):
                if t.dtype != dt:
                    raise ValueError("device sites: %s must be %s, got %s" % (name, dt, t.dtype))
                if t.device.index != self.device:
                    raise ValueError("device sites: %s is on %s, the engine on device %d" % (name, t.device, self.device))
                if t.dim() != 1 or not t.is_contiguous():
                    raise ValueError("device sites: %s must be a contiguous 1-d tensor" % name)
            if len({t.numel() for t in ts}) != 1:
                raise ValueError("pos0, genotype and qual must have the same length")
            self._release_sites()
            torch.cuda.current_stream(self.device).synchronize()   # (the tensors may still be being written on torch's stream)
            self._chk(self.lib.lcr_import_candidates(self.h, C.byref(self.params), _abi.LCR_MEM_DEVICE, int(pos0.numel()),
                                                     *[C.c_void_p(t.data_ptr()) for t in ts]), "lcr_import_candidates")
            self._sites = ts
            return self
        p = np.ascontiguousarray(pos0, dtype=np.int64)
        g = np.ascontiguousarray(genotype, dtype=np.uint8)
        q = np.ascontiguousarray(qual, dtype=np.float32)
        if not (p.size == g.size == q.size):
            raise ValueError("pos0, genotype and qual must have the same length")
        self._release_sites()
        self._chk(self.lib.lcr_import_candidates(self.h, C.byref(self.params), _abi.LCR_MEM_HOST, int(p.size), p.ctypes.data, g.ctypes.data,
                                                 q.ctypes.data), "lcr_import_candidates")   # (host arrays are copied before the call returns)
        return self

    def set_exon_mask(self, iv_off, start0, end0, mem=None):
        """lcr_set_exon_mask on the bound batch (longcallR --exon-only; include/lcr.h): region g owns intervals [iv_off[g], iv_off[g + 1])
        of start0 / end0, reference coordinates, 0-based half-open, in any order; get_candidate_snps then drops every column outside them.
        numpy arrays or sequences (converted to int32 / int64 / int64 and copied: LCR_MEM_HOST), or contiguous tensors of those types on
        this engine's device, read in place (LCR_MEM_DEVICE) and held by the engine until sync() or the next mask.  mem: None = by the
        arguments' kind, or _abi.LCR_MEM_HOST / LCR_MEM_DEVICE to insist.  The mask lasts until load_batch / bind_batch or clear_exon_mask()."""
        if self._n_regions is None:
            raise LcrError("set_exon_mask before load_batch / bind_batch")
        if len(iv_off) != self._n_regions + 1:
            raise ValueError("iv_off needs n_regions + 1 = %d entries, got %d" % (self._n_regions + 1, len(iv_off)))
        ts = (iv_off, start0, end0)
        dev = any(getattr(t, "is_cuda", False) for t in ts)
        if mem is not None and mem not in (_abi.LCR_MEM_HOST, _abi.LCR_MEM_DEVICE):
            raise ValueError("mem must be _abi.LCR_MEM_HOST or _abi.LCR_MEM_DEVICE, got %r" % (mem,))
        if mem is not None and (mem == _abi.LCR_MEM_DEVICE) != dev:
            raise ValueError("mem does not match the arrays: device tensors go with LCR_MEM_DEVICE, host arrays with LCR_MEM_HOST")
        if dev:
            import torch
            for name, t, dt in zip(("iv_off", "start0", "end0"), ts, (torch.int32, torch.int64, torch.int64)):
                if not getattr(t, "is_cuda", False) or t.dtype != dt or t.device.index != self.device or t.dim() != 1 or not t.is_contiguous():
                    raise ValueError("device intervals: %s must be a contiguous 1-d %s tensor on device %d" % (name, dt, self.device))
            if start0.numel() != end0.numel():
                raise ValueError("start0 and end0 must have the same length")
            torch.cuda.current_stream(self.device).synchronize()   # (the tensors may still be being written on torch's stream)
            if int(iv_off[-1]) > start0.numel():   # (the library takes the interval count from iv_off: it must not read past the tensors)
                raise ValueError("iv_off ends at %d, beyond the %d intervals" % (int(iv_off[-1]), start0.numel()))
            self._chk(self.lib.lcr_set_exon_mask(self.h, _abi.LCR_MEM_DEVICE, C.c_void_p(iv_off.data_ptr()),
                                                 C.c_void_p(start0.data_ptr()) if start0.numel() else None,
                                                 C.c_void_p(end0.data_ptr()) if end0.numel() else None), "lcr_set_exon_mask")
            self._mask_keep = ts
            return self
        o = np.ascontiguousarray(iv_off, dtype=np.int32)
        s = np.ascontiguousarray(start0, dtype=np.int64)
        e = np.ascontiguousarray(end0, dtype=np.int64)
        if s.size != e.size:
            raise ValueError("start0 and end0 must have the same length")
        if o[-1] != s.size and o[0] == 0 and np.all(np.diff(o) >= 0):   # (offsets the library would refuse are left to it)
            raise ValueError("iv_off must end at the number of intervals (%d), got %d" % (s.size, int(o[-1])))
        self._chk(self.lib.lcr_set_exon_mask(self.h, _abi.LCR_MEM_HOST, o.ctypes.data, s.ctypes.data if s.size else None,
                                             e.ctypes.data if e.size else None), "lcr_set_exon_mask")   # (host arrays are copied before the call returns)
        return self

    def clear_exon_mask(self):
        """lcr_set_exon_mask(NULL): the bound batch has no exon mask any more"""
        self._chk(self.lib.lcr_set_exon_mask(self.h, _abi.LCR_MEM_HOST, None, None, None), "lcr_set_exon_mask")
        return self

    def exon_mask_ms(self):
        """lcr_exon_mask_ms: HIP-event time of the last set_exon_mask's kernels (timing on)"""
        ms = C.c_float()
        self._chk(self.lib.lcr_exon_mask_ms(self.h, C.byref(ms)), "lcr_exon_mask_ms")
        return float(ms.value)

    def _release_sites(self):
        """drop the device sites of the last import once its kernels are done (they are queued behind the call's return)"""
        if self._sites is not None:
            self.sync()

    def get_fragments(self):
        self._chk(self.lib.lcr_fragments(self.h, C.byref(self.params)), "lcr_fragments")
        self._sites = None   # (lcr_fragments has waited for the candidate stage: the imported sites are read)
        return self

    def phase(self):
        self._chk(self.lib.lcr_phase(self.h, C.byref(self.params)), "lcr_phase")
        return self

    def haplotag(self, sites):
        """lcr_haplotag in place of phase(): the rows of fragmat() tagged on the haplotypes and phase sets of a phased VCF (include/lcr.h;
        `whatshap haplotag` on the fragment matrix).  sites: (pos0, h1, h2, phase_set) of the batch's contig -- vcf.haplotag_sites gives
        them --, pos0 ascending and unique, h1 / h2 the ASCII base on haplotype 1 / 2, phase_set != 0; None or empty arrays: every row is
        unassigned.  numpy arrays (converted), or contiguous int64 / uint8 / uint8 / uint32 tensors on this engine's device, read in place
        and held by the engine until sync().  Afterwards phase_result(), candidates(), collect_phase(), junctions(), ase() and the per-gene
        calls answer as behind phase(); haplotag_sites() has the per-candidate evidence.  Down-sampling is ignored."""
        if sites is None:
            rc = self.lib.lcr_haplotag(self.h, C.byref(self.params), _abi.LCR_MEM_HOST, 0, None, None, None, None)
        elif any(getattr(t, "is_cuda", False) for t in sites):
            import torch
            ts = tuple(sites)
            u32 = tuple(d for d in (getattr(torch, "uint32", None), torch.int32) if d is not None)   # (the same 32 bits either way)
            for name, t, dt in zip(("pos0", "h1", "h2", "phase_set"), ts, (torch.int64, torch.uint8, torch.uint8, u32)):
                dts = dt if isinstance(dt, tuple) else (dt,)
                if not getattr(t, "is_cuda", False) or t.dtype not in dts or t.device.index != self.device or t.dim() != 1 or not t.is_contiguous():
                    raise ValueError("device sites: %s must be a contiguous 1-d %s tensor on device %d" % (name, dts[0], self.device))
            if len({t.numel() for t in ts}) != 1:
                raise ValueError("pos0, h1, h2 and phase_set must have the same length")
            self._release_sites()
            torch.cuda.current_stream(self.device).synchronize()   # (the tensors may still be being written on torch's stream)
            n = int(ts[0].numel())
            rc = self.lib.lcr_haplotag(self.h, C.byref(self.params), _abi.LCR_MEM_DEVICE, n, *[C.c_void_p(t.data_ptr()) if n else None for t in ts])
            if rc == 0:
                self._sites = ts   # (the kernels behind the call's return read them: released by sync())
        else:
            pos = np.ascontiguousarray(sites[0], dtype=np.int64)
            h1 = np.ascontiguousarray(sites[1], dtype=np.uint8)
            h2 = np.ascontiguousarray(sites[2], dtype=np.uint8)
            ps = np.ascontiguousarray(sites[3], dtype=np.uint32)
            if not (pos.size == h1.size == h2.size == ps.size):
                raise ValueError("pos0, h1, h2 and phase_set must have the same length")
            n = int(pos.size)
            rc = self.lib.lcr_haplotag(self.h, C.byref(self.params), _abi.LCR_MEM_HOST, n, *[a.ctypes.data if n else None for a in (pos, h1, h2, ps)])
        self._chk(rc, "lcr_haplotag")
        return self

    def haplotag_sites(self):
        """lcr_get_haplotag_sites after haplotag(): one record per candidate of candidates() as a structured array of _abi.HAPSITE_DTYPE,
        copied -- zeros for a candidate the tagging did not use."""
        n, rec, dev = C.c_int32(), C.c_void_p(), C.c_void_p()
        self._chk(self.lib.lcr_get_haplotag_sites(self.h, C.byref(n), C.byref(rec), C.byref(dev)), "lcr_get_haplotag_sites")
        return _view(rec.value, _abi.HAPSITE_DTYPE, n.value)

    def haplotag_ms(self):
        """lcr_haplotag_ms: HIP-event time of the last haplotag()'s kernels behind the check of the sites (timing on)"""
        ms = C.c_float()
        self._chk(self.lib.lcr_haplotag_ms(self.h, C.byref(ms)), "lcr_haplotag_ms")
        return float(ms.value)

    def junctions(self, min_count=10, min_junctions=2):
        """lcr_junctions + lcr_get_junctions after phase(): the kept junctions of every region with their haplotype x presence tables
        (include/lcr.h; the table longcallR-asj.py builds per gene) -> (records as a structured array of _abi.JUNC_DTYPE, copied;
        junc_region_off, n_regions + 1).  Waits for an asynchronous phase stage in flight; may be repeated with other parameters."""
        p = _abi.LcrJunctionParams(int(min_count), int(min_junctions))
        self._chk(self.lib.lcr_junctions(self.h, C.byref(p)), "lcr_junctions")
        o = _abi.LcrJunctionList()
        self._chk(self.lib.lcr_get_junctions(self.h, C.byref(o)), "lcr_get_junctions")
        return _view(o.junc, _abi.JUNC_DTYPE, o.n_junctions), _view(o.junc_region_off, np.int32, o.n_regions + 1)

    def ase(self, sites=None, min_baseq=13, min_phase_score=None):
        """lcr_ase + lcr_get_ase after phase(): per region the phase set with the most assigned rows, its haplotype counts and -- with
        parental sites -- the parent-of-origin votes of those rows (include/lcr.h; what longcallR-ase.py computes per gene) -> a
        structured array of _abi.ASE_DTYPE, one record per region, copied.  sites: None (plain mode: the site and vote fields stay 0) or
        (pos0, pat, mat) of the batch's contig -- numpy arrays (converted), or contiguous int64 / uint8 / uint8 tensors on this engine's
        device, read in place.  min_phase_score: the VCF writer's (default: the engine's params).  Waits for an asynchronous phase stage
        in flight; may be repeated with other parameters or sites."""
        self._ase_call(self.lib.lcr_ase, "lcr_ase", sites, min_baseq, min_phase_score)
        o = _abi.LcrAseList()
        self._chk(self.lib.lcr_get_ase(self.h, C.byref(o)), "lcr_get_ase")   # (waits for the call's kernels: device sites are read by then)
        return _view(o.rec, _abi.ASE_DTYPE, o.n_regions)

    def site_counts(self, min_baseq=13):
        """lcr_site_counts + lcr_get_site_counts after phase() or haplotag(): per candidate of candidates() how often each base was seen
        on each haplotype of the site's phase set, and on every other row (include/lcr.h) -> a structured array of _abi.SITE_COUNT_DTYPE,
        one record per candidate, copied.  Waits for an asynchronous phase stage in flight; may be repeated with another threshold."""
        p = _abi.LcrSiteCountParams(int(min_baseq))
        self._chk(self.lib.lcr_site_counts(self.h, C.byref(p)), "lcr_site_counts")
        n, rec, dev = C.c_int32(), C.c_void_p(), C.c_void_p()
        self._chk(self.lib.lcr_get_site_counts(self.h, C.byref(n), C.byref(rec), C.byref(dev)), "lcr_get_site_counts")
        return _view(rec.value, _abi.SITE_COUNT_DTYPE, n.value)

    def site_counts_ms(self):
        """lcr_site_counts_ms: HIP-event time of the last site_counts()'s kernels (timing on)"""
        ms = C.c_float()
        self._chk(self.lib.lcr_site_counts_ms(self.h, C.byref(ms)), "lcr_site_counts_ms")
        return float(ms.value)

    def site_pairs(self, mode="all", max_partners=2, max_dist=2, min_baseq=13):
        """lcr_site_pairs + lcr_get_site_pairs after phase() or haplotag(): per pair of nearby eligible candidates of candidates() how
        many rows carry which base at the first site and which at the second (include/lcr.h) -> (records as a structured array of
        _abi.SITE_PAIR_DTYPE, ordered by a, then b; pair_off, n_cand + 1; n_eligible), copied.  mode: "all" (every candidate that is not
        dense) or "phased" (phased hets only); max_dist 0: no distance limit.  Waits for an asynchronous phase stage in flight; may be
        repeated with other parameters."""
        modes = {"all": _abi.PAIRS_ALL, "phased": _abi.PAIRS_PHASED}
        if mode not in modes:
            raise ValueError("site_pairs: mode must be 'all' or 'phased', got %r" % (mode,))
        p = _abi.LcrSitePairParams(modes[mode], int(max_partners), int(max_dist), int(min_baseq))
        self._chk(self.lib.lcr_site_pairs(self.h, C.byref(p)), "lcr_site_pairs")
        o = self.site_pairs_list()
        return _view(o.pair, _abi.SITE_PAIR_DTYPE, o.n_pairs), _view(o.pair_off, np.int32, o.n_cand + 1), int(o.n_eligible)

    def site_pairs_list(self):
        """lcr_get_site_pairs: the last site_pairs()'s list (pinned host and HBM pointers)"""
        o = _abi.LcrSitePairList()
        self._chk(self.lib.lcr_get_site_pairs(self.h, C.byref(o)), "lcr_get_site_pairs")
        return o

    def site_pairs_ms(self):
        """lcr_site_pairs_ms: HIP-event time of the last site_pairs()'s kernels (timing on)"""
        ms = C.c_float()
        self._chk(self.lib.lcr_site_pairs_ms(self.h, C.byref(ms)), "lcr_site_pairs_ms")
        return float(ms.value)

    def hap_coverage(self):
        """lcr_hap_coverage + lcr_get_hap_coverage after phase() or haplotag(): the covered depth of every window column per haplotype
        class (0 unassigned, 1 / 2 as the HP tag) as run-length segments, and per region the reads, maxima and covered bases per class
        (include/lcr.h) -> (segments as a structured array of _abi.HAP_COV_SEGMENT_DTYPE, ordered by region and start; seg_region_off,
        n_regions + 1; region records as _abi.HAP_COV_REGION_DTYPE), all copied.  Waits for an asynchronous phase stage in flight; may
        be repeated."""
        self._chk(self.lib.lcr_hap_coverage(self.h), "lcr_hap_coverage")
        o = self._hap_coverage_list()
        return (_view(o.seg, _abi.HAP_COV_SEGMENT_DTYPE, o.n_segments), _view(o.seg_region_off, np.int32, o.n_regions + 1),
                _view(o.reg, _abi.HAP_COV_REGION_DTYPE, o.n_regions))

    def _hap_coverage_list(self):
        """lcr_get_hap_coverage: the last hap_coverage()'s list (pinned host and HBM pointers)"""
        o = _abi.LcrHapCovList()
        self._chk(self.lib.lcr_get_hap_coverage(self.h, C.byref(o)), "lcr_get_hap_coverage")
        return o

    def hap_coverage_ms(self):
        """lcr_hap_coverage_ms: HIP-event time of the last hap_coverage()'s kernels, its host wait included (timing on)"""
        ms = C.c_float()
        self._chk(self.lib.lcr_hap_coverage_ms(self.h, C.byref(ms)), "lcr_hap_coverage_ms")
        return float(ms.value)

    def somatic(self, purity=0.3, som_rate=5e-6, het_rate=5e-4, min_baseq=0):
        """lcr_somatic + lcr_get_somatic after phase() or haplotag(): per candidate of candidates() the counted reference / alternate
        entries per haplotype of the site's phase set, the class of each haplotype (0 reference, 1 heterozygous, 2 somatic), the
        somatic call at a LCR_F_CAND_SOMATIC site, and the six fixed-point sums behind them (include/lcr.h; somatic.score for the
        score) -> a structured array of _abi.SOMATIC_SITE_DTYPE, one record per candidate, copied.  Waits for an asynchronous phase
        stage in flight; may be repeated with other parameters."""
        p = _abi.LcrSomaticParams(float(purity), float(som_rate), float(het_rate), int(min_baseq), 0)
        self._chk(self.lib.lcr_somatic(self.h, C.byref(p)), "lcr_somatic")
        n, rec, dev = C.c_int32(), C.c_void_p(), C.c_void_p()
        self._chk(self.lib.lcr_get_somatic(self.h, C.byref(n), C.byref(rec), C.byref(dev)), "lcr_get_somatic")
        return _view(rec.value, _abi.SOMATIC_SITE_DTYPE, n.value)

    def somatic_ms(self):
        """lcr_somatic_ms: HIP-event time of the last somatic()'s kernels (timing on)"""
        ms = C.c_float()
        self._chk(self.lib.lcr_somatic_ms(self.h, C.byref(ms)), "lcr_somatic_ms")
        return float(ms.value)

    def isoforms(self, min_count=10, min_junctions=1):
        """lcr_isoforms + lcr_get_isoforms after phase() or haplotag(): the kept intron chains of every region -- which whole transcript
        structure each haplotype uses -- with their haplotype x presence tables (include/lcr.h) -> (records as a structured array of
        _abi.ISOFORM_DTYPE, ordered by region and chain; iso_region_off, n_regions + 1; chain, the records' keys s << 32 | l as uint64,
        record r's at chain_first .. chain_first + n_junc; row_isoform, per row of fragmat() the record whose chain it holds or -1), all
        copied (isoforms.chains unpacks the keys).  Waits for an asynchronous phase stage in flight; may be repeated with other
        parameters."""
        p = _abi.LcrIsoformParams(int(min_count), int(min_junctions))
        self._chk(self.lib.lcr_isoforms(self.h, C.byref(p)), "lcr_isoforms")
        o = self._isoform_list()
        return (_view(o.iso, _abi.ISOFORM_DTYPE, o.n_isoforms), _view(o.iso_region_off, np.int32, o.n_regions + 1),
                _view(o.chain, np.uint64, o.n_chain), _view(o.row_isoform, np.int32, o.n_rows))

    def _isoform_list(self):
        """lcr_get_isoforms: the last isoforms()'s list (pinned host and HBM pointers)"""
        o = _abi.LcrIsoformList()
        self._chk(self.lib.lcr_get_isoforms(self.h, C.byref(o)), "lcr_get_isoforms")
        return o

    def isoforms_ms(self):
        """lcr_isoforms_ms: HIP-event time of the last isoforms()'s kernels, its two host waits included (timing on)"""
        ms = C.c_float()
        self._chk(self.lib.lcr_isoforms_ms(self.h, C.byref(ms)), "lcr_isoforms_ms")
        return float(ms.value)

    def transcript_ends(self, min_count=10, window=10, strand="ts"):
        """lcr_transcript_ends + lcr_get_transcript_ends after phase() or haplotag(): the kept transcript-end sites of every region --
        where each haplotype's transcripts start (TSS) and end (TES) -- with their haplotype x presence tables (include/lcr.h).  strand:
        "ts" takes a read's transcript strand from its ts tag only, "read" falls back to the read's own strand (direct RNA) -> (records
        as a structured array of _abi.END_SITE_DTYPE, ordered by region, peak, strand and side; site_region_off, n_regions + 1; row_site
        as an (n_rows, 2) array, per row of fragmat() the records its left and right end are assigned to or -1; totals, a dict of n_part
        and n_assigned), all copied.  Waits for an asynchronous phase stage in flight; may be repeated with other parameters."""
        modes = {"ts": _abi.LCR_ENDS_STRAND_TS, "read": _abi.LCR_ENDS_STRAND_READ}
        if strand not in modes:
            raise ValueError("transcript_ends: strand is 'ts' or 'read', not %r" % (strand,))
        p = _abi.LcrEndParams(int(min_count), int(window), modes[strand], 0)
        self._chk(self.lib.lcr_transcript_ends(self.h, C.byref(p)), "lcr_transcript_ends")
        o = self._end_list()
        return (_view(o.site, _abi.END_SITE_DTYPE, o.n_sites), _view(o.site_region_off, np.int32, o.n_regions + 1),
                _view(o.row_site, np.int32, 2 * o.n_rows).reshape(-1, 2), dict(n_part=int(o.n_part), n_assigned=int(o.n_assigned)))

    def _end_list(self):
        """lcr_get_transcript_ends: the last transcript_ends()'s list (pinned host and HBM pointers)"""
        o = _abi.LcrEndList()
        self._chk(self.lib.lcr_get_transcript_ends(self.h, C.byref(o)), "lcr_get_transcript_ends")
        return o

    def transcript_ends_ms(self):
        """lcr_transcript_ends_ms: HIP-event time of the last transcript_ends()'s kernels, its host waits included (timing on)"""
        ms = C.c_float()
        self._chk(self.lib.lcr_transcript_ends_ms(self.h, C.byref(ms)), "lcr_transcript_ends_ms")
        return float(ms.value)

    def intron_retention(self, min_count=10, anchor=10):
        """lcr_intron_retention + lcr_get_intron_retention after phase() or haplotag(): the kept introns of every region -- the junctions
        that at least min_count tagged rows splice -- with the rows that splice them, retain them (one aligned block covers the intron
        and `anchor` columns on either side) or do neither, and their haplotype x {spliced, retained} tables (include/lcr.h) -> (records
        as a structured array of _abi.RETAINED_INTRON_DTYPE, ordered by region, start and length; intron_region_off, n_regions + 1;
        row_retained, per row of fragmat() the number of kept introns it retains; totals, a dict of n_part and n_retained), all
        copied.  Waits for an asynchronous phase stage in flight; may be repeated with other parameters."""
        p = _abi.LcrRetentionParams(int(min_count), int(anchor))
        self._chk(self.lib.lcr_intron_retention(self.h, C.byref(p)), "lcr_intron_retention")
        o = self._retention_list()
        return (_view(o.intron, _abi.RETAINED_INTRON_DTYPE, o.n_introns), _view(o.intron_region_off, np.int32, o.n_regions + 1),
                _view(o.row_retained, np.int32, o.n_rows), dict(n_part=int(o.n_part), n_retained=int(o.n_retained_total)))

    def _retention_list(self):
        """lcr_get_intron_retention: the last intron_retention()'s list (pinned host and HBM pointers)"""
        o = _abi.LcrRetentionList()
        self._chk(self.lib.lcr_get_intron_retention(self.h, C.byref(o)), "lcr_get_intron_retention")
        return o

    def intron_retention_ms(self):
        """lcr_intron_retention_ms: HIP-event time of the last intron_retention()'s kernels, its host waits included (timing on)"""
        ms = C.c_float()
        self._chk(self.lib.lcr_intron_retention_ms(self.h, C.byref(ms)), "lcr_intron_retention_ms")
        return float(ms.value)

    def indels(self, min_count=10, min_permille=150, flank=5, max_ins=12, max_del=50):
        """lcr_indels + lcr_get_indels after phase() or haplotag(): the kept small indels of every region -- the normalised insertions and
        deletions that at least min_count fragment rows hold, and at least min_permille per mille of the depth at their anchor base --
        with the rows that hold them, lack them (one clean aligned block over the event's extent and `flank` columns on either side) or do
        neither, and their haplotype x {present, absent} tables (include/lcr.h) -> (records as a structured array of _abi.INDEL_DTYPE,
        ordered by region and key; indel_region_off, n_regions + 1; row_indels, per row of fragmat() the number of kept events it holds;
        totals, a dict of n_part, n_events and n_present), all copied.  Waits for an asynchronous phase stage in flight; may be repeated
        with other parameters."""
        p = _abi.LcrIndelParams(int(min_count), int(min_permille), int(flank), int(max_ins), int(max_del))
        self._chk(self.lib.lcr_indels(self.h, C.byref(p)), "lcr_indels")
        o = self._indel_list()
        return (_view(o.indel, _abi.INDEL_DTYPE, o.n_indels), _view(o.indel_region_off, np.int32, o.n_regions + 1),
                _view(o.row_indels, np.int32, o.n_rows), dict(n_part=int(o.n_part), n_events=int(o.n_events), n_present=int(o.n_present_total)))

    def _indel_list(self):
        """lcr_get_indels: the last indels()'s list (pinned host and HBM pointers)"""
        o = _abi.LcrIndelList()
        self._chk(self.lib.lcr_get_indels(self.h, C.byref(o)), "lcr_get_indels")
        return o

    def indels_ms(self):
        """lcr_indels_ms: HIP-event time of the last indels()'s kernels, its host waits included (timing on)"""
        ms = C.c_float()
        self._chk(self.lib.lcr_indels_ms(self.h, C.byref(ms)), "lcr_indels_ms")
        return float(ms.value)

    def _ase_call(self, fn, what, sites, min_baseq, min_phase_score):
        """lcr_ase / lcr_ase_genes with the parental sites marshalled: None, numpy arrays (converted) or device tensors (read in place)"""
        p = _abi.LcrAseParams(int(min_baseq), float(self.params.min_phase_score if min_phase_score is None else min_phase_score))
        if sites is None:
            rc = fn(self.h, C.byref(p), _abi.LCR_MEM_HOST, 0, None, None, None)
        elif any(getattr(t, "is_cuda", False) for t in sites):
            import torch
            ts = tuple(sites)
            for name, t, dt in zip(("pos0", "pat", "mat"), ts, (torch.int64, torch.uint8, torch.uint8)):
                if not getattr(t, "is_cuda", False) or t.dtype != dt or t.device.index != self.device or t.dim() != 1 or not t.is_contiguous():
                    raise ValueError("device sites: %s must be a contiguous 1-d %s tensor on device %d" % (name, dt, self.device))
            if len({t.numel() for t in ts}) != 1:
                raise ValueError("pos0, pat and mat must have the same length")
            torch.cuda.current_stream(self.device).synchronize()   # (the tensors may still be being written on torch's stream)
            rc = fn(self.h, C.byref(p), _abi.LCR_MEM_DEVICE, int(ts[0].numel()), *[C.c_void_p(t.data_ptr()) for t in ts])
        else:
            pos = np.ascontiguousarray(sites[0], dtype=np.int64)
            pat = np.ascontiguousarray(sites[1], dtype=np.uint8)
            mat = np.ascontiguousarray(sites[2], dtype=np.uint8)
            if not (pos.size == pat.size == mat.size):
                raise ValueError("pos0, pat and mat must have the same length")
            rc = fn(self.h, C.byref(p), _abi.LCR_MEM_HOST, int(pos.size), pos.ctypes.data, pat.ctypes.data, mat.ctypes.data)
        self._chk(rc, what)

    def assign_genes(self, genes):
        """lcr_assign_genes on the bound batch (any stage; the stage does not move): every read goes to the candidate gene whose merged
        exons its aligned blocks overlap most (include/lcr.h; longcallR-ase.py's assign_reads_to_gene).  genes: the contig's
        annotation.ContigGenes (or any object with its five arrays), or None for no gene at all -- every read then gets -1."""
        a, keep = self._annotation(genes)
        self._chk(self.lib.lcr_assign_genes(self.h, _abi.LCR_MEM_HOST, C.byref(a)), "lcr_assign_genes")   # (host arrays are copied before the call returns)
        return self

    @staticmethod
    def _annotation(genes):
        """lcr_gene_annotation over host arrays -> (the struct, the arrays it points to)"""
        a = _abi.LcrGeneAnnotation()
        keep = []
        if genes is not None and len(genes.span_start0):
            for f, dt in (("span_start0", np.int64), ("span_end0", np.int64), ("exon_off", np.int32), ("exon_start0", np.int64), ("exon_end0", np.int64)):
                keep.append(np.ascontiguousarray(getattr(genes, f), dtype=dt))
                setattr(a, f, keep[-1].ctypes.data)
            a.n_genes, a.n_exons = int(keep[0].size), int(keep[3].size)
            if keep[1].size != a.n_genes or keep[2].size != a.n_genes + 1 or keep[4].size != a.n_exons:
                raise ValueError("annotation arrays: span_end0 needs n_genes, exon_off n_genes + 1, exon_end0 n_exons entries")
        return a, keep

    def read_genes(self):
        """lcr_get_read_genes after assign_genes(): (gene index per read of the batch, -1 = none; its overlap in bases), copied"""
        n, g, ov, dg = C.c_int32(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(self.lib.lcr_get_read_genes(self.h, C.byref(n), C.byref(g), C.byref(ov), C.byref(dg)), "lcr_get_read_genes")
        return _view(g.value, np.int32, n.value), _view(ov.value, np.uint32, n.value)

    def ase_genes(self, sites=None, min_baseq=13, min_phase_score=None):
        """lcr_ase_genes + lcr_get_ase_genes after phase() and assign_genes(): ase()'s counts per (region, gene) pair that has a fragment
        row assigned to the gene -> (records as a structured array of _abi.AGENE_DTYPE, ordered by region and then gene, copied;
        pair_region_off, n_regions + 1).  Parameters as ase().  ase.merge_gene_records turns the pairs into one record per gene."""
        self._ase_call(self.lib.lcr_ase_genes, "lcr_ase_genes", sites, min_baseq, min_phase_score)
        o = _abi.LcrAseGeneList()
        self._chk(self.lib.lcr_get_ase_genes(self.h, C.byref(o)), "lcr_get_ase_genes")
        return _view(o.rec, _abi.AGENE_DTYPE, o.n_pairs), _view(o.pair_region_off, np.int32, o.n_regions + 1)

    def junctions_genes(self, genes, min_count=10, min_junctions=2):
        """lcr_junctions_genes + lcr_get_junctions_genes after phase() and assign_genes(genes): junctions()'s table per (region, gene) pair
        with the script's exon-overlap filter (include/lcr.h; the table longcallR-asj.py builds per gene) -> (records as a structured array
        of _abi.JUNC_GENE_DTYPE, ordered by region, gene, start0 and len, copied; junc_region_off, n_regions + 1).  genes: the annotation
        assign_genes() was called with -- the filter reads its exons.  Waits for an asynchronous phase stage in flight; may be repeated
        with other parameters.  last_junctions_genes_ms holds the call's HIP-event time when timing is on, else -1."""
        p = _abi.LcrJunctionParams(int(min_count), int(min_junctions))
        a, keep = self._annotation(genes)
        self._chk(self.lib.lcr_junctions_genes(self.h, C.byref(p), _abi.LCR_MEM_HOST, C.byref(a)), "lcr_junctions_genes")   # (host arrays are copied before the call returns)
        o = _abi.LcrJunctionGeneList()
        self._chk(self.lib.lcr_get_junctions_genes(self.h, C.byref(o)), "lcr_get_junctions_genes")
        self.last_junctions_genes_ms = float(o.kernel_ms)
        return _view(o.junc, _abi.JUNC_GENE_DTYPE, o.n_junctions), _view(o.junc_region_off, np.int32, o.n_regions + 1)

    def asj_genes(self, genes, min_count=10, min_junctions=2, exons=False, dna_pos0=None, coverage=False, min_phase_score=None):
        """lcr_asj_genes + lcr_get_asj_genes after phase() and assign_genes(genes): junctions_genes()'s table with the script's other modes
        (include/lcr.h).  exons: the interior exon blocks of the participating rows kept by min_count (--cluster_with_exons; the junction
        records do not change, asj.cluster takes the exons).  dna_pos0: the contig's heterozygous DNA SNV positions, 0-based, ascending and
        unique (ase.dna_het_sites) -- rows whose phase set no PASS phased het candidate at one of them supports are not counted
        (--dna_vcf / --rna_vcf); None = no filter, an empty array = nothing is supported.  coverage: reads per gene with more than
        min_junctions junctions (.gene_coverage.tsv).  min_phase_score: the VCF writer's (default: the engine's params).
        -> dict(junc, junc_region_off, exon (_abi.EXON_GENE_DTYPE), exon_region_off, gene_reads (int32 per gene, or None), kernel_ms),
        copied.  With every option off junc / junc_region_off are junctions_genes()'s byte for byte."""
        flags = (_abi.LCR_ASJ_EXONS if exons else 0) | (_abi.LCR_ASJ_DNA_FILTER if dna_pos0 is not None else 0) | (_abi.LCR_ASJ_COVERAGE if coverage else 0)
        p = _abi.LcrAsjParams(int(min_count), int(min_junctions), flags, float(self.params.min_phase_score if min_phase_score is None else min_phase_score))
        dna = None
        if dna_pos0 is not None:
            dna = np.ascontiguousarray(dna_pos0, dtype=np.int64)
            p.n_dna, p.dna_pos0 = int(dna.size), (dna.ctypes.data if dna.size else None)
        a, keep = self._annotation(genes)
        self._chk(self.lib.lcr_asj_genes(self.h, C.byref(p), _abi.LCR_MEM_HOST, C.byref(a)), "lcr_asj_genes")   # (host arrays are copied before the call returns)
        o = _abi.LcrAsjGeneList()
        self._chk(self.lib.lcr_get_asj_genes(self.h, C.byref(o)), "lcr_get_asj_genes")
        return {"junc": _view(o.junc, _abi.JUNC_GENE_DTYPE, o.n_junctions), "junc_region_off": _view(o.junc_region_off, np.int32, o.n_regions + 1),
                "exon": _view(o.exon, _abi.EXON_GENE_DTYPE, o.n_exons), "exon_region_off": _view(o.exon_region_off, np.int32, o.n_regions + 1),
                "gene_reads": _view(o.gene_reads, np.int32, o.n_genes) if o.gene_reads else None, "kernel_ms": float(o.kernel_ms)}

    def set_downsample(self, depth, seed=2025):
        """lcr_set_downsample: regions with at least `depth` fragment rows are phased on a sample of `depth` rows (longcallR --downsample /
        --downsample-depth; thread.rs:149 passes seed 2025).  Sticky; depth = 0 turns it off."""
        self._chk(self.lib.lcr_set_downsample(self.h, int(depth), int(seed)), "lcr_set_downsample")
        return self

    def set_downsample_rows(self, sampled):
        """lcr_set_downsample_rows: the caller's own sample for the next phase() only -- one byte per fragment row of fragmat(), non-zero =
        sampled; call it between get_fragments() and phase()."""
        m = np.ascontiguousarray(sampled, dtype=np.uint8)
        self._chk(self.lib.lcr_set_downsample_rows(self.h, _abi.LCR_MEM_HOST, int(m.size), m.ctypes.data), "lcr_set_downsample_rows")
        return self

    def downsample_info(self):
        """lcr_get_downsample after phase(): dict(applied = per region whether it was down-sampled, sampled = byte per fragment row -- None
        when no region was down-sampled --, dev_sampled = the bytes' address in HBM or 0)"""
        o = _abi.LcrDownsampleInfo()
        self._chk(self.lib.lcr_get_downsample(self.h, C.byref(o)), "lcr_get_downsample")
        return dict(applied=_view(o.region_applied, np.uint8, o.n_regions),
                    sampled=_view(o.sampled, np.uint8, o.n_rows) if o.sampled else None, dev_sampled=int(o.dev_sampled or 0))

    def run_all(self):
        return self.fill_data_into_freq_vec().get_candidate_snps().get_fragments().phase()

    # ---- results ---------------------------------------------------------------------------------
    def columns(self):
        o = _abi.LcrColumns()
        self._chk(self.lib.lcr_get_columns(self.h, C.byref(o)), "lcr_get_columns")
        return _view(o.planes, np.uint32, _abi.NPLANES * o.n_cols).reshape(_abi.NPLANES, o.n_cols)

    def candidates(self):
        o = _abi.LcrCandidateList()
        self._chk(self.lib.lcr_get_candidates(self.h, C.byref(o)), "lcr_get_candidates")
        self._sites = None   # (the getter has waited for the candidate stage)
        return (_view(o.cand, _abi.CAND_DTYPE, o.n_cand), _view(o.region_off, np.int32, o.n_regions + 1))

    def candidates_device(self):
        """(device pointer, count) of the candidate records in HBM (current after get_candidate_snps / phase)."""
        ptr, n = C.c_void_p(), C.c_int32()
        self._chk(self.lib.lcr_get_candidates_device(self.h, C.byref(ptr), C.byref(n)), "lcr_get_candidates_device")
        return int(ptr.value or 0), int(n.value)

    def read_records_device(self):
        """(device pointer, count) of the per-row results as 12-byte records in HBM (current after phase)."""
        ptr, n = C.c_void_p(), C.c_int32()
        self._chk(self.lib.lcr_get_read_records_device(self.h, C.byref(ptr), C.byref(n)), "lcr_get_read_records_device")
        return int(ptr.value or 0), int(n.value)

    def fragmat(self):
        o = _abi.LcrFragmat()
        self._chk(self.lib.lcr_get_fragmat(self.h, C.byref(o)), "lcr_get_fragmat")
        return dict(
            row_region_off=_view(o.row_region_off, np.int32, o.n_regions + 1),
            row_ptr=_view(o.row_ptr, np.int64, o.n_rows + 1), row_read=_view(o.row_read, np.int32, o.n_rows),
            col=_view(o.col, np.int32, o.nnz), val=_view(o.val, np.uint8, o.nnz),
            row_for_phasing=_view(o.row_for_phasing, np.uint8, o.n_rows),
            row_links=_view(o.row_links, np.uint32, o.n_rows))

    def phase_result(self):
        o = _abi.LcrPhaseResult()
        self._chk(self.lib.lcr_get_phase_result(self.h, C.byref(o)), "lcr_get_phase_result")
        return dict(haplotag=_view(o.haplotag, np.int8, o.n_rows), assignment=_view(o.assignment, np.uint8, o.n_rows),
                    phase_set=_view(o.phase_set, np.uint32, o.n_rows),
                    objective=_view(o.objective, np.float64, o.n_regions))

    def collect_phase(self, copy=False):
        """lcr_collect_phase: everything the last phase() produced -- valid after the NEXT batch has been bound and its pileup queued (until
        the next get_candidate_snps()): the getter of a pipelined caller under set_async_phase.  copy=False: the arrays ARE the context's
        buffers (read them before the next get_candidate_snps())."""
        o = _abi.LcrPhaseCollected()
        self._chk(self.lib.lcr_collect_phase(self.h, C.byref(o)), "lcr_collect_phase")
        v = _view if copy else _view_nocopy
        return dict(cand=v(o.cand, _abi.CAND_DTYPE, o.n_cand), cand_region_off=v(o.cand_region_off, np.int32, o.n_regions + 1),
                    row_region_off=v(o.row_region_off, np.int32, o.n_regions + 1),
                    haplotag=v(o.haplotag, np.int8, o.n_rows), assignment=v(o.assignment, np.uint8, o.n_rows),
                    phase_set=v(o.phase_set, np.uint32, o.n_rows), objective=v(o.objective, np.float64, o.n_regions),
                    dev_cand=(int(o.dev_cand or 0), int(o.n_cand)), dev_read_rec=(int(o.dev_read_rec or 0), int(o.n_rows)))

    def ld_blocks(self, region):
        """SNPFrag.ld_blocks of one region after phase(): list of lists of candidate indices (reference order)."""
        n, off, idx = C.c_int32(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        self._chk(self.lib.lcr_get_ld_blocks(self.h, int(region), C.byref(n), C.byref(off), C.byref(idx)), "lcr_get_ld_blocks")
        return [[idx[k] for k in range(off[b], off[b + 1])] for b in range(n.value)]

    TIE_FIELDS = ("sigma_f64", "sigma_flips", "delta_unresolved", "step_unresolved", "best_f64", "best_unresolved", "sigma_unresolved", "delta_step_f64")

    def tie_census(self):
        """exact fixed-point ties of the last phase() and how they were decided (include/lcr.h: lcr_get_tie_census)"""
        out = (C.c_uint64 * 8)()
        self._chk(self.lib.lcr_get_tie_census(self.h, out), "lcr_get_tie_census")
        return dict(zip(self.TIE_FIELDS, [int(x) for x in out]))

    def kernel_ms(self, k):
        ms = C.c_float()
        self._chk(self.lib.lcr_kernel_ms(self.h, k, C.byref(ms)), "lcr_kernel_ms")
        return float(ms.value)

    def pileup_bytes(self):
        b = C.c_int64()
        self._chk(self.lib.lcr_pileup_bytes(self.h, C.byref(b)), "lcr_pileup_bytes")
        return int(b.value)

    def pileup_stage_bytes(self):
        b = C.c_int64()
        self._chk(self.lib.lcr_pileup_stage_bytes(self.h, C.byref(b)), "lcr_pileup_stage_bytes")
        return int(b.value)

    def pileup_records(self):
        """(items, records) of the last pileup: counting CIGAR ops, and the tile records K0 cut them into."""
        items, recs = C.c_int64(), C.c_int64()
        self._chk(self.lib.lcr_pileup_records(self.h, C.byref(items), C.byref(recs)), "lcr_pileup_records")
        return int(items.value), int(recs.value)


def host_register(*arrays):
    """Page-lock the memory of numpy arrays (lcr_host_register) so that lcr_load_batch_async copies them without staging;
    returns the list to hand to host_unregister."""
    lib = _lib.load()
    done = []
    for a in arrays:
        if a is None or a.nbytes == 0:
            continue
        if lib.lcr_host_register(C.c_void_p(a.ctypes.data), a.nbytes) != 0:
            host_unregister(done)
            raise LcrError("lcr_host_register failed")
        done.append(a)
    return done


def host_unregister(arrays):
    lib = _lib.load()
    for a in arrays:
        lib.lcr_host_unregister(C.c_void_p(a.ctypes.data))

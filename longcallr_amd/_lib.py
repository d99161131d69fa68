"""ctypes loader of liblcr.so (the HIP product library).  Fails loudly: there is no CPU fallback."""
import ctypes as C
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("LCR_LIB") or os.path.join(_HERE, "liblcr.so")   # LCR_LIB: developer hook (A/B timing of two builds)

# every symbol include/lcr.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "lcr_params_preset", "lcr_ctx_create", "lcr_ctx_destroy", "lcr_last_error", "lcr_ctx_set_stream",
    "lcr_ctx_sync", "lcr_ctx_set_lock_dir", "lcr_ctx_set_async_phase", "lcr_debug_set", "lcr_load_batch", "lcr_load_batch_async", "lcr_bind_batch",
    "lcr_host_alloc", "lcr_host_free", "lcr_host_register", "lcr_host_unregister", "lcr_pileup", "lcr_get_columns", "lcr_candidates",
    "lcr_get_candidates", "lcr_get_candidates_device", "lcr_fragments", "lcr_get_fragmat", "lcr_phase", "lcr_get_phase_result", "lcr_get_read_records_device", "lcr_collect_phase", "lcr_get_ld_blocks", "lcr_get_tie_census",
    "lcr_enable_timing", "lcr_kernel_ms", "lcr_pileup_bytes", "lcr_pileup_stage_bytes", "lcr_pileup_records", "lcr_discover_regions", "lcr_discover_regions_truncated", "lcr_version", "lcr_release_cached_memory", "lcr_set_cache_limits",
    "lcr_bam_open", "lcr_bam_open_keep", "lcr_bam_close", "lcr_bam_last_error", "lcr_bam_refs", "lcr_bam_n_records", "lcr_bam_resident", "lcr_bam_spans", "lcr_bam_batch", "lcr_bam_write_phased", "lcr_bam_write_reads",
    "lcr_set_downsample", "lcr_set_downsample_rows", "lcr_get_downsample",
    "lcr_junctions", "lcr_get_junctions", "lcr_ase", "lcr_get_ase", "lcr_vcf_contig_alleles",
    "lcr_assign_genes", "lcr_get_read_genes", "lcr_ase_genes", "lcr_get_ase_genes",
    "lcr_junctions_genes", "lcr_get_junctions_genes", "lcr_asj_genes", "lcr_get_asj_genes",
    "lcr_load_batch_packed", "lcr_load_batch_packed_async", "lcr_unpack_bases", "lcr_unpack_ms", "lcr_bam_batch_packed",
    "lcr_set_exon_mask", "lcr_exon_mask_ms", "lcr_import_candidates", "lcr_vcf_open", "lcr_vcf_close", "lcr_vcf_last_error", "lcr_vcf_contigs", "lcr_vcf_contig",
    "lcr_haplotag", "lcr_get_haplotag_sites", "lcr_haplotag_ms", "lcr_vcf_contig_phase_sets",
    "lcr_site_counts", "lcr_get_site_counts", "lcr_site_counts_ms",
    "lcr_hap_coverage", "lcr_get_hap_coverage", "lcr_hap_coverage_ms",
    "lcr_somatic", "lcr_get_somatic", "lcr_somatic_ms",
    "lcr_isoforms", "lcr_get_isoforms", "lcr_isoforms_ms",
    "lcr_transcript_ends", "lcr_get_transcript_ends", "lcr_transcript_ends_ms",
    "lcr_intron_retention", "lcr_get_intron_retention", "lcr_intron_retention_ms",
    "lcr_indels", "lcr_get_indels", "lcr_indels_ms",
    "lcr_site_pairs", "lcr_get_site_pairs", "lcr_site_pairs_ms",
]

_lib = None


class LcrError(RuntimeError):
    pass


def load():
    """Load liblcr.so.  Raises if the HIP extension has not been built (python -m longcallr_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise LcrError("liblcr.so is missing: build it with `python -m longcallr_amd.build` "
                       "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7; importing torch first
    # makes liblcr.so (NEEDED libamdhip64.so.7) bind to that already-loaded runtime instead of a second
    # copy from /opt/rocm, which could not see the GPU ("No HIP GPUs are available").
    try:
        import torch  # noqa: F401
    except Exception:  # torch is plumbing only; liblcr works without it
        pass
    l = C.CDLL(SO_PATH)
    vp, i32 = C.c_void_p, C.c_int
    l.lcr_version.restype = C.c_char_p
    l.lcr_last_error.restype = C.c_char_p
    l.lcr_last_error.argtypes = [vp]
    l.lcr_params_preset.argtypes = [i32, C.POINTER(_abi.LcrParams)]
    l.lcr_ctx_create.argtypes = [i32, C.POINTER(vp)]
    l.lcr_ctx_destroy.argtypes = [vp]
    l.lcr_ctx_destroy.restype = None
    l.lcr_ctx_set_stream.argtypes = [vp, vp]
    l.lcr_ctx_sync.argtypes = [vp]
    l.lcr_ctx_set_lock_dir.argtypes = [vp, C.c_char_p]
    l.lcr_ctx_set_async_phase.argtypes = [vp, C.c_int32]
    l.lcr_debug_set.argtypes = [vp, C.c_char_p, C.c_int64]
    l.lcr_load_batch.argtypes = [vp, C.POINTER(_abi.LcrReads), C.POINTER(_abi.LcrRegions)]
    l.lcr_load_batch_async.argtypes = [vp, C.POINTER(_abi.LcrReads), C.POINTER(_abi.LcrRegions), C.c_int32]
    l.lcr_bind_batch.argtypes = [vp, C.c_int32]
    l.lcr_load_batch_packed.argtypes = [vp, C.POINTER(_abi.LcrReadsPacked), C.POINTER(_abi.LcrRegions)]
    l.lcr_load_batch_packed_async.argtypes = [vp, C.POINTER(_abi.LcrReadsPacked), C.POINTER(_abi.LcrRegions), C.c_int32]
    l.lcr_unpack_bases.argtypes = [vp, C.c_int32, vp, vp, vp, vp, C.c_int64, vp, C.c_int64]
    l.lcr_unpack_ms.argtypes = [vp, C.POINTER(C.c_float)]
    l.lcr_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    l.lcr_host_free.argtypes = [vp]
    l.lcr_host_free.restype = None
    l.lcr_host_register.argtypes = [vp, C.c_size_t]
    l.lcr_host_unregister.argtypes = [vp]
    for f in ("lcr_pileup", "lcr_candidates", "lcr_fragments", "lcr_phase"):
        getattr(l, f).argtypes = [vp, C.POINTER(_abi.LcrParams)]
    l.lcr_get_columns.argtypes = [vp, C.POINTER(_abi.LcrColumns)]
    l.lcr_get_candidates.argtypes = [vp, C.POINTER(_abi.LcrCandidateList)]
    l.lcr_get_candidates_device.argtypes = [vp, C.POINTER(vp), C.POINTER(i32)]
    l.lcr_get_read_records_device.argtypes = [vp, C.POINTER(vp), C.POINTER(i32)]
    l.lcr_get_fragmat.argtypes = [vp, C.POINTER(_abi.LcrFragmat)]
    l.lcr_get_phase_result.argtypes = [vp, C.POINTER(_abi.LcrPhaseResult)]
    l.lcr_collect_phase.argtypes = [vp, C.POINTER(_abi.LcrPhaseCollected)]
    l.lcr_release_cached_memory.argtypes = []
    l.lcr_set_cache_limits.argtypes = [C.c_int64, C.c_int64]
    l.lcr_get_tie_census.argtypes = [vp, C.POINTER(C.c_uint64)]
    l.lcr_get_ld_blocks.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_int32))]
    l.lcr_discover_regions.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_int64, C.POINTER(_abi.LcrRegionList)]
    l.lcr_discover_regions_truncated.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_int64, C.c_int32, C.c_uint32, C.POINTER(_abi.LcrRegionList),
                                                 C.POINTER(C.c_int64)]
    l.lcr_enable_timing.argtypes = [vp, i32]
    l.lcr_kernel_ms.argtypes = [vp, i32, C.POINTER(C.c_float)]
    l.lcr_pileup_bytes.argtypes = [vp, C.POINTER(C.c_int64)]
    l.lcr_pileup_stage_bytes.argtypes = [vp, C.POINTER(C.c_int64)]
    l.lcr_pileup_records.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    flt = C.POINTER(_abi.LcrReadFilter)
    l.lcr_bam_open.argtypes = [C.c_char_p, C.c_int32, C.POINTER(vp)]
    l.lcr_bam_open_keep.argtypes = [C.c_char_p, C.c_int32, C.c_int64, C.POINTER(vp)]
    l.lcr_bam_close.argtypes = [vp]
    l.lcr_bam_close.restype = None
    l.lcr_bam_last_error.argtypes = [vp]
    l.lcr_bam_last_error.restype = C.c_char_p
    l.lcr_bam_refs.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.POINTER(C.c_int64))]
    l.lcr_bam_n_records.argtypes = [vp, C.POINTER(C.c_int64)]
    l.lcr_bam_resident.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    l.lcr_bam_spans.argtypes = [vp, C.c_int32, flt, C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_int32))]
    l.lcr_bam_batch.argtypes = [vp, C.c_int32, flt, C.c_int32, vp, vp, C.POINTER(_abi.LcrReads), C.POINTER(C.POINTER(C.c_int32)),
                                C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_char_p)]
    l.lcr_bam_batch_packed.argtypes = [vp, C.c_int32, flt, C.c_int32, vp, vp, C.POINTER(_abi.LcrReadsPacked), C.POINTER(C.POINTER(C.c_int32)),
                                       C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_char_p)]
    l.lcr_bam_write_phased.argtypes = [vp, C.c_char_p, C.c_int32, vp, vp, vp, C.c_int64, vp, C.c_char_p, vp, vp, C.c_int32, C.c_int32]
    l.lcr_bam_write_reads.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.POINTER(_abi.LcrReads), C.c_int32, C.c_int32]
    l.lcr_import_candidates.argtypes = [vp, C.POINTER(_abi.LcrParams), C.c_int32, C.c_int32, vp, vp, vp]
    l.lcr_set_exon_mask.argtypes = [vp, C.c_int32, vp, vp, vp]
    l.lcr_exon_mask_ms.argtypes = [vp, C.POINTER(C.c_float)]
    l.lcr_set_downsample.argtypes = [vp, C.c_uint32, C.c_uint64]
    l.lcr_set_downsample_rows.argtypes = [vp, C.c_int32, C.c_int32, vp]
    l.lcr_get_downsample.argtypes = [vp, C.POINTER(_abi.LcrDownsampleInfo)]
    l.lcr_junctions.argtypes = [vp, C.POINTER(_abi.LcrJunctionParams)]
    l.lcr_get_junctions.argtypes = [vp, C.POINTER(_abi.LcrJunctionList)]
    l.lcr_vcf_open.argtypes = [C.c_char_p, C.c_int32, C.POINTER(vp)]
    l.lcr_vcf_close.argtypes = [vp]
    l.lcr_vcf_close.restype = None
    l.lcr_vcf_last_error.argtypes = [vp]
    l.lcr_vcf_last_error.restype = C.c_char_p
    l.lcr_vcf_contigs.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_char_p))]
    l.lcr_vcf_contig.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    l.lcr_ase.argtypes = [vp, C.POINTER(_abi.LcrAseParams), C.c_int32, C.c_int32, vp, vp, vp]
    l.lcr_get_ase.argtypes = [vp, C.POINTER(_abi.LcrAseList)]
    l.lcr_assign_genes.argtypes = [vp, C.c_int32, C.POINTER(_abi.LcrGeneAnnotation)]
    l.lcr_get_read_genes.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    l.lcr_ase_genes.argtypes = [vp, C.POINTER(_abi.LcrAseParams), C.c_int32, C.c_int32, vp, vp, vp]
    l.lcr_get_ase_genes.argtypes = [vp, C.POINTER(_abi.LcrAseGeneList)]
    l.lcr_junctions_genes.argtypes = [vp, C.POINTER(_abi.LcrJunctionParams), C.c_int32, C.POINTER(_abi.LcrGeneAnnotation)]
    l.lcr_get_junctions_genes.argtypes = [vp, C.POINTER(_abi.LcrJunctionGeneList)]
    l.lcr_asj_genes.argtypes = [vp, C.POINTER(_abi.LcrAsjParams), C.c_int32, C.POINTER(_abi.LcrGeneAnnotation)]
    l.lcr_get_asj_genes.argtypes = [vp, C.POINTER(_abi.LcrAsjGeneList)]
    l.lcr_vcf_contig_alleles.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    l.lcr_vcf_contig_phase_sets.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(vp)]
    l.lcr_haplotag.argtypes = [vp, C.POINTER(_abi.LcrParams), C.c_int32, C.c_int32, vp, vp, vp, vp]
    l.lcr_get_haplotag_sites.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(vp)]
    l.lcr_haplotag_ms.argtypes = [vp, C.POINTER(C.c_float)]
    l.lcr_site_counts.argtypes = [vp, C.POINTER(_abi.LcrSiteCountParams)]
    l.lcr_get_site_counts.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(vp)]
    l.lcr_site_counts_ms.argtypes = [vp, C.POINTER(C.c_float)]
    l.lcr_hap_coverage.argtypes = [vp]
    l.lcr_get_hap_coverage.argtypes = [vp, C.POINTER(_abi.LcrHapCovList)]
    l.lcr_hap_coverage_ms.argtypes = [vp, C.POINTER(C.c_float)]
    l.lcr_somatic.argtypes = [vp, C.POINTER(_abi.LcrSomaticParams)]
    l.lcr_get_somatic.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(vp)]
    l.lcr_somatic_ms.argtypes = [vp, C.POINTER(C.c_float)]
    l.lcr_isoforms.argtypes = [vp, C.POINTER(_abi.LcrIsoformParams)]
    l.lcr_get_isoforms.argtypes = [vp, C.POINTER(_abi.LcrIsoformList)]
    l.lcr_isoforms_ms.argtypes = [vp, C.POINTER(C.c_float)]
    l.lcr_transcript_ends.argtypes = [vp, C.POINTER(_abi.LcrEndParams)]
    l.lcr_get_transcript_ends.argtypes = [vp, C.POINTER(_abi.LcrEndList)]
    l.lcr_transcript_ends_ms.argtypes = [vp, C.POINTER(C.c_float)]
    l.lcr_intron_retention.argtypes = [vp, C.POINTER(_abi.LcrRetentionParams)]
    l.lcr_get_intron_retention.argtypes = [vp, C.POINTER(_abi.LcrRetentionList)]
    l.lcr_intron_retention_ms.argtypes = [vp, C.POINTER(C.c_float)]
    l.lcr_indels.argtypes = [vp, C.POINTER(_abi.LcrIndelParams)]
    l.lcr_get_indels.argtypes = [vp, C.POINTER(_abi.LcrIndelList)]
    l.lcr_indels_ms.argtypes = [vp, C.POINTER(C.c_float)]
    l.lcr_site_pairs.argtypes = [vp, C.POINTER(_abi.LcrSitePairParams)]
    l.lcr_get_site_pairs.argtypes = [vp, C.POINTER(_abi.LcrSitePairList)]
    l.lcr_site_pairs_ms.argtypes = [vp, C.POINTER(C.c_float)]
    _lib = l
    return l

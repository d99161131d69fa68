"""ctypes mirror of include/lcr.h (the C ABI of liblcr).

Only plain-data structures live here; no compute.  Both the product loader (``_lib.py``) and the
test-only oracle loader (``oracle/orc.py``) build their argument structs from these definitions.
"""
import ctypes as C

import numpy as np

LCR_PLATFORM_HIFI, LCR_PLATFORM_ONT = 0, 1
LCR_MEM_HOST, LCR_MEM_DEVICE = 0, 1

(PL_A, PL_C, PL_G, PL_T, PL_N, PL_D, PL_NI, PL_FWD_A, PL_FWD_C, PL_FWD_G, PL_FWD_T, PL_TS_FWD,
 PL_TS_REV, NPLANES) = range(14)
PLANE_NAMES = ["a", "c", "g", "t", "n", "d", "ni", "fwd_a", "fwd_c", "fwd_g", "fwd_t", "ts_fwd", "ts_rev"]

F_RNA_EDIT, F_DENSE, F_HET, F_FOR_PHASING, F_HOM, F_SINGLE, F_NON_SELECTED, F_CAND_SOMATIC = (
    1, 2, 4, 8, 16, 32, 64, 128)

(K_SPANS, K_PILEUP, K_CAND_FILTER, K_CAND_HIST, K_CAND_GT, K_FRAG_COUNT, K_FRAG_FILL, K_PHASE, K_BIND, K_BIND_TABLE,
 K_CAND_IMPORT, K_JUNCTIONS, K_ASE, NKERNELS) = range(14)
K_GENES, K_ASE_GENES, NTIMERS = NKERNELS, NKERNELS + 1, NKERNELS + 2   # include/lcr.h: the per-gene calls' slots follow LCR_NKERNELS


class LcrReads(C.Structure):
    _fields_ = [
        ("mem", C.c_int32), ("n_reads", C.c_int32), ("n_bases", C.c_int64), ("n_cigar", C.c_int64),
        ("pos", C.c_void_p), ("seq_len", C.c_void_p), ("lead_clip", C.c_void_p),
        ("trail_clip", C.c_void_p), ("flags", C.c_void_p), ("seq_off", C.c_void_p),
        ("cig_off", C.c_void_p), ("n_cig", C.c_void_p), ("bases", C.c_void_p),
        ("quals", C.c_void_p), ("cigar", C.c_void_p),
    ]


class LcrReadsPacked(C.Structure):   # include/lcr.h: lcr_reads_packed (lcr_reads with BAM nibbles in place of the bases)
    _fields_ = [
        ("mem", C.c_int32), ("n_reads", C.c_int32), ("n_bases", C.c_int64), ("n_cigar", C.c_int64), ("n_pack", C.c_int64),
        ("pos", C.c_void_p), ("seq_len", C.c_void_p), ("lead_clip", C.c_void_p),
        ("trail_clip", C.c_void_p), ("flags", C.c_void_p), ("seq_off", C.c_void_p),
        ("cig_off", C.c_void_p), ("n_cig", C.c_void_p), ("pack_off", C.c_void_p), ("seq4", C.c_void_p),
        ("quals", C.c_void_p), ("cigar", C.c_void_p),
    ]


class LcrReadFilter(C.Structure):   # include/lcr.h lcr_read_filter (util.rs:652-668)
    _fields_ = [("min_mapq", C.c_uint8), ("min_read_length", C.c_int32), ("divergence", C.c_float)]


class LcrRegions(C.Structure):
    _fields_ = [
        ("mem", C.c_int32), ("n_regions", C.c_int32), ("start0", C.c_void_p), ("len", C.c_void_p),
        ("col_off", C.c_void_p), ("read_begin", C.c_void_p), ("ref", C.c_void_p),
    ]


class LcrParams(C.Structure):
    _fields_ = [
        ("platform", C.c_int32), ("min_baseq", C.c_uint32), ("dist_to_end", C.c_uint32),
        ("polya_len", C.c_uint32), ("min_depth", C.c_uint32), ("max_depth", C.c_uint32),
        ("min_qual", C.c_uint32), ("dense_win", C.c_uint32), ("min_dense_cnt", C.c_uint32),
        ("low_cnt_cut", C.c_uint32), ("min_linkers", C.c_uint32), ("max_enum_snps", C.c_uint32),
        ("ld_weight_threshold", C.c_uint32), ("use_strand_bias", C.c_int32),
        ("min_af", C.c_float), ("min_af_intron", C.c_float), ("low_frac_cut", C.c_float),
        ("min_phase_score", C.c_float), ("read_assign_cutoff", C.c_double), ("seed", C.c_uint64),
    ]


class LcrColumns(C.Structure):
    _fields_ = [("n_cols", C.c_int64), ("planes", C.c_void_p)]


CAND_DTYPE = np.dtype([
    ("pos", "<i8"), ("region", "<i4"), ("ref_base", "u1"), ("allele1", "u1"), ("allele2", "u1"),
    ("n_alt", "u1"), ("cnt1", "<u4"), ("cnt2", "<u4"), ("depth", "<u4"), ("af1", "<f4"),
    ("af2", "<f4"), ("variant_type", "<i4"), ("genotype", "<i4"), ("haplotype", "<i4"),
    ("flags", "<u4"), ("phase_set", "<u4"), ("loglik", "<f8", 3),
    ("gt_prob", "<f8", 3), ("qual", "<f8"), ("gq", "<f8"), ("phase_score", "<f8"),
], align=True)
assert CAND_DTYPE.itemsize == 128, CAND_DTYPE.itemsize


class LcrCandidateList(C.Structure):
    _fields_ = [("n_cand", C.c_int32), ("n_regions", C.c_int32), ("cand", C.c_void_p),
                ("region_off", C.c_void_p)]


class LcrFragmat(C.Structure):
    _fields_ = [
        ("n_rows", C.c_int32), ("nnz", C.c_int64), ("n_regions", C.c_int32),
        ("row_region_off", C.c_void_p), ("row_ptr", C.c_void_p), ("row_read", C.c_void_p),
        ("col", C.c_void_p), ("val", C.c_void_p), ("row_for_phasing", C.c_void_p),
        ("row_links", C.c_void_p),
    ]


class LcrRegionList(C.Structure):
    _fields_ = [("n_regions", C.c_int32), ("start0", C.c_void_p), ("len", C.c_void_p), ("max_cov", C.c_void_p)]


class LcrPhaseResult(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_regions", C.c_int32), ("haplotag", C.c_void_p),
                ("assignment", C.c_void_p), ("phase_set", C.c_void_p), ("objective", C.c_void_p)]


class LcrPhaseCollected(C.Structure):   # include/lcr.h: lcr_phase_collected
    _fields_ = [("n_regions", C.c_int32), ("n_rows", C.c_int32), ("n_cand", C.c_int32), ("pad_", C.c_int32),
                ("cand", C.c_void_p), ("cand_region_off", C.c_void_p), ("row_region_off", C.c_void_p),
                ("haplotag", C.c_void_p), ("assignment", C.c_void_p), ("phase_set", C.c_void_p), ("objective", C.c_void_p),
                ("dev_cand", C.c_void_p), ("dev_read_rec", C.c_void_p)]


class LcrDownsampleInfo(C.Structure):   # include/lcr.h: lcr_downsample_info
    _fields_ = [("n_regions", C.c_int32), ("n_rows", C.c_int32), ("region_applied", C.c_void_p), ("sampled", C.c_void_p),
                ("dev_sampled", C.c_void_p)]


class LcrJunctionParams(C.Structure):   # include/lcr.h: lcr_junction_params (longcallR-asj.py defaults: 10, 2)
    _fields_ = [("min_count", C.c_uint32), ("min_junctions", C.c_uint32)]


# lcr_junction (include/lcr.h): one kept junction of a region with its haplotype x presence table
JUNC_DTYPE = np.dtype([("region", "<i4"), ("motif", "u1"), ("pad_", "u1", 3), ("start0", "<i8"), ("len", "<i4"), ("n_reads", "<u4"),
                       ("phase_set", "<u4"), ("n_phase_sets", "<u4"), ("h1_absent", "<u4"), ("h1_present", "<u4"),
                       ("h2_absent", "<u4"), ("h2_present", "<u4")], align=True)
assert JUNC_DTYPE.itemsize == 48, JUNC_DTYPE.itemsize


class LcrJunctionList(C.Structure):   # include/lcr.h: lcr_junction_list
    _fields_ = [("n_regions", C.c_int32), ("n_junctions", C.c_int32), ("junc", C.c_void_p), ("junc_region_off", C.c_void_p),
                ("dev_junc", C.c_void_p)]


class LcrAseParams(C.Structure):   # include/lcr.h: lcr_ase_params (13 = pysam's pileup default; the VCF writer's min_phase_score)
    _fields_ = [("min_baseq", C.c_uint32), ("min_phase_score", C.c_float)]


# lcr_ase_region (include/lcr.h): one region's haplotype counts and parent-of-origin votes
ASE_DTYPE = np.dtype([("region", "<i4"), ("phase_set", "<u4"), ("n_phase_sets", "<u4"), ("h1", "<u4"), ("h2", "<u4"), ("n_sites", "<u4"),
                      ("h1_pat", "<u4"), ("h1_mat", "<u4"), ("h2_pat", "<u4"), ("h2_mat", "<u4")], align=True)
assert ASE_DTYPE.itemsize == 40, ASE_DTYPE.itemsize


class LcrAseList(C.Structure):   # include/lcr.h: lcr_ase_list
    _fields_ = [("n_regions", C.c_int32), ("rec", C.c_void_p), ("dev_rec", C.c_void_p)]


# lcr_haplotag_site (include/lcr.h): one candidate's evidence under the caller's phase (lcr_haplotag), zeros when it is not usable
HAPSITE_DTYPE = np.dtype([("match_fx", "<i8"), ("total_fx", "<i8"), ("n_h1", "<u4"), ("n_h2", "<u4"), ("n_h1_match", "<u4"),
                          ("n_h2_match", "<u4")], align=True)
assert HAPSITE_DTYPE.itemsize == 32, HAPSITE_DTYPE.itemsize


class LcrSiteCountParams(C.Structure):   # include/lcr.h: lcr_site_count_params (13 = lcr_ase's default)
    _fields_ = [("min_baseq", C.c_uint32)]


# lcr_site_count (include/lcr.h): one candidate's allele x haplotype counts; n[k][b]: k = 0 other rows, 1 / 2 the site's set by haplotype, b = ACGT
SITE_COUNT_DTYPE = np.dtype([("phase_set", "<u4"), ("n_phase_sets", "<u4"), ("n_entries", "<u4"), ("n_lowq", "<u4"), ("n", "<u4", (3, 4))], align=True)
assert SITE_COUNT_DTYPE.itemsize == 64, SITE_COUNT_DTYPE.itemsize


PAIRS_ALL, PAIRS_PHASED, PAIRS_MAX_PARTNERS = 0, 1, 8   # include/lcr.h: LCR_PAIRS_*


class LcrSitePairParams(C.Structure):   # include/lcr.h: lcr_site_pair_params (defaults ALL, 2, 2, 13)
    _fields_ = [("mode", C.c_uint32), ("max_partners", C.c_uint32), ("max_dist", C.c_uint32), ("min_baseq", C.c_uint32)]


# lcr_site_pair (include/lcr.h): the joint rows of candidates a < b; n[x][y]: x / y = the base code ACGT at a / b
SITE_PAIR_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("n_rows", "<u4"), ("n_lowq", "<u4"), ("n", "<u4", (4, 4))], align=True)
assert SITE_PAIR_DTYPE.itemsize == 80, SITE_PAIR_DTYPE.itemsize


class LcrSitePairList(C.Structure):   # include/lcr.h: lcr_site_pair_list
    _fields_ = [("n_cand", C.c_int32), ("n_eligible", C.c_int32), ("n_pairs", C.c_int32), ("pad_", C.c_int32),
                ("pair", C.c_void_p), ("pair_off", C.c_void_p), ("dev_pair", C.c_void_p), ("dev_pair_off", C.c_void_p)]


# lcr_hap_cov_segment / lcr_hap_cov_region (include/lcr.h): a run of window columns with one depth triple n[k] (k = 0 unassigned, 1 / 2 the
# haplotypes); a region's reads, maxima and covered bases per class
HAP_COV_SEGMENT_DTYPE = np.dtype([("region", "<i4"), ("len", "<i4"), ("start0", "<i8"), ("n", "<u4", (3,)), ("pad_", "<u4")], align=True)
assert HAP_COV_SEGMENT_DTYPE.itemsize == 32, HAP_COV_SEGMENT_DTYPE.itemsize
HAP_COV_REGION_DTYPE = np.dtype([("region", "<i4"), ("n_reads", "<u4", (3,)), ("max_depth", "<u4", (3,)), ("pad_", "<u4"), ("bases", "<u8", (3,))], align=True)
assert HAP_COV_REGION_DTYPE.itemsize == 56, HAP_COV_REGION_DTYPE.itemsize


class LcrSomaticParams(C.Structure):   # include/lcr.h: lcr_somatic_params (the reference's 0.3, 5e-6, 1 / 2000; no threshold)
    _fields_ = [("purity", C.c_double), ("som_rate", C.c_double), ("het_rate", C.c_double), ("min_baseq", C.c_uint32), ("pad_", C.c_uint32)]


# lcr_somatic_site (include/lcr.h): one candidate's counts n[hap - 1][0 ref, 1 alt], classes per haplotype (0 ref, 1 het, 2 somatic), the
# call (0 none, 1 / 2 the haplotype with the somatic allele), the status, and L[hap - 1][ref, het, som] = log10(likelihood x prior) x 2^40
SOMATIC_SITE_DTYPE = np.dtype([("phase_set", "<u4"), ("n", "<u4", (2, 2)), ("n_other", "<u4"), ("n_lowq", "<u4"), ("cls", "u1", (2,)),
                               ("call", "u1"), ("status", "u1"), ("L", "<i8", (2, 3))], align=True)
assert SOMATIC_SITE_DTYPE.itemsize == 80, SOMATIC_SITE_DTYPE.itemsize


class LcrHapCovList(C.Structure):   # include/lcr.h: lcr_hap_cov_list
    _fields_ = [("n_regions", C.c_int32), ("n_segments", C.c_int32), ("seg", C.c_void_p), ("seg_region_off", C.c_void_p),
                ("reg", C.c_void_p), ("dev_seg", C.c_void_p), ("dev_reg", C.c_void_p)]


class LcrIsoformParams(C.Structure):   # include/lcr.h: lcr_isoform_params (defaults 10, 1)
    _fields_ = [("min_count", C.c_uint32), ("min_junctions", C.c_uint32)]


# lcr_isoform (include/lcr.h): one kept intron chain of a region -- its extent [start0, end0), its keys chain[chain_first .. + n_junc) --
# with its haplotype x presence table
ISOFORM_DTYPE = np.dtype([("region", "<i4"), ("n_junc", "<i4"), ("start0", "<i8"), ("end0", "<i8"), ("chain_first", "<i4"), ("n_reads", "<u4"),
                          ("n_h1", "<u4"), ("n_h2", "<u4"), ("phase_set", "<u4"), ("n_phase_sets", "<u4"), ("h1_absent", "<u4"),
                          ("h1_present", "<u4"), ("h2_absent", "<u4"), ("h2_present", "<u4")], align=True)
assert ISOFORM_DTYPE.itemsize == 64, ISOFORM_DTYPE.itemsize


class LcrIsoformList(C.Structure):   # include/lcr.h: lcr_isoform_list
    _fields_ = [("n_regions", C.c_int32), ("n_isoforms", C.c_int32), ("n_chain", C.c_int32), ("n_rows", C.c_int32),
                ("iso", C.c_void_p), ("iso_region_off", C.c_void_p), ("chain", C.c_void_p), ("row_isoform", C.c_void_p),
                ("dev_iso", C.c_void_p), ("dev_chain", C.c_void_p), ("dev_row_isoform", C.c_void_p)]


LCR_ENDS_STRAND_TS, LCR_ENDS_STRAND_READ = 0, 1   # include/lcr.h: lcr_end_params.strand_mode


class LcrEndParams(C.Structure):   # include/lcr.h: lcr_end_params (defaults 10, 10, LCR_ENDS_STRAND_TS)
    _fields_ = [("min_count", C.c_uint32), ("window", C.c_uint32), ("strand_mode", C.c_uint32), ("pad_", C.c_uint32)]


# lcr_end_site (include/lcr.h): one kept transcript-end site of a region -- the peak of a (strand, side) class of read ends, what was
# assigned to it -- with its haplotype x presence table
END_SITE_DTYPE = np.dtype([("region", "<i4"), ("strand", "u1"), ("side", "u1"), ("kind", "u1"), ("pad_", "u1"), ("peak0", "<i8"), ("min0", "<i4"),
                           ("max0", "<i4"), ("n_reads", "<u4"), ("n_h1", "<u4"), ("n_h2", "<u4"), ("n_peak", "<u4"), ("phase_set", "<u4"),
                           ("n_phase_sets", "<u4"), ("h1_absent", "<u4"), ("h1_present", "<u4"), ("h2_absent", "<u4"), ("h2_present", "<u4")],
                          align=True)
assert END_SITE_DTYPE.itemsize == 64, END_SITE_DTYPE.itemsize


class LcrEndList(C.Structure):   # include/lcr.h: lcr_end_list
    _fields_ = [("n_regions", C.c_int32), ("n_sites", C.c_int32), ("n_rows", C.c_int32), ("n_part", C.c_int32), ("n_assigned", C.c_int64),
                ("site", C.c_void_p), ("site_region_off", C.c_void_p), ("row_site", C.c_void_p), ("dev_site", C.c_void_p), ("dev_row_site", C.c_void_p)]


class LcrRetentionParams(C.Structure):   # include/lcr.h: lcr_retention_params (defaults 10, 10)
    _fields_ = [("min_count", C.c_uint32), ("anchor", C.c_uint32), ("pad_", C.c_uint32 * 2)]


# lcr_retained_intron (include/lcr.h): one kept intron of a region -- a junction that min_count tagged rows splice -- with the rows that
# splice it, retain it or do neither, and its haplotype x {spliced, retained} table
RETAINED_INTRON_DTYPE = np.dtype([("region", "<i4"), ("motif", "u1"), ("pad_", "u1", 3), ("start0", "<i8"), ("len", "<i4"), ("n_spliced", "<u4"),
                                  ("n_retained", "<u4"), ("n_other", "<u4"), ("phase_set", "<u4"), ("n_phase_sets", "<u4"), ("h1_spliced", "<u4"),
                                  ("h1_retained", "<u4"), ("h2_spliced", "<u4"), ("h2_retained", "<u4")], align=True)
assert RETAINED_INTRON_DTYPE.itemsize == 56, RETAINED_INTRON_DTYPE.itemsize


class LcrRetentionList(C.Structure):   # include/lcr.h: lcr_retention_list
    _fields_ = [("n_regions", C.c_int32), ("n_introns", C.c_int32), ("n_rows", C.c_int32), ("n_part", C.c_int32), ("n_retained_total", C.c_int64),
                ("intron", C.c_void_p), ("intron_region_off", C.c_void_p), ("row_retained", C.c_void_p), ("dev_intron", C.c_void_p),
                ("dev_row_retained", C.c_void_p)]


class LcrIndelParams(C.Structure):   # include/lcr.h: lcr_indel_params (defaults 10, 150, 5, 12, 50)
    _fields_ = [("min_count", C.c_uint32), ("min_permille", C.c_uint32), ("flank", C.c_uint32), ("max_ins", C.c_uint32), ("max_del", C.c_uint32),
                ("pad_", C.c_uint32 * 3)]


# lcr_indel (include/lcr.h): one kept small indel of a region in its left-shifted form, with the rows that hold it, lack it or do neither,
# and its haplotype x {present, absent} table
INDEL_DTYPE = np.dtype([("region", "<i4"), ("type", "u1"), ("hrun", "u1"), ("shift", "<u2"), ("start0", "<i8"), ("len", "<i4"), ("seq", "<u4"),
                        ("depth", "<u4"), ("n_present", "<u4"), ("n_absent", "<u4"), ("n_other", "<u4"), ("phase_set", "<u4"),
                        ("n_phase_sets", "<u4"), ("h1_present", "<u4"), ("h1_absent", "<u4"), ("h2_present", "<u4"), ("h2_absent", "<u4")], align=True)
assert INDEL_DTYPE.itemsize == 64, INDEL_DTYPE.itemsize


class LcrIndelList(C.Structure):   # include/lcr.h: lcr_indel_list
    _fields_ = [("n_regions", C.c_int32), ("n_indels", C.c_int32), ("n_rows", C.c_int32), ("n_part", C.c_int32), ("n_events", C.c_int64),
                ("n_present_total", C.c_int64), ("indel", C.c_void_p), ("indel_region_off", C.c_void_p), ("row_indels", C.c_void_p),
                ("dev_indel", C.c_void_p), ("dev_row_indels", C.c_void_p)]


class LcrGeneAnnotation(C.Structure):   # include/lcr.h: lcr_gene_annotation (one contig's genes, 0-based half-open)
    _fields_ = [("n_genes", C.c_int32), ("n_exons", C.c_int32), ("span_start0", C.c_void_p), ("span_end0", C.c_void_p),
                ("exon_off", C.c_void_p), ("exon_start0", C.c_void_p), ("exon_end0", C.c_void_p)]


# lcr_ase_gene (include/lcr.h): lcr_ase_region's fields for one (region, gene) pair, then the gene
AGENE_DTYPE = np.dtype([("region", "<i4"), ("phase_set", "<u4"), ("n_phase_sets", "<u4"), ("h1", "<u4"), ("h2", "<u4"), ("n_sites", "<u4"),
                        ("h1_pat", "<u4"), ("h1_mat", "<u4"), ("h2_pat", "<u4"), ("h2_mat", "<u4"), ("gene", "<i4"), ("pad_", "<u4")], align=True)
assert AGENE_DTYPE.itemsize == 48, AGENE_DTYPE.itemsize


class LcrAseGeneList(C.Structure):   # include/lcr.h: lcr_ase_gene_list
    _fields_ = [("n_regions", C.c_int32), ("n_pairs", C.c_int32), ("rec", C.c_void_p), ("pair_region_off", C.c_void_p), ("dev_rec", C.c_void_p)]


# lcr_junction_gene (include/lcr.h): lcr_junction's fields for one (region, gene) pair, then the gene
JUNC_GENE_DTYPE = np.dtype([("region", "<i4"), ("motif", "u1"), ("pad_", "u1", 3), ("start0", "<i8"), ("len", "<i4"), ("n_reads", "<u4"),
                            ("phase_set", "<u4"), ("n_phase_sets", "<u4"), ("h1_absent", "<u4"), ("h1_present", "<u4"),
                            ("h2_absent", "<u4"), ("h2_present", "<u4"), ("gene", "<i4"), ("pad2_", "<u4")], align=True)
assert JUNC_GENE_DTYPE.itemsize == 56, JUNC_GENE_DTYPE.itemsize


class LcrJunctionGeneList(C.Structure):   # include/lcr.h: lcr_junction_gene_list
    _fields_ = [("n_regions", C.c_int32), ("n_junctions", C.c_int32), ("junc", C.c_void_p), ("junc_region_off", C.c_void_p),
                ("dev_junc", C.c_void_p), ("kernel_ms", C.c_float)]


LCR_ASJ_EXONS, LCR_ASJ_DNA_FILTER, LCR_ASJ_COVERAGE = 1, 2, 4   # include/lcr.h: the flags of lcr_asj_params


class LcrAsjParams(C.Structure):   # include/lcr.h: lcr_asj_params
    _fields_ = [("min_count", C.c_uint32), ("min_junctions", C.c_uint32), ("flags", C.c_uint32), ("min_phase_score", C.c_float),
                ("n_dna", C.c_int32), ("pad_", C.c_int32), ("dna_pos0", C.c_void_p)]


# lcr_exon_gene (include/lcr.h): one kept interior exon block of a (region, gene) pair
EXON_GENE_DTYPE = np.dtype([("region", "<i4"), ("gene", "<i4"), ("start0", "<i8"), ("len", "<i4"), ("n_reads", "<u4")], align=True)
assert EXON_GENE_DTYPE.itemsize == 24, EXON_GENE_DTYPE.itemsize


class LcrAsjGeneList(C.Structure):   # include/lcr.h: lcr_asj_gene_list
    _fields_ = [("n_regions", C.c_int32), ("n_junctions", C.c_int32), ("junc", C.c_void_p), ("junc_region_off", C.c_void_p),
                ("dev_junc", C.c_void_p), ("n_exons", C.c_int32), ("n_genes", C.c_int32), ("exon", C.c_void_p), ("exon_region_off", C.c_void_p),
                ("dev_exon", C.c_void_p), ("gene_reads", C.c_void_p), ("kernel_ms", C.c_float)]


# presets: the code values of main.rs:272-396 (not the help text)
PRESETS = {
    "hifi-isoseq": dict(platform=LCR_PLATFORM_HIFI, min_depth=6, min_phase_score=11.0, min_af=0.15,
                        dist_to_end=40, use_strand_bias=1),
    "hifi-masseq": dict(platform=LCR_PLATFORM_HIFI, min_depth=6, min_phase_score=11.0, min_af=0.15,
                        dist_to_end=40, use_strand_bias=0),
    "ont-cdna": dict(platform=LCR_PLATFORM_ONT, min_depth=10, min_phase_score=13.0, min_af=0.20,
                     dist_to_end=20, use_strand_bias=1),
    "ont-drna": dict(platform=LCR_PLATFORM_ONT, min_depth=10, min_phase_score=13.0, min_af=0.20,
                     dist_to_end=20, use_strand_bias=0),
}
PRESET_IDS = {"hifi-isoseq": 0, "hifi-masseq": 1, "ont-cdna": 2, "ont-drna": 3}
# host-side read filters of the presets (main.rs: min_mapq, min_read_length, divergence)
READ_FILTER = dict(min_mapq=20, min_read_length=500, divergence=0.5)


def make_params(preset="hifi-masseq", seed=2025, **over):
    p = LcrParams()
    base = dict(min_baseq=10, polya_len=5, max_depth=50000, min_qual=2, dense_win=100,
                min_dense_cnt=5, low_cnt_cut=10, min_linkers=1, max_enum_snps=10,
                ld_weight_threshold=1, min_af_intron=0.0, low_frac_cut=0.05,
                read_assign_cutoff=0.0, seed=seed)
    base.update(PRESETS[preset])
    base.update(over)
    for k, v in base.items():
        setattr(p, k, v)
    return p


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# lcr_read_record (include/lcr.h): per-row results in HBM for the multi-GPU gather
READ_REC_DTYPE = np.dtype([("row", "<i4"), ("haplotag", "i1"), ("assignment", "u1"), ("pad_", "<u2"), ("phase_set", "<u4")])
assert READ_REC_DTYPE.itemsize == 12


class ReadBatch:
    """Host SoA of decoded reads + the regions that own them (numpy, C-contiguous)."""

    FIELDS = ["pos", "seq_len", "lead_clip", "trail_clip", "flags", "seq_off", "cig_off", "n_cig",
              "bases", "quals", "cigar"]
    DTYPES = dict(pos=np.int32, seq_len=np.int32, lead_clip=np.int32, trail_clip=np.int32,
                  flags=np.uint8, seq_off=np.uint64, cig_off=np.uint64, n_cig=np.uint32,
                  bases=np.uint8, quals=np.uint8, cigar=np.uint32)

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, np.ascontiguousarray(kw[f], dtype=self.DTYPES[f]))
        self.start0 = np.ascontiguousarray(kw["start0"], dtype=np.int64)
        self.len = np.ascontiguousarray(kw["len"], dtype=np.int32)
        self.read_begin = np.ascontiguousarray(kw["read_begin"], dtype=np.int32)
        self.ref = np.ascontiguousarray(kw["ref"], dtype=np.uint8)
        self.col_off = np.zeros(len(self.len) + 1, dtype=np.int64)
        np.cumsum(self.len, out=self.col_off[1:])
        self.names = kw.get("names")
        assert self.ref.size == self.col_off[-1]
        assert self.read_begin[-1] == self.pos.size

    @property
    def n_reads(self):
        return int(self.pos.size)

    @property
    def n_regions(self):
        return int(self.len.size)

    def c_reads(self):
        r = LcrReads()
        r.mem = LCR_MEM_HOST
        r.n_reads = self.n_reads
        r.n_bases = int(self.bases.size)
        r.n_cigar = int(self.cigar.size)
        for f in self.FIELDS:
            setattr(r, f, _ptr(getattr(self, f)))
        return r

    def c_regions(self):
        g = LcrRegions()
        g.mem = LCR_MEM_HOST
        g.n_regions = self.n_regions
        g.start0, g.len, g.col_off = _ptr(self.start0), _ptr(self.len), _ptr(self.col_off)
        g.read_begin, g.ref = _ptr(self.read_begin), _ptr(self.ref)
        return g

    def pileup_algorithmic_bytes(self):
        """2B + 4C + 32R + (4*NPLANES + 1)*L  (DESIGN.md, K1)."""
        return (2 * int(self.bases.size) + 4 * int(self.cigar.size) + 32 * self.n_reads
                + (4 * NPLANES + 1) * int(self.col_off[-1]))

    def pack(self):
        """The same batch with the bases as BAM nibbles (PackedReadBatch): pack_off back to back, (seq_len + 1) // 2 bytes per read, the
        low nibble behind an odd-length read 0.  A base outside "=ACMGRSVTWYHKDBN" is a ValueError.  The other arrays are shared, not
        copied.  (Tests and tools: the product path never expands the nibbles, NativeBam.batch(packed=True).)"""
        ln = self.seq_len.astype(np.int64)
        if ln.size and ln.min() < 0:
            raise ValueError("negative seq_len")
        pack_off = np.zeros(ln.size + 1, dtype=np.int64)
        np.cumsum((ln + 1) // 2, out=pack_off[1:])
        src, dst = _base_index(ln, self.seq_off, 2 * pack_off[:-1])
        code = _NT16_CODE[self.bases[src]]
        if code.size and code.max() > 15:
            bad = int(np.flatnonzero(code > 15)[0])
            raise ValueError("base %r (byte %d of bases) is not one of =ACMGRSVTWYHKDBN" % (chr(int(self.bases[src[bad]])), int(src[bad])))
        nib = np.zeros(2 * int(pack_off[-1]), dtype=np.uint8)
        nib[dst] = code
        kw = {f: getattr(self, f) for f in PackedReadBatch.FIELDS if f not in ("seq4", "pack_off")}
        out = PackedReadBatch(seq4=(nib[0::2] << 4) | nib[1::2], pack_off=pack_off[:-1].astype(np.uint64), start0=self.start0, len=self.len,
                              read_begin=self.read_begin, ref=self.ref, names=self.names, **kw)
        for f in ("name_off", "name_blob"):
            if hasattr(self, f):
                setattr(out, f, getattr(self, f))
        return out


_NT16 = np.frombuffer(b"=ACMGRSVTWYHKDBN", dtype=np.uint8)
_NT16_CODE = np.full(256, 255, dtype=np.uint8)
_NT16_CODE[_NT16] = np.arange(16, dtype=np.uint8)


def _base_index(ln, seq_off, nib_off):
    """for every base of every read, in read order: (its index in bases, its index in the nibble stream)"""
    total = int(ln.sum())
    first = np.zeros(ln.size, dtype=np.int64)
    if ln.size:
        np.cumsum(ln[:-1], out=first[1:])
    j = np.arange(total, dtype=np.int64) - np.repeat(first, ln)
    return np.repeat(seq_off.astype(np.int64), ln) + j, np.repeat(np.asarray(nib_off, dtype=np.int64), ln) + j


class PackedReadBatch:
    """ReadBatch with the bases as BAM stores them (include/lcr.h: lcr_reads_packed): `seq4` holds two bases per byte, read i's bases 0
    and 1 in byte pack_off[i]; quals keep one byte per base at seq_off, and n_bases = quals.size is the size of the bases the engine
    unpacks on the GPU.  Engine.load_batch / load_batch_async take it like a ReadBatch."""

    FIELDS = ["pos", "seq_len", "lead_clip", "trail_clip", "flags", "seq_off", "cig_off", "n_cig",
              "pack_off", "seq4", "quals", "cigar"]
    DTYPES = dict(ReadBatch.DTYPES, pack_off=np.uint64, seq4=np.uint8)

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, np.ascontiguousarray(kw[f], dtype=self.DTYPES[f]))
        self.start0 = np.ascontiguousarray(kw["start0"], dtype=np.int64)
        self.len = np.ascontiguousarray(kw["len"], dtype=np.int32)
        self.read_begin = np.ascontiguousarray(kw["read_begin"], dtype=np.int32)
        self.ref = np.ascontiguousarray(kw["ref"], dtype=np.uint8)
        self.col_off = np.zeros(len(self.len) + 1, dtype=np.int64)
        np.cumsum(self.len, out=self.col_off[1:])
        self.names = kw.get("names")
        assert self.ref.size == self.col_off[-1]
        assert self.read_begin[-1] == self.pos.size
        assert self.pack_off.size == self.pos.size

    n_reads = ReadBatch.n_reads
    n_regions = ReadBatch.n_regions
    c_regions = ReadBatch.c_regions

    @property
    def n_bases(self):
        return int(self.quals.size)

    @property
    def n_pack(self):
        return int(self.seq4.size)

    def c_reads(self):
        r = LcrReadsPacked()
        r.mem = LCR_MEM_HOST
        r.n_reads = self.n_reads
        r.n_bases, r.n_cigar, r.n_pack = self.n_bases, int(self.cigar.size), self.n_pack
        for f in self.FIELDS:
            setattr(r, f, _ptr(getattr(self, f)))
        return r

    def upload_bytes_saved(self):
        """bytes this batch uploads less than its unpacked form: n_bases - n_pack - 8 * n_reads (the pack_off array)"""
        return self.n_bases - self.n_pack - 8 * self.n_reads

    def unpack(self):
        """The ReadBatch this batch stands for (the inverse of ReadBatch.pack): bases of n_bases bytes, a read's at seq_off; bytes that
        belong to no read are 0.  The other arrays are shared, not copied."""
        ln = self.seq_len.astype(np.int64)
        dst, src = _base_index(ln, self.seq_off, 2 * self.pack_off.astype(np.int64))
        nib = np.empty(2 * self.seq4.size, dtype=np.uint8)
        nib[0::2] = self.seq4 >> 4
        nib[1::2] = self.seq4 & 15
        bases = np.zeros(self.n_bases, dtype=np.uint8)
        bases[dst] = _NT16[nib[src]]
        kw = {f: getattr(self, f) for f in ReadBatch.FIELDS if f != "bases"}
        out = ReadBatch(bases=bases, start0=self.start0, len=self.len, read_begin=self.read_begin, ref=self.ref, names=self.names, **kw)
        for f in ("name_off", "name_blob"):
            if hasattr(self, f):
                setattr(out, f, getattr(self, f))
        return out

// lcr_asj_args.h — argument checks that need no context and no device: an annotation's, as lcr_assign_genes, lcr_junctions_genes and
// lcr_asj_genes make them, and the whole of lcr_asj_genes'.  Plain C++ over include/lcr.h, so that a stand-alone host program can run
// them (tests/asj_args_main.cpp, built with the host sanitizers).
#pragma once
#include "../../include/lcr.h"

// The two checks of an annotation and the ends of their messages; every call puts its own name and first words in front.
#define LCR_ANNOTATION_SIZES_MSG ", a negative size or mem not LCR_MEM_HOST / LCR_MEM_DEVICE"
#define LCR_ANNOTATION_ARRAYS_MSG ": null annotation array, or fewer exons than genes"
inline bool lcr_annotation_sizes_ok(int32_t mem, const lcr_gene_annotation* a) {
  return a && (mem == LCR_MEM_HOST || mem == LCR_MEM_DEVICE) && a->n_genes >= 0 && a->n_exons >= 0;
}
inline bool lcr_annotation_arrays_ok(const lcr_gene_annotation* a) {
  return a->n_genes == 0 || (a->span_start0 && a->span_end0 && a->exon_off && a->exon_start0 && a->exon_end0 && a->n_exons >= a->n_genes);
}

// -> nullptr when the arguments pass, else the message of the LCR_E_ARG
inline const char* lcr_asj_check_args(const lcr_asj_params* p, int32_t mem, const lcr_gene_annotation* a) {
  if (!p || !lcr_annotation_sizes_ok(mem, a)) return "lcr_asj_genes: null params or annotation" LCR_ANNOTATION_SIZES_MSG;
  if (p->flags & ~(uint32_t)(LCR_ASJ_EXONS | LCR_ASJ_DNA_FILTER | LCR_ASJ_COVERAGE))
    return "lcr_asj_genes: flags outside LCR_ASJ_EXONS | LCR_ASJ_DNA_FILTER | LCR_ASJ_COVERAGE";
  if (p->n_dna < 0) return "lcr_asj_genes: n_dna < 0";
  if ((p->flags & LCR_ASJ_DNA_FILTER) && p->n_dna > 0 && !p->dna_pos0) return "lcr_asj_genes: null dna_pos0 with n_dna > 0";
  if (!lcr_annotation_arrays_ok(a)) return "lcr_asj_genes" LCR_ANNOTATION_ARRAYS_MSG;
  return nullptr;
}

// lcr_asj_args.h — the argument checks of lcr_asj_genes that need no context and no device: plain C++ over include/lcr.h, so that a
// stand-alone host program can run them (tests/asj_args_main.cpp, built with the host sanitizers).
#pragma once
#include "../../include/lcr.h"

// -> nullptr when the arguments pass, else the message of the LCR_E_ARG
inline const char* lcr_asj_check_args(const lcr_asj_params* p, int32_t mem, const lcr_gene_annotation* a) {
  if (!p || !a || (mem != LCR_MEM_HOST && mem != LCR_MEM_DEVICE) || a->n_genes < 0 || a->n_exons < 0)
    return "lcr_asj_genes: null params or annotation, a negative size or mem not LCR_MEM_HOST / LCR_MEM_DEVICE";
  if (p->flags & ~(uint32_t)(LCR_ASJ_EXONS | LCR_ASJ_DNA_FILTER | LCR_ASJ_COVERAGE))
    return "lcr_asj_genes: flags outside LCR_ASJ_EXONS | LCR_ASJ_DNA_FILTER | LCR_ASJ_COVERAGE";
  if (p->n_dna < 0) return "lcr_asj_genes: n_dna < 0";
  if ((p->flags & LCR_ASJ_DNA_FILTER) && p->n_dna > 0 && !p->dna_pos0) return "lcr_asj_genes: null dna_pos0 with n_dna > 0";
  if (a->n_genes > 0 && (!a->span_start0 || !a->span_end0 || !a->exon_off || !a->exon_start0 || !a->exon_end0 || a->n_exons < a->n_genes))
    return "lcr_asj_genes: null annotation array, or fewer exons than genes";
  return nullptr;
}

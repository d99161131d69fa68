// asj_args_main.cpp — the argument checks of lcr_asj_genes (longcallr_amd/csrc/lcr_asj_args.h) in a stand-alone host program: built by
// tests/test_asj_modes_host.py with -fsanitize=address,undefined and run there; exit status 0 iff every case gives the expected verdict.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../longcallr_amd/csrc/lcr_asj_args.h"

static int fails = 0;
static void expect(const char* what, const char* msg, const char* want /* substring, or nullptr for "passes" */) {
  const bool ok = want ? (msg && std::strstr(msg, want)) : msg == nullptr;
  if (!ok) { std::printf("FAIL %s: %s\n", what, msg ? msg : "(passed)"); fails++; }
}

int main() {
  std::vector<int64_t> s{10, 50}, e{40, 90}, xs{10, 50}, xe{40, 90}, dna{5, 7, 9};
  std::vector<int32_t> off{0, 1, 2};
  lcr_gene_annotation a{2, 2, s.data(), e.data(), off.data(), xs.data(), xe.data()};
  lcr_asj_params p{10, 2, 0, 0.f, 0, 0, nullptr};
  expect("plain", lcr_asj_check_args(&p, LCR_MEM_HOST, &a), nullptr);
  expect("null params", lcr_asj_check_args(nullptr, LCR_MEM_HOST, &a), "null params");
  expect("null annotation", lcr_asj_check_args(&p, LCR_MEM_HOST, nullptr), "null params");
  expect("mem", lcr_asj_check_args(&p, 7, &a), "mem");
  for (uint32_t f = 0; f < 8; f++) { p.flags = f & ~(uint32_t)LCR_ASJ_DNA_FILTER; expect("flag bits", lcr_asj_check_args(&p, LCR_MEM_DEVICE, &a), nullptr); }
  p.flags = 8; expect("flag 8", lcr_asj_check_args(&p, LCR_MEM_HOST, &a), "flags outside");
  p.flags = 0x80000001u; expect("flag bit 31", lcr_asj_check_args(&p, LCR_MEM_HOST, &a), "flags outside");
  p.flags = LCR_ASJ_DNA_FILTER; p.n_dna = -1; expect("n_dna < 0", lcr_asj_check_args(&p, LCR_MEM_HOST, &a), "n_dna < 0");
  p.flags = 0; expect("n_dna < 0 without the flag", lcr_asj_check_args(&p, LCR_MEM_HOST, &a), "n_dna < 0");
  p.flags = LCR_ASJ_DNA_FILTER; p.n_dna = 3; expect("null dna_pos0", lcr_asj_check_args(&p, LCR_MEM_HOST, &a), "null dna_pos0");
  p.dna_pos0 = dna.data(); expect("dna sites", lcr_asj_check_args(&p, LCR_MEM_HOST, &a), nullptr);
  p.n_dna = 0; p.dna_pos0 = nullptr; expect("no dna sites", lcr_asj_check_args(&p, LCR_MEM_HOST, &a), nullptr);
  lcr_gene_annotation b = a; b.n_genes = -1; expect("negative genes", lcr_asj_check_args(&p, LCR_MEM_HOST, &b), "negative size");
  b = a; b.exon_off = nullptr; expect("null array", lcr_asj_check_args(&p, LCR_MEM_HOST, &b), "null annotation array");
  b = a; b.n_exons = 1; expect("fewer exons", lcr_asj_check_args(&p, LCR_MEM_HOST, &b), "fewer exons");
  lcr_gene_annotation none{}; expect("no genes", lcr_asj_check_args(&p, LCR_MEM_HOST, &none), nullptr);
  std::printf("%s\n", fails ? "failed" : "ok");
  return fails ? 1 : 0;
}

/*
 * lcr.h — C ABI of liblcr: the MI355X-native replacement for longcallR's per-region
 * pileup -> candidate/genotype -> read x SNP fragment matrix -> haplotype phasing hot path.
 *
 * The reference (huangnengCSU/longcallR v1.12.0, Rust) has no FFI seam; the seam is cut at the
 * five call sites of the per-region closure src/thread.rs:77-222.  Each entry point below names
 * the reference method it replaces.  BAM/FASTA decode, the CLI and the VCF/BAM writers stay on
 * the host: the ABI takes *decoded, already filtered* reads (filters of src/util.rs:652-668 /
 * src/fragment.rs:32-49 are the caller's job), grouped by region.
 *
 * Batched form: the reference runs one rayon task per region (src/thread.rs:77).  A GPU launch
 * per region would be launch-bound, so every entry point takes a *batch* of regions; results are
 * per region and independent of batch composition.
 *
 * Conventions: plain pointers + sizes, no C++/torch types.  All functions return 0 (LCR_OK) or a
 * negative LCR_E_* code and never abort/throw across the boundary (the reference panics instead).
 * A ctx is single-threaded; create one per host worker thread (mirrors one rayon worker).  Output
 * pointers handed back by lcr_get_* point into ctx-owned pinned host buffers that stay valid until
 * the next call of the same getter on that ctx or lcr_ctx_destroy.
 */
#ifndef LCR_H
#define LCR_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LCR_OK 0
#define LCR_E_ARG (-1)     /* bad argument / inconsistent sizes                                   */
#define LCR_E_CIGAR (-2)   /* unknown CIGAR op (reference: panic, util.rs:944, fragment.rs:192)    */
#define LCR_E_DEVICE (-3)  /* HIP runtime error (message via lcr_last_error)                       */
#define LCR_E_STATE (-4)   /* call order violated (e.g. lcr_candidates before lcr_pileup)          */
#define LCR_E_NOMEM (-5)
#define LCR_W_HW_QUEUES 1  /* lcr_ctx_set_async_phase(on): accepted, but the process has fewer than 8 hardware queues (below) */

#define LCR_PLATFORM_HIFI 0 /* main.rs:35-38 Platform::Hifi */
#define LCR_PLATFORM_ONT 1  /* Platform::Ont  */

#define LCR_MEM_HOST 0   /* pointers in lcr_reads / lcr_regions are host memory (copied H2D)       */
#define LCR_MEM_DEVICE 1 /* pointers are device (HBM) memory, used in place                         */

typedef struct lcr_ctx lcr_ctx;

/* ---- inputs ------------------------------------------------------------------------------- */

/* Decoded reads, SoA, borrowed for the duration of the call.  Reads are grouped by region
 * (lcr_regions.read_begin) and inside a region keep BAM order (sorted by pos).  A read that a
 * caller fetches for two regions appears twice.
 * flags: bit0 = reverse strand; bits1-2 = `ts` aux tag: 0 absent, 1 '+', 2 '-' (util.rs:674-680). */
typedef struct {
  int32_t mem;              /* LCR_MEM_HOST or LCR_MEM_DEVICE                                       */
  int32_t n_reads;
  int64_t n_bases;          /* total bytes in bases/quals                                          */
  int64_t n_cigar;          /* total u32 in cigar                                                  */
  const int32_t* pos;       /* 0-based leftmost reference position (record.pos())                  */
  const int32_t* seq_len;   /* l_seq                                                               */
  const int32_t* lead_clip; /* cigar.leading_softclips()  (looks past a hard clip)                 */
  const int32_t* trail_clip;/* cigar.trailing_softclips()                                          */
  const uint8_t* flags;
  const uint64_t* seq_off;  /* offset of read's first base in bases/quals                          */
  const uint64_t* cig_off;  /* offset of read's first op in cigar                                  */
  const uint32_t* n_cig;
  const uint8_t* bases;     /* decoded upper-case ASCII, as htslib yields (=ACMGRSVTWYHKDBN)       */
  const uint8_t* quals;     /* raw phred                                                           */
  const uint32_t* cigar;    /* BAM encoding len<<4|op, ops MIDNSHP=X (P and B are LCR_E_CIGAR)     */
} lcr_reads;

/* A batch of regions.  Region i covers 0-based reference columns [start0[i], start0[i]+len[i])
 * (= util.rs:639-642: vec_size = end-start, first column = start-1) and owns reads
 * [read_begin[i], read_begin[i+1]).  ref holds the reference bytes of every window back to back
 * (case preserved, util.rs:646-648); window i starts at ref + col_off[i]. */
typedef struct {
  int32_t mem;
  int32_t n_regions;
  const int64_t* start0;    /* n_regions                                                            */
  const int32_t* len;       /* n_regions                                                            */
  const int64_t* col_off;   /* n_regions+1 prefix sums of len                                       */
  const int32_t* read_begin;/* n_regions+1                                                          */
  const uint8_t* ref;       /* col_off[n_regions] bytes                                             */
} lcr_regions;

/* Thresholds; the code values of main.rs:272-396 are the spec (see lcr_params_preset). */
typedef struct {
  int32_t platform;         /* LCR_PLATFORM_*                                                      */
  uint32_t min_baseq;       /* main.rs min_baseq (10)                                              */
  uint32_t dist_to_end;     /* distance_to_read_end                                                */
  uint32_t polya_len;       /* polya_tail_length (<= 16)                                           */
  uint32_t min_depth, max_depth;
  uint32_t min_qual;        /* min_variant_qual                                                    */
  uint32_t dense_win, min_dense_cnt;
  uint32_t low_cnt_cut;     /* low_allele_cnt_cutoff                                               */
  uint32_t min_linkers;
  uint32_t max_enum_snps;
  uint32_t ld_weight_threshold; /* thread.rs:166 passes 1                                           */
  int32_t use_strand_bias;
  float min_af;             /* min_allele_freq                                                     */
  float min_af_intron;      /* min_allele_freq_include_intron                                      */
  float low_frac_cut;       /* low_allele_frac_cutoff                                              */
  float min_phase_score;
  double read_assign_cutoff;/* min_read_assignment_diff                                            */
  uint64_t seed;            /* replaces rand::thread_rng() (phase.rs:444,611,674,1198)             */
} lcr_params;

/* preset: 0 hifi-isoseq, 1 hifi-masseq, 2 ont-cdna, 3 ont-drna (main.rs:272-396). */
int lcr_params_preset(int preset, lcr_params* out);

/* ---- outputs ------------------------------------------------------------------------------ */

/* Pileup columns (replaces Vec<BaseFreq>, util.rs:100-127) as u32 planes of n_cols each.
 * plane[k] = planes + k*n_cols.  Reverse-strand counts are cnt - fwd.  The never-read fields of
 * BaseFreq (forward_cnt, backward_cnt, distance_to_end, i) are not produced.
 * Materialised on request: lcr_pileup stores at most the planes of the tiles that hold records; the columns no
 * record touches (uncovered, or inside introns only: 0 everywhere, n = introns across them) are stored by
 * lcr_get_columns itself, once per pileup, before it copies.  On the ONT presets, from a context's second batch
 * on, lcr_pileup stores no plane at all (its candidate filter runs on the counts while they are on chip, and the
 * columns that pass go to lcr_candidates directly): the planes of the tiles with records are then tallied from
 * the pileup's records, bit for bit the same, by the first call that reads them -- lcr_get_columns,
 * lcr_import_candidates, or a lcr_candidates with other filter parameters than lcr_pileup's.  The getter returns
 * every column, whenever it is called between lcr_pileup and the next lcr_load_batch / lcr_bind_batch /
 * lcr_pileup; like the stage calls it reads the arrays of a LCR_MEM_DEVICE batch (regions, and for that second
 * tally the reads as well).  No other call needs those columns. */
enum {
  LCR_PL_A = 0, LCR_PL_C, LCR_PL_G, LCR_PL_T, /* a,c,g,t                                            */
  LCR_PL_N,                                    /* n  (intron)                                        */
  LCR_PL_D,                                    /* d  (deletion)                                      */
  LCR_PL_NI,                                   /* ni (insertion after this column)                   */
  LCR_PL_FWD_A, LCR_PL_FWD_C, LCR_PL_FWD_G, LCR_PL_FWD_T, /* base_strands.x[0]                      */
  LCR_PL_TS_FWD, LCR_PL_TS_REV,               /* transcript_strands[0], [1]                         */
  LCR_NPLANES
};
typedef struct {
  int64_t n_cols;
  const uint32_t* planes;   /* LCR_NPLANES * n_cols                                                 */
} lcr_columns;

/* One candidate site (replaces CandidateSNP, snp.rs:39-90).  Array sorted by (region, pos). */
enum {
  LCR_F_RNA_EDIT = 1, LCR_F_DENSE = 2, LCR_F_HET = 4, LCR_F_FOR_PHASING = 8, LCR_F_HOM = 16,
  LCR_F_SINGLE = 32, LCR_F_NON_SELECTED = 64, LCR_F_CAND_SOMATIC = 128
};
typedef struct {
  int64_t pos;              /* 0-based                                                              */
  int32_t region;
  uint8_t ref_base, allele1, allele2, n_alt; /* ASCII; n_alt = alternate_alleles.num               */
  uint32_t cnt1, cnt2, depth;
  float af1, af2;           /* allele_freqs (f32, candidate.rs:97-98)                               */
  int32_t variant_type;     /* 0 homref 1 het 2 homvar 3 triallelic                                 */
  int32_t genotype;         /* eta: -1 homvar, 0 het, 1 homref                                      */
  int32_t haplotype;        /* delta: +1/-1, 0 unassigned                                           */
  uint32_t flags;           /* LCR_F_*                                                              */
  uint32_t phase_set;
  double loglik[3];         /* log10 L: [0] homvar [1] het [2] homref (candidate.rs:267-282)        */
  double gt_prob[3];        /* genotype_probability                                                 */
  double qual;              /* variant_quality                                                      */
  double gq;                /* genotype_quality                                                     */
  double phase_score;
} lcr_candidate;
typedef struct {
  int32_t n_cand;
  int32_t n_regions;
  const lcr_candidate* cand;
  const int32_t* region_off; /* n_regions+1: candidates of region i are [off[i], off[i+1])          */
} lcr_candidate_list;

/* Read x SNP fragment matrix (replaces Vec<Fragment>, snp.rs:197-239) in CSR.  Row k = k-th
 * fragment pushed by get_fragments (fragment.rs:293-307), i.e. every read of the region that starts
 * at or before the region's last candidate, empty rows included.
 * val: bits0-4 q (clamped to 30), bit5 = 1 if p=+1 (ref) / 0 if p=-1 (alt), bits6-7 base code ACGT,
 * col: index into lcr_candidate_list.cand (global, batch-wide). */
typedef struct {
  int32_t n_rows;
  int64_t nnz;
  int32_t n_regions;
  const int32_t* row_region_off; /* n_regions+1                                                     */
  const int64_t* row_ptr;        /* n_rows+1                                                        */
  const int32_t* row_read;       /* n_rows: index into lcr_reads                                    */
  const int32_t* col;            /* nnz                                                             */
  const uint8_t* val;            /* nnz                                                             */
  const uint8_t* row_for_phasing;/* n_rows                                                          */
  const uint32_t* row_links;     /* n_rows: num_hete_links                                          */
} lcr_fragmat;

/* Phasing result: candidates updated in place (haplotype, genotype, variant_type, phase_score,
 * phase_set, flags) plus per row sigma / assignment / phase set. */
typedef struct {
  int32_t n_rows;
  int32_t n_regions;
  const int8_t* haplotag;    /* sigma in {-1,0,1}                                                   */
  const uint8_t* assignment; /* 0 unassigned, 1 hap1, 2 hap2 (snpfrags.rs:548-625)                   */
  const uint32_t* phase_set; /* read -> PS (snpfrags.rs:628-733), 0 = none                           */
  const double* objective;   /* n_regions: best cal_overall_probability (phase.rs:257-276)           */
} lcr_phase_result;

/* ---- entry points ---------------------------------------------------------------------------- */

int lcr_ctx_create(int device, lcr_ctx** out);
void lcr_ctx_destroy(lcr_ctx*);
const char* lcr_last_error(const lcr_ctx*);
/* Launch on an existing hipStream_t (e.g. torch's current stream); NULL = ctx-owned stream. */
int lcr_ctx_set_stream(lcr_ctx*, void* hip_stream);
int lcr_ctx_sync(lcr_ctx*);

/* Bind a batch (reads + regions).  LCR_MEM_HOST inputs are copied to HBM here (the call returns when the copies are done) --
 * page-locked arrays (lcr_host_alloc / lcr_host_register) straight by DMA, pageable ones through page-locked staging buffers of
 * the context, 8 MB at a time (four lanes on threads of their own for uploads of 64 MB and more: ~47 GB/s), not through the runtime's
 * pin-the-caller's-pages path, which raised device memory faults on ROCm 7 / MI355X.  LCR_MEM_DEVICE inputs are used in place and must outlive
 * the calls below. */
int lcr_load_batch(lcr_ctx*, const lcr_reads*, const lcr_regions*);
/* Asynchronous input path for a caller whose reads are decoded on the host (the reference's loop, thread.rs:77-143, decodes the
 * next region while the current one is processed).  A ctx has two staging slots in HBM and an upload stream of its own:
 *   lcr_load_batch_async(ctx, reads, regions, slot)  enqueues the H2D copies of a LCR_MEM_HOST batch into slot 0 / 1 and returns;
 *       the host arrays must stay valid -- and should be page-locked (lcr_host_alloc / lcr_host_register), otherwise the
 *       runtime stages the copy and the call blocks for most of it -- until lcr_bind_batch(slot) has returned.
 *   lcr_bind_batch(ctx, slot)  makes that batch the current one (waits for its upload, then as lcr_load_batch of a
 *       device-resident batch); the stage calls follow.  Uploading into the slot that is bound invalidates the bound batch.
 * So batch i + 1 crosses PCIe while batch i's kernels run; results are those of lcr_load_batch on the same arrays. */
int lcr_load_batch_async(lcr_ctx*, const lcr_reads*, const lcr_regions*, int32_t slot);
int lcr_bind_batch(lcr_ctx*, int32_t slot);
/* Packed batches: a batch whose bases are still BAM's 4-bit codes.  The fields of lcr_reads with seq4 / pack_off / n_pack in place of
 * bases; the library expands the nibbles on the GPU (csrc/k0_unpack.hip) into a buffer of its own, so half a byte per base crosses the
 * link instead of one: a batch uploads n_bases - n_pack - 8 * n_reads fewer bytes, n_pack = sum of (seq_len + 1) / 2.  Any layout the
 * plain form allows is allowed: gaps, and any order of seq_off and of pack_off. */
typedef struct {
  int32_t mem; int32_t n_reads;
  int64_t n_bases;          /* bytes of quals, and of the UNPACKED bases the context will hold                              */
  int64_t n_cigar;
  int64_t n_pack;           /* bytes in seq4                                                                             */
  const int32_t *pos, *seq_len, *lead_clip, *trail_clip; const uint8_t* flags;
  const uint64_t *seq_off, *cig_off; const uint32_t* n_cig;   /* as in lcr_reads                                        */
  const uint64_t* pack_off; /* byte of seq4 that holds the read's bases 0 and 1                                           */
  const uint8_t* seq4;      /* BAM encoding: base i of a read sits in byte pack_off + i / 2, high nibble for even i; code k stands
                               for "=ACMGRSVTWYHKDBN"[k]; the low nibble behind an odd-length read is ignored                 */
  const uint8_t* quals; const uint32_t* cigar;
} lcr_reads_packed;
/* lcr_load_batch of the equivalent unpacked batch: afterwards the context is in exactly that state, every stage call and getter gives
 * bit-identical results.  mem = LCR_MEM_HOST or LCR_MEM_DEVICE, equal in both structs.  The unpacked bases live in a buffer of the
 * context and are never in the caller's memory.  LCR_E_ARG for seq_len[i] < 0, seq_off[i] + seq_len[i] > n_bases,
 * pack_off[i] + (seq_len[i] + 1) / 2 > n_pack (sums in 64 bits), n_pack < 0 or n_bases < 0.  A host batch is checked on the host in
 * front of any work: a refused call changes nothing, the batch bound before it still answers.  A device batch is checked by the
 * unpack kernel -- a violating read is skipped whole, no load or store of it is issued -- whose verdict is read at the one host wait
 * lcr_load_batch of a device batch makes; that wait lies behind the point where binding has begun to rewrite the context's tables, so
 * a device batch refused there leaves NO batch bound (as a device batch whose region table is refused by lcr_load_batch does).
 * With the asynchronous phase stage the call waits for the stage in flight, like a host batch: a device batch is unpacked into the one
 * buffer that may hold the bases of the batch that stage belongs to (lcr_load_batch_packed_async has a buffer per slot and does not). */
int lcr_load_batch_packed(lcr_ctx*, const lcr_reads_packed*, const lcr_regions*);
/* lcr_load_batch_async of a packed LCR_MEM_HOST batch, into the same two slots: the packed bytes are uploaded on the upload stream, the
 * unpack kernel is queued on that stream behind them, then the slot's event is recorded -- the slot holds an ordinary device-resident
 * batch, and lcr_bind_batch(slot) is used unchanged.  Every rule of lcr_load_batch_async carries over; the layout is checked on the
 * host in front of any work (LCR_E_ARG, nothing changed). */
int lcr_load_batch_packed_async(lcr_ctx*, const lcr_reads_packed*, const lcr_regions*, int32_t slot);
/* The unpack kernel by itself, for a caller that keeps BAM nibbles in HBM: all pointers are device memory, complete with respect to
 * the context's stream.  Writes the bytes of every read's range [seq_off, seq_off + seq_len) of bases_out and no other byte; runs on
 * the context's stream and returns after its verdict (one host wait): LCR_E_ARG when a read violates one of the three rules above --
 * that read's range is left untouched, the other reads' ranges are written. */
int lcr_unpack_bases(lcr_ctx*, int32_t n_reads, const int32_t* seq_len, const uint64_t* seq_off, const uint64_t* pack_off,
                     const uint8_t* seq4, int64_t n_pack, uint8_t* bases_out, int64_t n_bases);
/* HIP-event time (ms) of the last unpack kernel of this context (any of the three calls above) with timing enabled; LCR_E_STATE
 * without one.  Not a slot of lcr_kernel_ms: that list is closed. */
int lcr_unpack_ms(lcr_ctx*, float* ms);
/* page-locked host memory for the arrays of lcr_reads / lcr_regions (hipHostMalloc), or page-lock memory the caller owns */
int lcr_host_alloc(size_t bytes, void** out);
void lcr_host_free(void* p);
int lcr_host_register(void* p, size_t bytes);
int lcr_host_unregister(void* p);

/* The four stage calls below queue their kernels on the context's stream and return as soon as the host has what it
 * needs to go on (error verdicts, sizes); the last kernels of a stage may still be running.  Later stage calls queue
 * behind them; the lcr_get_* calls and lcr_ctx_sync wait.  An error a stage can raise is always raised by that call.
 * A call refused on its arguments or on the call order (LCR_E_ARG / LCR_E_STATE in front of any work) changes nothing.  A call that
 * fails after it has begun to rewrite what the later stages read (lcr_pileup: LCR_E_CIGAR, unsorted reads, LCR_E_DEVICE; any stage:
 * a HIP or allocation error) leaves the context at the stage in front of it: a failed lcr_pileup at the bound batch, a failed
 * candidate stage at the pileup, a failed lcr_fragments at the candidate stage.  The stage calls and getters behind that point return
 * LCR_E_STATE ("... before lcr_...") until the failed stage has been run again with success; they never answer from an earlier pass. */
/* replaces Profile::fill_data_into_freq_vec (util.rs:621-949); thread.rs:93-103.
 * Returns LCR_E_CIGAR for an unknown CIGAR op or a CIGAR inconsistent with l_seq / soft clips. */
int lcr_pileup(lcr_ctx*, const lcr_params*);
int lcr_get_columns(lcr_ctx*, lcr_columns* out);

/* replaces SNPFrag::get_candidate_snps (candidate.rs:54-528); thread.rs:118-133.
 * May be called again on the same pileup, also after lcr_import_candidates / lcr_fragments / lcr_phase: each call is a fresh candidate
 * stage.  Its params may differ from lcr_pileup's in the fields the pileup does not read -- min_depth, max_depth, min_af,
 * min_af_intron, low_cnt_cut, low_frac_cut, use_strand_bias, min_baseq, min_qual, dense_win, min_dense_cnt (and the fields of the
 * later stages) --; platform and dist_to_end must be the pileup's (LCR_E_ARG otherwise, nothing changed), and so should polya_len
 * (the HiFi presets' histograms apply the poly-A mask again). */
int lcr_candidates(lcr_ctx*, const lcr_params*);
int lcr_get_candidates(lcr_ctx*, lcr_candidate_list* out);
/* The same records in device memory (HBM), current after lcr_candidates and after lcr_phase: for consumers that stay
 * on the device, e.g. the multi-GPU gather of result records (thread.rs:204-221 collects them per region). The pointer
 * is valid until the next lcr_candidates / lcr_load_batch on this ctx. */
int lcr_get_candidates_device(lcr_ctx*, const lcr_candidate** dev_cand, int32_t* n_cand);

/* replaces SNPFrag::import_external_candidates (candidate.rs:530-613, min_variant_qual = 0.0): the candidate stage of a run with
 * user-provided sites (longcallR -v, thread.rs:107-116), in place of lcr_candidates.  Sites of the batch (one batch's or a whole
 * contig's; those outside every region are ignored): pos0 0-based, ascending and unique; genotype codes of vcf.rs:440-446
 * (0 = 0/0, 1 = 0/1 | 1/0, 2 = 1/1, 3 = 1/2 | 2/1, 4 = anything else); qual = QUAL (NaN when missing).  Positions carry no
 * contig, and neither do the regions: the call is defined for a batch whose regions all lie on ONE contig, with that contig's
 * sites (pipeline.run batches per contig; a caller that mixes contigs in a batch must import per contig batch).
 * mem = LCR_MEM_HOST: the arrays are copied before the call returns (no host wait).  mem = LCR_MEM_DEVICE: the arrays are read
 * in place on the context's stream -- they must be complete with respect to that stream when the call is made (written by it,
 * or the writer's stream synchronised) and stay valid and unchanged until the candidate stage has been consumed (lcr_fragments,
 * lcr_get_candidates*, lcr_ctx_sync); they are checked by a kernel whose verdict the call waits for (its one host wait).
 * A site at column c of region g with
 * genotype 1-3 and a qual that is not < 0 (NaN is kept) becomes a record; codes 0 and 4 and negative quals none.  Record fields:
 *   pos, region; ref_base = the reference byte as stored (case kept); allele1 / cnt1, allele2 / cnt2 = get_two_major_alleles of
 *   the column's A/C/G/T counts; depth = a + c + g + t; af1 / af2 = cnt / depth as f32 (NaN when depth is 0); qual = gq = the
 *   site's qual; genotype 1: variant_type 1, genotype 0, flags HET | FOR_PHASING; 2: variant_type 2, genotype -1, HOM | FOR_PHASING;
 *   3: variant_type 3, genotype -1, HOM.  n_alt, haplotype, phase_set, loglik, gt_prob and phase_score are 0.  No dense-cluster
 *   sweep, no RNA-edit or low-fraction class.  Needs lcr_pileup (LCR_E_STATE); unsorted / duplicate positions or a code above 4:
 *   LCR_E_ARG.  Afterwards lcr_get_candidates*, lcr_fragments and lcr_phase work as after lcr_candidates; lcr_candidates on the same
 *   pileup is unaffected. */
int lcr_import_candidates(lcr_ctx*, const lcr_params*, int32_t mem, int32_t n_sites, const int64_t* pos0, const uint8_t* genotype,
                          const float* qual);

/* The exon-only mask (longcallR --exon-only -a annotation; candidate.rs:73-89): lcr_candidates drops, first of all its filters, every
 * column that lies in no interval of its region's list.  Region g of the BOUND batch owns intervals [iv_off[g], iv_off[g + 1]) of
 * iv_start0 / iv_end0 (iv_off: n_regions + 1 entries, iv_off[0] == 0, ascending), in reference coordinates, 0-based half-open -- in any
 * order, overlapping, nested or abutting; an interval that reaches past the region is clipped to it, one outside it is ignored, one with
 * end0 == start0 sets nothing.  A region without an interval has every column masked out: no record.  iv_off == NULL clears the mask (the
 * other two arguments are not read); so do lcr_load_batch of any batch and lcr_bind_batch -- the mask belongs to the bound batch.
 * A masked column is absent from the dense-cluster sweep too (candidate.rs:465-526): the result is not the unmasked record list with
 * records deleted.  The pileup does not depend on the mask -- lcr_get_columns behind a masked pileup returns what it returns without
 * one -- and lcr_import_candidates ignores it (thread.rs:107-116 gives the imported sites no mask).
 * mem = LCR_MEM_HOST: the arrays are copied before the call returns (no host wait).  mem = LCR_MEM_DEVICE: the arrays are read in
 * place on the context's stream -- complete with respect to that stream when the call is made, valid and unchanged until the stream
 * has passed the call (any lcr_get_*, lcr_pileup, lcr_ctx_sync) --; they are checked by a kernel whose verdict the call waits for
 * (its one host wait).
 * Needs a bound batch (LCR_E_STATE).  LCR_E_ARG, nothing changed: iv_off[0] != 0, a descending iv_off, end0 < start0, NULL interval
 * arrays beside a non-zero count, a mem that is neither.  Stage: before lcr_pileup a set or clear moves nothing.  After lcr_pileup it
 * leaves the pileup valid and the context AT the pileup: the stage calls and getters behind it return LCR_E_STATE until a candidate
 * stage has run again (lcr_collect_phase keeps the last lcr_phase's results until then, as across lcr_load_batch).  The filter
 * verdicts lcr_pileup computed in passing on the ONT presets count as made under another filter: the next lcr_candidates takes its
 * own pass over the planes. */
int lcr_set_exon_mask(lcr_ctx*, int32_t mem, const int32_t* iv_off, const int64_t* iv_start0, const int64_t* iv_end0);
/* HIP-event time (ms) of the last lcr_set_exon_mask's kernels (the plane's clear and the builder) with timing enabled (lcr_enable_timing);
 * LCR_E_STATE without one.  Not a slot of lcr_kernel_ms: that list is closed. */
int lcr_exon_mask_ms(lcr_ctx*, float* ms);

/* replaces SNPFrag::get_fragments (fragment.rs:10-309); thread.rs:136-143.
 * Reads the records of the last candidate stage (lcr_candidates or lcr_import_candidates); may be repeated until lcr_phase runs.
 * lcr_phase rewrites those records (FOR_PHASING, variant type, genotype: the post-phase steps), so after it lcr_fragments returns
 * LCR_E_STATE until a new candidate stage has run.  min_linkers = 0: LCR_E_ARG, nothing changed. */
int lcr_fragments(lcr_ctx*, const lcr_params*);
int lcr_get_fragmat(lcr_ctx*, lcr_fragmat* out);

/* replaces init_haplotypes/init_assignment + SNPFrag::phase (phase.rs:1087-1296) and the
 * post-phase sequence thread.rs:162-201 (assign_reads_haplotype, assign_snp_haplotype_genotype,
 * eval_rna_edit_var_phase, eval_low_frac_var_phase, assign_phase_set).
 * Once per candidate stage: it writes its results into the candidate records that K3 and the phase stage read, so a second lcr_phase
 * (or lcr_fragments) returns LCR_E_STATE -- "run the candidate stage again" -- until lcr_candidates / lcr_import_candidates has run;
 * the getters keep answering with this call's results.  ld_weight_threshold other than 1: LCR_E_ARG, nothing changed (a later
 * lcr_phase with good params still runs). */
int lcr_phase(lcr_ctx*, const lcr_params*);
int lcr_get_phase_result(lcr_ctx*, lcr_phase_result* out);
/* The per-row results once more as 12-byte records in device memory (HBM), current after lcr_phase: the second record type
 * of the multi-GPU gather (the reference collects read -> HP / PS per region, thread.rs:204-221).  row = fragment row of
 * lcr_get_fragmat (batch-wide).  The pointer is valid until the next lcr_phase / lcr_load_batch on this ctx. */
typedef struct {
  int32_t row;
  int8_t haplotag;           /* sigma */
  uint8_t assignment;        /* 0 unassigned, 1 hap1, 2 hap2 */
  uint16_t pad_;
  uint32_t phase_set;        /* 0 = none */
} lcr_read_record;
int lcr_get_read_records_device(lcr_ctx*, const lcr_read_record** dev_rec, int32_t* n_rows);

/* Everything the last lcr_phase produced, in one call -- the getter of a PIPELINED caller (thread.rs:204-221 collects per region what
 * the closure of thread.rs:93-201 returns).  The getters above answer for the batch that is bound: once the next batch has been bound
 * (lcr_load_batch of a device batch, lcr_bind_batch) they return LCR_E_STATE.  This one stays valid across lcr_load_batch / lcr_bind_batch
 * and lcr_pileup of the next batch -- none of them touches the buffers named here -- until the next lcr_candidates; with the
 * asynchronous phase stage it is the call that waits for the stage in flight, so the order
 *   lcr_phase(N); lcr_load_batch(N + 1); lcr_pileup(N + 1); lcr_collect_phase(results of N); lcr_candidates(N + 1); ...
 * delivers every batch's results while batch N + 1's pileup runs beside batch N's resolve / post-phase tails.  Host arrays as in
 * lcr_candidate_list / lcr_phase_result (candidates updated by the stage); dev_cand / dev_read_rec: the same records in HBM. */
typedef struct {
  int32_t n_regions, n_rows, n_cand, pad_;
  const lcr_candidate* cand;            /* n_cand records, region by region                         */
  const int32_t* cand_region_off;       /* n_regions + 1                                            */
  const int32_t* row_region_off;        /* n_regions + 1: fragment rows of every region              */
  const int8_t* haplotag;               /* n_rows, as lcr_phase_result                               */
  const uint8_t* assignment;
  const uint32_t* phase_set;
  const double* objective;              /* n_regions                                                */
  const lcr_candidate* dev_cand;        /* HBM: n_cand records                                      */
  const lcr_read_record* dev_read_rec;  /* HBM: n_rows records                                      */
} lcr_phase_collected;
int lcr_collect_phase(lcr_ctx*, lcr_phase_collected* out);

/* Haplotagging against a phased VCF (K11): stands in place of lcr_phase when the caller HOLDS the phase -- longcallR -v with a DNA-phased
 * file (trio, long-read WGS), the `whatshap haplotag` use.  The reference reads each site's phase bit (vcf.rs:397-451) and never uses it;
 * lcr_phase infers haplotypes per coverage island, so "haplotype 1" is an arbitrary label per region.  Here the rows of lcr_get_fragmat are
 * assigned to the caller's haplotypes and phase sets: labels are the same across regions, genes and contigs, and a site with monoallelic
 * expression stays usable.  DESIGN.md section 1i.
 *   sites              one contig's (the rule of lcr_import_candidates): pos0 0-based, ascending and unique; h1 / h2 the ASCII base A / C /
 *       G / T on haplotype 1 / 2, h1 != h2; phase_set != 0.  n_sites == 0 (NULL arrays) is legal: every row is then unassigned.
 *   usable candidate   variant_type == 1 with LCR_F_HET and LCR_F_FOR_PHASING both set, neither LCR_F_DENSE nor LCR_F_RNA_EDIT, pos one
 *       of pos0, and the upper-cased ref_base equal to that site's h1 or h2.  Its record gets haplotype = +1 when ref_base is h1 (the VCF
 *       writer prints 0|1), -1 when it is h2, and the site's phase_set.  Every other candidate keeps what the candidate stage wrote, with
 *       LCR_F_NON_SELECTED set in its flags (haplotype, phase_set and phase_score stay 0).
 *   usable entry       a CSR entry at a usable candidate whose base code (val bits 6-7) is the site's h1 or h2.  No quality threshold: q
 *       = val bits 0-4, the table of the phase stage (fe[q] = log10 eps_q, f1e[q] = log10(1 - eps_q), scale 2^40, q = 0 as q = 1).
 *       t1 = f1e[q] when the base is h1, else fe[q]; t2 the other one.
 *   row's phase set    the phase_set value with the most usable entries in the row, ties to the smallest value; only its entries count.
 *   sums               A1 = sum t1, A2 = sum t2, D = A1 + A2 (negative), int64.  A row takes part iff it has >= min_linkers counted
 *       entries.  It is assigned iff A1 != A2 and fabs((double)(A1 - A2)) >= read_assign_cutoff * fabs((double)D) -- |q - qn| >= cutoff
 *       of snpfrags.rs:590 with q = 1 - A / D; an exact tie is "no evidence" whatever the cutoff (snpfrags.rs:591 assigns it at cutoff 0:
 *       a stated deviation).  A1 > A2: assignment 1, haplotag +1; otherwise 2 and -1; the row's phase set.  Every other row: 0 / 0 / 0.
 *   site record        per candidate (zeros when not usable), over the assigned rows with a counted entry at it: n_h1 / n_h2 rows by
 *       assignment, n_h*_match those whose base is their haplotype's allele, total_fx = sum (fe[q] + f1e[q]), match_fx = sum (match ?
 *       f1e[q] : fe[q]).  The candidate's phase_score = -10 log10((double)match_fx / (double)total_fx) when n_h1 >= 1 and n_h2 >= 1
 *       (cal_phase_score_log at the fixed delta, phase.rs:238-255), else the reference's constant 0.19940219.
 * Every decision is taken on integers: the result is independent of the batch's composition and bit-reproducible.  The sums stay below
 * 2^53 for rows and sites of up to about 2 000 entries (|fe[1]| < 2^40, so 2 000 terms of at most 2 * 2^40 stay below 2^52), so the
 * int64 -> double conversions are exact there; beyond it they round to nearest, the same on every run.
 * Needs lcr_fragments (LCR_E_STATE), after either candidate stage; settles an asynchronous phase stage in flight first; once per
 * candidate stage like lcr_phase -- a second lcr_haplotag, lcr_phase or lcr_fragments returns LCR_E_STATE until a candidate stage has run.
 * Afterwards lcr_get_phase_result, lcr_get_read_records_device, lcr_collect_phase, lcr_get_candidates*, lcr_junctions, lcr_ase,
 * lcr_ase_genes, lcr_junctions_genes and lcr_asj_genes answer exactly as behind lcr_phase; objective is 0.0 per region, lcr_get_tie_census
 * returns zeros, lcr_get_ld_blocks no blocks, lcr_get_downsample "no region".  Down-sampling (lcr_set_downsample*) is IGNORED: tagging is
 * linear in the entries and sees every row.  Of params the call reads min_linkers and read_assign_cutoff.
 * mem as in lcr_import_candidates: LCR_MEM_HOST arrays are copied before the call returns; LCR_MEM_DEVICE arrays are read in place on the
 * context's stream and stay valid and unchanged until a getter or lcr_ctx_sync has returned.  A kernel checks them and writes its verdict
 * to pinned memory: the call's one host wait, taken before anything the last stage left is touched -- unsorted or duplicate positions,
 * a base outside ACGT, h1 == h2 or phase_set == 0 are LCR_E_ARG and change nothing.  The site records die with the phase results (the
 * next candidate stage, lcr_load_batch / lcr_bind_batch): lcr_get_haplotag_sites answers LCR_E_STATE then.  rec: pinned host memory the
 * call's last kernel wrote, one record per candidate of lcr_get_candidates, valid until the next lcr_haplotag; dev_rec: the same in HBM. */
typedef struct { int64_t match_fx, total_fx; uint32_t n_h1, n_h2, n_h1_match, n_h2_match; } lcr_haplotag_site;  /* 32 bytes, one per candidate */
int lcr_haplotag(lcr_ctx*, const lcr_params*, int32_t mem, int32_t n_sites, const int64_t* pos0,
                 const uint8_t* h1, const uint8_t* h2, const uint32_t* phase_set);
int lcr_get_haplotag_sites(lcr_ctx*, int32_t* n_cand, const lcr_haplotag_site** rec, const lcr_haplotag_site** dev_rec);
/* HIP-event time (ms) of the last lcr_haplotag's kernels behind the check of the sites with timing enabled (lcr_enable_timing); LCR_E_STATE
 * without one.  Not a slot of lcr_kernel_ms: that list is closed. */
int lcr_haplotag_ms(lcr_ctx*, float* ms);

/* Allele-specific junctions (K6): the haplotype x junction table of the allele-specific analysis that consumes the phased reads
 * (allele_specific/longcallR-asj.py: get_exon_intron_regions' N arm, process_chunk :229-236, analyze_gene :671-676 / :734,
 * check_absent_present, haplotype_event_test), counted on the GPU from what lcr_phase left there.  Defined per region -- a region
 * stands where the script has a gene.  Row r of region g is a row of lcr_get_fragmat: its read is row_read[r], its haplotype
 * assignment[r], its phase set phase_set[r] (0 = none, the script's PS ".").
 *   junctions of a read   every N op of length >= 1 gives (s, l): s = 0-based contig column of the first skipped base = pos + the
 *       lengths of the earlier M, D, N, = and X ops (I, S, H, P consume nothing); the script's 1-based inclusive junction is
 *       (s + 1, s + l).  rend = pos + all reference-consuming lengths (exclusive).
 *   participating rows    assignment 1 or 2 (the rule by which an HP tag is written) and more than min_junctions junctions.  Every
 *       other read takes no part, neither as present nor as absent: assignment 0, reads that are no row, too few junctions.
 *   kept junctions        n_reads(g, s, l) = participating rows of g that have the junction; kept iff n_reads >= min_count.
 *   overlap               a participating row overlaps a kept junction iff pos < s + l && rend > s; it is PRESENT if one of its
 *       junctions has the same s and l, ABSENT otherwise.
 *   phase set             among the overlapping rows, count per value of ps; the junction's phase_set is the value with the most rows,
 *       ties to the smallest value, 0 a value like any other; n_phase_sets = distinct values seen; h1_absent, h1_present, h2_absent,
 *       h2_present count the rows of that phase set only.
 *   motif                 the reference bytes at s, s+1 and s+l-2, s+l-1 of the region's window, upper-cased: 1 = GT..AG, 2 = CT..AC,
 *       0 otherwise, for l < 2, or when either pair lies outside the window.
 *   order                 by region, then s, then l, ascending; independent of the batch's composition and bit-reproducible (integer adds).
 * Not the script's: no annotation here (no gene assignment of reads, no exon-overlap filter, no Novel / Strand / Gene_name --
 * lcr_junctions_genes below is the per-gene form, on top of lcr_assign_genes); the tie between
 * equally large phase sets goes to the smallest value (the script: a Python set's iteration order); zero-length N ops are ignored;
 * rows are not restricted to reads contained in the region (with --truncation a read that spans a cut is a row of both flanks).
 * lcr_junctions needs the bound batch after lcr_phase (LCR_E_STATE otherwise, nothing changed; params == NULL: LCR_E_ARG), collects an
 * asynchronous phase stage in flight first, queues on the context's stream, writes no buffer another stage or getter reads, and may be
 * repeated with other parameters.  Its results die with the phase stage's: at the next candidate stage and at lcr_load_batch /
 * lcr_bind_batch; lcr_get_junctions answers LCR_E_STATE then.  junc / junc_region_off: pinned host memory the stage's last kernels
 * wrote, valid until the next lcr_junctions; dev_junc: the same records in HBM. */
typedef struct { uint32_t min_count, min_junctions; } lcr_junction_params;   /* script defaults: 10, 2 */
typedef struct {
  int32_t region; uint8_t motif; uint8_t pad_[3];
  int64_t start0;            /* contig coordinate of the first skipped base */
  int32_t len; uint32_t n_reads;
  uint32_t phase_set, n_phase_sets;
  uint32_t h1_absent, h1_present, h2_absent, h2_present;
} lcr_junction;              /* 48 bytes */
typedef struct { int32_t n_regions, n_junctions; const lcr_junction* junc; const int32_t* junc_region_off;
                 const lcr_junction* dev_junc; } lcr_junction_list;
int lcr_junctions(lcr_ctx*, const lcr_junction_params*);
int lcr_get_junctions(lcr_ctx*, lcr_junction_list* out);

/* Allele-specific expression (K7): the haplotype counts and the parent-of-origin votes of the analysis that consumes the phased reads
 * (allele_specific/longcallR-ase.py: calculate_ase_pvalue, the vote loops of calculate_ase_pvalue_pat_mat), counted on the GPU from what
 * lcr_phase left there.  Defined per region -- a region stands where the script has a gene, as for lcr_junctions.  Row r of region g is a
 * row of lcr_get_fragmat: its haplotype a = assignment[r], its phase set ps = phase_set[r].
 *   counting rows      a is 1 or 2 and ps != 0 (the script's `if ps and hp`); every other row takes no part.
 *   phase set          count the counting rows per value of ps; the region's phase_set is the value with the most rows, ties to the
 *       smallest value; n_phase_sets = distinct values seen; h1 / h2 = counting rows of that phase set with a = 1 / 2.  Without a
 *       counting row: phase_set 0, every count 0.
 *   parental sites     (optional) pos0 0-based, ascending and unique; pat / mat ASCII A / C / G / T, pat != mat.  They carry no contig:
 *       the call is defined for a batch on ONE contig with that contig's sites, the rule of lcr_import_candidates.
 *   eligible site      a candidate of region g that (1) the VCF writer would print as PASS with a phased het GT -- LCR_F_DENSE and
 *       LCR_F_NON_SELECTED not set, variant_type == 1, phase_score >= min_phase_score, allele1 or allele2 differs from ref_base --,
 *       (2) has a phase_set != 0 that (3) equals the region's, and (4) whose pos is one of the parental pos0.  n_sites counts them.
 *   votes              every counting row of the region's phase set; every CSR entry of that row at an eligible site whose q field (the
 *       fragment matrix clamps it to 30) is >= min_baseq counts as pat if its base code equals the site's pat, else as mat if it equals
 *       mat, else as nothing.  The row votes paternal if pat > mat, maternal if pat < mat, not at all if they are equal (a row without
 *       an eligible entry among them).  h1_pat, h1_mat, h2_pat, h2_mat count the votes by the row's haplotype.
 *   order              one record per region, in region order; integer adds only: bit-reproducible, independent of the batch's composition.
 * Not the script's: no annotation here (no gene assignment of reads -- lcr_assign_genes / lcr_ase_genes below are the per-gene form --, no
 * exon filter); the tie between equally large phase sets goes to the smallest value (the script: a dict's order); a read's base is seen only where the fragment matrix has an entry -- the base is the
 * site's reference or one of its two major alleles (fragment.rs:134-152) --, so a parental allele that is neither is never counted; only
 * single-base REF / ALT parental records are used; rows are not restricted to reads contained in the region.
 * lcr_ase needs the bound batch after lcr_phase (LCR_E_STATE otherwise, nothing changed; params == NULL or min_baseq > 30: LCR_E_ARG),
 * collects an asynchronous phase stage in flight first, queues on the context's stream, writes no buffer another stage or getter reads,
 * and may be repeated with other parameters or sites.  n_sites == 0 (NULL arrays) is the plain mode: phase_set, n_phase_sets, h1, h2 are
 * filled, the site and vote fields are 0.  mem as in lcr_import_candidates: LCR_MEM_HOST arrays are copied before the call returns,
 * LCR_MEM_DEVICE arrays are read in place on the context's stream and stay valid until lcr_get_ase / lcr_ctx_sync.  Unsorted or duplicate
 * positions, a pat / mat byte outside ACGT and pat == mat are LCR_E_ARG, found by a kernel whose verdict the call waits for (its one host
 * wait; the last call's records stay valid).  The records die with the phase stage's results: at the next candidate stage and at
 * lcr_load_batch / lcr_bind_batch; lcr_get_ase answers LCR_E_STATE then.  rec: pinned host memory the call's last kernel wrote, valid
 * until the next lcr_ase; dev_rec: the same records in HBM. */
typedef struct { uint32_t min_baseq; float min_phase_score; } lcr_ase_params;   /* 13 (pysam's pileup default), the VCF writer's value */
typedef struct {
  int32_t region;
  uint32_t phase_set, n_phase_sets;   /* the phase set with the most counting rows (0 = none), distinct sets seen */
  uint32_t h1, h2;                    /* counting rows of that phase set per haplotype                             */
  uint32_t n_sites;                   /* eligible sites                                                            */
  uint32_t h1_pat, h1_mat, h2_pat, h2_mat;
} lcr_ase_region;            /* 40 bytes */
typedef struct { int32_t n_regions; const lcr_ase_region* rec; const lcr_ase_region* dev_rec; } lcr_ase_list;
int lcr_ase(lcr_ctx*, const lcr_ase_params*, int32_t mem, int32_t n_sites, const int64_t* pos0, const uint8_t* pat, const uint8_t* mat);
int lcr_get_ase(lcr_ctx*, lcr_ase_list* out);

/* Per-site allele x haplotype counts (K12): how often each base was seen on each haplotype at every candidate -- the SNP-level table
 * that allelic-count tools consume, the 2 x 2 table behind "is this RNA edit allele-specific?", and the check of a phase --, counted on the
 * GPU from what lcr_phase or lcr_haplotag left there.  DESIGN.md section 1j.  Row r of lcr_get_fragmat has assignment a and phase set ps
 * (lcr_read_record); candidate c is an index into lcr_get_candidates.
 *   entries of c       every CSR entry with col == c, from any row; n_entries is their number.  A LCR_F_DENSE candidate has none.
 *   counted entry      q = val & 31 >= min_baseq; the entries below it are counted in n_lowq and take no further part.  min_baseq 0
 *       counts everything; above 30 is LCR_E_ARG (the fragment matrix clamps qualities to 30), as in lcr_ase.
 *   counting row       a is 1 or 2 and ps != 0 (lcr_ase's rule).
 *   n_phase_sets       the number of distinct ps values among the counted entries of counting rows at c.
 *   site's phase set   the candidate's own phase_set where it is not 0 -- also where another set has more rows at the site --; otherwise
 *       the ps with the most counted entries of counting rows at c, ties to the smallest value; without any, 0.
 *   counts             n[k][b], b = base code A, C, G, T (val >> 6), over the counted entries: k = 1 / 2 for counting rows of the site's
 *       phase set with a = 1 / 2; k = 0 for every other row -- unassigned, assigned without a phase set, or in another set.
 *   invariant          the twelve cells and n_lowq add up to n_entries.
 *   order              one record per candidate, in candidate order; integer adds only: bit-reproducible, independent of the batch's
 *       composition.
 * Not a pileup: a read's base is seen only where the fragment matrix has an entry -- the base is the site's reference or one of its two
 * major alleles (fragment.rs:134-152) --, and never at a dense candidate.
 * lcr_site_counts needs the phase results of lcr_phase or lcr_haplotag (LCR_E_STATE otherwise, nothing changed; params == NULL or
 * min_baseq > 30: LCR_E_ARG, the last call's records stay valid), collects an asynchronous phase stage in flight first, queues a fixed
 * number of kernels on the context's stream without a host wait of its own, writes no buffer another stage or getter reads, and may be
 * repeated with another threshold.  The records die with the phase results: at the next candidate stage and at lcr_load_batch /
 * lcr_bind_batch; lcr_get_site_counts answers LCR_E_STATE then.  rec: pinned host memory the call's last kernel wrote, valid until the
 * next lcr_site_counts; dev_rec: the same records in HBM. */
typedef struct { uint32_t min_baseq; } lcr_site_count_params;   /* 13, lcr_ase's default */
typedef struct { uint32_t phase_set, n_phase_sets, n_entries, n_lowq; uint32_t n[3][4]; } lcr_site_count;   /* 64 bytes, one per candidate */
int lcr_site_counts(lcr_ctx*, const lcr_site_count_params*);
int lcr_get_site_counts(lcr_ctx*, int32_t* n_cand, const lcr_site_count** rec, const lcr_site_count** dev_rec);
/* HIP-event time (ms) of the last lcr_site_counts' kernels with timing enabled (lcr_enable_timing); LCR_E_STATE without one.  Not a
 * slot of lcr_kernel_ms: that list is closed. */
int lcr_site_counts_ms(lcr_ctx*, float* ms);

/* Per-haplotype coverage (K13): covered depth per haplotype class at EVERY column of every region window, run-length encoded -- the
 * bedGraph / bigWig pair that is loaded beside the junction and expression tables --, counted on the GPU from the bound batch's positions
 * and CIGARs and from what lcr_phase or lcr_haplotag left there.  DESIGN.md section 1k.  All coordinates 0-based half-open; region g of the
 * bound batch has the window [start0[g], start0[g] + len[g]) and the reads [read_begin[g], read_begin[g+1]) of lcr_regions.
 *   class of a read    read i has class k = assignment[r] when a row r of lcr_get_fragmat has row_read[r] == i and assignment[r] is 1 or 2:
 *       the rule by which an HP tag is written, and lcr_junctions' rule.  The phase set is not consulted.  Every other read has class 0:
 *       rows with assignment 0, reads that are no row (they start behind the region's last candidate), all reads of a region without
 *       candidates.  A read listed in two regions is classed in each by that region's own row.
 *   covered columns    walk the CIGAR from pos: M, =, X and D of length >= 1 cover [p, p + l) and advance p; N advances p and covers
 *       nothing; I, S, H, P and zero-length ops do neither.  Each covered block is clipped to the region's window; a block wholly outside
 *       it contributes nothing (reads do reach outside: the flanks of a truncation cut, gene-clipped regions).
 *   depth              depth[k][c] = the number of reads of class k that cover window column c; u32, no narrowing anywhere.
 *   segments           within one region a segment is a maximal run of consecutive columns with the same triple (depth[0], depth[1],
 *       depth[2]) other than (0, 0, 0); all-zero runs are not stored; a segment never crosses a region boundary; order: region, then start.
 *   region record      n_reads[k]: the region's reads per class, those without a block inside the window included; bases[k]: the sum of
 *       depth[k][c] over c (u64); max_depth[k]: the maximum over the window; seg_region_off[g] .. [g+1]: the region's segments.
 *   reproducibility    integer adds only: bit-reproducible and independent of the batch's composition -- a region processed alone gives
 *       the same records as inside any batch, apart from its region index.
 * Instance: start0 = 1000, len = 40; r0 pos 1000 10M class 1; r1 pos 1005 5M10N5M class 2; r2 pos 1008 4M2D4M class 0; r3 pos 1020
 * 3S5M2I5M class 1.  Six segments, [start, end) -> (n0, n1, n2): [1000,1005) (0,1,0); [1005,1008) (0,1,1); [1008,1010) (1,1,1);
 * [1010,1018) (1,0,0); [1020,1025) (0,1,1); [1025,1030) (0,1,0).  bases = (10, 20, 10), max_depth = (1, 1, 1), n_reads = (1, 2, 1).
 * lcr_hap_coverage needs the bound batch with the phase results of lcr_phase or lcr_haplotag (LCR_E_STATE otherwise, nothing changed),
 * collects an asynchronous phase stage in flight first, queues its kernels on the context's stream, writes no buffer another stage or
 * getter reads, and may be repeated.  The number of segments is data dependent: the call is the count-pass form -- it waits ONCE on the
 * host, like lcr_junctions, for the segment count, and sizes the records from it (no capacity bound is guessed).  Dense form: 12 bytes of
 * HBM per window column of the batch while the call runs.  More than 2^31 - 1 segments in one batch: LCR_E_ARG.  The records die with the
 * phase results: at the next candidate stage and at lcr_load_batch / lcr_bind_batch; lcr_get_hap_coverage answers LCR_E_STATE then.
 * seg, seg_region_off (n_regions + 1) and reg (n_regions): pinned host memory the call's last kernels wrote, valid until the next
 * lcr_hap_coverage; dev_*: the same records in HBM.  seg / dev_seg are NULL without a segment, reg / dev_reg without a region.
 * Measured: 0.78 ms per warm call on the benchmark's C3 workload (DESIGN.md section 1k has the command and the sizes). */
typedef struct { int32_t region; int32_t len; int64_t start0; uint32_t n[3]; uint32_t pad_; } lcr_hap_cov_segment;   /* 32 bytes */
typedef struct { int32_t region; uint32_t n_reads[3]; uint32_t max_depth[3]; uint32_t pad_; uint64_t bases[3]; } lcr_hap_cov_region;  /* 56 bytes */
typedef struct { int32_t n_regions, n_segments; const lcr_hap_cov_segment* seg; const int32_t* seg_region_off;
                 const lcr_hap_cov_region* reg; const lcr_hap_cov_segment* dev_seg; const lcr_hap_cov_region* dev_reg; } lcr_hap_cov_list;
int lcr_hap_coverage(lcr_ctx*);
int lcr_get_hap_coverage(lcr_ctx*, lcr_hap_cov_list* out);
/* HIP-event time (ms) from the first to the last kernel of the last lcr_hap_coverage with timing enabled (lcr_enable_timing), the host's
 * wait for the segment count included; LCR_E_STATE without one.  Not a slot of lcr_kernel_ms: that list is closed. */
int lcr_hap_coverage_ms(lcr_ctx*, float* ms);

/* Haplotype-resolved somatic scores (K14): at every candidate, per haplotype of the phased reads, is the site reference, heterozygous or
 * somatic -- the stage the reference ends its per-region closure with (snpfrags.rs:735-771 detect_somatic_by_het, somatic.rs
 * calculate_prob_somatic; commented out at its call site, thread.rs:187) --, computed on the GPU from what lcr_phase or lcr_haplotag left
 * there.  DESIGN.md section 1l.  Row r of lcr_get_fragmat has assignment a and phase set ps (lcr_read_record); candidate c is an index
 * into lcr_get_candidates.
 *   entries of c       every CSR entry with col == c, from any row.  q = val & 31.  An entry with q < min_baseq is counted in n_lowq and
 *       takes no further part; the others are the counted entries.  min_baseq 0 (the reference has no threshold) counts everything; above 30
 *       is LCR_E_ARG (the fragment matrix clamps qualities to 30, as the reference's collector does, snpfrags.rs:118).
 *   site's phase set   lcr_site_counts' rule at the same min_baseq: the candidate's own phase_set where it is not 0; otherwise the ps with
 *       the most counted entries of counting rows at c, ties to the smallest value; without any, 0.  For the same min_baseq phase_set equals
 *       lcr_site_count.phase_set at every candidate.  (The reference keys on the assignment alone; haplotype labels mean something only
 *       inside one phase set.)
 *   counting row       a is 1 or 2, ps != 0 and ps == the site's phase set.  n[a - 1][0 ref, 1 alt] counts its counted entries; the counted
 *       entries of every other row go to n_other.
 *   invariant          n[0][0] + n[0][1] + n[1][0] + n[1][1] + n_other + n_lowq = the number of entries of c.
 *   allele of an entry ref when its base code (val >> 6) is the code of ref_base (A, C, G, T in either case), else alt.
 *   status             LCR_SOM_ALLELES when neither allele1 nor allele2 equals ref_base (snpfrags.rs:121): the counts are filled; L, cls and
 *       call are 0 and nothing else is evaluated.  LCR_SOM_DEEP when a haplotype has more than 2^20 counted entries at the site: likewise.
 *       LCR_SOM_OK otherwise.
 *   tables             four of 31 int64 each, built on the host per call as llround(log10(x) * 2^40) -- the phase stage's fixed point --:
 *       eps_q = 10^(-q / 10), q = 0 treated as q = 1 (the phase stage's rule; the reference would take log 0 there); fe[q] = eps,
 *       f1e[q] = 1 - eps, fs_ref[q] = purity * eps + (1 - purity) * (1 - eps), fs_alt[q] = purity * (1 - eps) + (1 - purity) * eps; the
 *       priors log10(1 - het_rate - som_rate), log10(het_rate), log10(som_rate), rounded the same way.
 *   sums               per haplotype h over the counted entries of its counting rows (somatic.rs:12-34 in logs; int64, any order):
 *       L[h][0 ref] = prior_ref + sum over ref of f1e[q] + sum over alt of fe[q]
 *       L[h][1 het] = prior_het + sum over ref of fe[q]  + sum over alt of f1e[q]
 *       L[h][2 som] = prior_som + sum over ref of fs_ref[q] + sum over alt of fs_alt[q]
 *       Every table entry is below 2^42 in magnitude, so the sums are exact up to 2^20 counted entries per haplotype (LCR_SOM_DEEP above).
 *   class              cls[h] = 2 when L[h][2] > L[h][0] and L[h][2] > L[h][1]; else 1 when L[h][1] > L[h][0] and L[h][1] > L[h][2]; else 0
 *       (somatic.rs:38-44, the same strict comparisons, on integers).  A haplotype without counted entries has its priors only: class 0.
 *   call               only at a candidate whose flags hold LCR_F_CAND_SOMATIC when the call runs (a low-fraction site the rescue did not
 *       promote): 2 when cls = {0, 2}, 1 when cls = {2, 0}, else 0 (snpfrags.rs:753-765).  cls and L are filled at EVERY candidate with
 *       status LCR_SOM_OK, flagged or not: at an ordinary het site they read "ref on one haplotype, het on the other".  Candidate records
 *       are not modified.  (The reference walks its candidate-time list, rescued sites included; that is not reproduced.)
 *   score              not in the record, which holds integers only.  With l = L[call - 1][.] / 2^40:
 *       SQ = -10 * (log10(10^l_ref + 10^l_het) - log10(10^l_ref + 10^l_het + 10^l_som)),
 *       each log evaluated after subtracting the maximum of its own terms, so that nothing cancels or underflows: the reference's
 *       -10 log10(1 - prob_som), whose f64 products of per-read probabilities are 0 from 108 reads at q30 on (NaN once all three are)
 *       and whose 1 - prob cancels to 0 (a score of inf).  longcallr_amd/somatic.py: score().
 *   order              one record per candidate, in candidate order; integer adds and compares only: bit-reproducible, independent of the
 *       batch's composition.
 * Instance (purity 0.3, the default rates, every q = 30): a LCR_F_CAND_SOMATIC site with 6 ref entries on haplotype 1 and 7 ref + 3 alt on
 * haplotype 2: n = {{6, 0}, {7, 3}}, L[0] = {-3107708873, -23420730163838, -6852080807812}, L[1] = {-9899190109605,
 * -26720698299410, -8745495261838}, cls = {0, 2}, call = 2, SQ = 10.8642 (10.86 in the VCF).
 * lcr_somatic needs the phase results of lcr_phase or lcr_haplotag (LCR_E_STATE otherwise, nothing changed; params == NULL, purity outside
 * (0, 1], a rate <= 0, het_rate + som_rate >= 1 or min_baseq > 30: LCR_E_ARG, the last call's records stay valid), collects an
 * asynchronous phase stage in flight first, queues a fixed number of kernels on the context's stream without a host wait of its own,
 * writes no buffer another stage or getter reads, and may be repeated with other params.  The records die with the phase results: at the
 * next candidate stage and at lcr_load_batch / lcr_bind_batch; lcr_get_somatic answers LCR_E_STATE then.  rec: pinned host memory the
 * call's last kernel wrote, valid until the next lcr_somatic; dev_rec: the same records in HBM.
 * Measured: 0.28 ms per warm call on the benchmark's C3 workload, beside lcr_site_counts' 0.27 ms in the same process (DESIGN.md
 * section 1l). */
enum { LCR_SOM_OK = 0, LCR_SOM_ALLELES = 1, LCR_SOM_DEEP = 2 };
typedef struct { double purity, som_rate, het_rate; uint32_t min_baseq; uint32_t pad_; } lcr_somatic_params;
   /* reference values: 0.3 (snpfrags.rs:752), 5e-6, 1/2000 (somatic.rs:8-9); min_baseq 0 (the reference has no threshold) */
typedef struct {                      /* 80 bytes, one per candidate, candidate order */
  uint32_t phase_set;                 /* the site's phase set, lcr_site_counts' rule */
  uint32_t n[2][2];                   /* [hap-1][0 ref, 1 alt]: counted entries of counting rows */
  uint32_t n_other, n_lowq;           /* counted entries of all other rows; entries below min_baseq */
  uint8_t  cls[2];                    /* per haplotype: 0 ref, 1 het, 2 somatic (snp.rs:19) */
  uint8_t  call;                      /* 0 none, 1 / 2: somatic allele on haplotype 1 / 2 */
  uint8_t  status;                    /* LCR_SOM_OK 0, LCR_SOM_ALLELES 1, LCR_SOM_DEEP 2 */
  int64_t  L[2][3];                   /* [hap-1][ref, het, som]: log10(likelihood x prior) x 2^40 */
} lcr_somatic_site;
int lcr_somatic(lcr_ctx*, const lcr_somatic_params*);
int lcr_get_somatic(lcr_ctx*, int32_t* n_cand, const lcr_somatic_site** rec, const lcr_somatic_site** dev_rec);
/* HIP-event time (ms) of the last lcr_somatic's kernels with timing enabled (lcr_enable_timing); LCR_E_STATE without one.  Not a slot of
 * lcr_kernel_ms: that list is closed. */
int lcr_somatic_ms(lcr_ctx*, float* ms);

/* Allele-specific isoforms (K15): the haplotype x intron-chain table -- which whole transcript structure does each haplotype use --,
 * counted on the GPU from what lcr_phase or lcr_haplotag left there.  DESIGN.md section 1m.  Defined per region, as lcr_junctions.  Row r
 * of region g is a row of lcr_get_fragmat: its read is row_read[r], its haplotype assignment[r], its phase set phase_set[r] (0 = none).
 *   junctions of a read, rend   exactly lcr_junctions': an N op of length >= 1 gives (s, l) in contig coordinates, zero-length N ops are
 *       ignored, rend is exclusive, s rises along a read.
 *   chain                 the ordered list of a read's junctions (s_1, l_1) ... (s_k, l_k).  Two chains are the same iff they have the same k
 *       and are equal pair for pair: identity is exact (a hash routes a chain to its slot and never decides).
 *   participating rows    assignment 1 or 2 and k >= min_junctions (">=": lcr_junctions has "more than").  min_junctions == 0 is LCR_E_ARG,
 *       so an unspliced read never takes part.  Every other read takes no part, neither as present nor as absent.
 *   kept chains           n_reads(g, chain) = participating rows of g whose chain is that chain; n_h1 / n_h2 the same per haplotype, over
 *       every phase set; kept iff n_reads >= min_count.
 *   extent                of a kept chain: a = s_1, e = s_k + l_k.
 *   spanning              a participating row spans the chain iff pos <= a && rend >= e (a row that holds the chain always does).
 *   presence              a junction (s, l) of the row meets the extent iff s < e && s + l > a; these form a contiguous run.  The row is
 *       PRESENT iff that run, in order, equals the chain, ABSENT otherwise: a longer isoform that contains the chain unchanged inside the
 *       extent is present; a read truncated inside the extent does not span and is neither; a junction that straddles a or e makes the row
 *       absent.
 *   phase set             lcr_junctions' rule over the spanning rows: count them per value of ps; phase_set is the value with the most rows,
 *       ties to the smallest value, 0 a value like any other; n_phase_sets = distinct values; h1_absent, h1_present, h2_absent, h2_present
 *       count the rows of that phase set only.
 *   order                 by region, then lexicographically over the chain's (s, l) pairs, s before l, a proper prefix first;
 *       bit-reproducible, independent of the batch's composition and of the order in which atomics land.
 *   chain pool            chain[chain_first .. chain_first + n_junc) of a record are its keys s << 32 | l, in record order.
 *   row_isoform           one int32 per fragment row of the batch: the index of the kept record whose chain the row holds exactly, -1 for
 *       rows that do not participate or whose chain is not kept.
 * Not here: splice-site wobble (near-identical chains stay apart), annotation matching, a per-gene form.
 * lcr_isoforms needs the bound batch with the phase results of lcr_phase or lcr_haplotag (LCR_E_STATE otherwise, nothing changed;
 * params == NULL or min_junctions == 0: LCR_E_ARG, the last call's records stay valid; more than 2^28 junction occurrences of participating
 * rows in a batch: LCR_E_ARG), collects an asynchronous phase stage in flight first, queues a fixed number of kernels on the context's
 * stream around two host waits on sizes, writes no buffer another stage or getter reads, and may be repeated with other params.  The
 * records die with the phase results: at the next candidate stage and at lcr_load_batch / lcr_bind_batch; lcr_get_isoforms answers
 * LCR_E_STATE then.  iso / iso_region_off (n_regions + 1) / chain / row_isoform: pinned host memory, valid until the next lcr_isoforms --
 * the call's last kernels' stores (the zero offsets of a call that keeps nothing are the host's) --; dev_*: the same bytes in HBM.  iso / dev_iso are NULL without a record, chain /
 * dev_chain without a pool entry, row_isoform / dev_row_isoform without a fragment row. */
typedef struct { uint32_t min_count, min_junctions; } lcr_isoform_params;      /* defaults 10, 1 */
typedef struct {
  int32_t region, n_junc;
  int64_t start0, end0;          /* a, e */
  int32_t chain_first;           /* chain[chain_first .. chain_first + n_junc) */
  uint32_t n_reads, n_h1, n_h2;
  uint32_t phase_set, n_phase_sets;
  uint32_t h1_absent, h1_present, h2_absent, h2_present;
} lcr_isoform;                   /* 64 bytes */
typedef struct { int32_t n_regions, n_isoforms, n_chain, n_rows;
                 const lcr_isoform* iso; const int32_t* iso_region_off; const uint64_t* chain /* s << 32 | l */; const int32_t* row_isoform;
                 const lcr_isoform* dev_iso; const uint64_t* dev_chain; const int32_t* dev_row_isoform; } lcr_isoform_list;
int lcr_isoforms(lcr_ctx*, const lcr_isoform_params*);
int lcr_get_isoforms(lcr_ctx*, lcr_isoform_list* out);
/* HIP-event time (ms) from the first to the last kernel of the last lcr_isoforms with timing enabled (lcr_enable_timing), the host's two
 * waits for the sizes included; LCR_E_STATE without one.  Not a slot of lcr_kernel_ms: that list is closed. */
int lcr_isoforms_ms(lcr_ctx*, float* ms);

/* Allele-specific transcript ends (K16): the haplotype x TSS / TES site table -- where do each haplotype's transcripts start and end --,
 * counted on the GPU from what lcr_phase or lcr_haplotag left there.  DESIGN.md section 1o.  Defined per region, as lcr_junctions.  Row r
 * of region g is a row of lcr_get_fragmat: its read is row_read[r], its haplotype assignment[r], its phase set phase_set[r] (0 = none).
 *   ends of a read        left = pos; right = rend - 1, where rend = pos + the lengths of all M, D, N, = and X ops (exclusive, exactly
 *       lcr_junctions' rend).  Soft and hard clips play no part.
 *   transcript strand t   of a read (util.rs:803-819), from its flags: rev = bit 0, ts = bits 1-2.  ts == 1 ('+'): t = '+' if !rev, else
 *       '-'.  ts == 2 ('-'): t = '-' if !rev, else '+'.  ts == 0 (no tag; ts == 3 counts as no tag too): with strand_mode ==
 *       LCR_ENDS_STRAND_TS (0, the default) the read has no strand; with LCR_ENDS_STRAND_READ (1: direct RNA, where the read's strand is
 *       the transcript's) t = '+' if !rev, else '-'.  In the records 1 = '+', 2 = '-'.
 *   kind of an end        the left end of a '+' read and the right end of a '-' read are 5' ends (kind 0, "TSS"); the other two are 3'
 *       ends (kind 1, "TES").
 *   participating rows    assignment 1 or 2, and a strand.  Unspliced reads take part.  Every other read takes no part, neither as present
 *       nor as absent.
 *   histogram             for region g, strand t and side d (0 left, 1 right), c(g, t, d, x) = participating rows of g with strand t whose
 *       side-d end is column x.  x is a contig coordinate; ends outside the region's window count like any other.  The four (t, d) classes
 *       of a region never mix.
 *   peaks                 non-maximum suppression with the window W = `window`: x with c(x) > 0 is a peak iff, for every other y of the
 *       same (g, t, d) with c(y) > 0 and |y - x| <= W, either c(x) > c(y), or c(x) == c(y) and x < y.  That order is strict and total, so
 *       two peaks of a class are always more than W apart, and every non-empty class has at least one peak.  W == 0 makes every distinct
 *       coordinate a peak.  Deliberately not single-linkage clustering: with the ragged 5' ends of cDNA reads single linkage chains a whole
 *       exon into one cluster.
 *   assignment            an end at x belongs to the nearest peak p of its class with |p - x| <= W; a tie (p = x - k and p' = x + k) goes
 *       to the smaller coordinate.  If no peak lies within W (a shoulder of a shoulder) the end is unassigned and counts for no site.
 *   sites, kept sites     a site is a peak.  n_reads = rows assigned to it, over every phase set; n_h1 / n_h2 the same per haplotype;
 *       n_peak = c(p), the rows ending exactly at the peak; min0 / max0 = the smallest and largest assigned coordinate.  Kept iff
 *       n_reads >= min_count.
 *   present / absent      at a kept site (g, t, d, p) only the participating rows of g with strand t are looked at.  PRESENT: the row's
 *       side-d end is assigned to this site.  ABSENT: the row is not present and its alignment covers the site's whole window,
 *       pos <= p - W && rend >= p + W + 1 (signed 64-bit arithmetic; a window reaching below column 0 is covered by no row): a read-through
 *       at a TES, a transcript that started further upstream at a TSS.  Presence is asked first, so an absent row is never also present (a
 *       row whose end lies exactly W from p and is assigned to p is present, whatever it covers).  A row that ends inside the window but
 *       is assigned elsewhere or unassigned is neither; so is a row that stops short of the window.  Only the extent counts: a read whose
 *       intron spans the window is absent, which is the alternative to terminating at an intronic site.
 *   phase set             lcr_junctions' rule over the present and absent rows: count them per value of ps; phase_set is the value with
 *       the most rows, ties to the smallest value, 0 a value like any other; n_phase_sets = distinct values; h1_absent, h1_present,
 *       h2_absent, h2_present count the rows of that phase set only.
 *   order                 by region, then p, then strand ('+' first), then side (left first); independent of the batch's composition and of
 *       the order in which atomics land.  All arithmetic is integer adds: bit-reproducible.
 *   row_site              two int32 per fragment row of the batch, [2 r] for the left end and [2 r + 1] for the right: the index of the
 *       kept record the end is assigned to, or -1.  (What a TSS / TES tag in the phased BAM would consume.)
 *   totals                n_part = participating rows; n_assigned = ends assigned to a kept site.
 * Not here: clip-length or poly-A-sequence evidence, annotation matching, a per-gene form, smoothing of the histogram.
 * lcr_transcript_ends needs the bound batch with the phase results of lcr_phase or lcr_haplotag (LCR_E_STATE otherwise, nothing changed;
 * params == NULL, window > 4096 or strand_mode > 1: LCR_E_ARG, the last call's records stay valid; min_count == 0 is treated as 1; more
 * than 2^27 participating rows in a batch: LCR_E_ARG), collects an asynchronous phase stage in flight first, queues a fixed number of
 * kernels on the context's stream around at most two host waits on sizes, writes no buffer another stage or getter reads, and may be
 * repeated with other params.  The records die with the phase results: at the next candidate stage and at lcr_load_batch /
 * lcr_bind_batch; lcr_get_transcript_ends answers LCR_E_STATE then.  site / site_region_off (n_regions + 1) / row_site: pinned host
 * memory, valid until the next lcr_transcript_ends -- the call's last kernels' stores (the zero offsets of a call that keeps nothing are the
 * host's) --; dev_*: the same bytes in HBM.  site / dev_site are NULL without a record, row_site / dev_row_site without a fragment row. */
enum { LCR_ENDS_STRAND_TS = 0, LCR_ENDS_STRAND_READ = 1 };
typedef struct { uint32_t min_count, window, strand_mode, pad_; } lcr_end_params;      /* defaults 10, 10, LCR_ENDS_STRAND_TS */
typedef struct {                 /* 64 bytes */
  int32_t region; uint8_t strand, side, kind, pad_;
  int64_t peak0;
  int32_t min0, max0;
  uint32_t n_reads, n_h1, n_h2, n_peak;
  uint32_t phase_set, n_phase_sets;
  uint32_t h1_absent, h1_present, h2_absent, h2_present;
} lcr_end_site;
typedef struct { int32_t n_regions, n_sites, n_rows, n_part; int64_t n_assigned;
                 const lcr_end_site* site; const int32_t* site_region_off; const int32_t* row_site;
                 const lcr_end_site* dev_site; const int32_t* dev_row_site; } lcr_end_list;
int lcr_transcript_ends(lcr_ctx*, const lcr_end_params*);
int lcr_get_transcript_ends(lcr_ctx*, lcr_end_list* out);
/* HIP-event time (ms) from the first to the last kernel of the last lcr_transcript_ends with timing enabled (lcr_enable_timing), the host's
 * waits for the sizes included; LCR_E_STATE without one.  Not a slot of lcr_kernel_ms: that list is closed. */
int lcr_transcript_ends_ms(lcr_ctx*, float* ms);

/* Allele-specific intron retention (K17): the haplotype x {spliced, retained} table per intron -- which haplotype leaves an intron in its
 * transcripts --, counted on the GPU from what lcr_phase or lcr_haplotag left there.  DESIGN.md section 1p.  Defined per region, as
 * lcr_junctions.  Row r of region g is a row of lcr_get_fragmat: its read is row_read[r], its haplotype assignment[r], its phase set
 * phase_set[r] (0 = none).
 *   junctions, extent, blocks   of a read: the junction (s, l) of every N op with l >= 1, and rend, are exactly lcr_junctions'.  The
 *       read's aligned blocks are the maximal stretches of [pos, rend) that hold none of those N ops: M, =, X and D all cover
 *       (lcr_hap_coverage's rule); I, S, H, P and zero-length ops change nothing.
 *   participating rows    assignment 1 or 2, and nothing else: there is no junction minimum, unspliced reads take part.  Every other read
 *       takes no part in any count.
 *   introns, kept introns n_spliced(g, s, l) = participating rows of g that hold the junction (s, l).  Kept iff n_spliced >= min_count
 *       (min_count == 0 is treated as 1): an intron that no tagged read splices is not an event here.
 *   classes               of a participating row at a kept intron [s, e), e = s + l, with the anchor a = `anchor`.  The row is looked at only
 *       if it overlaps: pos < e && rend > s (signed 64-bit arithmetic throughout).
 *         SPLICED   one of the row's junctions is exactly (s, l).
 *         RETAINED  the row is not spliced, and one of its aligned blocks [bs, be) has bs <= s - a && be >= e + a; equivalently
 *                   pos <= s - a, rend >= e + a and none of the row's N ops (s_i, l_i) has s_i < e + a && s_i + l_i > s - a.  s - a < 0
 *                   is covered by no row.
 *         OTHER     any other overlapping row: another donor or acceptor, a nested junction, a read that ends inside the intron, anchors
 *                   that are too short.
 *       SPLICED is asked first, so no row is in two classes.
 *   record                n_spliced, n_retained, n_other: the rows of each class over every phase set.  motif: lcr_junctions' (1 = GT-AG,
 *       2 = CT-AC, 0 = neither).  phase_set, n_phase_sets: lcr_junctions' rule over the SPLICED and RETAINED rows only -- count them per
 *       value of ps; phase_set is the value with the most rows, ties to the smallest value, 0 a value like any other; n_phase_sets =
 *       distinct values.  h1_spliced, h1_retained, h2_spliced, h2_retained count the rows of that phase set only.
 *   order                 by region, then s, then l; independent of the batch's composition and of the order in which atomics land.  All
 *       arithmetic is integer adds: bit-reproducible.
 *   row_retained          one int32 per fragment row of the batch: the number of kept introns the row is RETAINED at, 0 for rows that
 *       retain none or take no part.  (What a retention tag in the phased BAM would consume.)
 *   totals                n_part = participating rows; n_retained_total = the sum of row_retained (64 bit) = the sum of n_retained.
 * Not here: annotated introns or a per-gene form, partial retention (a read that covers part of the intron is OTHER), a cap on the length
 * of D ops inside the intron, skipped exons, tags in the phased BAM.
 * lcr_intron_retention needs the bound batch with the phase results of lcr_phase or lcr_haplotag (LCR_E_STATE otherwise, nothing changed;
 * params == NULL or anchor > 4096: LCR_E_ARG, the last call's records stay valid; more than 2^28 junction occurrences of participating
 * rows in a batch: LCR_E_ARG), collects an asynchronous phase stage in flight first, queues a fixed number of kernels on the context's
 * stream around at most two host waits on sizes, writes no buffer another stage or getter reads, and may be repeated with other params.
 * The records die with the phase results: at the next candidate stage and at lcr_load_batch / lcr_bind_batch; lcr_get_intron_retention
 * answers LCR_E_STATE then.  intron / intron_region_off (n_regions + 1) / row_retained: pinned host memory, valid until the next
 * lcr_intron_retention -- the call's last kernels' stores (the zero offsets of a call that keeps nothing are the host's) --; dev_*: the same
 * bytes in HBM.  intron / dev_intron are NULL without a record, row_retained / dev_row_retained without a fragment row. */
typedef struct { uint32_t min_count, anchor, pad_[2]; } lcr_retention_params;      /* defaults 10, 10 */
typedef struct {                 /* 56 bytes */
  int32_t region; uint8_t motif; uint8_t pad_[3];
  int64_t start0;                /* s: contig coordinate of the first skipped base */
  int32_t len;                   /* l */
  uint32_t n_spliced, n_retained, n_other;
  uint32_t phase_set, n_phase_sets;
  uint32_t h1_spliced, h1_retained, h2_spliced, h2_retained;
} lcr_retained_intron;
typedef struct { int32_t n_regions, n_introns, n_rows, n_part; int64_t n_retained_total;
                 const lcr_retained_intron* intron; const int32_t* intron_region_off; const int32_t* row_retained;
                 const lcr_retained_intron* dev_intron; const int32_t* dev_row_retained; } lcr_retention_list;
int lcr_intron_retention(lcr_ctx*, const lcr_retention_params*);
int lcr_get_intron_retention(lcr_ctx*, lcr_retention_list* out);
/* HIP-event time (ms) from the first to the last kernel of the last lcr_intron_retention with timing enabled (lcr_enable_timing), the
 * host's waits for the sizes included; LCR_E_STATE without one.  Not a slot of lcr_kernel_ms: that list is closed. */
int lcr_intron_retention_ms(lcr_ctx*, float* ms);

/* Phased small indels (K18): the insertions and deletions of a few bases that sit on one haplotype's reads -- a pileup count cannot tell a
 * real 1-base deletion from homopolymer noise; the haplotype of every fragment row can --, normalised, counted and classed on the GPU from
 * what lcr_phase or lcr_haplotag left there.  DESIGN.md section 1q.  Defined per region g with the window [w0, w1) = [start0, start0 + len),
 * as lcr_junctions.  All arithmetic is signed 64 bit; the window's reference is compared without regard to case.  Row r of region g is a
 * row of lcr_get_fragmat: its read is row_read[r], its haplotype assignment[r], its phase set phase_set[r] (0 = none).
 *   participating rows    every fragment row of g, whatever its assignment (row k is the region's k-th read).  n_part is their number.
 *   gaps of a row         walking the CIGAR from pos: every I, D and N op of length L >= 1 is a gap; its raw column s is the reference
 *       column at the op, its reference length Lr is L for D and N and 0 for I.  Aligned blocks and rend are lcr_intron_retention's (M, =,
 *       X and D cover; only an N of length >= 1 breaks a block).  An I or D op with s <= pos or s + Lr >= rend has no aligned base on one
 *       side and is ignored entirely: it is no gap.  A row's gaps are in walk order; their starts and their ends (s + Lr) both ascend.
 *   events                a D gap with L <= max_del is an event iff its raw placement has s >= w0 + 1 && s + Lr <= w1; an I gap with
 *       L <= max_ins on the same condition, and only if its inserted bases (the L bases at the op's query offset: M, I, S, = and X consume
 *       the query, from offset 0) are all A, C, G or T, either case.  Every other gap -- an over-long I or D, an insertion that holds
 *       another letter, a placement outside the window, every N -- is a gap only.
 *   left shift            DEL: while s > w0 + 1 && ref[s-1] == ref[s+L-1]: s -= 1.  INS with bases q: while s > w0 + 1 && ref[s-1] ==
 *       q[L-1]: q = ref[s-1] + q[:L-1], s -= 1.  A reference letter outside ACGT stops the shift, and so do 1024 steps.  -> s_left and,
 *       for INS, the rotated q.
 *   right shift           from the left-shifted form, for the extent only.  DEL: while s + L < w1 && ref[s] == ref[s+L]: s += 1.  INS:
 *       while s < w1 && ref[s] == q[0]: q = q[1:] + ref[s], s += 1.  The same stops, at most 1024 steps.  -> s_right; shift = s_right -
 *       s_left.  The extent is [lo, hi) with lo = s_left and hi = s_right + L (DEL) or s_right (INS).
 *   key                   (uint32)s_left << 32 | type << 31 | payload, payload = L (DEL) or L << 24 | seq (INS; seq: 2 bits per base of the
 *       rotated q, A C G T = 0..3, first base lowest).  The key is exact: hashes only route, identity is the key's equality.  Hence
 *       max_ins <= 12 and max_del <= 65535.
 *   depth(g, x)           participating rows with an aligned block that holds column x (M, =, X and D cover, N does not).
 *   kept events           cnt = participating rows that hold the key.  A row may hold a key twice -- two 1-base deletions inside one
 *       homopolymer normalise to one placement --; it is counted once.  Kept iff cnt >= max(min_count, 1) && cnt * 1000 >=
 *       (uint64)min_permille * depth(g, s_left - 1)  (s_left - 1 >= w0: the anchor base lies inside the window).
 *   classes               of a participating row at a kept event, with lo_f = lo - flank, hi_f = hi + flank.  The row is looked at iff
 *       pos < hi_f && rend > lo_f.
 *         PRESENT   one of the row's event keys is the key.  Asked first.
 *         ABSENT    not PRESENT, pos <= lo_f && rend >= hi_f, and none of the row's gaps -- those that are no events included -- touches
 *                   [lo_f, hi_f]: a D or N gap touches iff s <= hi_f && s + L >= lo_f, an I gap iff lo_f <= s <= hi_f.  So: one clean
 *                   aligned block over the whole extent plus flanks.  (lo_f < 0 is covered by no row.)
 *         OTHER     every other row that is looked at.
 *   record                n_present, n_absent, n_other: the rows of each class over all participating rows.  depth = depth(g, s_left - 1).
 *       hrun: the length of the run of equal reference letters that starts at column s_left, inside the window, at most 255 (0 for an
 *       insertion at w1).  phase_set, n_phase_sets: lcr_junctions' rule over the PRESENT and ABSENT rows with assignment 1 or 2 -- the
 *       value with the most rows, ties to the smallest, 0 a value like any other; distinct values --; h1_present, h1_absent, h2_present,
 *       h2_absent count those rows of that phase set only.
 *   order                 by region, then by the key's numeric value (s_left, deletions before insertions, then L, then seq);
 *       independent of the batch's composition and of the order in which atomics land.  All arithmetic is integer adds: bit-reproducible.
 *   row_indels            one int32 per fragment row of the batch: the number of kept events the row is PRESENT at.
 *   totals                n_part; n_events = event occurrences over all participating rows (a key a row holds twice counts twice here);
 *       n_present_total = the sum of row_indels (64 bit) = the sum of n_present.
 * Not here: indels in regions without fragment rows, insertions above 12 bases, multi-allelic merging, realignment, BAM tags.
 * lcr_indels needs the bound batch with the phase results of lcr_phase or lcr_haplotag (LCR_E_STATE otherwise, nothing changed; params ==
 * NULL, flank > 4096, max_ins > 12, max_del > 65535 or more than 2^31 - 2 window columns plus regions: LCR_E_ARG, the last call's records
 * stay valid; more than 2^28 gaps or event occurrences of participating rows in a batch: LCR_E_ARG), collects an asynchronous phase stage
 * in flight first, queues a fixed number of kernels on the context's stream around at most two host waits on sizes, writes no buffer
 * another stage or getter reads, and may be repeated with other params.  The records die with the phase results: at the next candidate
 * stage and at lcr_load_batch / lcr_bind_batch; lcr_get_indels answers LCR_E_STATE then.  indel / indel_region_off (n_regions + 1) /
 * row_indels: pinned host memory, valid until the next lcr_indels -- the call's last kernels' stores (the zero offsets of a call that keeps
 * nothing are the host's) --; dev_*: the same bytes in HBM.  indel / dev_indel are NULL without a record, row_indels / dev_row_indels
 * without a fragment row. */
typedef struct { uint32_t min_count, min_permille, flank, max_ins, max_del, pad_[3]; } lcr_indel_params;  /* defaults 10, 150, 5, 12, 50 */
typedef struct {                     /* 64 bytes */
  int32_t region; uint8_t type;      /* 0 = DEL, 1 = INS */
  uint8_t hrun; uint16_t shift;
  int64_t start0;                    /* s_left */
  int32_t len; uint32_t seq;         /* INS: 2 bits per base (A C G T = 0..3), first base in the lowest bits; DEL: 0 */
  uint32_t depth, n_present, n_absent, n_other;
  uint32_t phase_set, n_phase_sets;
  uint32_t h1_present, h1_absent, h2_present, h2_absent;
} lcr_indel;
typedef struct { int32_t n_regions, n_indels, n_rows, n_part; int64_t n_events, n_present_total;
                 const lcr_indel* indel; const int32_t* indel_region_off; const int32_t* row_indels;
                 const lcr_indel* dev_indel; const int32_t* dev_row_indels; } lcr_indel_list;
int lcr_indels(lcr_ctx*, const lcr_indel_params*);
int lcr_get_indels(lcr_ctx*, lcr_indel_list* out);
/* HIP-event time (ms) from the first to the last kernel of the last lcr_indels with timing enabled (lcr_enable_timing), the host's waits
 * for the sizes included; LCR_E_STATE without one.  Not a slot of lcr_kernel_ms: that list is closed. */
int lcr_indels_ms(lcr_ctx*, float* ms);

/* Read-backed linkage of nearby sites (K19): per pair of nearby candidates, how many rows of the fragment matrix carry which base at the
 * first site AND which base at the second -- the count behind multi-nucleotide variants (two or three SNVs of one codon on one haplotype)
 * and behind a check of the phase that consults neither lcr_phase's decisions nor the rows' haplotags --, counted on the GPU from what
 * lcr_phase or lcr_haplotag left there.  DESIGN.md section 1r.  Candidate c is an index into lcr_get_candidates.
 *   eligible site      LCR_PAIRS_ALL: a candidate without LCR_F_DENSE (a dense candidate has no entries).  LCR_PAIRS_PHASED: additionally
 *       variant_type == 1, haplotype != 0 and phase_set != 0.
 *   pairs              e_0 < e_1 < ... the eligible candidates of one region in candidate order: (a, b) = (e_i, e_{i+k}) is a pair iff
 *       1 <= k <= max_partners (at most LCR_PAIRS_MAX_PARTNERS), both sites are in the same region and, with max_dist != 0,
 *       pos[b] - pos[a] <= max_dist (inclusive; 0 = no distance limit).  k is a difference of ELIGIBLE RANKS -- not of candidate indices
 *       and not the adjacency of entries inside a row: a candidate that is not eligible between two eligible ones takes no partner slot,
 *       and a row without an entry at an intermediate site still counts for the outer pair.
 *   joint row          a row with a CSR entry at a and one at b; any row: assignment and phase set are not consulted.  n_rows is their
 *       number.  A joint row in which either entry has q = val & 31 < min_baseq goes to n_lowq; every other one adds 1 to n[x][y], x and y
 *       the base codes A, C, G, T (val >> 6) at a and b.  min_baseq 0 counts everything; above 30 is LCR_E_ARG.
 *   invariant          the sixteen cells and n_lowq add up to n_rows.
 *   order              one record per pair, pairs with n_rows == 0 included, ordered by a, then b.  pair_off has n_cand + 1 entries: the
 *       pairs whose first site is candidate c are [pair_off[c], pair_off[c + 1]), empty for a c that is not eligible.  Integer adds only:
 *       bit-reproducible; a region processed alone gives the same records as inside any batch, apart from the candidate indices' offset.
 * Instance: one region with non-dense het sites at columns 10, 11, 13, 40 (candidates 0..3), reference A and alternate G at each; ALL,
 * max_partners 2, max_dist 3, min_baseq 13.  Pairs (10,11), (10,13), (11,13) and pair_off = [0, 2, 3, 3, 3]: (11,40) and (13,40) fail the
 * distance, (10,40) is rank 3.  Row r0 has the reference base everywhere and adds n[A][A] to all three; r1 has G at 10 and 11 and a third
 * base at 13 (no entry there): n[G][G] of (10,11) only; r2 has G at all three with quality 5 at column 11: n_lowq of (10,11) and (11,13),
 * n[G][G] of (10,13).  With max_dist 2, (10,13) is gone and pair_off = [0, 1, 2, 2, 2].  PHASED with site 11 homozygous, max_partners 1
 * and max_dist 0: the pairs are (10,13) and (13,40).
 * lcr_site_pairs needs the phase results of lcr_phase or lcr_haplotag (LCR_E_STATE otherwise, nothing changed).  LCR_E_ARG, with the last
 * call's records still valid: params == NULL, an unknown mode, max_partners 0 or above 8, min_baseq > 30, n_cand x max_partners above
 * 2^31 - 1.  It collects an asynchronous phase stage in flight first, queues a fixed number of kernels on the context's stream without a
 * host wait of its own (its buffers are sized from n_cand x max_partners; the last kernel leaves n_eligible and n_pairs in pinned memory,
 * read behind the call's event in lcr_get_site_pairs), writes no buffer another stage or getter reads, and may be repeated with other
 * parameters.  The records die with the phase results: at the next candidate stage and at lcr_load_batch / lcr_bind_batch;
 * lcr_get_site_pairs answers LCR_E_STATE then.  pair / pair_off: pinned host memory the call's last kernel wrote, valid until the next
 * lcr_site_pairs (pair is NULL without a pair); dev_pair / dev_pair_off: the same bytes in HBM. */
enum { LCR_PAIRS_ALL = 0, LCR_PAIRS_PHASED = 1 };
#define LCR_PAIRS_MAX_PARTNERS 8
typedef struct { uint32_t mode, max_partners, max_dist, min_baseq; } lcr_site_pair_params;     /* defaults ALL, 2, 2, 13 */
typedef struct { int32_t a, b; uint32_t n_rows, n_lowq; uint32_t n[4][4]; } lcr_site_pair;    /* 80 bytes */
typedef struct { int32_t n_cand, n_eligible, n_pairs, pad_;
                 const lcr_site_pair* pair; const int32_t* pair_off;
                 const lcr_site_pair* dev_pair; const int32_t* dev_pair_off; } lcr_site_pair_list;
int lcr_site_pairs(lcr_ctx*, const lcr_site_pair_params*);
int lcr_get_site_pairs(lcr_ctx*, lcr_site_pair_list* out);
/* HIP-event time (ms) of the last lcr_site_pairs' kernels with timing enabled (lcr_enable_timing); LCR_E_STATE without one.  Not a
 * slot of lcr_kernel_ms: that list is closed. */
int lcr_site_pairs_ms(lcr_ctx*, float* ms);

/* Read -> gene (K8): the gene assignment of reads of the allele-specific scripts (allele_specific/longcallR-ase.py: assign_reads_to_gene
 * :197-305, repeated in longcallR-asj.py :238-272), on the GPU from the CIGARs and positions of the bound batch, and the per-gene form of
 * the K7 counts on top of it (lcr_ase_genes).  All coordinates 0-based half-open; DESIGN.md section 1d.
 *   annotation         one contig's genes (the rule of lcr_import_candidates: the batch lies on ONE contig), sorted by (span_start0,
 *       span_end0); gene k's merged exons are exon_start0 / exon_end0 [exon_off[k], exon_off[k + 1]): at least one, ascending and disjoint
 *       (abutting exons are allowed), the first one starting at span_start0[k], the last one ending at span_end0[k].  The index k is the
 *       gene's id.  longcallr_amd/annotation.py builds these arrays from a GTF / GFF3.
 *   blocks of a read   walk the CIGAR from pos: M, D, = and X add to the current block; an N op of ANY length, 0 included, ends the block
 *       and starts the next one behind it (the script resets at every op 3; lcr_junctions' "zero-length N ignored" does not apply here);
 *       I, S, H and P do nothing; a block of length 0 is no block.  rend = pos + all reference-consuming lengths (exclusive).
 *   candidate genes    of a read [pos, rend): span_start0 < rend && span_end0 > pos.
 *   overlap            a block [s, e) and a merged exon [x, y) contribute min(e, y) - max(s, x) iff e - s >= 2, y > s and x < e - 1 (the
 *       script queries its interval tree with the block's inclusive end as an exclusive one: a one-base block contributes nothing, and
 *       neither does an exon that meets only the block's last base; restated as it is, not repaired).  A read's overlap with a gene is
 *       the sum over its blocks and the gene's exons.
 *   choice             the candidate with the largest overlap, ties to the smallest gene index (the script: the iteration order of a
 *       Python set); a largest overlap of 0 still assigns.  Without a candidate: gene -1, overlap 0.
 * Per read of the batch, independent of the batch's composition, integer only.
 * lcr_assign_genes needs a bound batch at any stage and does not move the stage (LCR_E_STATE without one; a NULL annotation, negative
 * sizes or NULL arrays with n_genes > 0: LCR_E_ARG).  mem as in lcr_import_candidates: LCR_MEM_HOST arrays are copied before the call
 * returns; LCR_MEM_DEVICE arrays are read in place on the context's stream, also by the kernel that runs BEHIND the call's return: they
 * must be complete with respect to that stream when the call is made and stay valid and unchanged until lcr_get_read_genes or
 * lcr_ctx_sync has returned.  The arrays are checked by a kernel whose verdict the call waits for (its one host wait): a refused
 * annotation is LCR_E_ARG and changes nothing -- the last call's result still answers.  As in every stage, a read's pos plus its
 * reference-consuming lengths is below 2^31 (the batch's int32 contig coordinates; lcr_junctions walks under the same bound): the walk
 * sums the lengths of sixteen ops in 32 bits.
 * n_genes == 0 is valid: every read gets -1.  The result dies at lcr_load_batch / lcr_bind_batch; lcr_get_read_genes answers LCR_E_STATE
 * then; a successful call also drops the records of an earlier lcr_ase_genes, which counted the rows of the assignment it replaces.
 * gene / overlap: pinned host memory, n_reads entries in the batch's read order, valid until the next lcr_assign_genes;
 * dev_gene: the gene indices in HBM (the input of a per-gene consumer that stays on the device). */
typedef struct { int32_t n_genes, n_exons; const int64_t *span_start0, *span_end0; const int32_t* exon_off;
                 const int64_t *exon_start0, *exon_end0; } lcr_gene_annotation;   /* one contig's genes, the rule of lcr_import_candidates */
int lcr_assign_genes(lcr_ctx*, int32_t mem, const lcr_gene_annotation*);
int lcr_get_read_genes(lcr_ctx*, int32_t* n_reads, const int32_t** gene, const uint32_t** overlap, const int32_t** dev_gene);

/* Per-gene allele-specific expression: the contract of lcr_ase with "region" read as "(region, gene) pair" and two changes.
 *   pairs              one record per region g and gene k with at least one fragment row of g whose read is assigned to k (whatever the
 *       row's haplotype), ordered by region, then gene; pair_region_off[g] .. [g + 1] are region g's records.
 *   counting rows      of pair (g, k): rows of g with assignment 1 / 2, a phase set != 0 and gene[read of the row] == k.  phase_set,
 *       n_phase_sets, h1, h2 as in lcr_ase over those rows.
 *   eligible site      lcr_ase's (1) - (4) against the PAIR's phase set: a candidate of g may be eligible for several pairs of g.  No
 *       restriction to the gene's coordinates (the script's pileup() call does not truncate).  n_sites counts them per pair.
 *   votes              as in lcr_ase, over the pair's counting rows of its phase set.
 * A gene that lies in several regions (or chunks) has several records: longcallr_amd/ase.py merge_gene_records picks the one with the
 * most reads, which is exact because phase sets of different regions are distinct.  Same parameters, mem rule and site checks as lcr_ase.
 * Needs lcr_phase and a valid lcr_assign_genes of the bound batch (LCR_E_STATE otherwise); one host wait on the number of pairs (beside
 * the sites' verdict).  The records die with the phase stage's results and with the gene assignment -- at lcr_load_batch /
 * lcr_bind_batch and at the next successful lcr_assign_genes --; lcr_get_ase_genes answers LCR_E_STATE then. */
typedef struct {
  int32_t region;
  uint32_t phase_set, n_phase_sets;
  uint32_t h1, h2;
  uint32_t n_sites;
  uint32_t h1_pat, h1_mat, h2_pat, h2_mat;
  int32_t gene;                       /* index into the annotation of lcr_assign_genes */
  uint32_t pad_;
} lcr_ase_gene;              /* 48 bytes: lcr_ase_region's fields, then the gene */
typedef struct { int32_t n_regions, n_pairs; const lcr_ase_gene* rec; const int32_t* pair_region_off; const lcr_ase_gene* dev_rec; } lcr_ase_gene_list;
int lcr_ase_genes(lcr_ctx*, const lcr_ase_params*, int32_t mem, int32_t n_sites, const int64_t* pos0, const uint8_t* pat, const uint8_t* mat);
int lcr_get_ase_genes(lcr_ctx*, lcr_ase_gene_list* out);

/* Per-gene allele-specific junctions (K9): the contract of lcr_junctions with "region" read as "(region g, gene k) pair", plus the
 * script's exon-overlap filter, in the script's order (longcallR-asj.py analyze_gene: junctions are counted and thresholded at :691
 * BEFORE the filter at :696-717; absent / present are taken at :734 AFTER it).  DESIGN.md section 1e.
 *   junctions of a read, rend, motif   as in lcr_junctions: N ops of length >= 1, zero-length N ignored.
 *   participating rows    of pair (g, k): rows of g with assignment 1 or 2, more than min_junctions junctions and gene[read of the row]
 *       == k, k >= 0 (the gene of lcr_assign_genes).  A read with gene -1 takes no part anywhere.
 *   kept junctions        n_reads(g, k, s, l) = participating rows of the pair that have the junction; kept iff n_reads >= min_count.
 *       The same (s, l) may be kept for two genes of a region, each with its own count.
 *   counted rows          the participating rows that pass the filter: at least one reference base covered by an M, =, X or D op of the
 *       read lies inside a merged exon of gene k.  That is the script's test (the read's exon blocks against every transcript's exons
 *       through an interval tree): the union of a gene's transcript exons is the union of its merged exons, and how a read's bases are
 *       grouped into blocks cannot change whether one of them is shared.  It is NOT overlap > 0 of lcr_assign_genes, whose overlap
 *       restates a query quirk (one-base blocks, an exon met only by a block's last base): a read with overlap 0 can share a base.  A
 *       participating row without a shared base is not counted but did count toward n_reads.
 *   overlap, presence, phase set, n_phase_sets, the four cells   as in lcr_junctions, over the COUNTED rows of the pair; ties between
 *       equally large phase sets go to the smallest value, 0 a value like any other.  A kept junction that no counted row overlaps
 *       still has a record: phase_set 0, n_phase_sets 0, the four cells 0 (the script's haplotype_event_test returns None there;
 *       longcallr_amd/asj.py drops such records).
 *   order                 by region, then gene, then s, then l; junc_region_off[g] .. [g + 1] are region g's records.  Independent of the
 *       batch's composition and bit-reproducible: nothing depends on the order in which atomics land.
 * Needs lcr_phase and a valid lcr_assign_genes of the bound batch (LCR_E_STATE otherwise, nothing changed); collects an asynchronous
 * phase stage in flight first, as lcr_junctions does; may be repeated with other parameters.  The filter needs the annotation's exons
 * at call time and lcr_assign_genes does not keep them (a LCR_MEM_DEVICE annotation is read in place), so the call takes the annotation
 * again: mem, the NULL / negative-size rules and the check of the arrays are lcr_assign_genes' (one verdict wait; a refused call is
 * LCR_E_ARG and changes nothing); n_genes must equal the n_genes of the valid assignment (LCR_E_ARG otherwise) -- that it is the SAME
 * annotation beyond that is the caller's duty.  LCR_MEM_DEVICE arrays stay valid and unchanged until lcr_get_junctions_genes or
 * lcr_ctx_sync has returned.  n_genes == 0 is valid and gives no records.  More than 2^28 junction occurrences in a batch: LCR_E_ARG.
 * The records die with the phase stage's results and at the next successful lcr_assign_genes; lcr_get_junctions_genes answers
 * LCR_E_STATE then.  The call writes no buffer another stage or getter reads: lcr_junctions / lcr_get_junctions on the same context
 * keep working before and after it.  junc / junc_region_off: pinned host memory the call's last kernels wrote, valid until the next
 * lcr_junctions_genes; dev_junc: the same records in HBM.  kernel_ms: the HIP-event time from the first kernel to the last of the
 * last call (its host waits included) when timing is enabled, -1 otherwise (no slot of lcr_kernel_ms). */
typedef struct {
  int32_t region; uint8_t motif; uint8_t pad_[3];
  int64_t start0;
  int32_t len; uint32_t n_reads;
  uint32_t phase_set, n_phase_sets;
  uint32_t h1_absent, h1_present, h2_absent, h2_present;
  int32_t gene;              /* index into the annotation of lcr_assign_genes */
  uint32_t pad2_;
} lcr_junction_gene;         /* 56 bytes: lcr_junction's fields, then the gene */
typedef struct { int32_t n_regions, n_junctions; const lcr_junction_gene* junc; const int32_t* junc_region_off;
                 const lcr_junction_gene* dev_junc; float kernel_ms; } lcr_junction_gene_list;
int lcr_junctions_genes(lcr_ctx*, const lcr_junction_params*, int32_t mem, const lcr_gene_annotation*);
int lcr_get_junctions_genes(lcr_ctx*, lcr_junction_gene_list* out);

/* The other modes of the per-gene junction table (K10): longcallR-asj.py's --cluster_with_exons, its --dna_vcf / --rna_vcf filter and its
 * .gene_coverage.tsv, each a flag of one more call behind lcr_junctions_genes.  The contract is lcr_junctions_genes', unchanged, plus
 * what follows; with flags == 0 the junction records are lcr_junctions_genes' byte for byte.  DESIGN.md section 1f.
 *   LCR_ASJ_EXONS         blocks of a read: the maximal runs of reference bases covered by M, =, X and D ops; an N op of length >= 1 ends
 *       a run, I, S, H, P and a zero-length N end nothing (the script's "extend if contiguous" arm joins the two sides), a run of zero
 *       bases is no block (zero-length M / D ops are ignored: the script can open an empty block there).  INTERIOR blocks are all but the
 *       first and the last block of a read with more than two (cluster_junctions_exons_connected_components :399-403).
 *       n_reads(g, k, start, len) = participating rows of the pair with this interior block, taken before both filters like a junction's;
 *       a block is kept iff n_reads >= min_count.  One lcr_exon_gene per kept block, ordered by region, gene, start0, len;
 *       exon_region_off[g] .. [g + 1] are region g's.  Without the flag n_exons is 0.  The junction records do not depend on the flag:
 *       exons only change how the host clusters (longcallr_amd/asj.py cluster).
 *   LCR_ASJ_DNA_FILTER    dna_pos0: one contig's heterozygous DNA SNV positions, 0-based, ascending and unique (n_dna of them; mem as for
 *       the annotation; checked by a kernel beside the annotation's check -- unsorted or duplicate positions are LCR_E_ARG and the last
 *       result stays valid; n_dna == 0 is valid).  A candidate of region g SUPPORTS its phase set when it is what lcr_ase's (1) - (2)
 *       describe -- the VCF writer would print it PASS with a phased het GT under min_phase_score, phase_set != 0: the script's
 *       load_longcallR_phased_vcf applied to the run's own VCF -- and its pos is one of dna_pos0.  A row of g with phase set ps != 0 is
 *       supported iff a supporting candidate of g has phase_set == ps.  Counted rows are lcr_junctions_genes' counted rows that are also
 *       supported (analyze_gene_with_filtering :781-790): an unsupported row still counts toward n_reads and the exon counts, is in no
 *       cell and adds no phase set to n_phase_sets.  Not the script's: it keys the RNA variants by PS value across all contigs; here a
 *       phase set belongs to its region.
 *   LCR_ASJ_COVERAGE      gene_reads[k] = reads of the bound batch with gene[r] == k and more than min_junctions N ops of length >= 1,
 *       rows and non-rows and every assignment alike (process_chunk :231-272).  Only reads that passed the batch's read filter exist, a
 *       read in both flanks of a --truncation cut counts twice, zero-length N ops do not count.  n_genes entries in pinned host memory,
 *       NULL without the flag.
 * State and argument rules are lcr_junctions_genes' (lcr_phase and a valid lcr_assign_genes with the same n_genes; the annotation again,
 * checked; a refused call changes nothing; the result dies with the phase stage's results and at the next successful lcr_assign_genes);
 * flags outside the three bits and n_dna < 0 are LCR_E_ARG; dna_pos0 is not read without LCR_ASJ_DNA_FILTER.  The call writes no buffer
 * another stage or getter reads: lcr_junctions_genes and its getter keep working before and after it.  The host waits are
 * lcr_junctions_genes': the verdict (now for both lists) and two sets of sizes.  kernel_ms as in lcr_junction_gene_list. */
enum { LCR_ASJ_EXONS = 1, LCR_ASJ_DNA_FILTER = 2, LCR_ASJ_COVERAGE = 4 };
typedef struct { uint32_t min_count, min_junctions, flags; float min_phase_score;
                 int32_t n_dna, pad_; const int64_t* dna_pos0; } lcr_asj_params;
typedef struct { int32_t region, gene; int64_t start0; int32_t len; uint32_t n_reads; } lcr_exon_gene;   /* 24 bytes */
typedef struct { int32_t n_regions, n_junctions; const lcr_junction_gene* junc; const int32_t* junc_region_off;
                 const lcr_junction_gene* dev_junc;
                 int32_t n_exons, n_genes; const lcr_exon_gene* exon; const int32_t* exon_region_off; const lcr_exon_gene* dev_exon;
                 const int32_t* gene_reads; float kernel_ms; } lcr_asj_gene_list;
int lcr_asj_genes(lcr_ctx*, const lcr_asj_params*, int32_t mem, const lcr_gene_annotation*);
int lcr_get_asj_genes(lcr_ctx*, lcr_asj_gene_list* out);

/* Down-sampling: phase deep regions on a read sample (longcallR --downsample / --downsample-depth: thread.rs:144-151, phase.rs:693-701).
 * A region with at least `depth` fragment rows (all rows of lcr_get_fragmat, empty ones included) is down-sampled: the optimiser
 * (cross_optimize and its checks, cal_overall_probability, cross_optimize_by_block), the first two post-phase rounds
 * (assign_reads_haplotype / assign_snp_haplotype_genotype, thread.rs:168-172) and the evidence of the two rescue evaluations see `depth`
 * sampled rows only; LD blocks and LD seeding, every random draw (init_assignment, the perturbation rounds, the rescue commit), the
 * THIRD post-phase round -- which assigns every read against the final haplotypes -- and assign_phase_set see all rows, as in the
 * reference.  The sample replaces StdRng + shuffle (which cannot be restated here) by the rule of the project's other draws: the
 * `depth` rows with the smallest keys  mix64(region_seed(seed, start0) + (r + 1) * 0x9E3779B97F4A7C15), r = the row's index inside
 * its region -- a uniform depth-subset, a pure function of (seed, region start, row).  The reference calls with seed 2025.
 *   lcr_set_downsample       sticky on the context; depth = 0 (the default) turns it off: lcr_phase is then exactly what it was.
 *   lcr_set_downsample_rows  the caller's own sample (e.g. the reference's StdRng shuffle over row_region_off) for the NEXT lcr_phase
 *       only, overriding lcr_set_downsample for it: one byte per fragment row of lcr_get_fragmat, non-zero = sampled (mem =
 *       LCR_MEM_HOST or LCR_MEM_DEVICE; copied before the call returns).  A region is down-sampled iff one of its rows is unsampled.
 *       Call it between lcr_fragments and lcr_phase (LCR_E_STATE otherwise; a new lcr_fragments drops it); n_rows other than the
 *       fragment stage's: LCR_E_ARG.
 *   lcr_get_downsample       what the last lcr_phase did: per region whether it was down-sampled (the reference prints this,
 *       thread.rs:153-157), per fragment row the sampled byte (0 / 1) in pinned host memory and in HBM -- both NULL when no region was
 *       down-sampled (every row counts as sampled); n_regions / n_rows are those of that lcr_phase.  Like lcr_collect_phase it outlives
 *       lcr_load_batch / lcr_bind_batch / lcr_pileup of the next batch and waits for an asynchronous phase stage: call it before the
 *       next candidate stage (LCR_E_STATE after it, and before the first lcr_phase).
 * While down-sampling is on (depth > 0, or a sample was given), lcr_phase answers LCR_E_ARG, nothing changed, to
 * read_assign_cutoff <= 0 (an unsampled row's haplotag carries no sign: the last round gives the same assignment for either sign only
 * because |q - qn| = 0 is below every positive cutoff).  The asynchronous phase stage and lcr_collect_phase work as without it. */
typedef struct {
  int32_t n_regions, n_rows;
  const uint8_t* region_applied; /* n_regions: 1 = the region was down-sampled                        */
  const uint8_t* sampled;        /* n_rows (pinned host memory), or NULL                              */
  const uint8_t* dev_sampled;    /* the same bytes in HBM, or NULL                                    */
} lcr_downsample_info;
int lcr_set_downsample(lcr_ctx*, uint32_t depth, uint64_t seed);
int lcr_set_downsample_rows(lcr_ctx*, int32_t mem, int32_t n_rows, const uint8_t* sampled);
int lcr_get_downsample(lcr_ctx*, lcr_downsample_info* out);

/* LD blocks of one region of the last lcr_phase (SNPFrag.ld_blocks, snpfrags.rs:29; built by divide_snps_into_blocks,
 * candidate.rs:615-747): block b = snp_idx[block_off[b] .. block_off[b + 1]) (candidate indices inside the region), in
 * the reference's block and node order.  Only regions with more than max_enum_snps candidates build blocks (the
 * enumeration branch, phase.rs:1097-1122, never reads them): others report n_blocks = 0. */
int lcr_get_ld_blocks(lcr_ctx*, int32_t region, int32_t* n_blocks, const int32_t** block_off, const int32_t** snp_idx);

/* Decision arithmetic of the optimiser and its census (round 4).  The reference decides sigma flips, the delta / eta choice and
 * `prob > largest_prob` on f64 ratio scores / sums accumulated in list order (phase.rs:77-96, 128-176, 257-276, 845-858, 905-940,
 * 1117); every term is one of 62 constants, so liblcr takes each decision on the EXACT fixed-point sums (order-free, hence
 * parallel and reproducible) and, where those sums tie exactly -- the only decisions on which summation order can matter --,
 * on the reference-order f64 scores of that row / configuration.  lcr_get_tie_census reports the ties of the last lcr_phase:
 *   out[0] sigma decisions with A == B at rows with an entry at a het site, decided by the f64 scores of phase.rs:77-96
 *   out[1] ... of which flipped (q < qn)
 *   out[2] delta / eta choices with a tie at the maximum where the first maximum was kept (UNRESOLVED; round 6: reported by chain regions of
 *          workgroup scope only when lcr_debug_set("chain_ties", 0) keeps them from running again under the complete contract -- the
 *          all-CU chain kernels, regions of >= 2^17 phase entries, neither resolve nor count them)
 *   out[3] steps whose only changes were tie changes, taken as "no improvement" (check_new_*, phase.rs:278-355; UNRESOLVED: as out[2])
 *   out[4] enumeration branch: regions whose configurations of maximal objective differ and were compared by their f64 sums
 *          (phase.rs:257-276); chain regions of workgroup scope (round 6): compares of two configurations of equal objective whose
 *          match bits differ, decided by their f64 sums
 *   out[5] compares that fell to "first maximum wins" (UNRESOLVED: more maxima than the list holds, states beyond the memory budget;
 *          chain regions with "chain_ties" = 0)
 *   out[6] sigma ties met by kernels without the f64 path (UNRESOLVED)
 *   out[7] (round 5: enumeration branch; round 6: chain regions of workgroup scope too) delta / eta ties at the maximum decided by the f64
 *          scores of phase.rs:128-176 + tie-only steps decided by the reference's sums of scores (check_new_haplotag /
 *          check_new_haplotype_genotype)
 * All UNRESOLVED counts zero = every decision of the call was the reference arithmetic's decision. */
int lcr_get_tie_census(lcr_ctx*, uint64_t out[8]);

/* Region discovery: replaces find_isolated_regions_with_depth (util.rs:236-332, with and
 * without --truncation) for one contig.  ref_start / ref_end are record.reference_start() / reference_end() of
 * the reads that pass the filters of util.rs:264-279 (mem = LCR_MEM_HOST or LCR_MEM_DEVICE).  Region i covers
 * 0-based columns [start0[i], start0[i] + len[i]) — the reference's 1-based [start, end) = [start0+1, start0+len+1).
 *
 * The rule (util.rs:287-330).  A column is a BREAK when its depth is 0 or, with truncation on, above
 * truncation_coverage (a depth equal to it is kept); islands are the maximal runs of the other columns.  At a
 * break a pending region with region_end > region_start is emitted, and only then are the cursors and
 * max_coverage reset; after the last column a pending region is emitted the same way.  So a single-column island
 * stays pending and starts the region that ends with the next island, the breaks between them included, and the
 * columns above the cap are in no region unless they lie between such a pair: the flanks of an over-deep stretch
 * become regions of their own (a read that spans the stretch is listed in both by lcr_bam_batch).
 *
 * max_cov is NOT the maximum over the region's columns: the reference takes it from every column before the
 * break test and resets it at an emission.  Region k gets the maximum depth over (p_{k-1}, p_k], p_k the column
 * at which it is emitted (the first break behind its last island, or the contig's last column; p_{-1} = -1): the
 * over-deep column that closes a region counts for that region, the rest of the stretch for the NEXT region, a
 * stretch in front of the first island for the first region, and columns behind the last emission for nothing.
 * With truncation a region's max_cov can therefore exceed the cap although none of its columns does. */
typedef struct {
  int32_t n_regions;
  const int64_t* start0;
  const int32_t* len;
  const uint32_t* max_cov;
} lcr_region_list;
int lcr_discover_regions(lcr_ctx*, int32_t mem, int32_t n_reads, const int32_t* ref_start, const int32_t* ref_end,
                         int64_t contig_len, lcr_region_list* out);
/* The same with longcallR's --truncation / --truncation-coverage (default 200000).  truncation == 0 ignores the cap
 * and is exactly lcr_discover_regions (which is this call with 0, 0, NULL).  *n_truncated (may be NULL): the
 * columns whose depth exceeds the cap, 0 when truncation is off.  The depth vector stays on the device; the host
 * receives per-island arrays only. */
int lcr_discover_regions_truncated(lcr_ctx*, int32_t mem, int32_t n_reads, const int32_t* ref_start, const int32_t* ref_end,
                                   int64_t contig_len, int32_t truncation, uint32_t truncation_coverage, lcr_region_list* out,
                                   int64_t* n_truncated);

/* ---- BGZF / BAM decode -> lcr_reads on the host -------------------------------------------
 * Replaces the rust-htslib IndexedReader calls of util.rs:636-691 and fragment.rs:19-59 (and the read pass of
 * region discovery, util.rs:256-287): the file is inflated once (all BGZF blocks in parallel on n_threads host
 * threads, <= 0: all hardware threads), every record is indexed once, and the batches for lcr_load_batch are cut
 * out of that index, so the pileup and the fragment stage share one decode (the reference inflates every
 * region's blocks twice).  The compressed file is mapped; only ONE contig's inflated bytes and record index are
 * resident at a time (loaded on demand, replaced when another contig is asked for).  The file must be coordinate-sorted (the reference needs its .bai too).  No GPU is
 * involved; a handle is used by one thread at a time, output pointers stay valid until the next call on the
 * handle or lcr_bam_close. */
typedef struct lcr_bam lcr_bam;
typedef struct {            /* util.rs:652-668 / fragment.rs:32-49                                        */
  uint8_t min_mapq;         /* mapq < min_mapq is dropped                                                 */
  int32_t min_read_length;  /* l_seq < min_read_length is dropped                                         */
  float divergence;         /* a `de` tag of type f with value >= divergence drops the read               */
} lcr_read_filter;          /* unmapped / secondary / supplementary records are always dropped            */
/* *out is set even when the call fails (unless out of memory): lcr_bam_last_error explains, lcr_bam_close frees */
int lcr_bam_open(const char* path, int32_t n_threads, lcr_bam** out);
/* The same with the residency policy spelled out: a file whose INFLATED size is at most keep_bytes is inflated once, at open, and
 * stays inflated (lcr_bam_spans / lcr_bam_batch / lcr_bam_write_phased then never inflate a block again); a larger one keeps
 * one contig at a time resident and inflates a contig's blocks when it is first used.  lcr_bam_open = keep_bytes of 4 GiB;
 * 0 = never keep (the memory bound of one contig). */
int lcr_bam_open_keep(const char* path, int32_t n_threads, int64_t keep_bytes, lcr_bam** out);
void lcr_bam_close(lcr_bam*);
const char* lcr_bam_last_error(const lcr_bam*);
int lcr_bam_refs(lcr_bam*, int32_t* n_ref, const char* const** names, const int64_t** lengths);
int lcr_bam_n_records(lcr_bam*, int64_t* n);
/* bytes of inflated stream + record index held right now (the whole stream of a file within keep_bytes, else one contig at a time) and their peak since lcr_bam_open */
int lcr_bam_resident(lcr_bam*, int64_t* now, int64_t* peak);
/* record.reference_start() / reference_end() of the reads of contig ref_id that pass the filter, in file order:
 * the input of lcr_discover_regions (util.rs:264-285) */
int lcr_bam_spans(lcr_bam*, int32_t ref_id, const lcr_read_filter*, int32_t* n, const int32_t** ref_start,
                  const int32_t** ref_end);
/* The passing reads of contig ref_id grouped by region with htslib's fetch rule on the reference's numbers
 * (util.rs:637: [start0 + 1, start0 + len + 1) as 0-based half-open; a read that overlaps two regions is listed
 * in both): fills *reads (mem = LCR_MEM_HOST) and *read_begin (n_regions + 1) for lcr_load_batch.  name_off /
 * names (optional): read names, NUL-terminated, name i at names + name_off[i] (the qname maps of thread.rs). */
int lcr_bam_batch(lcr_bam*, int32_t ref_id, const lcr_read_filter*, int32_t n_regions, const int64_t* start0,
                  const int32_t* len, lcr_reads* reads, const int32_t** read_begin, const uint64_t** name_off,
                  const char** names);
/* The same batch with the bases left as the file has them: selection, order, names and lifetime are lcr_bam_batch's; seq4 holds every
 * record's own (l_seq + 1) / 2 sequence bytes, copied, pack_off back to back; seq_off, quals, cigar and the per-read arrays are what
 * lcr_bam_batch yields for the same arguments.  No nibble is expanded on the host: input of lcr_load_batch_packed(_async). */
int lcr_bam_batch_packed(lcr_bam*, int32_t ref_id, const lcr_read_filter*, int32_t n_regions, const int64_t* start0,
                         const int32_t* len, lcr_reads_packed* reads, const int32_t** read_begin, const uint64_t** name_off,
                         const char** names);

/* ---- user-provided candidates: VCF reader, replaces get_genotype_quality_phase_from_vcf (vcf.rs:400-462) ----------------------
 * Reads a plain-text VCF or a gzip / BGZF .vcf.gz (every gzip member) into per-contig site lists for lcr_import_candidates.  For
 * every record and every sample whose GT has exactly two alleles: genotype code as in lcr_import_candidates (a missing allele counts
 * as 3, so ./. and 0/. give 4); qual = QUAL as f32, NaN for '.'.  A later sample or a later record at the same position overwrites
 * the earlier value (a code 4 included).  Samples with another GT length are skipped, a sites-only file yields no sites.  The phase
 * bit, REF and ALT are not used; an indel is a site at its POS.  BCF input and records without a GT key fail with LCR_E_ARG (the
 * reference panics).  No GPU is involved; *out is set even when the call fails (unless out of memory): lcr_vcf_last_error explains,
 * lcr_vcf_close frees.  n_threads is reserved (the reader runs on the calling thread). */
typedef struct lcr_vcf lcr_vcf;
int lcr_vcf_open(const char* path, int32_t n_threads, lcr_vcf** out);
void lcr_vcf_close(lcr_vcf*);
const char* lcr_vcf_last_error(const lcr_vcf*);
/* contig names that hold at least one site, in the order of their first record */
int lcr_vcf_contigs(lcr_vcf*, int32_t* n, const char* const** names);
/* the sites of one contig sorted by position (n = 0 for a contig without sites); pointers valid until lcr_vcf_close */
int lcr_vcf_contig(lcr_vcf*, const char* name, int32_t* n, const int64_t** pos0, const uint8_t** genotype, const float** qual);
/* REF, ALT and the phase bit of the same sites: arrays parallel to lcr_vcf_contig's (same n, same order, the same winning record and
 * sample).  ref = REF's byte when REF is one base, else 0; alt = the first ALT's byte when EVERY ALT allele is one base, else 0 (the
 * indel test of longcallR-ase.py's VCF loaders); phase: 0 = the GT is unphased, 1 = `0|1`, 2 = `1|0`, 3 = phased, any other alleles. */
int lcr_vcf_contig_alleles(lcr_vcf*, const char* name, int32_t* n, const uint8_t** ref, const uint8_t** alt, const uint8_t** phase);
/* The phase sets of the same sites, one more parallel array: the FORMAT `PS` integer of the same winning record and sample; 0 when the
 * record has no PS key, the sample's value is `.` or missing, or it is not an unsigned 32-bit decimal integer (the input of lcr_haplotag). */
int lcr_vcf_contig_phase_sets(lcr_vcf*, const char* name, int32_t* n, const uint32_t** ps);

/* ---- phased BAM, replaces thread.rs:307-361 ------------------------------------------------
 * Writes to out_path the header of the opened file and, region by region in the order given (region i = columns
 * [start0[i], start0[i] + len[i]) of contig region_ref[i]), the records the reference's loop keeps: fetched by the
 * region (util.rs:637 rule), not unmapped / secondary / supplementary, and lying inside the region
 * (reference_start + 1 >= start && reference_end + 1 <= end, thread.rs:340-345).  A record whose name is among the
 * n_tagged names gets `HP:i:<hp>` (int32) appended when hp is 1 or 2 and `PS:I:<ps>` (uint32) when ps != 0, unless
 * it already carries that tag; of several entries with one name the first counts (hp < 0: no assignment entry,
 * thread.rs:308-325).  BGZF blocks of 0xff00 bytes are deflated on n_threads threads (<= 0: as lcr_bam_open) at
 * `level` (-1 = zlib default, as the reference's writer).  Parity is defined on the inflated stream. */
int lcr_bam_write_phased(lcr_bam*, const char* out_path, int32_t n_regions, const int32_t* region_ref, const int64_t* start0,
                         const int32_t* len, int64_t n_tagged, const uint64_t* name_off, const char* names, const int32_t* hp,
                         const uint32_t* ps, int32_t level, int32_t n_threads);

/* Decoded reads -> BAM, the inverse of lcr_bam_batch (synthetic data sets, round-trip tests; the reference has no such
 * writer: its inputs come from minimap2): one contig, the reads of `rd` (LCR_MEM_HOST, sorted by position) as records
 * "r<index>", mapq 60, flag 0 / 16, `ts:A:+` / `-` from lcr_reads.flags; BGZF at `level`, deflated on n_threads threads. */
int lcr_bam_write_reads(const char* out_path, const char* contig, int64_t contig_len, const lcr_reads* rd, int32_t level, int32_t n_threads);

/* Asynchronous phase stage (round 5; off by default).  on = 1: lcr_phase returns as soon as its kernels are queued -- on queues of the
 * stage's own, behind the fragment stage's kernels -- and its results are collected by whoever asks for them first: lcr_collect_phase
 * (valid after the next batch has been bound: the pipelined order is spelled out there), every getter of the bound batch
 * (lcr_get_candidates*, lcr_get_phase_result, lcr_get_read_records_device, lcr_get_tie_census, lcr_get_ld_blocks), lcr_ctx_sync, the
 * next lcr_candidates / lcr_phase.  The caller's loop (thread.rs:93-201 per region; here per batch) can then bind the next
 * device-resident batch and queue its pileup at once: lcr_pileup's kernels are held back until the dense part of the stage in flight
 * -- the enumeration restarts -- is done, and run beside its resolve / post-phase tails, which leave most CUs idle.
 * CONTRACT CHANGE while it is on: the input arrays of a device-resident batch must stay unchanged until that batch's results have
 * been collected (a getter or lcr_ctx_sync) -- with the synchronous stage they are free when lcr_phase returns.  A host batch
 * (lcr_load_batch with LCR_MEM_HOST, lcr_load_batch_async) waits for the stage in flight by itself.  Persistent all-CU launches
 * and phase_prof make lcr_phase wait as before.  The stage then uses four queues: the process should run with
 * GPU_MAX_HW_QUEUES >= 8 in its environment (ROCm's default of 4 maps two of them onto one hardware queue: correct, but measured
 * without gain).  The HIP runtime reads that variable when it starts, so the library cannot set it: lcr_ctx_set_async_phase(ctx, 1)
 * returns LCR_W_HW_QUEUES (> 0: the mode IS on) when the variable is unset or below 8, and lcr_last_error says what to export. */
int lcr_ctx_set_async_phase(lcr_ctx*, int on);

/* Regions whose phase matrix is far beyond one CU are phased by persistent all-CU kernels; two such launches on one GPU --
 * of two contexts or two processes -- must not overlap, so they are serialised per device by a process-local mutex and an
 * flock on <dir>/grid_<pci bus id>.lock.  dir defaults to /tmp/liblcr-locks (created 1777 by whoever comes first); it has to be this user's
 * or root's, and sticky if others may write into it -- otherwise lcr_phase fails with LCR_E_DEVICE and says so (round 6: it used to fall back
 * to a per-user directory silently, which would have left two users' launches unserialised).  A directory named here is created 0700 and
 * has to pass the same test; "/tmp/liblcr-<uid>" is the per-user lock for a machine whose GPUs are not shared.  Processes that share a GPU must see the same directory
 * (containers without a common /tmp: name one on a shared mount).  The lock is waited for at most ten minutes; a lock that cannot
 * be taken makes lcr_phase fail with LCR_E_DEVICE -- it is never skipped. */
int lcr_ctx_set_lock_dir(lcr_ctx*, const char* dir);

/* Debug / test switches (the library reads no environment variable): key = "phase_prof", "grid_min_entries",
 * "grid_generic", "grid_spec_lanes", "post_half", "enum_force_big", "enum_force_stream" (1: every LDS-resident enumeration region by the
 * streaming kernel, one restart per wave), "enum_elide" (0: the enumeration restarts execute every sigma / delta step; default 1: a step whose inputs
 * have not changed since it last ran is skipped -- same results, same tie census), "tie_arith", "timing_mask",
 * "k3_hits" (0: the fragment stage walks the CIGARs itself), "k3_list_blocks" (workgroups of the fragment stage's two passes that walk the
 * reads beyond their hit lists; 0 = sized from the batch), "async_phase" (1: lcr_phase returns with its kernels in flight),
 * "grid_spec_batch" (0: the all-CU chain kernel's speculative half-rounds side by side on sub-grids; default 1: as eight bits of one state)
 * (bit k: only the kernel groups LCR_K_* k are timed when timing is enabled; 0 = all) (see PhaseDebug in
 * csrc/lcr_phase_host.h), "hist_tiles" (quality histograms from K0's records: 0 = when the survivors are dense, 1 = whenever the
 * preset allows, -1 = never); round 6: "chain_ties" (0: chain regions of workgroup scope keep the tie contract of round 5: sigma ties
 * only), "redo_lds" (bytes of dynamic LDS of the enumeration branch's repair pass; 0: its matrices in global memory), "fuse_filter",
 * "spec_compact" (0: lcr_candidates waits for the survivors' number before it queues their compaction), "lean_planes" (0: lcr_pileup always stores
 * the planes of the tiles with records -- and, on the ONT presets, the filter flags -- instead of handing the filter's survivors to lcr_candidates), "fold_indels" (0: the CIGAR
 * decode gives every 1-base insertion / deletion a record of its own instead of a flag of the aligned block in front of it; same results, more
 * records: lcr_pileup_records), "own_fill" (0: hipMemsetAsync instead of the
 * library's fill kernels), "fill_selftest" (checks those kernels against the host; LCR_E_DEVICE on a difference), "host_trace" (1: a
 * "[host]" line of wall-clock marks per lcr_phase on stderr; process-wide like own_fill), "iso_hash_bits" (0 .. 64, default 64: lcr_isoforms
 * routes a chain by the low n bits of its hash only -- 0 sends every chain of a region down one probe sequence; the results are the same
 * bytes for every n, which is how the comparison of whole chains is tested), "ends_hash_bits" (0 .. 32, default 32: lcr_transcript_ends
 * routes an end's key by the low n bits of its hash only -- 0 makes every key of a region probe from its segment's first slot; the same
 * bytes for every n), "ir_hash_bits" (0 .. 32, default 32: the same for lcr_intron_retention's junction keys), "indel_hash_bits"
 * (0 .. 32, default 32: the same for lcr_indels' event keys).  Unknown key: LCR_E_ARG.  The defaults are the
 * product behaviour. */
int lcr_debug_set(lcr_ctx*, const char* key, int64_t value);

/* Timing: HIP-event time (ms) of the last launch of each kernel on the ctx's stream.  (LCR_K_PHASE brackets what lcr_phase puts on the
 * ctx's stream: with the asynchronous phase stage that is the hand-over to the stage's queues only, not the stage.) */
enum { LCR_K_SPANS = 0 /* K0: CIGAR decode + binning */, LCR_K_PILEUP, LCR_K_CAND_FILTER, LCR_K_CAND_HIST, LCR_K_CAND_GT,
       LCR_K_FRAG_COUNT, LCR_K_FRAG_FILL, LCR_K_PHASE,
       LCR_K_BIND /* lcr_load_batch: read headers, read / tile -> region tables, op blocks' first reads (part of the pileup stage) */,
       LCR_K_BIND_TABLE /* lcr_load_batch of a device batch: region table + CIGAR layout check, before its one host wait */,
       LCR_K_CAND_IMPORT /* lcr_import_candidates: count, scan, emit */, LCR_K_JUNCTIONS /* lcr_junctions, first kernel to last */,
       LCR_K_ASE /* lcr_ase, first kernel to last behind the check of the parental sites */, LCR_NKERNELS };
/* The two slots of the per-gene calls follow LCR_NKERNELS in a list of their own -- the slots above keep their numbers and LCR_K_ASE stays
 * the last one in front of LCR_NKERNELS, which tests/test_ase_host.py pins --; lcr_kernel_ms and the "timing_mask" bits take every slot
 * below LCR_NTIMERS. */
enum { LCR_K_GENES = LCR_NKERNELS /* lcr_assign_genes: k8_assign and the two copies of its result, behind the annotation's check */,
       LCR_K_ASE_GENES /* lcr_ase_genes, first kernel to last behind the check of the parental sites, the wait for the number of pairs included */,
       LCR_NTIMERS };
int lcr_enable_timing(lcr_ctx*, int on);
int lcr_kernel_ms(lcr_ctx*, int kernel, float* ms);
/* Bytes the pileup tally kernel (K1) of the last lcr_pileup has to move: read bases once (B) + 8-byte
 * records + (1 + 4 + 4*LCR_NPLANES)*L; and the implementation-independent figure of the whole pileup
 * stage (K0 + K1): B + 4C + 37R + (4*LCR_NPLANES + 1)*L.  The 4*LCR_NPLANES bytes count only at the columns whose
 * planes that lcr_pileup stored itself (tiles with records); when it stored none (see lcr_columns) both figures
 * carry 48 bytes per survivor handed to lcr_candidates instead, and the getters wait for the tally to learn their
 * number if lcr_candidates has not run yet.  Planes stored later for a getter are not counted.  See DESIGN.md. */
int lcr_pileup_bytes(lcr_ctx*, int64_t* bytes);
int lcr_pileup_stage_bytes(lcr_ctx*, int64_t* bytes);
/* What the last lcr_pileup's CIGAR decode produced: `items` = the M / D / I / N ops that count somewhere (the N above), `records` = the 8-byte
 * records it cut them into for the tally -- one per tile an item touches, none for a 1-base insertion or deletion that directly follows an
 * aligned block of its read and travels as a flag of that block's record ("K0").  Both are the words lcr_pileup has
 * fetched anyway: no wait, no copy.  LCR_E_STATE before lcr_pileup. */
int lcr_pileup_records(lcr_ctx*, int64_t* items, int64_t* records);

/* Memory given back by contexts (lcr_ctx_destroy, buffers that grow) is kept in a process-wide cache per device -- at most 24 GiB of HBM
 * and 2 GiB of page-locked host memory each -- and handed to the next context: a worker that recreates its context per task does not
 * churn hipMalloc / hipFree.  lcr_release_cached_memory returns all of it to the runtime (a process that shares the GPU with another
 * allocator calls it between phases); lcr_set_cache_limits changes the two bounds (bytes per device; 0 = keep nothing). */
int lcr_release_cached_memory(void);
int lcr_set_cache_limits(int64_t device_bytes, int64_t host_bytes);

const char* lcr_version(void);

#ifdef __cplusplus
}
#endif
#endif

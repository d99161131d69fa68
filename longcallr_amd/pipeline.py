"""The driver loop around the hot path: BAM + reference FASTA -> phased VCF (+ phased BAM).

Host orchestration only; the work is done behind the C ABI (include/lcr.h).  It replaces what
`multithread_phase_haplotag_germline` (reference src/thread.rs:26-361) and its callers in src/main.rs do around
the five hot-path calls, with one context per GPU instead of one rayon task per region:

  util.rs:214-234 load_reference / parse_fai                 -> load_reference / parse_fai below
  util.rs:558-600 extract_isolated_regions_parallel          -> lcr_bam_spans + lcr_discover_regions_truncated per contig
                                                                (--truncation / --truncation-coverage included)
  thread.rs:77-221 the per-region closure                    -> one lcr_load_batch + pileup / candidates /
                                                                fragments / phase per contig (all its regions)
  thread.rs:223-305 VCF header + records                     -> write_vcf (records from vcf.format_records)
  thread.rs:307-361 phased BAM                               -> lcr_bam_write_phased

  thread.rs:70-74,107-116 user-provided candidates (-v)   -> vcf.read_sites once + lcr_import_candidates per chunk
  (no counterpart: the reference reads the phase bit and drops it) -> haplotag=True: lcr_haplotag per chunk in place of lcr_phase
  main.rs:216-225, thread.rs:80-92 -a / --exon-only          -> annotation.calling_annotation + intersect_regions per contig,
                                                                lcr_set_exon_mask per chunk

Not here (out of scope): the somatic model.  Records are written in contig order of the .fai and position order inside
a contig (the reference writes them in region-completion order, thread.rs:216-221: compare as a set)."""
import os

import numpy as np

from . import _abi, annotation, api, ase, asj, bamio, coverage, ends, indels, isoforms, retention, somatic, vcf
from . import pairs as _pairs   # (run() has a local of that name)

_ann = annotation    # (run() has a parameter of the module's name, as the reference's -a)

VCF_HEADER_TAIL = (   # thread.rs:232-262, verbatim
    '##FILTER=<ID=PASS,Description="All filters passed">\n'
    '##FILTER=<ID=LowQual,Description="Low phasing quality">\n'
    '##FILTER=<ID=HomRef,Description="Homo reference">\n'
    '##FILTER=<ID=RnaEdit,Description="RNA editing">\n'
    '##FILTER=<ID=Multiallelic,Description="Multiallelic SNP">\n'
    '##FILTER=<ID=dn,Description="Dense cluster of variants">\n'
    '##INFO=<ID=RDS,Number=1,Type=String,Description="RNA editing or Dense SNP or Single SNP.">\n'
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
    '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase Set">\n'
    '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype Quality">\n'
    '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Read Depth">\n'
    '##FORMAT=<ID=AF,Number=A,Type=Float,Description="Allele Frequency">\n'
    '##FORMAT=<ID=PQ,Number=1,Type=Float,Description="Phasing Quality">\n'
    '##FORMAT=<ID=AE,Number=A,Type=Integer,Description="Haplotype expression of two alleles">\n'
    '##FORMAT=<ID=SQ,Number=1,Type=Float,Description="Somatic Score">\n'
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSample\n")


def load_reference(path):
    """util.rs:214-222: record id (first word of the '>' line) -> sequence bytes, case preserved."""
    seqs, name, parts = {}, None, []
    with open(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                if name is not None:
                    seqs[name] = np.frombuffer(b"".join(parts), dtype=np.uint8)
                name, parts = line[1:].split()[0].decode(), []
            else:
                parts.append(line.strip())
    if name is not None:
        seqs[name] = np.frombuffer(b"".join(parts), dtype=np.uint8)
    return seqs


def parse_fai(path):
    """util.rs:224-234: [(contig, length)] in file order."""
    out = []
    with open(path) as f:
        for line in f:
            p = line.rstrip("\n").split("\t")
            if len(p) >= 2:
                out.append((p[0], int(p[1])))
    return out


def write_vcf(path, contig_lengths, body_lines, extra_header=""):
    """extra_header: further ## lines, written in front of the #CHROM line (the somatic VCF's INFO tags)"""
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.3\n")
        for name, length in contig_lengths:   # thread.rs:225-230
            f.write("##contig=<ID=%s,length=%d>\n" % (name, length))
        at = VCF_HEADER_TAIL.index("#CHROM")
        f.write(VCF_HEADER_TAIL[:at] + extra_header + VCF_HEADER_TAIL[at:])
        f.writelines(body_lines)


def chunk_regions(regions, max_cost=2.0e9, max_cols=2.0e8, max_regions=8192):
    """Cut a contig's regions [(start0, len, max_cov)] into consecutive chunks whose estimated work (sum of
    len x max_coverage, an upper bound of the aligned bases) and column count stay below the budgets: liblcr's
    per-batch limits (32-bit record pool, 2^31 reads, 2^28 matrix entries) then never surface as a failed run.
    Results are independent of batch composition, so the cut changes nothing in the output."""
    chunks, cur, cost, cols = [], [], 0.0, 0
    for r in regions:
        c = float(r[1]) * max(int(r[2]), 1)
        if cur and (cost + c > max_cost or cols + r[1] > max_cols or len(cur) >= max_regions):
            chunks.append(cur)
            cur, cost, cols = [], 0.0, 0
        cur.append(r)
        cost += c
        cols += r[1]
    if cur:
        chunks.append(cur)
    return chunks


def _gather_names(name_off, blob, rows):
    """(name_off, blob) of the reads `rows` out of a batch's name blob, without a Python object per read"""
    off = name_off.astype(np.int64)
    lens = off[rows + 1] - off[rows]
    new_off = np.zeros(rows.size + 1, dtype=np.int64)
    np.cumsum(lens, out=new_off[1:])
    idx = np.repeat(off[rows] - new_off[:-1], lens) + np.arange(int(new_off[-1]))
    return new_off.astype(np.uint64), blob[idx]


def run(bam_path, ref_path, out_vcf, out_bam=None, preset="hifi-masseq", contigs=None, device=0, threads=0, seed=2025,
        read_filter=None, devices=None, chunk_cost=2.0e9, async_phase=True, input_vcf=None,
        downsample=False, downsample_depth=10000, downsample_seed=2025, truncation=False, truncation_coverage=200000,
        asj_out=None, asj_min_count=10, asj_min_junctions=2,
        ase_out=None, ase_min_support=10, ase_overdispersion=0.001, ase_parental_vcf=None, ase_dna_vcf=None,
        ase_annotation=None, ase_gene_types=annotation.GENE_TYPES, asj_annotation=None, asj_gene_types=annotation.GENE_TYPES,
        asj_cluster_with_exons=False, asj_dna_vcf=None, asj_gene_coverage=False, annotation=None, exon_only=False, packed_upload=False,
        haplotag=False, ase_sites_out=None, ase_sites_min_baseq=13, hap_coverage_out=None,
        somatic_out=None, somatic_purity=0.3, somatic_min_baseq=0, somatic_min_score=0.0,
        isoforms_out=None, isoform_min_count=10, isoform_min_junctions=1,
        ends_out=None, ends_min_count=10, ends_window=10, ends_strand="ts",
        retention_out=None, retention_min_count=10, retention_anchor=10, retention_min_retained=1,
        indels_out=None, indel_min_count=10, indel_min_permille=150, indel_flank=5, indel_max_ins=12, indel_max_del=50,
        pairs_out=None, pairs_partners=2, pairs_min_count=10, pairs_min_baseq=13, mnv_out=None, mnv_max_dist=2, mnv_min_count=3, mnv_min_frac=0.8,
        **param_overrides):
    """BAM + FASTA (+ .fai) -> phased VCF and, with out_bam, the phased BAM.  Returns a dict of counts.
    devices: GPUs to use (default [device]); a contig's regions are cut into chunks (chunk_regions) that the engines --
    one context and one host thread per device -- take in turn (regions are independent units, thread.rs:77; the BAM
    decoder cuts the batches on the calling thread).  A GPU may be named more than once (devices=[0, 0, 0]): that many
    chunks are then in flight on it, each filling the queue gaps of the others' host round trips (bench.py
    stages.batches_in_flight: +25 % at three).  async_phase: the engines run the asynchronous phase stage (a chunk's upload + pileup
    beside the previous chunk's resolve / post-phase tails, results through lcr_collect_phase).  The output does not depend on devices,
    chunk_cost or async_phase.
    input_vcf: phase the sites of this VCF / .vcf.gz instead of calling candidates (longcallR -v, thread.rs:107-116): the file is read
    once (vcf.read_sites), every chunk takes its contig's sites inside its span (none when the contig is not in the file) through
    lcr_import_candidates.  Adds the stats input_sites (sites read) and imported_sites (sites handed to the candidate stage).
    downsample / downsample_depth: longcallR --downsample / --downsample-depth (thread.rs:144-151): a region with at least
    downsample_depth fragments is phased on a sample of that many (lcr_set_downsample, include/lcr.h; the sample is the project's
    counter-based one, not StdRng's); the last post-phase round still assigns every read.  Off by default.  It needs a positive
    read_assign_cutoff (the presets' is 0.0: pass e.g. read_assign_cutoff=1e-6), ValueError otherwise.
    truncation / truncation_coverage: longcallR --truncation / --truncation-coverage (util.rs:294-296): a column deeper than
    truncation_coverage ends a region like an uncovered one, so an over-deep stretch is neither piled up nor phased and its flanks
    become regions of their own (a read that spans it is listed in both; the phased BAM keeps the reads contained in a region).
    Adds the stat truncated_columns (columns above the cap, summed over contigs).  Off by default; truncation_coverage outside
    [0, 2^32) is a ValueError.
    asj_out / asj_min_count / asj_min_junctions: the allele-specific junction table of longcallR-asj.py (--min_count / --min_junctions;
    a region stands where the script has a gene, there is no annotation: include/lcr.h, lcr_junctions) as that script's .asj.tsv, written
    to asj_out.  Every chunk calls Engine.junctions right behind phase(); that call waits for the phase stage, so the chunk's overlap with
    the next chunk's upload and pileup (async_phase) is given up.  Adds the stat junctions (kept junctions, summed over chunks).  VCF and
    phased BAM do not depend on it; without asj_out nothing changes.
    ase_out / ase_min_support / ase_overdispersion: the allele-specific expression table of longcallR-ase.py (--min_support / -d; regions in
    place of genes: include/lcr.h, lcr_ase), written to ase_out.  Every chunk calls Engine.ase right behind phase() (behind junctions() when
    both are on).  Alone it is the script's .ase.tsv; with ase_parental_vcf (--vcf2, a whole-genome phased VCF) the .patmat_ase.tsv with
    the parent-of-origin votes of every haplotype's reads over this run's own PASS phased sites; with ase_dna_vcf (--vcf3) the
    .filter_ase.tsv, which drops the regions none of whose sites is a DNA heterozygote with a significant imbalance.  The two VCFs together
    are a ValueError (the script takes one mode), and so is either without ase_out.  Adds the stat ase_regions (rows written).  VCF, phased
    BAM and .asj.tsv do not depend on it; without ase_out nothing changes.
    ase_annotation / ase_gene_types: a GTF / GFF3 (.gz) annotation and the gene types kept from it (the script's -a / --gene_types): the
    table of ase_out is then per GENE, as the script's -- every chunk calls Engine.assign_genes after binding (every read to the gene
    whose merged exons its aligned blocks overlap most, include/lcr.h: lcr_assign_genes) and Engine.ase_genes in place of Engine.ase;
    the (region, gene) pair records of a contig's chunks are merged per gene (ase.merge_gene_records) and written in contig and then gene
    order with the annotation's Gene_name, in each of the three modes.  Adds the stat ase_genes (rows written) in place of ase_regions.
    ase_annotation without ase_out is a ValueError; without ase_annotation nothing changes.
    asj_annotation / asj_gene_types: the same for the junction table (the script's longcallR-asj.py -a / --gene_types): the table of
    asj_out is then per GENE -- every chunk calls Engine.assign_genes after binding (once, also when ase_annotation is given: the two
    must then name the same file and gene types, ValueError otherwise) and Engine.junctions_genes in place of Engine.junctions (include/lcr.h:
    lcr_junctions_genes); asj_out gets asj.format_tsv_genes' text with the annotation's Strand, Novel and Gene_name, and the script's
    .asj_gene.tsv goes beside it (X.asj.tsv -> X.asj_gene.tsv, any other name -> name + ".gene.tsv").  junctions stays the number of
    records; adds the stat asj_genes (rows of the gene file).  asj_annotation without asj_out is a ValueError; without asj_annotation
    nothing changes.
    asj_cluster_with_exons / asj_dna_vcf / asj_gene_coverage: the other modes of the script's annotated run (--cluster_with_exons,
    --dna_vcf with the run's own VCF as --rna_vcf, the .gene_coverage.tsv); each needs asj_annotation (ValueError without it).  With
    any of them on a chunk calls Engine.asj_genes in place of Engine.junctions_genes (include/lcr.h: lcr_asj_genes); with none on the
    code path is the one above.  asj_cluster_with_exons: the kept interior exon blocks join the clustering (asj.cluster), which changes
    Junction_set only.  asj_dna_vcf: a DNA VCF read with ase.dna_het_sites; every chunk gets its contig's heterozygous SNV positions
    inside its span, and rows whose phase set none of them supports are not counted.  asj_gene_coverage: reads with more than
    asj_min_junctions junctions per gene, summed over a contig's chunks and written for every `gene` feature of the annotation in file
    order (annotation.gene_features) beside the table (X.asj.tsv -> X.gene_coverage.tsv, any other name -> name +
    ".gene_coverage.tsv").  Adds the stats asj_exons (kept exon records, summed over chunks) and asj_coverage_genes (rows of the
    coverage file).
    annotation / exon_only: longcallR -a / --exon-only (main.rs:216-225, 436-438): a GTF / GFF3 (.gz) read by annotation.calling_annotation
    -- every `gene` and `CDS` line, no gene type filter; not the parser of the two tables above.  exon_only without annotation is a
    ValueError; annotation alone is parsed, so its errors surface, and changes nothing in any output.  With both, each contig's discovered
    regions (plain or truncated) are clipped to the clusters of overlapping genes (annotation.intersect_regions: a contig the file does not
    name loses its regions), a clipped region none of whose genes has a CDS is dropped before batching (thread.rs:88-91: no pileup, no
    record, no phased read), and every chunk hands its regions' CDS lists to Engine.set_exon_mask between binding and the pileup:
    candidates are called at CDS columns only, and a masked column does not count in the dense-cluster sweep either.  With input_vcf the
    regions are clipped and dropped all the same, but no mask is set: the imported sites outside CDS are phased (thread.rs:107-116).  The
    phased BAM tags the reads contained in a clipped region.  Adds the stats exon_regions (regions after clipping and dropping) and
    exon_skipped_regions (dropped for want of CDS); regions stays the number discovered.
    packed_upload: every chunk is cut with the bases left as the BAM's 4-bit codes (NativeBam.batch(packed=True)) and loaded through the
    asynchronous packed path (lcr_load_batch_packed_async: the nibbles cross the link, a kernel expands them in HBM).  Every output is
    byte for byte the one of a run without it.  Adds the stat upload_bytes_saved: n_bases - n_pack - 8 n_reads, summed over chunks.
    Off by default.
    haplotag: with input_vcf, keep the input's phase (`whatshap haplotag` on the fragment matrix; include/lcr.h: lcr_haplotag): the file
    is read with its alleles and PS (vcf.read_sites(alleles=True, phase_sets=True)), every chunk imports its sites as before and then
    calls Engine.haplotag with the contig's phased heterozygous SNVs inside its span (vcf.haplotag_sites) where phase() stands otherwise.
    Reads are tagged on the VCF's haplotypes with the VCF's phase sets -- the same labels in every region, gene and contig --, and the
    junction / expression tables and the phased BAM behind it are keyed by them, unchanged code.  The VCF writer, the expression and the
    junction-filter calls get min_phase_score = 0.0 in this mode: the phase is the input's, PQ is informational.  Per-gene expression
    records are merged with ase.merge_gene_records(shared_phase_sets=True): a phase set now spans regions (the junction tables are
    still merged per region: DESIGN.md section 1i).  Down-sampling does not apply to it.  Adds the stats haplotag_sites (candidates
    tagged with the input's phase) and haplotag_reads (fragment rows assigned).  haplotag without input_vcf is a ValueError.
    ase_sites_out / ase_sites_min_baseq: the per-site allele x haplotype table (include/lcr.h: lcr_site_counts; ase.format_sites_tsv),
    written to ase_sites_out: one row per VCF record of the run with the reference / alternate counts on haplotype 1, haplotype 2 and
    the other reads, the SNP-level imbalance test and the allele x haplotype Fisher test.  Every chunk calls Engine.site_counts right
    behind phase() / haplotag() and the other table calls; that call waits for the phase stage, like theirs.  Entries with a base
    quality below ase_sites_min_baseq are not counted (0 - 30, ValueError otherwise); ase_min_support and ase_overdispersion are the
    expression table's.  Adds the stat ase_sites (rows written).  No other output depends on it; without ase_sites_out nothing changes.
    hap_coverage_out: a path prefix for the per-haplotype coverage tracks (include/lcr.h: lcr_hap_coverage; coverage.py): the covered
    depth -- M, =, X and D columns, clipped to the region windows -- of the reads tagged HP 1, of those tagged HP 2 and of all other
    reads, as PREFIX.h1.bedgraph, PREFIX.h2.bedgraph and PREFIX.unassigned.bedgraph (contig, start, end, value; 0-based half-open, no
    header line; the .fai's contig order, then position; lines sorted and non-overlapping -- the writer raises ValueError otherwise).
    The labels are the HP tag's: behind lcr_phase "haplotype 1" is a label per phase set, so a track mixes the arbitrary labels of
    different sets; with haplotag=True it is the input VCF's haplotype 1 across the whole run.  Every chunk calls Engine.hap_coverage
    right behind phase() / haplotag() and the other table calls; that call waits for the phase stage, like theirs.  Adds the stats
    hap_coverage_segments (segments of all chunks) and hap_coverage_bases (covered bases of class 0, 1, 2: a 3-tuple).  No other output
    depends on it; without hap_coverage_out nothing changes.
    somatic_out / somatic_purity / somatic_min_baseq / somatic_min_score: the haplotype-resolved somatic calls (include/lcr.h:
    lcr_somatic; somatic.py), written to somatic_out: a VCF with the run's header plus the INFO tags SHP, H1 and H2, and one record per
    low-fraction site (LCR_F_CAND_SOMATIC behind the phase stage: printed 0/1 LowQual RDS=noselect in the main VCF) at which one
    haplotype reads "reference" and the other "somatic" at the given purity -- QUAL the candidate's, FILTER PASS when the score reaches
    somatic_min_score, else LowQual, INFO RDS=somatic;SHP=h;H1=ref,alt;H2=ref,alt, FORMAT GT:DP:AF:PS:SQ --, in contig then position
    order.  Every chunk calls Engine.somatic behind phase() / haplotag() and the other table calls; that call waits for the phase
    stage, like theirs.  Purity outside (0, 1] or a somatic_min_baseq outside 0 - 30 is a ValueError before any GPU work.  Adds the
    stats somatic_sites (flagged candidates evaluated with status OK) and somatic_calls.  No other output depends on it; without
    somatic_out nothing changes.
    isoforms_out / isoform_min_count / isoform_min_junctions: the allele-specific isoform table (include/lcr.h: lcr_isoforms;
    isoforms.format_tsv), written to isoforms_out: one row per intron chain that at least isoform_min_count tagged reads of a region hold
    exactly, with the reads per haplotype and the absent / present table of the reads that span the chain, tested like a junction's.
    Reads with fewer than isoform_min_junctions junctions take no part (at least 1: ValueError otherwise).  Every chunk calls
    Engine.isoforms behind phase() / haplotag() and the other table calls; that call waits for the phase stage, like theirs.  Adds the
    stats isoforms (kept records, summed over chunks) and isoform_reads (fragment rows that hold a kept chain).  No other output depends
    on it; without isoforms_out nothing changes.
    ends_out / ends_min_count / ends_window / ends_strand: the allele-specific transcript-end table (include/lcr.h: lcr_transcript_ends;
    ends.format_tsv), written to ends_out: one row per TSS / TES site -- a peak of the tagged reads' 5' or 3' ends that at least
    ends_min_count ends within ends_window columns are assigned to -- with the reads per haplotype and the absent / present table of the
    reads that end there or cover the site's window, tested like a junction's.  ends_strand: "ts" takes a read's transcript strand from
    its ts tag only, "read" from the read's own strand where the tag is missing (direct RNA).  ends_window above 4096 or another
    ends_strand is a ValueError before any GPU work.  Every chunk calls Engine.transcript_ends behind phase() / haplotag() and the other
    table calls; that call waits for the phase stage, like theirs.  Adds the stats end_sites (kept records, summed over chunks) and
    end_reads (ends assigned to a kept site).  No other output depends on it; without ends_out nothing changes.
    retention_out / retention_min_count / retention_anchor / retention_min_retained: the allele-specific intron-retention table
    (include/lcr.h: lcr_intron_retention; retention.format_tsv), written to retention_out: one row per intron that at least
    retention_min_count tagged reads of a region splice, with the tagged reads that splice it, retain it -- one aligned block covers the
    intron and retention_anchor columns on either side -- or do neither, the spliced / retained table per haplotype, tested like a
    junction's, and the percent-intron-retention per haplotype.  Written are the introns whose table sums to retention_min_count and
    whose retained cells sum to retention_min_retained.  A retention_anchor above 4096 or a negative value is a ValueError before any GPU
    work.  Every chunk calls Engine.intron_retention behind phase() / haplotag() and the other table calls; that call waits for the phase
    stage, like theirs.  Adds the stats retention_introns (kept records, summed over chunks) and retention_reads (fragment rows that
    retain a kept intron).  No other output depends on it; without retention_out nothing changes.
    indels_out / indel_min_count / indel_min_permille / indel_flank / indel_max_ins / indel_max_del: the phased small-indel calls
    (include/lcr.h: lcr_indels; indels.format_vcf), written to indels_out: a VCF with the run's header plus the tags HRUN, SHIFT, AD, HC
    and PV, and one record per kept event -- a normalised insertion of at most indel_max_ins (<= 12) or deletion of at most
    indel_max_del (<= 65535) bases that at least indel_min_count fragment rows of a region hold, and at least indel_min_permille per
    mille of the depth at its anchor base -- genotyped from the rows of each haplotype that hold it or cover it cleanly with indel_flank
    (<= 4096) columns on either side (indels.genotype).  A value outside its range is a ValueError before any GPU work.  Every chunk
    calls Engine.indels behind phase() / haplotag() and the other table calls; that call waits for the phase stage, like theirs.  Adds
    the stats indel_events (kept records, summed over chunks) and indel_calls (records written with PASS).  No other output depends on
    it; without indels_out nothing changes.
    pairs_out / pairs_partners / pairs_min_count / pairs_min_baseq: the read-backed check of the phase (include/lcr.h: lcr_site_pairs;
    pairs.format_pairs_tsv), written to pairs_out: one row per pair of phased het sites of eligible rank difference 1..pairs_partners
    (1..8; no distance limit) that at least pairs_min_count rows hold with both qualities >= pairs_min_baseq (0..30) -- the 2 x 2 table
    of their bases, the reads' own orientation (cis / trans / tie), whether the phase agrees, and a Fisher p-value.
    mnv_out / mnv_max_dist / mnv_min_count / mnv_min_frac: the multi-nucleotide variants (pairs.mnv_records), written to mnv_out as a
    second VCF with the run's header plus the tags SITES and RB: runs of two or three PASS calls of the main VCF at most mnv_max_dist
    (>= 1) apart, all 1/1 or all on one haplotype of one phase set, merged where at least mnv_min_count rows, and at least mnv_min_frac
    (0..1) of the rows with an ALT base at either site, carry the ALT base at both.  The main VCF keeps the constituent sites.  A value
    outside its range is a ValueError before any GPU work.  Every chunk calls Engine.site_pairs("phased", pairs_partners, 0,
    pairs_min_baseq) and / or Engine.site_pairs("all", 2, mnv_max_dist, pairs_min_baseq) behind phase() / haplotag() and the other table
    calls; the call waits for the phase stage, like theirs.  Adds the stats site_pairs (records, summed over chunks) and
    phase_disagreements (rows of the table whose phase is contradicted) with pairs_out, mnv_records with mnv_out.  No other output
    depends on them; without the two options nothing changes."""
    from concurrent.futures import ThreadPoolExecutor
    import threading
    truncation = bool(truncation)
    haplotag = bool(haplotag)
    if haplotag and input_vcf is None:
        raise ValueError("haplotag needs input_vcf: the phase to keep is the input VCF's")
    if ase_sites_out is not None and (isinstance(ase_sites_min_baseq, bool) or int(ase_sites_min_baseq) != ase_sites_min_baseq
                                      or not 0 <= int(ase_sites_min_baseq) <= 30):
        raise ValueError("ase_sites_min_baseq must be an integer in [0, 30] (the fragment matrix clamps qualities to 30), got %r" % (ase_sites_min_baseq,))
    if hap_coverage_out is not None and (not str(hap_coverage_out) or str(hap_coverage_out).endswith(os.sep)
                                         or not os.path.isdir(os.path.dirname(os.path.abspath(str(hap_coverage_out))))):
        raise ValueError("hap_coverage_out must be a path prefix in an existing directory (PREFIX.h1.bedgraph, ...), got %r" % (hap_coverage_out,))
    if somatic_out is not None:
        somatic.check_params(somatic_purity, 5e-6, 5e-4, somatic_min_baseq)
    if isoforms_out is not None:
        for what, v, least in (("isoform_min_count", isoform_min_count, 0), ("isoform_min_junctions", isoform_min_junctions, 1)):
            if isinstance(v, bool) or int(v) != v or not least <= int(v) < 1 << 32:
                raise ValueError("%s must be an integer in [%d, 2^32), got %r" % (what, least, v))
    if ends_out is not None:
        for what, v, most in (("ends_min_count", ends_min_count, (1 << 32) - 1), ("ends_window", ends_window, 4096)):
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= most:
                raise ValueError("%s must be an integer in [0, %d], got %r" % (what, most, v))
        if ends_strand not in ("ts", "read"):
            raise ValueError("ends_strand is 'ts' or 'read', got %r" % (ends_strand,))
    if retention_out is not None:
        for what, v, most in (("retention_min_count", retention_min_count, (1 << 32) - 1), ("retention_anchor", retention_anchor, 4096),
                              ("retention_min_retained", retention_min_retained, (1 << 32) - 1)):
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= most:
                raise ValueError("%s must be an integer in [0, %d], got %r" % (what, most, v))
    if indels_out is not None:
        for what, v, most in (("indel_min_count", indel_min_count, (1 << 32) - 1), ("indel_min_permille", indel_min_permille, (1 << 32) - 1),
                              ("indel_flank", indel_flank, 4096), ("indel_max_ins", indel_max_ins, 12), ("indel_max_del", indel_max_del, 65535)):
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= most:
                raise ValueError("%s must be an integer in [0, %d], got %r" % (what, most, v))
    if pairs_out is not None or mnv_out is not None:
        for what, v, least, most in (("pairs_partners", pairs_partners, 1, _abi.PAIRS_MAX_PARTNERS), ("pairs_min_count", pairs_min_count, 0, (1 << 32) - 1),
                                     ("pairs_min_baseq", pairs_min_baseq, 0, 30), ("mnv_max_dist", mnv_max_dist, 1, (1 << 32) - 1),
                                     ("mnv_min_count", mnv_min_count, 0, (1 << 32) - 1)):
            if isinstance(v, bool) or int(v) != v or not least <= int(v) <= most:
                raise ValueError("%s must be an integer in [%d, %d], got %r" % (what, least, most, v))
        if isinstance(mnv_min_frac, bool) or not 0.0 <= float(mnv_min_frac) <= 1.0:      # (NaN fails both comparisons)
            raise ValueError("mnv_min_frac must be a number in [0, 1], got %r" % (mnv_min_frac,))
    if exon_only and annotation is None:
        raise ValueError("exon_only is set, but annotation file is not provided")      # main.rs:436-438
    gene_clusters, gene_cds = _ann.calling_annotation(annotation) if annotation is not None else (None, None)
    if isinstance(truncation_coverage, bool) or int(truncation_coverage) != truncation_coverage or not 0 <= int(truncation_coverage) < 1 << 32:
        raise ValueError("truncation_coverage must be an integer in [0, 2^32) (the reference's u32), got %r" % (truncation_coverage,))
    truncation_coverage = int(truncation_coverage)
    params = _abi.make_params(preset, seed=seed, **param_overrides)
    downsample = bool(downsample) and downsample_depth > 0
    if downsample and not params.read_assign_cutoff > 0:    # (lcr_phase would answer LCR_E_ARG in the first chunk: include/lcr.h)
        raise ValueError("downsample=True needs read_assign_cutoff > 0 (preset %r has %r): an unsampled read's haplotag carries no sign, "
                         "pass e.g. read_assign_cutoff=1e-6" % (preset, float(params.read_assign_cutoff)))
    if ase_parental_vcf is not None and ase_dna_vcf is not None:
        raise ValueError("ase_parental_vcf and ase_dna_vcf are two modes of one table: give one of them")
    if ase_out is None and (ase_parental_vcf is not None or ase_dna_vcf is not None):
        raise ValueError("ase_parental_vcf / ase_dna_vcf need ase_out")
    if ase_out is None and ase_annotation is not None:
        raise ValueError("ase_annotation needs ase_out")
    if asj_out is None and asj_annotation is not None:
        raise ValueError("asj_annotation needs asj_out")
    asj_modes = bool(asj_cluster_with_exons) or asj_dna_vcf is not None or bool(asj_gene_coverage)
    if asj_modes and asj_annotation is None:
        raise ValueError("asj_cluster_with_exons / asj_dna_vcf / asj_gene_coverage need asj_annotation")
    if asj_annotation is not None and ase_annotation is not None and (
            os.path.abspath(str(asj_annotation)) != os.path.abspath(str(ase_annotation)) or tuple(asj_gene_types) != tuple(ase_gene_types)):
        raise ValueError("asj_annotation and ase_annotation must be the same file with the same gene types: a chunk has one gene assignment")
    fai = ref_path + ".fai"
    if not os.path.exists(fai):
        raise FileNotFoundError("Reference index file .fai does not exist.")   # util.rs:575-577
    contig_lengths = parse_fai(fai)
    refs = load_reference(ref_path)
    flt = dict(_abi.READ_FILTER)
    flt.update(read_filter or {})
    nb = bamio.NativeBam(bam_path, threads)
    bam_ids = {n: i for i, (n, _) in enumerate(nb.refs)}
    devices = list(devices) if devices else [device]
    engines = [api.Engine(d, params) for d in devices]
    if downsample:
        for e in engines:
            e.set_downsample(downsample_depth, downsample_seed)
    # a ctx is single-threaded (include/lcr.h): the producer thread below never touches a working engine -- region
    # discovery has a context of its own (its kernels share scratch buffers and a stream with nothing else)
    scout = api.Engine(devices[0], params)
    free = list(range(len(engines)))
    free_lock = threading.Condition()
    stats = dict(contigs=0, regions=0, reads=0, candidates=0, vcf_records=0, chunks=0)
    sites = None
    if input_vcf is not None:
        sites = vcf.read_sites(input_vcf, alleles=haplotag, phase_sets=haplotag)      # vcf.rs:400-462, once for the whole run (thread.rs:70-74)
        stats["input_sites"] = sum(int(v[0].size) for v in sites.values())
        stats["imported_sites"] = 0
    hap_sites = None
    if haplotag:        # {contig: (pos0, h1, h2, ps)}: the phased heterozygous SNVs
        hap_sites = {k: vcf.haplotag_sites(v) for k, v in sites.items()}
        sites = {k: v[:3] for k, v in sites.items()}
        stats["haplotag_sites"] = stats["haplotag_reads"] = 0
    min_ps = 0.0 if haplotag else params.min_phase_score    # (the input's phase is not second-guessed by PQ)
    if truncation:
        stats["truncated_columns"] = 0
    if exon_only:
        stats["exon_regions"] = stats["exon_skipped_regions"] = 0
    if packed_upload:
        stats["upload_bytes_saved"] = 0
    parental = ase.parental_sites(ase_parental_vcf) if ase_parental_vcf is not None else None    # {contig: (pos0, pat, mat)}
    dna = ase.dna_het_sites(ase_dna_vcf) if ase_dna_vcf is not None else None                    # {contig: pos0}
    genes = _ann.load(ase_annotation, ase_gene_types) if ase_annotation is not None else None   # {contig: _ann.ContigGenes}
    jgenes = None                                                                                      # the same for the junction table
    if asj_annotation is not None:
        jgenes = genes if genes is not None else _ann.load(asj_annotation, asj_gene_types)
    jdna = ase.dna_het_sites(asj_dna_vcf) if asj_dna_vcf is not None else None                   # {contig: pos0} for the junction table's filter
    no_sites = (np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.float32))

    # Every engine is a long-lived worker with the ASYNCHRONOUS phase stage (lcr_ctx_set_async_phase, include/lcr.h): a chunk is uploaded
    # into one of the context's two staging slots (lcr_load_batch_async + lcr_bind_batch: the device-resident form, which does not wait
    # for the stage in flight), its pileup is queued, THEN the previous chunk's results are collected (lcr_collect_phase: the getter that
    # outlives the binding) and turned into VCF text / read tags while this chunk's kernels run, then candidates / fragments / phase.
    results = {}            # chunk index -> dict(text, n_cand[, hp, ps, names])
    in_flight = [None] * len(engines)   # per engine: (chunk index, name, batch, want_reads, fragmat info, junction records, expression records, site records, coverage records, somatic records, isoform results, end-site results) of the chunk whose phase stage runs
    n_slot = [0] * len(engines)
    for E in engines:
        E.set_async_phase(async_phase)

    def finish(k):          # collect engine k's chunk in flight
        E = engines[k]
        idx, name, batch, want_reads, fm, junc, arec, srec, hcov, som, iso, tends, ret, ind, prs, mnv = in_flight[k]
        in_flight[k] = None
        res = E.collect_phase()
        cands = res["cand"]
        lines = vcf.format_records(cands, name, min_ps)
        out = dict(text=lines if isinstance(lines, str) else "".join(lines), n_cand=int(cands.size))
        if haplotag:
            out["hap"] = (int(np.count_nonzero(cands["haplotype"])), int(np.count_nonzero(res["assignment"])))
        if want_reads:
            asg = res["assignment"].astype(np.int32)
            # thread.rs:204-214: every for_phasing fragment has an assignment entry (0 / 1 / 2), a phase set only if set
            out["hp"] = np.where((fm["row_for_phasing"] != 0) | (asg != 0), asg, -1)
            out["ps"] = res["phase_set"].copy()
            out["names"] = _gather_names(batch.name_off, batch.name_blob, fm["row_read"].astype(np.int64))
        if junc is not None and asj_modes:      # Engine.asj_genes' dict
            out["junc"] = (name, junc["junc"], jgenes.get(name, _ann.ContigGenes())) + ((junc["exon"],) if asj_cluster_with_exons else ())
            out["asj_exons"], out["gene_reads"] = int(junc["exon"].size), junc["gene_reads"]
        elif junc is not None and jgenes is not None:
            out["junc"] = (name, junc, jgenes.get(name, _ann.ContigGenes()))
        elif junc is not None:
            out["junc"] = (name, junc, batch.start0, batch.len)
        if arec is not None and genes is not None:      # (region, gene) pair records; merged per gene when every chunk is in
            out["ase"] = (name, arec[0])
            if dna is not None:
                out["ase"] += (ase.filter_pairs(arec[0], cands, dna.get(name, np.zeros(0, np.int64)), min_ps,
                                                ase_min_support, ase_overdispersion),)
        elif arec is not None:
            out["ase"] = (name, arec, batch.start0, batch.len)
            if dna is not None:
                out["ase"] += (ase.filter_regions(arec, cands, dna.get(name, np.zeros(0, np.int64)), min_ps,
                                                  ase_min_support, ase_overdispersion),)
        if srec is not None:
            out["sites"] = (name, cands.copy(), srec)     # (cands is the context's buffer: the table is written when every chunk is in)
        if hcov is not None:
            out["hap_cov"] = (name, hcov[0], hcov[2])     # (Engine.hap_coverage copied them out of the context's buffers)
        if som is not None:     # (the candidates are those the call saw: it ran behind the settled phase stage)
            flagged = (cands["flags"] & _abi.F_CAND_SOMATIC) != 0
            out["somatic"] = (somatic.format_vcf_records(cands, som, name, somatic_min_score),
                              int(np.count_nonzero(flagged & (som["status"] == somatic.SOM_OK))), int(np.count_nonzero(som["call"])))
        if iso is not None:     # (Engine.isoforms copied them out of the context's buffers)
            out["iso"] = (name, iso[0], iso[2], batch.start0, batch.len, int(np.count_nonzero(iso[3] >= 0)))
        if tends is not None:   # (Engine.transcript_ends copied them out of the context's buffers)
            out["ends"] = (name, tends[0], batch.start0, batch.len, tends[3]["n_assigned"])
        if ret is not None:     # (Engine.intron_retention copied them out of the context's buffers)
            out["retention"] = (name, ret[0], batch.start0, batch.len, int(np.count_nonzero(ret[2] > 0)))
        if ind is not None:     # (Engine.indels copied them out of the context's buffers)
            out["indels"] = (name, ind[0], [indels.alleles(r, batch.start0, batch.col_off, batch.ref) for r in ind[0]])
        if prs is not None:     # (Engine.site_pairs copied them out of the context's buffers; cands is the context's buffer)
            out["pairs"] = (name, cands.copy(), prs[0])
        if mnv is not None:
            out["mnv"] = (name, _pairs.mnv_records(cands, mnv[0], mnv[1], refs[name], 0, min_ps, mnv_max_dist, mnv_min_count, mnv_min_frac, 2))
        results[idx] = out

    def work(idx, batch, name, want_reads, imp, mask, hs=None):   # one chunk on whichever engine is free (imp: its sites, or None: call candidates; mask: its CDS lists, or None; hs: its phased sites, or None: phase())
        with free_lock:
            while not free:
                free_lock.wait()
            k = free.pop()
        try:
            E = engines[k]
            slot = n_slot[k] & 1
            n_slot[k] += 1
            E.load_batch_async(batch, slot).bind_batch(slot)
            if genes is not None or jgenes is not None:     # one assignment per chunk, whichever table asks for it
                E.assign_genes((genes if genes is not None else jgenes).get(name))
            if mask is not None:
                E.set_exon_mask(*mask)
            E.fill_data_into_freq_vec()
            if in_flight[k] is not None:
                finish(k)
            if imp is None:
                E.get_candidate_snps()
            else:
                E.import_external_candidates(*imp)
            E.get_fragments()
            fm = None
            if want_reads:      # rows of the fragment matrix (read of every row, num_hete_links >= min_linkers): known before the phase stage
                f = E.fragmat()
                fm = dict(row_for_phasing=f["row_for_phasing"], row_read=f["row_read"])
            if hs is not None:
                E.haplotag(hs)
            else:
                E.phase()
            junc = None
            if asj_out is not None and asj_modes:
                dpos = None
                if jdna is not None:        # the contig's DNA sites inside the chunk's span (none when the VCF does not name the contig)
                    dp = jdna.get(name, np.zeros(0, np.int64))
                    lo, hi = np.searchsorted(dp, [int(batch.start0[0]), int(batch.start0[-1]) + int(batch.len[-1])])
                    dpos = dp[lo:hi]
                junc = E.asj_genes(jgenes.get(name), asj_min_count, asj_min_junctions, exons=bool(asj_cluster_with_exons), dna_pos0=dpos,
                                   coverage=bool(asj_gene_coverage), min_phase_score=min_ps)                                       # (waits for the phase stage)
            elif asj_out is not None and jgenes is not None:
                junc = E.junctions_genes(jgenes.get(name), asj_min_count, asj_min_junctions)[0]           # (waits for the phase stage)
            elif asj_out is not None:
                junc = E.junctions(asj_min_count, asj_min_junctions)[0]                                    # (waits for the phase stage)
            arec = None
            if ase_out is not None:
                psites = None
                if parental is not None:    # the contig's parental sites inside the chunk's span (none when the VCF does not name the contig)
                    pp, ppat, pmat = parental.get(name, (np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.uint8)))
                    lo, hi = np.searchsorted(pp, [int(batch.start0[0]), int(batch.start0[-1]) + int(batch.len[-1])])
                    psites = (pp[lo:hi], ppat[lo:hi], pmat[lo:hi]) if hi > lo else None
                arec = E.ase_genes(psites, min_phase_score=min_ps) if genes is not None else E.ase(psites, min_phase_score=min_ps)
            srec = E.site_counts(ase_sites_min_baseq) if ase_sites_out is not None else None                  # (waits for the phase stage)
            hcov = E.hap_coverage() if hap_coverage_out is not None else None                                 # (waits for the phase stage)
            som = E.somatic(purity=somatic_purity, min_baseq=somatic_min_baseq) if somatic_out is not None else None   # (waits for the phase stage)
            iso = E.isoforms(isoform_min_count, isoform_min_junctions) if isoforms_out is not None else None           # (waits for the phase stage)
            tends = E.transcript_ends(ends_min_count, ends_window, ends_strand) if ends_out is not None else None     # (waits for the phase stage)
            ret = E.intron_retention(retention_min_count, retention_anchor) if retention_out is not None else None   # (waits for the phase stage)
            ind = (E.indels(indel_min_count, indel_min_permille, indel_flank, indel_max_ins, indel_max_del)
                   if indels_out is not None else None)   # (waits for the phase stage)
            prs = E.site_pairs("phased", pairs_partners, 0, pairs_min_baseq) if pairs_out is not None else None   # (waits for the phase stage)
            mnv = E.site_pairs("all", 2, mnv_max_dist, pairs_min_baseq) if mnv_out is not None else None          # (waits for the phase stage)
            in_flight[k] = (idx, name, batch, want_reads, fm, junc, arec, srec, hcov, som, iso, tends, ret, ind, prs, mnv)
        finally:
            with free_lock:
                free.append(k)
                free_lock.notify()

    regions_out = []
    n_chunks = 0
    with ThreadPoolExecutor(max_workers=len(engines)) as pool:
        pending = []
        for name, length in contig_lengths:
            if contigs is not None and name not in contigs:
                continue
            if name not in bam_ids or name not in refs:
                continue
            rid = bam_ids[name]
            rs, re_ = nb.spans(rid, **flt)
            if rs.size == 0:
                continue
            regions = scout.discover_regions(rs, re_, length, truncation, truncation_coverage)     # util.rs:236-332
            if truncation:
                stats["truncated_columns"] += scout.last_truncated_columns
            if not regions:
                continue
            stats["contigs"] += 1; stats["regions"] += len(regions)
            cds_of = {}     # start0 of a clipped region -> its CDS list (clipped regions of a contig are disjoint)
            if exon_only:   # main.rs:221-224, thread.rs:80-92
                kept = []
                for s0, l0, q, ids in _ann.intersect_regions([r[0] for r in regions], [r[1] for r in regions], gene_clusters.get(name)):
                    iv = _ann.region_intervals(ids, gene_cds)
                    if iv:
                        kept.append((s0, l0, regions[q][2]))
                        cds_of[s0] = iv
                    else:
                        stats["exon_skipped_regions"] += 1
                regions = kept
                stats["exon_regions"] += len(regions)
                if not regions:
                    continue
            ref = refs[name]
            for chunk in chunk_regions(regions, max_cost=chunk_cost):
                wins = [ref[s:s + l] if s + l <= ref.size else np.concatenate([ref[s:], np.full(s + l - ref.size, ord("N"), np.uint8)])
                        for s, l, _ in chunk]
                batch = nb.batch(rid, [(s, l) for s, l, _ in chunk], wins, name_format="blob", packed=bool(packed_upload), **flt)
                stats["reads"] += batch.n_reads; stats["chunks"] += 1
                if packed_upload:
                    stats["upload_bytes_saved"] += batch.upload_bytes_saved()
                imp = None
                if sites is not None:       # thread.rs:108: a contig the VCF does not name gets no candidates
                    sp, sg, sq = sites.get(name, no_sites)
                    lo, hi = np.searchsorted(sp, [chunk[0][0], chunk[-1][0] + chunk[-1][1]])
                    imp = (sp[lo:hi], sg[lo:hi], sq[lo:hi])
                    stats["imported_sites"] += int(hi - lo)
                hs = None
                if hap_sites is not None:
                    hp_, h1_, h2_, hps_ = hap_sites.get(name, (np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint32)))
                    lo, hi = np.searchsorted(hp_, [chunk[0][0], chunk[-1][0] + chunk[-1][1]])
                    hs = (hp_[lo:hi], h1_[lo:hi], h2_[lo:hi], hps_[lo:hi])
                mask = None
                if exon_only and sites is None:     # (thread.rs:107-116: the imported sites get no mask)
                    ivs = [cds_of[s] for s, _, _ in chunk]
                    mask = (np.cumsum([0] + [len(v) for v in ivs], dtype=np.int64).astype(np.int32),
                            np.array([a for v in ivs for a, _ in v], np.int64), np.array([b for v in ivs for _, b in v], np.int64))
                while len(pending) > len(engines):     # bounded: at most one batch waiting per engine
                    pending.pop(0).result()
                pending.append(pool.submit(work, n_chunks, batch, name, out_bam is not None, imp, mask, hs))
                n_chunks += 1
                regions_out.extend((rid, s, l) for s, l, _ in chunk)
        for f in pending:
            f.result()
    for k in range(len(engines)):       # the last chunk of every engine
        if in_flight[k] is not None:
            finish(k)
    results = [results[i] for i in range(n_chunks)]
    for E in engines + [scout]:
        E.close()
    text = "".join(r["text"] for r in results)
    stats["candidates"] = sum(r["n_cand"] for r in results)
    if haplotag:
        stats["haplotag_sites"] = sum(r["hap"][0] for r in results)
        stats["haplotag_reads"] = sum(r["hap"][1] for r in results)
    stats["vcf_records"] = text.count("\n")
    write_vcf(out_vcf, contig_lengths, [text])
    if asj_out is not None:
        stats["junctions"] = sum(int(r["junc"][1].size) for r in results)
        if jgenes is not None:
            events = asj.gene_events([r["junc"] for r in results], asj_min_count)
            text, gene_text = asj.format_tsv_genes(None, events=events), asj.format_gene_tsv(None, events=events)
            stats["asj_genes"] = gene_text.count("\n") - 1
            asj_out = str(asj_out)
            with open(asj_out[:-len(".asj.tsv")] + ".asj_gene.tsv" if asj_out.endswith(".asj.tsv") else asj_out + ".gene.tsv", "w") as f:
                f.write(gene_text)
            if asj_modes:
                stats["asj_exons"] = sum(r["asj_exons"] for r in results)
            if asj_gene_coverage:
                cov = {}    # (contig, gene_id) -> reads, summed over the contig's chunks
                for r in results:
                    g = r["junc"][2]
                    for k, n in enumerate(r["gene_reads"].tolist()):
                        cov[(r["junc"][0], g.gene_id[k])] = cov.get((r["junc"][0], g.gene_id[k]), 0) + n
                rows = [(gname, c, s1, e1, cov.get((c, gid), 0)) for c, gid, gname, s1, e1 in _ann.gene_features(asj_annotation, asj_gene_types)]
                stats["asj_coverage_genes"] = len(rows)
                with open(asj_out[:-len(".asj.tsv")] + ".gene_coverage.tsv" if asj_out.endswith(".asj.tsv") else asj_out + ".gene_coverage.tsv", "w") as f:
                    f.write(asj.format_gene_coverage(rows))
        else:
            text = asj.format_tsv([r["junc"] for r in results], asj_min_count)
        with open(asj_out, "w") as f:
            f.write(text)
    if ase_out is not None and genes is not None:
        per_contig = {}     # contig -> its chunks' pair records (and masks), in chunk order
        for r in results:
            per_contig.setdefault(r["ase"][0], []).append(r["ase"][1:])
        tables = []
        for name, parts in per_contig.items():
            pairs = np.concatenate([x[0] for x in parts])
            if dna is not None:
                tables.append((name,) + ase.merge_gene_records(pairs, np.concatenate([x[1] for x in parts]), shared_phase_sets=haplotag))
            else:
                tables.append((name, ase.merge_gene_records(pairs, shared_phase_sets=haplotag)))
            tables[-1] = tables[-1][:2] + (genes.get(name, _ann.ContigGenes()),) + tables[-1][2:]
        text = ase.format_tsv(tables, ase_min_support, ase_overdispersion, patmat=parental is not None)
        stats["ase_genes"] = text.count("\n") - 1
        with open(ase_out, "w") as f:
            f.write(text)
    elif ase_out is not None:
        text = ase.format_tsv([r["ase"] for r in results], ase_min_support, ase_overdispersion, patmat=parental is not None)
        stats["ase_regions"] = text.count("\n") - 1
        with open(ase_out, "w") as f:
            f.write(text)
    if ase_sites_out is not None:
        text = ase.format_sites_tsv([r["sites"] for r in results], ase_min_support, ase_overdispersion, min_ps)
        stats["ase_sites"] = text.count("\n") - 1
        with open(ase_sites_out, "w") as f:
            f.write(text)
    if hap_coverage_out is not None:
        per_contig = {}     # contig -> its chunks' segments, in chunk order (= the .fai's contig order, then position)
        for r in results:
            per_contig.setdefault(r["hap_cov"][0], []).append(r["hap_cov"][1])
        w = coverage.TrackWriter(str(hap_coverage_out))
        try:
            for name, parts in per_contig.items():
                w.add_contig(name, np.concatenate(parts))
        finally:
            w.close()
        stats["hap_coverage_segments"] = w.segments
        stats["hap_coverage_bases"] = tuple(sum(int(r["hap_cov"][2]["bases"][:, k].sum()) for r in results) for k in range(3))
        if tuple(w.bases) != stats["hap_coverage_bases"]:      # (the lines' sum against the kernels' own per-region sums)
            raise ValueError("hap coverage: the tracks hold %r bases, the region records %r" % (tuple(w.bases), stats["hap_coverage_bases"]))
    if somatic_out is not None:
        stats["somatic_sites"] = sum(r["somatic"][1] for r in results)
        stats["somatic_calls"] = sum(r["somatic"][2] for r in results)
        write_vcf(somatic_out, contig_lengths, [r["somatic"][0] for r in results], somatic.INFO_LINES)
    if isoforms_out is not None:
        stats["isoforms"] = sum(int(r["iso"][1].size) for r in results)
        stats["isoform_reads"] = sum(r["iso"][5] for r in results)
        with open(isoforms_out, "w") as f:
            f.write(isoforms.format_tsv([r["iso"][:5] for r in results], isoform_min_count))
    if ends_out is not None:
        stats["end_sites"] = sum(int(r["ends"][1].size) for r in results)
        stats["end_reads"] = sum(r["ends"][4] for r in results)
        with open(ends_out, "w") as f:
            f.write(ends.format_tsv([r["ends"][:4] for r in results], ends_min_count))
    if retention_out is not None:
        stats["retention_introns"] = sum(int(r["retention"][1].size) for r in results)
        stats["retention_reads"] = sum(r["retention"][4] for r in results)
        with open(retention_out, "w") as f:
            f.write(retention.format_tsv([r["retention"][:4] for r in results], retention_min_count, retention_min_retained))
    if indels_out is not None:
        text, n_pass = indels.format_vcf([r["indels"] for r in results], [name for name, _ in contig_lengths])
        stats["indel_events"] = sum(int(r["indels"][1].size) for r in results)
        stats["indel_calls"] = n_pass
        write_vcf(indels_out, contig_lengths, [text], indels.INFO_LINES)
    if pairs_out is not None:
        text = _pairs.format_pairs_tsv([r["pairs"] for r in results], pairs_min_count, min_ps)
        stats["site_pairs"] = sum(int(r["pairs"][2].size) for r in results)
        stats["phase_disagreements"] = sum(1 for line in text.splitlines()[1:] if line.split("\t")[18] == "disagree")
        with open(pairs_out, "w") as f:
            f.write(text)
    if mnv_out is not None:
        text, stats["mnv_records"] = _pairs.format_mnv_vcf([r["mnv"] for r in results], [name for name, _ in contig_lengths])
        write_vcf(mnv_out, contig_lengths, [text], _pairs.INFO_LINES)
    if out_bam is not None:
        hp = np.concatenate([r["hp"] for r in results]) if results else np.zeros(0, np.int32)
        ps = np.concatenate([r["ps"] for r in results]) if results else np.zeros(0, np.uint32)
        offs, blobs, base = [np.zeros(1, np.uint64)], [], 0
        for r in results:
            o, bl = r["names"]
            offs.append(o[1:] + np.uint64(base)); blobs.append(bl)
            base += int(o[-1])
        name_off = np.concatenate(offs)
        blob = np.concatenate(blobs) if blobs else np.zeros(0, np.uint8)
        nb.write_phased(out_bam, regions_out, (name_off, blob), hp, ps, threads=threads)
    nb.close()
    return stats

#!/usr/bin/env python
"""BAM + reference FASTA (+ .fai) -> phased VCF (and phased BAM) on one MI355X: longcallr_amd.pipeline.run.

  python tools/run_pipeline.py -b reads.bam -f ref.fa -o out.vcf [--out-bam phased.bam] [-p hifi-masseq] [-c chr20,chr21]
                                 [-v known_snps.vcf.gz]   (phase these sites instead of calling candidates)
                                 [-v phased.vcf.gz --haplotag]   (keep the file's phase: tag reads on its haplotypes and phase sets)
                                 [--truncation [--truncation-coverage N]]   (split regions at columns deeper than N)
                                 [-a genes.gtf.gz --exon-only]   (call inside annotated genes, at CDS columns only)
                                 [--packed-upload]   (upload the BAM's 4-bit bases and unpack them on the GPU; same outputs)
                                 [--asj-out out.asj.tsv [--asj-min-count N] [--asj-min-junctions N]   (allele-specific junction table)
                                  [--asj-annotation genes.gtf.gz [--asj-gene-types protein_coding,lncRNA]]]   (... per annotated gene, + the gene file)
                                 [--ase-out out.ase.tsv [--ase-min-support N] [--ase-overdispersion R]
                                  [--ase-parental-vcf phased.vcf.gz | --ase-dna-vcf dna.vcf.gz]   (allele-specific expression table)
                                  [--ase-annotation genes.gtf.gz [--ase-gene-types protein_coding,lncRNA]]]   (... per annotated gene)
                                 [--ase-sites-out out.ase_sites.tsv [--ase-sites-min-baseq N]]   (allele x haplotype counts per VCF record)
                                 [--hap-coverage-out PREFIX]   (PREFIX.h1 / .h2 / .unassigned.bedgraph: covered depth per HP tag)
                                 [--somatic-out out.somatic.vcf [--somatic-purity P] [--somatic-min-baseq N] [--somatic-min-score S]]   (haplotype-resolved somatic calls at low-fraction sites)
                                 [--isoforms-out out.isoforms.tsv [--isoform-min-count N] [--isoform-min-junctions N]]   (allele-specific isoform table: haplotype x intron chain)
                                 [--pairs-out out.pairs.tsv [--pairs-partners K] [--pairs-min-count N] [--pairs-min-baseq N]]   (read-backed check of the phase: cis / trans rows per pair of phased sites)
                                 [--mnv-out out.mnv.vcf [--mnv-max-dist D] [--mnv-min-count N] [--mnv-min-frac F]]   (adjacent calls on one haplotype merged into multi-nucleotide variants)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longcallr_amd import pipeline  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-b", "--bam", required=True)
    ap.add_argument("-f", "--ref", required=True, help="FASTA with a .fai next to it")
    ap.add_argument("-o", "--out-vcf", required=True)
    ap.add_argument("--out-bam")
    ap.add_argument("-p", "--preset", default="hifi-masseq", choices=["hifi-isoseq", "hifi-masseq", "ont-cdna", "ont-drna"])
    ap.add_argument("-c", "--contigs", help="comma-separated subset")
    ap.add_argument("-t", "--threads", type=int, default=0, help="host threads of the BAM decoder / writer (0 = all)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("-v", "--input-vcf", help="user-provided candidate sites (VCF / .vcf.gz with GT): phased instead of called")
    ap.add_argument("--haplotag", action="store_true", help="keep the phase of -v: tag reads on the VCF's haplotypes and phase sets instead of phasing its sites again (needs -v)")
    ap.add_argument("--downsample", action="store_true", help="phase regions of at least --downsample-depth fragments on a sample of that many (needs --read-assign-cutoff > 0)")
    ap.add_argument("--downsample-depth", type=int, default=10000)
    ap.add_argument("--truncation", action="store_true", help="end a region at columns deeper than --truncation-coverage, as at uncovered ones")
    ap.add_argument("--truncation-coverage", type=int, default=200000)
    ap.add_argument("-a", "--annotation", help="GTF / GFF3 (.gz) annotation of --exon-only (its gene and CDS lines; sorted by start per contig)")
    ap.add_argument("--exon-only", action="store_true", help="clip the regions to the annotated genes and call candidates at CDS columns only (needs -a)")
    ap.add_argument("--packed-upload", action="store_true", help="upload the bases as the BAM's 4-bit codes and expand them on the GPU (outputs unchanged)")
    ap.add_argument("--asj-out", help="write the allele-specific junction table (longcallR-asj.py's .asj.tsv; regions in place of genes)")
    ap.add_argument("--asj-min-count", type=int, default=10, help="reads a junction needs to be kept, and a table needs to be written")
    ap.add_argument("--asj-min-junctions", type=int, default=2, help="a read takes part with MORE junctions than this")
    ap.add_argument("--asj-annotation", help="GTF / GFF3 (.gz) annotation: the junction table gets one row per (gene, junction) and the .asj_gene.tsv is written beside it")
    ap.add_argument("--asj-gene-types", default="protein_coding,lncRNA", help="comma-separated gene types kept from the annotation")
    ap.add_argument("--asj-cluster-with-exons", action="store_true", help="cluster junctions through the kept interior exons of the reads too (needs --asj-annotation)")
    ap.add_argument("--asj-dna-vcf", help="DNA VCF: count only reads whose phase set holds a DNA-heterozygous site (needs --asj-annotation)")
    ap.add_argument("--asj-gene-coverage", action="store_true", help="write the reads per gene beside the table (.gene_coverage.tsv; needs --asj-annotation)")
    ap.add_argument("--ase-out", help="write the allele-specific expression table (longcallR-ase.py's .ase.tsv; regions in place of genes)")
    ap.add_argument("--ase-min-support", type=int, default=10, help="assigned reads a region's phase set needs to be written")
    ap.add_argument("--ase-overdispersion", type=float, default=0.001, help="rho of the beta-binomial test")
    ap.add_argument("--ase-parental-vcf", help="whole-genome phased VCF (0|1: ALT paternal): adds the parent-of-origin votes (.patmat_ase.tsv)")
    ap.add_argument("--ase-dna-vcf", help="DNA VCF: keep the regions with a significant DNA-heterozygous site (.filter_ase.tsv)")
    ap.add_argument("--ase-annotation", help="GTF / GFF3 (.gz) annotation: the table gets one row per gene, reads assigned to genes on the GPU")
    ap.add_argument("--ase-gene-types", default="protein_coding,lncRNA", help="comma-separated gene types kept from the annotation")
    ap.add_argument("--ase-sites-out", help="write the per-site table: reference / alternate counts per haplotype at every VCF record, with --ase-min-support and --ase-overdispersion")
    ap.add_argument("--ase-sites-min-baseq", type=int, default=13, help="base quality an entry needs to be counted in --ase-sites-out (0 - 30)")
    ap.add_argument("--hap-coverage-out", metavar="PREFIX", help="write PREFIX.h1.bedgraph, PREFIX.h2.bedgraph and PREFIX.unassigned.bedgraph: the covered depth of the reads tagged HP 1, HP 2 and of all others")
    ap.add_argument("--somatic-out", help="write a VCF of the low-fraction sites at which one haplotype reads reference and the other somatic (FORMAT/SQ: the somatic score)")
    ap.add_argument("--somatic-purity", type=float, default=0.3, help="fraction of a somatic haplotype's reads that carry the allele, in (0, 1]")
    ap.add_argument("--somatic-min-baseq", type=int, default=0, help="base quality an entry needs to be counted in --somatic-out (0 - 30)")
    ap.add_argument("--somatic-min-score", type=float, default=0.0, help="records with a somatic score below it are LowQual")
    ap.add_argument("--isoforms-out", help="write the allele-specific isoform table: one row per intron chain held by enough tagged reads, with its haplotype x presence table")
    ap.add_argument("--isoform-min-count", type=int, default=10, help="reads that must hold a chain exactly for it to be kept, and a table needs to be written")
    ap.add_argument("--isoform-min-junctions", type=int, default=1, help="a read takes part with AT LEAST this many junctions (>= 1)")
    ap.add_argument("--ends-out", help="write the allele-specific transcript-end table: one row per TSS / TES site that enough tagged reads start or end at, with its haplotype x presence table")
    ap.add_argument("--ends-min-count", type=int, default=10, help="read ends a site needs to be kept, and a table needs to be written")
    ap.add_argument("--ends-window", type=int, default=10, help="columns around a peak whose ends belong to it (0 - 4096)")
    ap.add_argument("--ends-strand", choices=("ts", "read"), default="ts", help="transcript strand from the ts tag only, or from the read's own strand where the tag is missing (direct RNA)")
    ap.add_argument("--retention-out", help="write the allele-specific intron-retention table: one row per intron that enough tagged reads splice, with the reads that splice or retain it per haplotype")
    ap.add_argument("--retention-min-count", type=int, default=10, help="tagged reads that must splice an intron for it to be kept, and a table needs to be written")
    ap.add_argument("--retention-anchor", type=int, default=10, help="columns on either side of the intron a retaining read's aligned block must cover (0 - 4096)")
    ap.add_argument("--retention-min-retained", type=int, default=1, help="retaining reads a table needs to be written")
    ap.add_argument("--indels-out", help="write the phased small-indel calls: a VCF with one record per normalised insertion or deletion that enough reads of a region hold, genotyped per haplotype")
    ap.add_argument("--indel-min-count", type=int, default=10, help="reads that must hold an indel for it to be kept")
    ap.add_argument("--indel-min-permille", type=int, default=150, help="... and their share of the depth at its anchor base, per mille")
    ap.add_argument("--indel-flank", type=int, default=5, help="clean columns on either side of an indel's extent a read without it must cover (0 - 4096)")
    ap.add_argument("--indel-max-ins", type=int, default=12, help="longest insertion that is an event (0 - 12)")
    ap.add_argument("--indel-max-del", type=int, default=50, help="longest deletion that is an event (0 - 65535)")
    ap.add_argument("--pairs-out", help="write the read-backed check of the phase: a TSV with one row per pair of nearby phased het sites, the 2 x 2 table of the bases their shared reads carry, cis / trans, and whether the phase agrees")
    ap.add_argument("--pairs-partners", type=int, default=2, help="following phased sites every site is paired with (1 - 8)")
    ap.add_argument("--pairs-min-count", type=int, default=10, help="counted shared reads a pair needs for a row")
    ap.add_argument("--pairs-min-baseq", type=int, default=13, help="base quality both entries of a read need to be counted in --pairs-out / --mnv-out (0 - 30)")
    ap.add_argument("--mnv-out", help="write the multi-nucleotide variants: a second VCF with one record per run of two or three adjacent PASS calls on one haplotype (or all 1/1) that the reads carry together")
    ap.add_argument("--mnv-max-dist", type=int, default=2, help="largest distance of consecutive sites of a run (>= 1)")
    ap.add_argument("--mnv-min-count", type=int, default=3, help="reads that must carry the ALT base at both sites of every pair of a run")
    ap.add_argument("--mnv-min-frac", type=float, default=0.8, help="... and their share of the reads with an ALT base at either site (0 - 1)")
    ap.add_argument("--read-assign-cutoff", type=float, default=None, help="min_read_assignment_diff (preset: 0.0)")
    a = ap.parse_args()
    if a.haplotag and not a.input_vcf:
        ap.error("--haplotag needs -v / --input-vcf")
    if a.exon_only and not a.annotation:
        ap.error("--exon-only needs -a / --annotation")
    if a.ase_parental_vcf and a.ase_dna_vcf:
        ap.error("--ase-parental-vcf and --ase-dna-vcf are two modes of one table: give one of them")
    if (a.ase_parental_vcf or a.ase_dna_vcf) and not a.ase_out:
        ap.error("--ase-parental-vcf / --ase-dna-vcf need --ase-out")
    if a.ase_annotation and not a.ase_out:
        ap.error("--ase-annotation needs --ase-out")
    if not 0 <= a.ase_sites_min_baseq <= 30:
        ap.error("--ase-sites-min-baseq must lie in 0 - 30 (the fragment matrix clamps qualities to 30)")
    if a.hap_coverage_out is not None and (not a.hap_coverage_out or a.hap_coverage_out.endswith(os.sep)
                                           or not os.path.isdir(os.path.dirname(os.path.abspath(a.hap_coverage_out)))):
        ap.error("--hap-coverage-out takes a path prefix in an existing directory")
    if not (a.somatic_purity > 0.0 and a.somatic_purity <= 1.0):
        ap.error("--somatic-purity must lie in (0, 1]")
    if not 0 <= a.somatic_min_baseq <= 30:
        ap.error("--somatic-min-baseq must lie in 0 - 30 (the fragment matrix clamps qualities to 30)")
    if a.isoform_min_count < 0 or a.isoform_min_junctions < 1:
        ap.error("--isoform-min-count must be >= 0 and --isoform-min-junctions >= 1 (an unspliced read has no chain)")
    if a.ends_min_count < 0 or not 0 <= a.ends_window <= 4096:
        ap.error("--ends-min-count must be >= 0 and --ends-window lie in 0 - 4096")
    if a.retention_min_count < 0 or a.retention_min_retained < 0 or not 0 <= a.retention_anchor <= 4096:
        ap.error("--retention-min-count and --retention-min-retained must be >= 0 and --retention-anchor lie in 0 - 4096")
    if (not 1 <= a.pairs_partners <= 8 or a.pairs_min_count < 0 or not 0 <= a.pairs_min_baseq <= 30 or a.mnv_max_dist < 1 or a.mnv_min_count < 0
            or not 0.0 <= a.mnv_min_frac <= 1.0):
        ap.error("--pairs-partners must lie in 1 - 8, --pairs-min-baseq in 0 - 30 and --mnv-min-frac in 0 - 1, --mnv-max-dist be >= 1, --pairs-min-count and --mnv-min-count >= 0")
    if (a.indel_min_count < 0 or a.indel_min_permille < 0 or not 0 <= a.indel_flank <= 4096 or not 0 <= a.indel_max_ins <= 12
            or not 0 <= a.indel_max_del <= 65535):
        ap.error("--indel-min-count and --indel-min-permille must be >= 0, --indel-flank lie in 0 - 4096, --indel-max-ins in 0 - 12 and --indel-max-del in 0 - 65535")
    if a.asj_annotation and not a.asj_out:
        ap.error("--asj-annotation needs --asj-out")
    if (a.asj_cluster_with_exons or a.asj_dna_vcf or a.asj_gene_coverage) and not a.asj_annotation:
        ap.error("--asj-cluster-with-exons / --asj-dna-vcf / --asj-gene-coverage need --asj-annotation")
    extra = {} if a.read_assign_cutoff is None else dict(read_assign_cutoff=a.read_assign_cutoff)
    st = pipeline.run(a.bam, a.ref, a.out_vcf, a.out_bam, preset=a.preset, contigs=a.contigs.split(",") if a.contigs else None,
                      device=a.device, threads=a.threads, seed=a.seed, input_vcf=a.input_vcf,
                      downsample=a.downsample, downsample_depth=a.downsample_depth,
                      truncation=a.truncation, truncation_coverage=a.truncation_coverage,
                      asj_out=a.asj_out, asj_min_count=a.asj_min_count, asj_min_junctions=a.asj_min_junctions,
                      ase_out=a.ase_out, ase_min_support=a.ase_min_support, ase_overdispersion=a.ase_overdispersion,
                      ase_parental_vcf=a.ase_parental_vcf, ase_dna_vcf=a.ase_dna_vcf,
                      ase_annotation=a.ase_annotation, ase_gene_types=tuple(t for t in a.ase_gene_types.split(",") if t),
                      asj_annotation=a.asj_annotation, asj_gene_types=tuple(t for t in a.asj_gene_types.split(",") if t),
                      asj_cluster_with_exons=a.asj_cluster_with_exons, asj_dna_vcf=a.asj_dna_vcf, asj_gene_coverage=a.asj_gene_coverage,
                      annotation=a.annotation, exon_only=a.exon_only, packed_upload=a.packed_upload, haplotag=a.haplotag,
                      ase_sites_out=a.ase_sites_out, ase_sites_min_baseq=a.ase_sites_min_baseq, hap_coverage_out=a.hap_coverage_out,
                      somatic_out=a.somatic_out, somatic_purity=a.somatic_purity, somatic_min_baseq=a.somatic_min_baseq,
                      somatic_min_score=a.somatic_min_score,
                      isoforms_out=a.isoforms_out, isoform_min_count=a.isoform_min_count, isoform_min_junctions=a.isoform_min_junctions,
                      ends_out=a.ends_out, ends_min_count=a.ends_min_count, ends_window=a.ends_window, ends_strand=a.ends_strand,
                      retention_out=a.retention_out, retention_min_count=a.retention_min_count, retention_anchor=a.retention_anchor,
                      retention_min_retained=a.retention_min_retained,
                      indels_out=a.indels_out, indel_min_count=a.indel_min_count, indel_min_permille=a.indel_min_permille, indel_flank=a.indel_flank,
                      indel_max_ins=a.indel_max_ins, indel_max_del=a.indel_max_del,
                      pairs_out=a.pairs_out, pairs_partners=a.pairs_partners, pairs_min_count=a.pairs_min_count, pairs_min_baseq=a.pairs_min_baseq,
                      mnv_out=a.mnv_out, mnv_max_dist=a.mnv_max_dist, mnv_min_count=a.mnv_min_count, mnv_min_frac=a.mnv_min_frac, **extra)
    print(json.dumps(st))


if __name__ == "__main__":
    main()

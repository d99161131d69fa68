"""Gene annotation for the per-gene allele-specific tables: GTF / GFF3 -> per contig the arrays Engine.assign_genes takes
(include/lcr.h: lcr_gene_annotation).  Plain Python, gene-scale only: the read-scale work -- every read against every candidate gene's
exons -- is K8 on the GPU.

Restates get_gene_regions and merge_gene_exon_regions of allele_specific/longcallR-ase.py (:64-194):
  * lines that start with '#' are skipped; the feature is column 3, the attributes column 9;
  * GTF attributes are `key value` pairs split on ";" and then on " " (quotes dropped), repeated `tag` keys joined with ","; GFF3
    attributes are `key=value` pairs;
  * `gene` and `exon` features are kept iff gene_type (else gene_biotype) is one of gene_types and no tag contains "readthrough";
  * gene_name defaults to ".";
  * a gene whose exons lie on more than one contig is dropped;
  * per gene the exons of all its transcripts are merged when they share at least one base.  Abutting exons (end + 1 == next start)
    stay separate: the script calls intervaltree's merge_overlaps() with its default strict=True, which joins only intervals that
    overlap; that is the rule this project follows.

Coordinates leave this module 0-based half-open (a GTF's 1-based inclusive [a, b] is [a - 1, b)).  Genes of a contig are sorted by (span
start, span end, gene_id); that index is the gene's id in every per-gene result.  A gene that has exons but no kept `gene` feature
competes for reads as in the script and, as there, is never printed: reported is False.

For the per-gene junction table (longcallR-asj.py's get_gene_regions :106-116) every gene also keeps its annotated introns: per transcript
(transcript_id; exons without one form one nameless transcript of their gene) the exons sorted by start, every consecutive pair gives the
gap between them, kept when the script's 1-based intron_start < intron_end holds, i.e. when it is at least two bases long."""
import gzip

import numpy as np

GENE_TYPES = ("protein_coding", "lncRNA")
SUFFIXES = (".gff3", ".gtf", ".gff3.gz", ".gtf.gz")


class ContigGenes:
    """One contig's genes: span_start0 / span_end0 (first merged exon's start to last merged exon's end: what the script puts into its
    per-contig tree), exon_off (n_genes + 1) into exon_start0 / exon_end0 (merged exons, ascending and disjoint), gene_id / gene_name /
    strand (lists), reported (bool per gene), introns (per gene a frozenset of (start0, len): the annotated introns of its transcripts)."""

    def __init__(self, genes=()):
        genes = sorted(genes, key=lambda g: (g[1][0][0], g[1][-1][1], g[0]))   # (gene_id, exons, name, strand, reported[, transcripts])
        self.introns = [transcript_introns(g[5]) if len(g) > 5 else frozenset() for g in genes]
        self.gene_id = [g[0] for g in genes]
        self.gene_name = [g[2] for g in genes]
        self.strand = [g[3] for g in genes]
        self.reported = np.array([g[4] for g in genes], dtype=bool)
        self.span_start0 = np.array([g[1][0][0] for g in genes], dtype=np.int64)
        self.span_end0 = np.array([g[1][-1][1] for g in genes], dtype=np.int64)
        self.exon_off = np.zeros(len(genes) + 1, dtype=np.int32)
        np.cumsum([len(g[1]) for g in genes], out=self.exon_off[1:])
        self.exon_start0 = np.array([x for g in genes for x, _ in g[1]], dtype=np.int64)
        self.exon_end0 = np.array([y for g in genes for _, y in g[1]], dtype=np.int64)

    @property
    def n_genes(self):
        return len(self.gene_id)

    @classmethod
    def from_exons(cls, genes):
        """genes: [(gene_id, [(start0, end0), ...])] or [(gene_id, exons, gene_name, strand, reported)] or the same with a sixth entry, the
        gene's transcripts as a list of exon lists (the source of its annotated introns; without it the gene has none) -- exons in any
        order, merged here"""
        return cls([(g[0], merge_exons(g[1])) + (tuple(g[2:]) if len(g) > 2 else (".", ".", True)) for g in genes])


def transcript_introns(transcripts):
    """[[(start0, end0), ...] per transcript] -> frozenset of (start0, len): between consecutive exons of a transcript sorted by start (a
    stable sort, as the script's), gaps of at least two bases"""
    out = set()
    for exons in transcripts:
        ex = sorted(((int(x), int(y)) for x, y in exons), key=lambda e: e[0])
        for (_, y0), (x1, _) in zip(ex, ex[1:]):
            if x1 - y0 >= 2:     # 1-based inclusive [y0 + 1, x1]: intron_start < intron_end
                out.add((y0, x1 - y0))
    return frozenset(out)


def merge_exons(exons):
    """half-open exons of one gene -> ascending, disjoint; two are joined iff they share a base (abutting ones stay apart)"""
    out = []
    for x, y in sorted((int(x), int(y)) for x, y in exons):
        if out and x < out[-1][1]:
            out[-1][1] = max(out[-1][1], y)
        else:
            out.append([x, y])
    return [(x, y) for x, y in out]


def _attrs_gtf(text):
    d, tags = {}, []
    for attr in text.strip().split(";"):
        attr = attr.strip()
        if not attr:
            continue
        key, _, value = attr.partition(" ")
        value = value.replace('"', "")
        if key == "tag":
            tags.append(value)
        else:
            d[key] = value
    d["tag"] = ",".join(tags)
    return d


def _attrs_gff3(text):
    d = {}
    for attr in text.strip().split(";"):
        attr = attr.strip()
        if not attr:
            continue
        key, _, value = attr.partition("=")
        d[key] = value.replace('"', "")
    return d


def load(path, gene_types=GENE_TYPES):
    """-> {contig: ContigGenes}"""
    path = str(path)
    if not path.endswith(SUFFIXES):
        raise ValueError("unknown annotation file format (want .gtf, .gff3, .gtf.gz or .gff3.gz): %r" % path)
    parse = _attrs_gff3 if ".gff3" in path else _attrs_gtf
    gene_types = set(gene_types)
    genes = {}   # gene_id -> (name, strand) of the kept `gene` features
    exons = {}   # gene_id -> [(contig, start0, end0, transcript_id or None)]
    with (gzip.open if path.endswith(".gz") else open)(path, "rt") as f:
        for line in f:
            if line.startswith("#"):
                continue
            parts = line.strip().split("\t")
            if len(parts) < 9 or parts[2] not in ("gene", "exon"):
                continue
            a = parse(parts[8])
            if a.get("gene_type", a.get("gene_biotype")) not in gene_types or "readthrough" in a.get("tag", ""):
                continue
            if parts[2] == "gene":
                genes[a["gene_id"]] = (a.get("gene_name", "."), parts[6])
            else:
                exons.setdefault(a["gene_id"], []).append((parts[0], int(parts[3]) - 1, int(parts[4]), a.get("transcript_id")))
    per_contig = {}
    for gid, ex in exons.items():
        contigs = {e[0] for e in ex}
        if len(contigs) > 1:
            continue
        name, strand = genes.get(gid, (".", "."))
        transcripts = {}
        for _, x, y, tid in ex:
            transcripts.setdefault(tid, []).append((x, y))
        per_contig.setdefault(contigs.pop(), []).append((gid, merge_exons([(x, y) for _, x, y, _ in ex]), name, strand, gid in genes,
                                                         list(transcripts.values())))
    return {c: ContigGenes(g) for c, g in per_contig.items()}


def gene_features(path, gene_types=GENE_TYPES):
    """Every kept `gene` feature of the file, in file order, as (contig, gene_id, gene_name, start1, end1) with the line's own 1-based
    inclusive coordinates: the genes longcallR-asj.py lists in its .gene_coverage.tsv (:870-878, anno_gene_regions' order).  Kept as in
    load(): gene_type (else gene_biotype) in gene_types, no tag with "readthrough".  A gene_id seen twice keeps its first place and its
    last line (a dict).  A gene without exons is listed (nobody is assigned to it); a gene that has exons only takes reads and is not."""
    path = str(path)
    if not path.endswith(SUFFIXES):
        raise ValueError("unknown annotation file format (want .gtf, .gff3, .gtf.gz or .gff3.gz): %r" % path)
    parse = _attrs_gff3 if ".gff3" in path else _attrs_gtf
    gene_types = set(gene_types)
    genes = {}
    with (gzip.open if path.endswith(".gz") else open)(path, "rt") as f:
        for line in f:
            if line.startswith("#"):
                continue
            parts = line.strip().split("\t")
            if len(parts) < 9 or parts[2] != "gene":
                continue
            a = parse(parts[8])
            if a.get("gene_type", a.get("gene_biotype")) not in gene_types or "readthrough" in a.get("tag", ""):
                continue
            genes[a["gene_id"]] = (parts[0], a["gene_id"], a.get("gene_name", "."), int(parts[3]), int(parts[4]))
    return list(genes.values())

"""Gene annotation for the per-gene allele-specific tables: GTF / GFF3 -> per contig the arrays Engine.assign_genes takes
(include/lcr.h: lcr_gene_annotation) -- and, at the end of the file and with rules of its own, the calling annotation of --exon-only
(calling_annotation, intersect_regions, region_intervals).  Plain Python, gene-scale only: the read-scale work -- every read against every candidate gene's
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


# ---- the calling annotation of --exon-only (longcallR -a / --exon-only): another parser than the scripts' above ----------------------------
# Restates parse_annotation, intersect_gene_regions(merge = true) and the per-region CDS list of the reference (util.rs:334-556,
# thread.rs:80-92) as they are, oddities included:
#   * lines that start with '#' are skipped, every other line is split on tabs; only the features `gene` and `CDS` count, no gene type filter;
#   * a `gene` line first stores the CDS list collected so far under the CURRENT gene id, if it is not empty -- a plain insert: a gene id that
#     comes again replaces its earlier list --, then takes its id from the first attribute that starts with `gene_id=` (GFF3) or `gene_id `
#     (GTF, quotes trimmed); without one the previous gene's id stays.  Its span joins the contig's stack of clusters: behind the top
#     cluster's end (abutting included) it starts a new one, else it extends or lies inside the top one, whose id string grows by ",id";
#   * a `CDS` line must carry the current gene id and adds its interval to the list; the last list is stored at the end of the file.
# Coordinates leave this module 0-based half-open: a line's 1-based inclusive [a, b] is [a - 1, b).

def _calling_gene_id(attrs):
    for part in attrs.rstrip().split(";"):
        part = part.strip()
        if part.startswith("gene_id="):
            return part[len("gene_id="):]
        if part.startswith("gene_id "):
            return part[len("gene_id "):].strip('"')
    return None


def calling_annotation(path):
    """-> (clusters, cds): clusters = {contig: [(start0, end0, (gene_id, ...)), ...]} in file order, the merged gene spans with the ids of
    their genes (the reference's comma-joined id string, split on ","); cds = {gene_id: [(start0, end0), ...]} in file order, unmerged.
    Plain or .gz.  ValueError with the line's number for: a gene that starts in front of the top cluster of its contig ("annotation file is
    not sorted"), a CDS whose gene id is not the current gene's, a line without its five leading fields or with a start / end that is no
    unsigned integer (the reference panics on each)."""
    path = str(path)
    stacks, cds = {}, {}     # contig -> [[start0, end0, id string]]
    invs, gene_id = [], ""
    with (gzip.open if path.endswith(".gz") else open)(path, "rt") as f:
        for n, line in enumerate(f, 1):
            line = line.rstrip("\n")
            if line.startswith("#"):
                continue
            parts = line.split("\t")
            try:
                contig, feature, start, end = parts[0], parts[2], int(parts[3]), int(parts[4])
                if start < 0 or end < 0:
                    raise ValueError
            except (IndexError, ValueError):
                raise ValueError("%s line %d: not an annotation line (want tab-separated fields with an unsigned start and end)" % (path, n)) from None
            if feature not in ("gene", "CDS"):
                continue
            if len(parts) < 9:
                raise ValueError("%s line %d: a %s line without an attribute field" % (path, n, feature))
            if feature == "gene":
                if invs:
                    cds[gene_id] = invs
                    invs = []
                got = _calling_gene_id(parts[8])
                if got is not None:
                    gene_id = got
                stack = stacks.setdefault(contig, [])
                s0, e0 = start - 1, end
                if not stack:
                    stack.append([s0, e0, gene_id])
                    continue
                top = stack[-1]
                if s0 < top[0]:
                    raise ValueError("%s line %d: annotation file is not sorted. %s:%d-%d" % (path, n, contig, start, end))
                if top[1] <= s0:              # (the top's end is exclusive: abutting is no overlap)
                    stack.append([s0, e0, gene_id])
                else:
                    top[1] = max(top[1], e0)  # extends the top cluster, or lies inside it
                    top[2] += "," + gene_id
            else:
                got = _calling_gene_id(parts[8])
                if (got or "") != gene_id:
                    raise ValueError("%s line %d: gene_id in gene and exon are different: gene_id:%s, exon_gene_id:%s" % (path, n, gene_id, got or ""))
                invs.append((start - 1, end))
    if invs:
        cds[gene_id] = invs
    return {c: [(s, e, tuple(ids.split(","))) for s, e, ids in st] for c, st in stacks.items()}, cds


def intersect_regions(start0, length, clusters):
    """One contig's discovered regions against its clusters (calling_annotation()[0][contig], or None / [] for a contig the annotation does
    not name: it loses its regions).  start0 / length: the regions, in order.  -> [(start0, len, region index, ids)]: for every region q,
    in order, one clipped region per cluster h with h.start < q.end and h.end > q.start, in cluster order -- [max(starts), min(ends)) with
    h's ids; the region index says whose max_coverage it keeps."""
    out = []
    for q, (qs, ql) in enumerate(zip(start0, length)):
        qs, qe = int(qs), int(qs) + int(ql)
        for hs, he, ids in clusters or ():
            if hs < qe and he > qs:
                s, e = max(qs, hs), min(qe, he)
                out.append((s, e - s, q, ids))
    return out


def region_intervals(ids, cds):
    """thread.rs:80-92: the CDS list of a clipped region = the lists of its ids, one after the other (an id without a list gives nothing;
    an id named twice gives its list twice).  Empty: the region is skipped altogether."""
    out = []
    for gid in ids:
        out.extend(cds.get(gid, ()))
    return out

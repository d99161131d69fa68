"""The contract of lcr_asj_genes (include/lcr.h) restated loop for loop in plain Python over dicts, on top of
asj_genes_ref.py and in the script's OWN coordinates (1-based, first and last base inclusive): get_exon_intron_regions' exon arm as
written (asj_genes_ref.read_exon_regions), the interior-exon count of cluster_junctions_exons_connected_components (:388-404),
analyze_gene_with_filtering's two removals in the script's order (:781-806), the coverage dict of process_chunk / transform_read_assignment
(:231-272, :870-878), and the exon-aware graph (:405-431) as a plain adjacency walk with the project's "first junction" rule.  Stated
differences from the script: those of asj_genes_ref.py; zero-length M / D ops are dropped before the exon arm (the script can open an empty
block there); a phase set belongs to its region (the script keys rna_vcfs by PS value across contigs).  Like asj_genes_ref.py it is fed with
the GPU's own phasing results and gene map."""
import numpy as np

import ase_ref
import asj_genes_ref
import asj_ref
import genes_ref
from longcallr_amd import _abi


def read_exons(batch, i):
    """the read's exon_regions, 1-based inclusive (zero-length M / = / X / D ops dropped first: the stated deviation)"""
    return asj_genes_ref.read_exon_regions(int(batch.pos[i]), [(op, n) for op, n in genes_ref.cigartuples(batch, i) if not (op in (0, 7, 8, 2) and n == 0)])


def interior_exons(reads_exons, min_count):
    """:388-404 -> {(start, end): count}, thresholded"""
    exons = {}
    for read_name, exon_regions in reads_exons.items():
        if len(exon_regions) > 2:
            for i, exon_region in enumerate(exon_regions):
                if i == 0 or i == len(exon_regions) - 1:
                    continue
                exons[exon_region] = exons.get(exon_region, 0) + 1
    return {k: v for k, v in exons.items() if v >= min_count}


def analyze_gene_with_filtering(gene_exons, gene_reads, reads_positions, reads_tags, reads_exons, reads_introns, min_count, rna_vcfs, dna_vcfs):
    """asj_genes_ref.analyze_gene with the DNA removal in front of the exon removal (:781-806).  rna_vcfs: {phase set: [pos1]} of the
    region, dna_vcfs: a set of pos1, or None for no DNA filter.  -> analyze_gene's tuples"""
    sub_reads_positions = {name: reads_positions[name] for name in gene_reads}
    sub_reads_tags = {name: reads_tags[name] for name in gene_reads}
    sub_reads_exons = {name: reads_exons[name] for name in gene_reads}
    sub_reads_introns = {name: reads_introns[name] for name in gene_reads}
    junctions = {}
    for read_name, list_of_junctions in sub_reads_introns.items():
        for junction_region in list_of_junctions:
            junctions[junction_region] = junctions.get(junction_region, 0) + 1
    junctions = {k: v for k, v in junctions.items() if v >= min_count}
    intervalt = [(exon_start, exon_end + 1, None) for exon_start, exon_end in gene_exons]
    reads_to_remove = []
    if dna_vcfs is not None:
        for qname in sub_reads_tags.keys():
            phase_set = sub_reads_tags[qname][1]
            ps_variants = rna_vcfs.get(phase_set, []) if phase_set != 0 else []      # PS "." has no entry
            overlapped_snps_cnt = 0
            for snp in ps_variants:
                if snp in dna_vcfs:
                    overlapped_snps_cnt += 1
            if overlapped_snps_cnt == 0:
                reads_to_remove.append(qname)
    for qname, read_exons_ in sub_reads_exons.items():
        overlapped = False
        for exon_start, exon_end in read_exons_:
            if genes_ref.tree_overlap(intervalt, exon_start, exon_end + 1):
                overlapped = True
                break
        if not overlapped:
            reads_to_remove.append(qname)
    for qname in set(reads_to_remove):
        del sub_reads_positions[qname], sub_reads_exons[qname], sub_reads_introns[qname], sub_reads_tags[qname]
    out = []
    for junction_start, junction_end in sorted(junctions):
        absences, presents = asj_genes_ref.check_absent_present(junction_start, junction_end, sub_reads_positions, sub_reads_introns)
        counts = {}
        for present, names in ((0, absences), (1, presents)):
            for read_name in names:
                hap, ps = sub_reads_tags[read_name]
                counts.setdefault(ps, [0, 0, 0, 0])[(hap - 1) * 2 + present] += 1
        best = None
        for ps in sorted(counts):
            if best is None or sum(counts[ps]) > sum(counts[best]):
                best = ps
        cells = counts[best] if best is not None else [0, 0, 0, 0]
        out.append((junction_start, junction_end, junctions[(junction_start, junction_end)], best or 0, len(counts)) + tuple(cells))
    return out


def n_junctions(batch, i):
    return len(asj_ref.read_junctions(batch, i)[0])


def asj_genes(batch, row_region_off, row_read, assignment, phase_set, read_gene, genes, cands, cand_off, min_count=10, min_junctions=2,
              exons=False, dna_pos0=None, coverage=False, min_phase_score=0.0):
    """-> dict(junc, junc_region_off, exon, exon_region_off, gene_reads) as Engine.asj_genes returns them"""
    recs, off, xrecs, xoff = [], [0], [], [0]
    dna_vcfs = None if dna_pos0 is None else {int(p) + 1 for p in dna_pos0}
    for g in range(batch.n_regions):
        rna_vcfs = {}
        if dna_vcfs is not None:
            for i in range(int(cand_off[g]), int(cand_off[g + 1])):
                ps = int(cands["phase_set"][i])
                if ps and ase_ref.pass_phased_het(cands[i:i + 1], min_phase_score):
                    rna_vcfs.setdefault(ps, []).append(int(cands["pos"][i]) + 1)
        gene_assigned_reads = {}
        reads_positions, reads_tags, reads_exons, reads_introns = {}, {}, {}, {}
        for r in range(int(row_region_off[g]), int(row_region_off[g + 1])):
            a = int(assignment[r])
            if a not in (1, 2):
                continue
            i = int(row_read[r])
            js, rend = asj_ref.read_junctions(batch, i)
            if len(js) <= min_junctions:
                continue
            k = int(read_gene[i])
            if k < 0:
                continue
            gene_assigned_reads.setdefault(k, []).append(r)
            reads_positions[r] = (int(batch.pos[i]) + 1, rend)
            reads_tags[r] = (a, int(phase_set[r]))
            reads_exons[r] = read_exons(batch, i)
            reads_introns[r] = [(s + 1, s + l) for s, l in js]
        start0, length = int(batch.start0[g]), int(batch.len[g])
        win = bytes(batch.ref[int(batch.col_off[g]):int(batch.col_off[g + 1])]).upper()
        for k in sorted(gene_assigned_reads):
            gene_exons = [(int(genes.exon_start0[x]) + 1, int(genes.exon_end0[x])) for x in range(int(genes.exon_off[k]), int(genes.exon_off[k + 1]))]
            for js, je, n_reads, ps, n_sets, h1a, h1p, h2a, h2p in analyze_gene_with_filtering(
                    gene_exons, gene_assigned_reads[k], reads_positions, reads_tags, reads_exons, reads_introns, min_count, rna_vcfs, dna_vcfs):
                s, l = js - 1, je - js + 1
                motif, sl = 0, s - start0
                if l >= 2 and sl >= 0 and sl + l <= length:
                    pair = (win[sl:sl + 2], win[sl + l - 2:sl + l])
                    motif = 1 if pair == (b"GT", b"AG") else 2 if pair == (b"CT", b"AC") else 0
                recs.append((g, motif, [0, 0, 0], s, l, n_reads, ps, n_sets, h1a, h1p, h2a, h2p, k, 0))
            if exons:
                kept = interior_exons({r: reads_exons[r] for r in gene_assigned_reads[k]}, min_count)
                for es, ee in sorted(kept, key=lambda x: (x[0], x[1] - x[0])):
                    xrecs.append((g, k, es - 1, ee - es + 1, kept[(es, ee)]))
        off.append(len(recs))
        xoff.append(len(xrecs))
    gene_reads = None
    if coverage:
        n_genes = 0 if genes is None else len(genes.span_start0)
        gene_assigned = {}
        for i in range(batch.n_reads):
            if n_junctions(batch, i) <= min_junctions:
                continue
            k = int(read_gene[i])
            if k >= 0:
                gene_assigned.setdefault(k, []).append(i)
        gene_reads = np.array([len(gene_assigned.get(k, [])) for k in range(n_genes)], dtype=np.int32)
    return {"junc": np.array(recs, dtype=_abi.JUNC_GENE_DTYPE), "junc_region_off": np.array(off, dtype=np.int32),
            "exon": np.array(xrecs, dtype=_abi.EXON_GENE_DTYPE), "exon_region_off": np.array(xoff, dtype=np.int32), "gene_reads": gene_reads}


def cluster(junc, exons=None):
    """cluster_junctions_exons_connected_components' graph (:405-431) per (region, gene) pair as an adjacency walk, in the script's
    coordinates: junction node (s + 1, s + l), exon node (start - 1, end + 1) of the 1-based inclusive exon.  -> per junction the index
    of the first junction of its component (the project's rule)"""
    out = np.arange(len(junc), dtype=np.int64)
    pairs = {}
    for i in range(len(junc)):
        pairs.setdefault((int(junc["region"][i]), int(junc["gene"][i])), []).append(i)
    for key, idx in pairs.items():
        nodes = [(int(junc["start0"][i]) + 1, int(junc["start0"][i]) + int(junc["len"][i]), "junction", i) for i in idx]
        if exons is not None:
            for e in range(len(exons)):
                if (int(exons["region"][e]), int(exons["gene"][e])) == key:
                    s1, e1 = int(exons["start0"][e]) + 1, int(exons["start0"][e]) + int(exons["len"][e])
                    nodes.append((s1 - 1, e1 + 1, "exon", -1))
        adj = {n: [] for n in range(len(nodes))}
        for a in range(len(nodes)):
            for b in range(a + 1, len(nodes)):
                start1, end1, type1, _ = nodes[a]
                start2, end2, type2, _ = nodes[b]
                if type1 == type2:
                    edge = start1 == start2 or end1 == end2
                else:
                    edge = start1 == end2 or end1 == start2
                if edge:
                    adj[a].append(b)
                    adj[b].append(a)
        seen = set()
        for a in range(len(nodes)):
            if a in seen:
                continue
            comp, todo = [], [a]
            seen.add(a)
            while todo:
                x = todo.pop()
                comp.append(x)
                for y in adj[x]:
                    if y not in seen:
                        seen.add(y)
                        todo.append(y)
            members = sorted(nodes[x][3] for x in comp if nodes[x][2] == "junction")
            for i in members:
                out[i] = members[0]
    return out

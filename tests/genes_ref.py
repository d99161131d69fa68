"""The contract of lcr_assign_genes / lcr_ase_genes (include/lcr.h) restated loop for loop in plain Python, in the
script's OWN coordinates: assign_reads_to_gene of allele_specific/longcallR-ase.py (:197-258) with 1-based inclusive splice regions and
exons, and calculate_ase_pvalue / calculate_ase_pvalue_pat_mat per gene.  Plain lists stand where the script has interval trees; the two
predicates of the library it uses are written out in tree_overlap.  The GPU code works in 0-based half-open coordinates, so a test
against this file also checks that restatement.  The stated differences from the script: equally good genes go to the smallest gene
index, equally large phase sets to the smallest value.  This is the yardstick of the GPU tests."""
import numpy as np

import ase_ref
from longcallr_amd import _abi


def tree_overlap(intervals, begin, end):
    """IntervalTree.overlap(begin, end) over half-open intervals (b, e, data): nothing for an empty query (begin >= end), else every
    interval with b < end and e > begin"""
    if begin >= end:
        return []
    return [iv for iv in intervals if iv[0] < end and iv[1] > begin]


ALIGNED_OPS = (0, 2, 7, 8)   # M, D, =, X: what the script adds to a block; 3 (N) closes it; I, S, H, P pass


def splice_regions(start_pos, cigartuples):
    """The aligned blocks of a read as the script's CIGAR loop (:228-241) lists them: 1-based, first and last base inclusive.  `first`
    is the 1-based position of the open block's first base, `run` the bases gathered into it so far; every N, of whatever length,
    closes the block (listed only when it holds a base) and opens the next one behind the gap."""
    blocks = []
    first, run = start_pos + 1, 0
    for op, n in cigartuples:
        if op in ALIGNED_OPS:
            run += n
        elif op == 3:
            if run:
                blocks.append((first, first + run - 1))
            first, run = first + run + n, 0
    if run:
        blocks.append((first, first + run - 1))
    return blocks


def block_exon_bases(block, exon):
    """bases a 1-based inclusive block (a, b) shares with an exon's tree interval [lo, hi) = 1-based inclusive [lo, hi - 1], as the
    script counts them (:251); never negative"""
    a, b = block
    lo, hi = exon[0], exon[1]
    return max(0, min(b, hi - 1) - max(a, lo) + 1)


def script_trees(genes):
    """the per-contig tree of gene spans and the per-gene exon trees (:203-212) from the 0-based half-open arrays of one contig"""
    tree, gene_intervals = [], {}
    for k in range(len(genes.span_start0)):
        merged_exons = [(int(genes.exon_start0[i]) + 1, int(genes.exon_end0[i])) for i in range(int(genes.exon_off[k]), int(genes.exon_off[k + 1]))]
        gene_region = (merged_exons[0][0], merged_exons[-1][1])
        assert gene_region == (int(genes.span_start0[k]) + 1, int(genes.span_end0[k]))
        tree.append((gene_region[0], gene_region[1] + 1, k))
        gene_intervals[k] = [(s, e + 1, None) for s, e in merged_exons]
    return tree, gene_intervals


def assign_read(start_pos, cigartuples, tree, gene_intervals):
    """-> (gene index or -1, overlap)"""
    end_pos = start_pos + sum(l for op, l in cigartuples if op in (0, 2, 3, 7, 8))     # reference_end, 0-based exclusive
    candidate_gene_ids = sorted(iv[2] for iv in tree_overlap(tree, start_pos + 1, end_pos + 1))    # (the script: a set's order)
    regions = splice_regions(start_pos, cigartuples)
    best, best_len = -1, 0
    for gene_id in candidate_gene_ids:
        total = 0
        for block in regions:
            # the block's inclusive end goes into the query as an exclusive one, as in the script
            for exon in tree_overlap(gene_intervals[gene_id], block[0], block[1]):
                total += block_exon_bases(block, exon)
        if best < 0 or total > best_len:      # max(): the first of the largest
            best, best_len = gene_id, total
    return best, best_len


def cigartuples(batch, r):
    o, n = int(batch.cig_off[r]), int(batch.n_cig[r])
    return [(int(w) & 15, int(w) >> 4) for w in batch.cigar[o:o + n]]


def assign(batch, genes):
    """every read of a batch -> (gene int32, overlap uint32)"""
    n = 0 if genes is None else len(genes.span_start0)
    tree, gi = script_trees(genes) if n else ([], {})
    out = [assign_read(int(batch.pos[r]), cigartuples(batch, r), tree, gi) for r in range(batch.n_reads)]
    return np.array([g for g, _ in out], dtype=np.int32), np.array([o for _, o in out], dtype=np.uint32)


def pairs(fm, assignment, phase_set, cands, cand_off, read_gene, parental=None, min_baseq=13, min_phase_score=0.0):
    """ase_ref.regions per (region, gene): fm = Engine.fragmat(), read_gene = gene per read of the batch -> (records as _abi.AGENE_DTYPE,
    pair_region_off)"""
    rro, row_ptr, col, val, row_read = fm["row_region_off"], fm["row_ptr"], fm["col"], fm["val"], fm["row_read"]
    out, off = [], [0]
    for g in range(len(rro) - 1):
        gene_assigned_rows = {}
        for r in range(int(rro[g]), int(rro[g + 1])):
            k = int(read_gene[int(row_read[r])])
            if k >= 0:
                gene_assigned_rows.setdefault(k, []).append(r)
        for k in sorted(gene_assigned_rows):
            rows = gene_assigned_rows[k]
            phase_set_hap_count = {}
            for r in rows:
                ps, hp = int(phase_set[r]), int(assignment[r])
                if ps and hp in (1, 2):
                    phase_set_hap_count.setdefault(ps, {1: 0, 2: 0})[hp] += 1
            most = 0
            for ps in sorted(phase_set_hap_count):
                c = phase_set_hap_count[ps]
                if most == 0 or c[1] + c[2] > phase_set_hap_count[most][1] + phase_set_hap_count[most][2]:
                    most = ps
            rec = dict(region=g, phase_set=most, n_phase_sets=len(phase_set_hap_count), h1=0, h2=0, n_sites=0, h1_pat=0, h1_mat=0, h2_pat=0,
                       h2_mat=0, gene=k, pad_=0)
            if most:
                rec["h1"], rec["h2"] = phase_set_hap_count[most][1], phase_set_hap_count[most][2]
            if most and parental:
                site = {}
                for i in range(int(cand_off[g]), int(cand_off[g + 1])):      # no restriction to the gene's coordinates
                    s = cands[i:i + 1]
                    if int(s["phase_set"][0]) == most and ase_ref.pass_phased_het(s, min_phase_score) and int(s["pos"][0]) in parental:
                        site[i] = parental[int(s["pos"][0])]
                rec["n_sites"] = len(site)
                reads_pat_mat_cnt = {}
                for r in rows:
                    if int(phase_set[r]) != most or int(assignment[r]) not in (1, 2):
                        continue
                    for e in range(int(row_ptr[r]), int(row_ptr[r + 1])):
                        i, v = int(col[e]), int(val[e])
                        if i not in site or (v & 31) < min_baseq:
                            continue
                        base = "ACGT"[v >> 6]
                        cnt = reads_pat_mat_cnt.setdefault(r, {"pat": 0, "mat": 0})
                        if base == site[i][0]:
                            cnt["pat"] += 1
                        elif base == site[i][1]:
                            cnt["mat"] += 1
                for r, cnt in reads_pat_mat_cnt.items():
                    h = "h%d" % int(assignment[r])
                    if cnt["pat"] > cnt["mat"]:
                        rec[h + "_pat"] += 1
                    elif cnt["pat"] < cnt["mat"]:
                        rec[h + "_mat"] += 1
            out.append(tuple(rec[f] for f in _abi.AGENE_DTYPE.names))
        off.append(len(out))
    return np.array(out, dtype=_abi.AGENE_DTYPE), np.array(off, dtype=np.int32)


def genes_of(pair_records, keep=None):
    """ase.merge_gene_records restated with dicts: per gene the pair record with the most reads, ties to the smallest phase set, the
    numbers of phase sets summed -> [(record as a tuple[, keep])] in gene order"""
    per = {}
    for n, r in enumerate(pair_records.tolist()):
        per.setdefault(r[10], []).append((r, None if keep is None else bool(keep[n])))
    out = []
    for k in sorted(per):
        rs = per[k]
        chosen = sorted(rs, key=lambda x: (-(x[0][3] + x[0][4]), x[0][1]))[0]
        rec = list(chosen[0])
        rec[2] = sum(x[0][2] for x in rs)
        out.append(tuple(rec) if keep is None else (tuple(rec), chosen[1]))
    return out

"""TEST INFRASTRUCTURE ONLY -- CPU reference of down-sampled phasing (longcallR --downsample): oracle/oracle_np_phase.SNPFrag with the
methods that carry `apply_downsampling` in the Rust text (phase.rs:257-355, 810-976, 1298-1394; snpfrags.rs:191-376, 378-625) restated
with the extra test `apply && !fragment.downsampled`, and the call sequence of thread.rs:144-201.  init_assignment, phase (its
perturbation loop, phase.rs:1218-1225), divide_snps_into_blocks, get_fragments and assign_phase_set are inherited: the reference does
not filter them.  The sample itself follows the project's convention for rand (include/lcr.h: lcr_set_downsample): sample_rows()."""
import math

import numpy as np

from oracle import oracle_np as onp
from oracle import oracle_np_phase as onp2
from oracle.oracle_np_phase import _mix64, region_seed, M64


def sample_rows(seed, start0, n_rows, depth):
    """bytes (0 / 1) of a region with n_rows >= depth fragment rows: the `depth` rows with the smallest keys"""
    rs = region_seed(int(seed), int(start0))
    keys = [_mix64((rs + (r + 1) * 0x9E3779B97F4A7C15) & M64) for r in range(n_rows)]
    out = np.zeros(n_rows, np.uint8)
    out[np.argsort(np.array(keys, dtype=np.uint64), kind="stable")[:depth]] = 1
    return out


def batch_mask(seed, start0, row_region_off, depth):
    """(bytes per fragment row of a batch, per region whether it applies) under lcr_set_downsample(depth, seed)"""
    off = [int(x) for x in row_region_off]
    mask, applied = np.ones(off[-1], np.uint8), []
    for g in range(len(off) - 1):
        n = off[g + 1] - off[g]
        applied.append(depth > 0 and n > 0 and n >= depth)
        if applied[-1]:
            mask[off[g]:off[g + 1]] = sample_rows(seed, start0[g], n, depth)
    return mask, applied


class DSFrag(onp2.SNPFrag):
    apply = False      # apply_downsampling of the call in progress

    def _out(self, f):
        return self.apply and not f.downsampled

    def col_view(self, i):                                  # phase.rs:880-890
        sg, ps, pr = [], [], []
        for k in self.candidate_snps[i].snp_cover_fragments:
            f = self.fragments[k]
            if not f.for_phasing or f.haplotag == 0 or self._out(f):
                continue
            for fe in f.list:
                if fe.snp_idx == i and fe.phase_site:
                    ps.append(fe.p); pr.append(fe.prob); sg.append(f.haplotag)
        return sg, ps, pr

    def cal_overall_probability(self):                      # phase.rs:257-276
        logp = 0.0
        for f in self.fragments:
            if not f.for_phasing or f.haplotag == 0 or self._out(f):
                continue
            for fe in f.list:
                if fe.phase_site:
                    s = self.candidate_snps[fe.snp_idx]
                    logp += math.log10(onp.aki(f.haplotag, s.haplotype, s.genotype, fe.p, fe.prob))
        return logp

    def cross_optimize(self, conserved, keep_conserved, with_genotype):   # phase.rs:810-976 (+ check_new_*, 278-355)
        self.n_cross += 1
        hg_inc = h_inc = True
        num_iters = 0
        snps = self.candidate_snps
        while hg_inc or h_inc:
            tmp, logp, pre = {}, 0.0, 0.0
            for k, f in enumerate(self.fragments):
                if not f.for_phasing or f.haplotag == 0 or self._out(f):
                    continue
                d, e, ps, pr = self.row_view(k)
                if not d:
                    continue
                q = onp.cal_sigma_delta_eta_log(f.haplotag, d, e, ps, pr)
                qn = onp.cal_sigma_delta_eta_log(-f.haplotag, d, e, ps, pr)
                tmp[k] = -f.haplotag if q < qn else f.haplotag
                logp += qn if q < qn else q
                pre += q
            check = 1 if logp > pre else 0
            for k, h in tmp.items():
                self.fragments[k].haplotag = h
            if check == 0:
                h_inc = False
            else:
                h_inc = hg_inc = True
            tmp, logp, pre = {}, 0.0, 0.0
            for i, s in enumerate(snps):
                if not s.for_phasing or (keep_conserved and i in conserved):
                    continue
                sg, ps, pr = self.col_view(i)
                if not sg:
                    continue
                q1 = onp.cal_delta_eta_sigma_log(s.haplotype, 0, sg, ps, pr)
                q2 = onp.cal_delta_eta_sigma_log(-s.haplotype, 0, sg, ps, pr)
                q3 = onp.cal_delta_eta_sigma_log(s.haplotype, 1, sg, ps, pr)
                q4 = onp.cal_delta_eta_sigma_log(s.haplotype, -1, sg, ps, pr)
                cur = {0: q1, 1: q3, -1: q4}[s.genotype]
                if with_genotype:
                    mx = max(q1, max(q2, max(q3, q4)))
                    pick = ((s.haplotype, 0), q1) if q1 == mx else ((-s.haplotype, 0), q2) if q2 == mx else \
                        ((s.haplotype, 1), q3) if q3 == mx else ((s.haplotype, -1), q4)
                elif s.genotype == 0:
                    mx = max(q1, q2)
                    pick = ((s.haplotype, 0), q1) if q1 == mx else ((-s.haplotype, 0), q2)
                else:
                    mx = max(q3, q4)
                    pick = ((s.haplotype, 1), q3) if q3 == mx else ((s.haplotype, -1), q4)
                tmp[i] = pick[0]
                logp += pick[1]
                pre += cur
            check = 1 if logp > pre else 0
            for i, (h, gt) in tmp.items():
                snps[i].haplotype, snps[i].genotype = h, gt
            if check == 0:
                hg_inc = False
            else:
                hg_inc = h_inc = True
            num_iters += 1
            if num_iters > 20:
                break
        return self.cal_overall_probability()

    def cross_optimize_by_block(self):                      # phase.rs:1298-1394
        snps = self.candidate_snps
        tmp_hap, tmp_tag = {}, {}
        for block in self.ld_blocks:
            bset = set(block)
            db, dbf, eb, sb, sbf, psb, prb = [], [], [], [], [], [], []
            flip_map = {}
            for idx in block:
                db.append(snps[idx].haplotype); dbf.append(-snps[idx].haplotype); eb.append(snps[idx].genotype)
                sg, sgf, ps, pr = [], [], [], []
                for k in snps[idx].snp_cover_fragments:
                    f = self.fragments[k]
                    if not f.for_phasing or f.haplotag == 0 or self._out(f):
                        continue
                    flip_read = True
                    for fe in f.list:
                        if fe.snp_idx not in bset:
                            flip_read = False
                        if fe.snp_idx == idx:
                            if not fe.phase_site:
                                continue
                            ps.append(fe.p); pr.append(fe.prob)
                            t = -f.haplotag if flip_read else f.haplotag
                            sgf.append(t); flip_map[k] = t
                            sg.append(f.haplotag)
                sb.append(sg); sbf.append(sgf); psb.append(ps); prb.append(pr)
            q = onp2.sum_block(db, eb, sb, psb, prb)
            qf = onp2.sum_block(dbf, eb, sbf, psb, prb)
            if q < qf:
                for i, idx in enumerate(block):
                    tmp_hap[idx] = dbf[i]
                for k, f in enumerate(self.fragments):
                    tmp_tag[k] = flip_map.get(k, f.haplotag)
            else:
                for i, idx in enumerate(block):
                    tmp_hap[idx] = db[i]
                for k, f in enumerate(self.fragments):
                    tmp_tag[k] = f.haplotag
        for i, h in tmp_hap.items():
            snps[i].haplotype = h
        for k, h in tmp_tag.items():
            self.fragments[k].haplotag = h
        return self.cal_overall_probability()

    def _eval_rescue(self, lst, min_phase_score, low_frac):   # snpfrags.rs:191-376: the evidence loop is filtered, the commit loop is not
        snps = self.candidate_snps
        for ti in lst:
            s = snps[ti]
            if not s.snp_cover_fragments:
                s.single = True
                continue
            if s.variant_type != 1:
                s.non_selected = True
                continue
            sg, ps, pr = [], [], []
            h1 = h2 = 0
            for k in s.snp_cover_fragments:
                f = self.fragments[k]
                if self._out(f):
                    continue
                if not f.for_phasing or f.assignment == 0 or f.num_hete_links < self.min_linkers:
                    continue
                for fe in f.list:
                    if fe.snp_idx == ti:
                        if f.assignment == 1:
                            h1 += 1
                        elif f.assignment == 2:
                            h2 += 1
                        ps.append(fe.p); pr.append(fe.prob); sg.append(f.haplotag)
            if not sg or h1 < 2 or h2 < 2:
                s.single = True
                continue
            p1 = -10.0 * math.log10(1.0 - onp.cal_phase_score_log(1, 0, sg, ps, pr))
            p2 = -10.0 * math.log10(1.0 - onp.cal_phase_score_log(-1, 0, sg, ps, pr))
            s.single = False
            if max(p1, p2) >= float(min_phase_score):
                s.non_selected = False
                if low_frac:
                    s.cand_somatic = False
                s.rna_editing = False
                s.for_phasing = True
                for k in s.snp_cover_fragments:
                    f = self.fragments[k]
                    f.for_phasing = True
                    if f.haplotag == 0 or f.assignment == 0:
                        f.haplotag = -1 if self.rnd() < 0.5 else 1
                s.haplotype = 1 if p1 >= p2 else -1
                s.genotype, s.variant_type, s.phase_score = 0, 1, max(p1, p2)
            else:
                s.non_selected = True
                if low_frac:
                    s.cand_somatic = True
                    s.for_phasing = False
                else:
                    s.rna_editing = True

    def assign_snp_haplotype_genotype(self):                # snpfrags.rs:378-546
        for ti, s in enumerate(self.candidate_snps):
            if not s.for_phasing:
                s.non_selected = True
                continue
            if not s.snp_cover_fragments:
                s.single = True
                continue
            d = s.haplotype
            sg, ps, pr = [], [], []
            h1 = h2 = 0
            for k in s.snp_cover_fragments:
                f = self.fragments[k]
                if self._out(f):
                    continue
                if not f.for_phasing or f.num_hete_links < self.min_linkers:
                    continue
                if s.variant_type == 1 and f.assignment == 0:
                    continue
                for fe in f.list:
                    if fe.snp_idx == ti:
                        if f.assignment == 1:
                            h1 += 1
                        elif f.assignment == 2:
                            h2 += 1
                        ps.append(fe.p); pr.append(fe.prob); sg.append(f.haplotag)
            if not sg:
                s.non_selected = True
                continue
            q1 = onp.cal_delta_eta_sigma_log(d, 0, sg, ps, pr)
            q2 = onp.cal_delta_eta_sigma_log(-d, 0, sg, ps, pr)
            q3 = onp.cal_delta_eta_sigma_log(d, 1, sg, ps, pr)
            q4 = onp.cal_delta_eta_sigma_log(d, -1, sg, ps, pr)
            mx = max(q1, max(q2, max(q3, q4)))
            if q1 == mx:
                s.haplotype, s.genotype, s.variant_type = d, 0, 1
            elif q2 == mx:
                s.haplotype, s.genotype, s.variant_type = -d, 0, 1
            elif q3 == mx:
                s.haplotype, s.genotype, s.variant_type = d, 1, 0
            elif q4 == mx:
                s.haplotype, s.genotype = d, -1
                if s.variant_type not in (2, 3):
                    s.variant_type = 2
            else:
                raise ArithmeticError("genotype optimization failed")
            if s.genotype != 0:
                s.non_selected = True
                continue
            if sg and h1 >= 1 and h2 >= 1:
                s.phase_score = -10.0 * math.log10(1.0 - onp.cal_phase_score_log(s.haplotype, s.genotype, sg, ps, pr))
            else:
                s.phase_score = 0.19940219

    def assign_reads_haplotype(self, cutoff):               # snpfrags.rs:548-625
        snps = self.candidate_snps
        for f in self.fragments:
            if not f.for_phasing or self._out(f):
                continue
            d, e, ps, pr = [], [], [], []
            for fe in f.list:
                s = snps[fe.snp_idx]
                if not fe.phase_site and s.for_phasing:
                    fe.phase_site = True
                if not s.for_phasing or s.haplotype == 0 or s.genotype != 0:
                    continue
                ps.append(fe.p); pr.append(fe.prob); d.append(s.haplotype); e.append(s.genotype)
            if f.haplotag == 0 or not d:
                f.assignment = f.haplotag = 0
                continue
            q = onp.cal_sigma_delta_eta_log(f.haplotag, d, e, ps, pr)
            qn = onp.cal_sigma_delta_eta_log(-f.haplotag, d, e, ps, pr)
            if abs(q - qn) >= cutoff:
                if q >= qn:
                    f.assignment = 1 if f.haplotag == 1 else 2
                elif f.haplotag == 1:
                    f.assignment, f.haplotag = 2, -1
                else:
                    f.assignment, f.haplotag = 1, 1
            else:
                f.assignment = f.haplotag = 0


def run_region(batch, g, prm, cands, depth=0, seed=2025, rows=None):
    """thread.rs:136-201 for region g with --downsample-depth `depth` (0 = off), or with the explicit sample `rows` (bytes per fragment row
    of the region).  Returns (SNPFrag, read -> phase set, apply_downsampling)."""
    F = dict(edit=1, dense=2, het=4, fp=8, hom=16, single=32, nonsel=64, som=128)
    snps = [onp2.Snp(int(c["pos"]), chr(c["ref_base"]), (chr(c["allele1"]), chr(c["allele2"])), (float(c["af1"]), float(c["af2"])),
                     int(c["variant_type"]), int(c["genotype"]), bool(c["flags"] & F["edit"]), bool(c["flags"] & F["dense"]),
                     bool(c["flags"] & F["fp"]), bool(c["flags"] & F["hom"]), bool(c["flags"] & F["som"]), float(c["phase_score"]))
            for c in cands]
    sf = DSFrag(snps, int(prm.min_linkers), int(prm.seed), int(batch.start0[g]))
    sf.get_fragments(batch, g)
    n = len(sf.fragments)
    if rows is not None:
        rows = np.asarray(rows, np.uint8)
        assert rows.size == n
        apply = bool((rows == 0).any())
    else:
        apply = depth > 0 and n > 0 and n >= depth                          # thread.rs:144-146
        rows = sample_rows(seed, int(batch.start0[g]), n, depth) if apply else np.ones(n, np.uint8)
    for f, b in zip(sf.fragments, rows.tolist()):
        f.downsampled = bool(b)
    sf.sampled = rows
    if not snps:
        return sf, {}, apply
    sf.apply = apply
    sf.init_haplotypes()
    sf.init_assignment()
    sf.phase(1, int(prm.max_enum_snps))
    cut = float(prm.read_assign_cutoff)
    sf.assign_reads_haplotype(cut); sf.assign_snp_haplotype_genotype()
    sf.assign_reads_haplotype(cut); sf.assign_snp_haplotype_genotype()
    relaxed = float(prm.min_phase_score) - 3.0
    sf.eval_rna_edit_var_phase(relaxed)
    sf.eval_low_frac_var_phase(relaxed)
    sf.apply = False                                                        # thread.rs:181-182: the third round is called with `false`
    sf.assign_reads_haplotype(cut); sf.assign_snp_haplotype_genotype()
    read_ps = sf.assign_phase_set(float(prm.min_phase_score))
    return sf, read_ps, apply


def summary(sf, read_ps):
    """the fields the parity tests compare, as plain values"""
    return dict(tag=[f.haplotag for f in sf.fragments], asg=[f.assignment for f in sf.fragments],
                ps=[read_ps.get(k, 0) for k in range(len(sf.fragments))],
                snp=[(s.haplotype, s.genotype, s.variant_type, s.phase_set, s.rna_editing, s.dense, s.for_phasing, s.hom_var, s.single,
                      s.non_selected, s.cand_somatic, s.phase_score) for s in sf.candidate_snps],
                obj=getattr(sf, "objective", None))

"""Builds liblcr.so (HIP, gfx950 only) in-tree with hipcc. No fallbacks, no other targets."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "liblcr.so")
SOURCES = ["k0_ops.hip", "k0_unpack.hip", "k1_pileup.hip", "k2_candidates.hip", "k2_import.hip", "k2_exon.hip", "k3_fragments.hip", "k4_phase.hip", "k4_enum.hip", "k4_stage.hip", "k4_sample.hip", "k4_post.hip", "k4_grid.hip", "k5_regions.hip", "k6_junctions.hip", "k7_ase.hip", "k8_genes.hip", "k9_gene_junctions.hip", "k10_asj_modes.hip", "lcr_api.hip", "lcr_batch.hip", "lcr_pileup.hip", "lcr_calls.hip", "lcr_junctions.hip", "lcr_ase.hip", "lcr_genes.hip", "lcr_junctions_genes.hip", "lcr_asj_genes.hip",
           "lcr_bam.cpp", "lcr_vcf.cpp",   # lcr_bam.cpp / lcr_vcf.cpp: host-only BGZF / BAM decode and VCF reader (zlib)
           "k11_haplotag.hip", "lcr_haplotag.hip",
           "k12_site_counts.hip", "lcr_site_counts.hip",
           "k13_hap_coverage.hip", "lcr_hap_coverage.hip",
           "k14_somatic.hip", "lcr_somatic.hip",
           "k15_isoforms.hip", "lcr_isoforms.hip",
           "k16_ends.hip", "lcr_ends.hip",
           "k17_retention.hip", "lcr_retention.hip",
           "k18_indels.hip", "lcr_indels.hip",
           "k19_site_pairs.hip", "lcr_site_pairs.hip"]   # (new units go to the end: the link order moves the bench line)
HEADERS = ["lcr_dev.h", "k0_unpack.h", "lcr_ctx.h", "lcr_phase_host.h", "k4_dev.h", "k4_types.h", "k4_grid.h", "k4_grid_batch.h", "k4_kernels.h", "k4_post.h", "k2_eval.h", "k7_sweep.h", "lcr_asj_args.h", "k13_hap_coverage.h", "k6_walk.h", "k18_walk.h", "col_segments.h", os.path.join("..", "..", "include", "lcr.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall",
         "-Wno-unused-function"]


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force=False, verbose=False):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(CSRC, "build")
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs, procs = [], []
    for src in SOURCES:
        obj = os.path.join(objdir, os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        if force or _stale(obj, [os.path.join(CSRC, src)] + hdrs):
            cmd = [hipcc] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (src, out.decode()))
        if verbose and out:
            print(out.decode(), file=sys.stderr)
    if force or procs or _stale(SO, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", SO] + objs + ["-lz"]
        subprocess.check_call(cmd)
    return SO


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))

"""decodes the census slots of a measurement build from lines "... HIP tie census {...}" on stdin (tools/tie_check.py prints one)
  prof_decode.py          -DENUM_PROF build: the slowest workgroup of k4_enum_resolve up to each of its phases
  prof_decode.py steps    -DENUM_PROF=2 build: sigma / delta steps the restart kernels executed and skipped, weighted by the regions' phase entries"""
import sys,re,ast
steps = len(sys.argv) > 1 and sys.argv[1] == "steps"
for line in sys.stdin:
    if "HIP tie census" in line:
        d=ast.literal_eval(line.split("census",1)[1].strip())
        v=list(d.values())
        if steps:
            for name, o in (("k4_enum_bits", 0), ("k4_enum_reg", 4)):
                se, ss, de, ds = v[o:o + 4]
                tot = se + ss + de + ds
                if tot:
                    print("%-13s sigma steps: executed %d skipped %d | delta steps: executed %d skipped %d | executed share %.3f (skipped %.3f)" % (name, se, ss, de, ds, (se + de) / tot, (ss + ds) / tot))
            continue
        print("pts(us):",[x/100 for x in v[:7]], "worst: total %.1f us chunks %.1f us local %.1f us full_sum %.1f us"%((v[7]>>44)/100, ((v[7]>>24)&0xfffff)/100, ((v[7]>>12)&4095)*0.16, (v[7]&4095)*0.16))

#!/usr/bin/env python3
"""Compares two gfx950 listings of rt_kernels.hip (make -C raytracer-in-cpp_amd/csrc isa, one at each commit) kernel by kernel: the
.amdhsa_kernel names and their order, and every function's instruction stream with comments stripped and the function's index taken out
of its local labels (.LBB<index>_<block>: the index shifts for every function behind a kernel that came or went).  With the two compiler logs
(-Rpass-analysis=kernel-resource-usage, the stderr of the same command) it prints the resource lines of the kernels that changed.
usage: python tools/isa_diff.py OLD.s NEW.s [OLD.log NEW.log]      exit status 1: the kernel sets or their order differ"""
import re, subprocess, sys

def listing(path):
    order, body, cur = [], {}, None
    for ln in open(path):
        m = re.match(r"(_Z\w+):", ln)
        if m:
            cur = body.setdefault(m.group(1), [])
        elif ln.startswith(".Lfunc_end"):
            cur = None
        elif ln.lstrip().startswith(".amdhsa_kernel "):
            order.append(ln.split()[1])
        elif cur is not None:
            ln = ln.split(";")[0].strip()
            if ln:
                cur.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
    return order, body

def resources(path):
    rows, cur = {}, None
    for ln in open(path):
        m = re.search(r"remark:\s+(.*?):\s+(.*?) \[-Rpass", ln)
        if m and m.group(1).strip() == "Function Name":
            cur = rows.setdefault(m.group(2).strip(), [])
        elif m and cur is not None:
            cur.append(m.group(2).strip())
    return rows          # SGPRs, VGPRs, AGPRs, scratch, dynamic stack, occupancy, SGPR spills, VGPR spills, LDS

def short(name):
    d = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    return d.replace("void rtamd::", "").replace("rtamd::", "").split("(")[0]

(o_order, o_body), (n_order, n_body) = listing(sys.argv[1]), listing(sys.argv[2])
res = [resources(p) for p in sys.argv[3:5]]
print(f"kernels: {len(o_order)} -> {len(n_order)}, same names in the same order: {o_order == n_order}")
for k in sorted(set(o_order) ^ set(n_order)):
    print(("  only in NEW: " if k in n_body else "  only in OLD: ") + short(k))
changed = [k for k in n_order if k in o_body and o_body[k] != n_body[k]]
print(f"instruction streams that differ: {len(changed)}")
for k in changed:
    print(f"  {short(k):56s} {len(o_body[k]):6d} -> {len(n_body[k]):6d} lines")
    for r in res:
        print("      sgpr/vgpr/agpr/scratch/dyn/occ/sspill/vspill/lds: " + " ".join(r.get(k, ["?"])))
sys.exit(0 if o_order == n_order else 1)

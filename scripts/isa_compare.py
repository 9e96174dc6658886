#!/usr/bin/env python3
"""Compare two gfx950 assembly listings of one source file function by function.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S x.hip -o x.s   (both trees)
    scripts/isa_compare.py parent/x.s tree/x.s [name-substring [lines]]

For every function: the .amdhsa_ block and the instruction text, labels renumbered by first
appearance, comments dropped. Template instances pair by demangled name with the streaming
counters' parameter type read as the u32 pointer it replaced. For each function whose text
differs it prints the resources of both sides (VGPR, AGPR, SGPR, scratch, SGPR and VGPR
spills, static LDS, occupancy). With a name substring: the unified diff of those functions.
"""
import collections
import difflib
import re
import subprocess
import sys

FIELDS = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def role(d):
    return d.replace("ajx::StreamCounters*", "unsigned int*").replace("stream_fin_list_call", "stream_fin_list")


def parse(path):
    funcs, hsa, info, spills = collections.OrderedDict(), {}, {}, {}
    cur = curh = last = name = None
    for line in open(path):
        s = line.rstrip("\n")
        m = re.match(r"^(_Z\w+):", s)
        if m:
            cur = last = m.group(1)
            funcs[cur] = []
            info[cur] = {}
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^; (\w+): (\d+)", s)
        if m and last and cur is None and m.group(1) in FIELDS:
            info[last].setdefault(m.group(1), int(m.group(2)))
            continue
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", s)
        if m:
            curh = m.group(1)
            hsa[curh] = []
            continue
        if re.match(r"^\s*\.end_amdhsa_kernel", s):
            curh = None
            continue
        if curh is not None:
            hsa[curh].append(s.strip())
            continue
        m = re.match(r"^\s+\.name:\s+(_Z\w+)$", s)
        if m:
            name = m.group(1)
        m = re.match(r"^\s+\.(sgpr|vgpr)_spill_count:\s+(\d+)", s)
        if m and name:
            spills.setdefault(name, {})[m.group(1)] = int(m.group(2))
        if cur is not None:
            t = s.split(";")[0].strip()
            if t and not t.startswith((".p2align", ".cfi")):
                funcs[cur].append(t)
    return funcs, hsa, info, spills


def norm(lines, dm):
    lab = {}
    out = []
    for t in lines:
        t = re.sub(r"\.L\w+", lambda m: lab.setdefault(m.group(0), ".L%d" % len(lab)), t)
        out.append(re.sub(r"_Z\w+", lambda m: role(dm.get(m.group(0), m.group(0))), t))
    return out


def main():
    fa, ha, ia, sa = parse(sys.argv[1])
    fb, hb, ib, sb = parse(sys.argv[2])
    dm = demangle(sorted(set(fa) | set(fb)))
    ra = {role(dm[k]): k for k in fa if "(" in dm[k]}  # (functions: not the data tables)
    rb = {role(dm[k]): k for k in fb if "(" in dm[k]}
    same = 0
    for r in sorted(set(ra) | set(rb)):
        if r not in ra or r not in rb:
            print("only in %s: %s" % ("parent" if r in ra else "tree", r))
            continue
        ka, kb = ra[r], rb[r]
        na, nb = norm(fa[ka], dm), norm(fb[kb], dm)
        if na == nb and ha.get(ka) == hb.get(kb):
            same += 1
            continue
        short = re.sub(r"\(.*", "", r).replace("void ajx::", "").replace("ajx::", "")
        print("differs: %s" % short)
        print("    instructions %d | %d, .amdhsa_ block %s" %
              (len(na), len(nb), "identical" if ha.get(ka) == hb.get(kb) else "differs"))
        for side, inf, sp in (("parent", ia[ka], sa.get(ka, {})), ("tree  ", ib[kb], sb.get(kb, {}))):
            print("    %s VGPR %3d AGPR %3d SGPR %3d scratch %5d spills SGPR %4s VGPR %4s LDS %5d occupancy %d" %
                  (side, inf.get("NumVgprs", 0), inf.get("NumAgprs", 0), inf.get("TotalNumSgprs", 0),
                   inf.get("ScratchSize", 0), sp.get("sgpr", "-"), sp.get("vgpr", "-"), inf.get("LDSByteSize", 0),
                   inf.get("Occupancy", 0)))
        if len(sys.argv) > 3 and sys.argv[3] in r:
            for l in list(difflib.unified_diff(na, nb, lineterm="", n=2))[:int(sys.argv[4]) if len(sys.argv) > 4 else 80]:
                print("        " + l)
    print("functions with identical text: %d of %d" % (same, len(set(ra) & set(rb))))


if __name__ == "__main__":
    main()

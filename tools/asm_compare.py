#!/usr/bin/env python3
"""Compare two `make -C wireguard-java_amd/csrc asm` outputs kernel by kernel.

    python tools/asm_compare.py OLD_DIR NEW_DIR

Each directory holds wgaead-gfx950.s and resource-usage.txt (build/ after `make asm`). For every kernel
present in both, the instruction text of the function body (labels renumbered, so a shift of the
translation unit's label counter is no difference) and its resource-usage lines (SGPRs, VGPRs, AGPRs,
scratch, occupancy, spills, LDS) must be identical. Prints one JSON line and exits 1 on a difference:
a change meant to leave the existing kernels alone is checked with this, without a GPU."""
import json
import os
import re
import sys


def bodies(path):
    out, name, cur = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+|k_\w+):\s", line)
        if m and name is None:
            name, cur = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = cur
                name = None
                continue
            s = line.split(";")[0].rstrip() if not line.lstrip().startswith(";") else ""
            if s.strip():
                cur.append(s)
    return out


def renumber(lines):
    """Local labels (.LBB<fn>_<k>, .Ltmp<k>, ...) by order of first appearance."""
    seen = {}

    def sub(m):
        return seen.setdefault(m.group(0), f".L{len(seen)}")
    return [re.sub(r"\.L[A-Za-z_]*\d+(?:_\d+)?", sub, s) for s in lines]


def usage(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        m = re.search(r"remark:\s+(\S.*?) \[-Rpass-analysis", line)
        if m and name:
            out[name].append(m.group(1))
    return out


def main():
    old, new = sys.argv[1], sys.argv[2]
    a, b = bodies(os.path.join(old, "wgaead-gfx950.s")), bodies(os.path.join(new, "wgaead-gfx950.s"))
    ua, ub = usage(os.path.join(old, "resource-usage.txt")), usage(os.path.join(new, "resource-usage.txt"))
    kernels = sorted(k for k in ua if k in ub)
    asm_diff = [k for k in kernels if k not in a or k not in b or renumber(a[k]) != renumber(b[k])]
    use_diff = [k for k in kernels if ua[k] != ub[k]]
    res = {"kernels_in_both": len(kernels), "only_old": sorted(set(ua) - set(ub)), "only_new": sorted(set(ub) - set(ua)),
           "asm_differs": asm_diff, "resource_usage_differs": use_diff}
    print(json.dumps(res))
    sys.exit(1 if asm_diff or use_diff or not kernels else 0)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Per-kernel diff of two sets of gfx950 listings, for refactors of csrc/:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Icsrc --cuda-device-only \
        -S csrc/shallow_water.hip -o new_sw.s         # same for the old tree
    tools/asm_diff.py --old old_sw.s old_halo.s --new new_sw.s new_halo.s

Kernels pair up by symbol across all files of a side (one may have moved to
another file).  Comments are dropped and `.LBB<n>_` prefixes normalised.
Prints IDENTICAL, or the number of differing lines and whether the
register/LDS/scratch metadata and the histogram of floating-point, global,
LDS and scalar-load mnemonics agree; -v lists the lines.  Only diffs and
counts; exit status 1 if a kernel is missing or metadata/histogram moved.
"""
import argparse
import collections
import difflib
import re

META = (".vgpr_count", ".agpr_count", ".group_segment_fixed_size",
        ".private_segment_fixed_size")
HIST = re.compile(r"(v_\w*_f(16|32|64)\w*|global_\w+|ds_\w+|s_load\w+)$")


def parse(paths):
    body, meta = {}, {}
    for text in (open(p).read() for p in paths):
        cur = None
        for ln in text.splitlines():
            if m := re.match(r"(\S+):\s*; @\1$", ln):  # function label
                cur = body[m.group(1)] = []
            elif re.match(r"\s*\.section|\.Lfunc_end", ln):
                cur = None
            elif cur is not None and (ln := ln.split(";")[0].strip()):
                cur.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        for entry in re.split(r"^  - (?=\.)", text, flags=re.M)[1:]:
            kv = dict(re.findall(r"^(?:    )?(\.\w+):\s+(\S+)$", entry, re.M))
            meta[kv[".name"]] = [kv.get(k) for k in META]
    return {k: (body[k], meta[k]) for k in meta}


def hist(lines):
    return collections.Counter(
        w for ln in lines if HIST.match(w := ln.split()[0]))


ap = argparse.ArgumentParser()
ap.add_argument("--old", nargs="+", required=True)
ap.add_argument("--new", nargs="+", required=True)
ap.add_argument("-v", action="store_true", help="print the differing lines")
args = ap.parse_args()
old, new = parse(args.old), parse(args.new)
bad = 0
for k in sorted(set(old) | set(new)):
    if k not in old or k not in new:
        print("ONLY-OLD " if k in old else "ONLY-NEW ", k)
        bad += 1
    elif old[k] == new[k]:
        print("IDENTICAL", k, f"({len(old[k][0])} lines)")
    else:
        (a, ma), (b, mb) = old[k], new[k]
        d = [x for x in difflib.unified_diff(a, b, lineterm="", n=0)
             if x[0] in "+-" and x[:3] not in ("+++", "---")]
        same = ["same" if x else "CHANGED" for x in (ma == mb,
                                                     hist(a) == hist(b))]
        bad += "CHANGED" in same
        print("DIFFERS  ", k, f"{len(a)}->{len(b)} lines, {len(d)} differing;"
              f" metadata {same[0]}, histogram {same[1]}")
        if args.v:
            print("\n".join("    " + x for x in d))
print(f"{len(set(old) | set(new))} kernels, {bad} not equivalent")
raise SystemExit(1 if bad else 0)

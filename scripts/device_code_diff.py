#!/usr/bin/env python3
"""Compare the device assembly of two builds, kernel by kernel.

usage: device_code_diff.py OLD_DIR NEW_DIR   (each holds <unit>.s from `hipcc <Makefile flags> --cuda-device-only -S`)

Per unit: the kernel symbols of both sides, and for every common symbol its code (from its label to its end label)
and its kernel descriptor (.amdhsa_kernel block).  Local label numbers and trailing comments follow the order of
emission and are not compared.  A kernel that changed unit is looked up by its symbol in the parent's other units and
reported as moved.  Prints one line per unit and the symbols present on one side only; exit status 1 if a
common symbol differs, a symbol's code was not found, or the new side has a symbol the old one lacks.
"""
import os
import re
import sys


def norm(lines):
    res = []
    for ln in lines:
        ln = re.sub(r"\s*;.*$", "", ln)
        ln = re.sub(r"\.L(BB|tmp|func_begin|func_end|JTI)\d+(_\d+)?", lambda m: ".L" + m.group(1) + (m.group(2) or ""), ln)
        if ln.strip():
            res.append(ln.strip())
    return res


def kernels(path):
    """{symbol: (code lines, descriptor lines)} of one assembly file"""
    text = open(path).read().split("\n")
    names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in text) if m}
    code, desc = {}, {}
    body = block = None  # the code / descriptor the current line belongs to (a descriptor lies inside its code)
    for ln in text:
        label = re.match(r"^([A-Za-z_][\w$.]*):", ln)
        begin = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if body is None and label and label.group(1) in names:
            body = code.setdefault(label.group(1), [])
        elif re.match(r"^\.Lfunc_end\d+:", ln):
            body = None
        elif begin:
            block = desc.setdefault(begin.group(1), [])
        elif ".end_amdhsa_kernel" in ln:
            block = None
        else:
            if body is not None:
                body.append(ln)
            if block is not None:
                block.append(ln)
    return {k: (norm(code.get(k, [])), norm(desc[k])) for k in names}


def main():
    old, new = sys.argv[1], sys.argv[2]
    bad = False
    units = lambda d: sorted(f for f in os.listdir(d) if f.endswith(".s"))
    olds = {f: kernels(os.path.join(old, f)) for f in units(old)}
    news = {f: kernels(os.path.join(new, f)) for f in units(new)}
    for f in units(new):
        a, b = dict(olds.get(f, {})), news[f]
        # a kernel that changed unit is compared with the parent's code where the parent had it
        moved = {k: g for k in set(b) - set(a) for g in olds if g != f and k in olds[g]}
        for k, g in sorted(moved.items()):
            a[k] = olds[g][k]
            print("    %s: %s was in %s at the parent" % (f.replace(".s", ".hip"), k, g.replace(".s", ".hip")))
        common = sorted(set(a) & set(b))
        diff = [k for k in common if a[k] != b[k] or not b[k][0]]
        elsewhere = {k for k in set(a) - set(b) if any(k in news[g] for g in news if g != f)}
        gone, added = sorted(set(a) - set(b) - elsewhere), sorted(set(b) - set(a))
        print("%s: %d kernels at the parent, %d at this tree; common symbols identical: %s" %
              (f.replace(".s", ".hip"), len(a), len(b), "NO" if diff else "yes"))
        for k in gone:
            print("    only at the parent: " + k)
        for k in added:
            print("    only at this tree: " + k)
        for k in diff:
            print("    differs or not found: " + k)
        bad = bad or bool(diff or added)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

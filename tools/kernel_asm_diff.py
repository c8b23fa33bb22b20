#!/usr/bin/env python3
"""kernel_asm_diff.py — compare the kernels of AMDGPU assembly files, symbol by symbol.

For a change that moves kernels between translation units without meaning to change them:

    hipcc $(HIPFLAGS) --offload-device-only -S -o old.s  old/kernels.hip
    hipcc $(HIPFLAGS) --offload-device-only -S -o new1.s kernels.hip      (and so on)
    tools/kernel_asm_diff.py --old old.s --new new1.s new2.s [--removed removed.txt [--exact]]

Per kernel symbol (every `.amdhsa_kernel`) it compares
  - the instruction stream: comments and blank lines dropped, the local `.LBB<f>_<b>` labels
    renumbered by first appearance (their function index shifts when functions move);
  - the `.amdhsa_` block and the symbol's `.set <kernel>.<resource>` lines: registers, LDS, scratch.
It passes (exit 0) when every kernel of the new files exists in the old files and is identical and,
with --removed, when every old kernel missing from the new files matches one of the file's regular
expressions (one per line, `#` comments, matched against the demangled name); with --exact every
expression must also match a missing kernel, so the list describes exactly what went. A kernel that
occurs in several files of one side (a template instantiated by two translation units) must be
identical in all of them. Text processing only: no GPU, no compiler.
"""
import argparse
import re
import shutil
import subprocess
import sys

LABEL = re.compile(r"\.LBB\d+_\d+")


def kernels_of(path):
    """{symbol: (instruction lines, resource lines)} of one .s file."""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    wanted, out = set(names), {}
    i = 0
    while i < len(lines):
        m = re.match(r"(\S+):\s*(;.*)?$", lines[i])
        if not (m and m.group(1) in wanted):
            i += 1
            continue
        name, body, res, seen = m.group(1), [], [], {}
        i += 1
        while not re.match(r"\s*\.amdhsa_kernel\s", lines[i]):  # the function's instructions
            text = lines[i].split(";", 1)[0].strip()
            if text and not text.startswith(".section") and not text.startswith(".p2align"):
                body.append(LABEL.sub(lambda k: seen.setdefault(k.group(0), ".L%d" % len(seen)), text))
            i += 1
        while not re.match(r"\s*\.end_amdhsa_kernel", lines[i]):  # .amdhsa_kernel ... .end_amdhsa_kernel
            res.append(lines[i].strip())
            i += 1
        while i < len(lines) and "; -- End function" not in lines[i]:
            i += 1
        i += 1
        while i < len(lines) and re.match(r"\s*\.set\s+" + re.escape(name) + r"\.", lines[i]):
            res.append(lines[i].strip())
            i += 1
        out[name] = (body, res)
    missing = wanted - set(out)
    if missing:
        sys.exit("%s: no function body found for %d kernels, e.g. %s" % (path, len(missing), sorted(missing)[0]))
    return out


def side(paths, what):
    merged, clash = {}, []
    for p in paths:
        ks = kernels_of(p)
        print("%s: %d kernels" % (p, len(ks)))
        for name, k in ks.items():
            if name in merged and merged[name] != k:
                clash.append(name)
            merged.setdefault(name, k)
    if len(paths) > 1:
        print("%s files together: %d distinct kernels" % (what, len(merged)))
    return merged, clash


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.split("\n")))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True, metavar="FILE.s")
    ap.add_argument("--new", nargs="+", required=True, metavar="FILE.s")
    ap.add_argument("--removed", metavar="FILE", help="regular expressions for the old kernels that may be missing")
    ap.add_argument("--exact", action="store_true", help="every expression of --removed must match a missing kernel")
    ap.add_argument("--list", action="store_true", help="print every old-only kernel, not only the count per expression")
    a = ap.parse_args()
    old, old_clash = side(a.old, "old")
    new, new_clash = side(a.new, "new")
    added = sorted(set(new) - set(old))
    gone = sorted(set(old) - set(new))
    differ = sorted(n for n in new if n in old and new[n] != old[n])
    same = len(new) - len(added) - len(differ)
    print("identical: %d   differing: %d   only in new: %d   only in old: %d" % (same, len(differ), len(added), len(gone)))
    names = demangle(differ + added + gone + old_clash + new_clash)
    ok = not (differ or added or old_clash or new_clash)
    for title, group in (("DIFFERS", differ), ("ONLY IN NEW", added), ("DIFFERS BETWEEN THE OLD FILES", old_clash),
                         ("DIFFERS BETWEEN THE NEW FILES", new_clash)):
        for n in group:
            print("%s: %s" % (title, names[n]))
            if title == "DIFFERS":
                for part, label in ((0, "instructions"), (1, "resources")):
                    if new[n][part] != old[n][part]:
                        print("    %s: %d lines old, %d lines new" % (label, len(old[n][part]), len(new[n][part])))
    if a.removed:
        exprs = [l.strip() for l in open(a.removed) if l.strip() and not l.startswith("#")]
        hits = {e: 0 for e in exprs}
        for n in gone:
            matched = [e for e in exprs if re.search(e, names[n])]
            for e in matched[:1]:
                hits[e] += 1
            if not matched:
                print("MISSING, NOT ON THE REMOVAL LIST: %s" % names[n])
                ok = False
        for e in exprs:
            print("removed %4d  %s" % (hits[e], e))
            if a.exact and not hits[e]:
                print("REMOVAL LIST ENTRY MATCHES NOTHING: %s" % e)
                ok = False
    if a.list or not a.removed:
        for n in gone:
            print("only in old: %s" % names[n])
    print("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Compare the device assembly of two builds, kernel by kernel.

    tools/asm_cmp.py A_DIR B_DIR [--map OLD=NEW ...] [--removed NAME ...]

A_DIR and B_DIR hold the `.s` files of `hipcc <Makefile flags> -S --cuda-device-only` for every
`.hip` of the two trees (any file names: a kernel may have moved to another file).  Per function
symbol the instruction lines (comments, .loc / .file lines dropped; the function numbers of
.LBB<n>_ / .LJTI<n>_ and the .Ltmp<n> numbers normalised) and the kernel's .amdhsa_* descriptor
block must be the same text.  --map matches a kernel of A whose mangled name changed to its name in
B; --removed names kernels of A that B drops on purpose.  One line per kernel; exit status 1 on any
difference, on a kernel of one side only and on a kernel defined by two files of one side.
"""
import argparse
import pathlib
import re
import sys


def functions(path):
    """{symbol: (instruction lines, descriptor lines)} of one .s file."""
    out, name, body, desc, in_desc = {}, None, [], [], False
    tmp, pending = {}, None
    for raw in path.read_text().splitlines():
        line = raw.split(";", 1)[0].rstrip()
        s = line.strip()
        if name is None:
            m = re.fullmatch(r"\.type\s+(\S+),@function", s)
            if m:
                pending = m.group(1)
            elif pending and s == pending + ":":
                name, pending, body, desc, tmp = pending, None, [], [], {}
            continue
        if s.startswith(".Lfunc_end"):
            out[name] = (body, desc)
            name = None
        elif s.startswith(".amdhsa_kernel"):
            in_desc = True
        elif s.startswith(".end_amdhsa_kernel"):
            in_desc = False
        elif in_desc:
            desc.append(s)
        elif s and not s.startswith((".loc", ".file", ".section", ".p2align", ".Lfunc_begin", ".cfi_")):
            s = re.sub(r"\.(LBB|LJTI)\d+_", r".\1_", s)
            s = re.sub(r"\.Ltmp\d+", lambda t: ".Ltmp%d" % tmp.setdefault(t.group(0), len(tmp)), s)
            body.append(s)
    return out


def load(d, errors):
    syms = {}
    for f in sorted(pathlib.Path(d).glob("*.s")):
        text = f.read_text()
        kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
        for name, (body, desc) in functions(f).items():
            if name in syms:
                errors.append("DUPLICATE %s: %s and %s" % (name, syms[name][0], f.name))
            syms[name] = (f.name, body, desc, name in kernels)
    return syms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a_dir")
    ap.add_argument("b_dir")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--removed", action="append", default=[], metavar="NAME")
    args = ap.parse_args()
    errors = []
    a, b = load(args.a_dir, errors), load(args.b_dir, errors)
    for line in errors:
        print(line)
    bad = len(errors)
    rename = dict(m.split("=", 1) for m in args.map)
    seen = set()
    for old in sorted(a):
        fa, body_a, desc_a, is_kernel = a[old]
        kind = "kernel" if is_kernel else "function"
        new = rename.get(old, old)
        if old in args.removed:
            ok = new not in b
            print("%s %s %s: %s" % ("REMOVED" if ok else "STILL-PRESENT", kind, old, fa))
            bad += not ok
            seen.add(new)
            continue
        if new not in b:
            print("ONLY-IN-A %s %s: %s" % (kind, old, fa))
            bad += 1
            continue
        seen.add(new)
        fb, body_b, desc_b, _ = b[new]
        body_a = [s.replace(old, new) for s in body_a]
        if body_a == body_b and desc_a == desc_b:
            verdict = "identical"
        else:
            verdict = "DIFFERENT (%s)" % ", ".join(
                w for w, x, y in (("instructions", body_a, body_b), ("descriptor", desc_a, desc_b)) if x != y)
            bad += 1
        print("%s %s %s%s: %s -> %s, %d instruction lines" % (
            verdict, kind, old, "" if new == old else " => " + new, fa, fb, len(body_b)))
    for new in sorted(set(b) - seen):
        print("ONLY-IN-B %s: %s" % (new, b[new][0]))
        bad += 1
    print("%d symbols in A, %d in B, %d problems" % (len(a), len(b), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device assemblies of the library (hipcc -S --cuda-device-only with the
project's flags, same compiler): does a change of the source leave every kernel's instructions as they were?

Usage: isa_diff.py PARENT.s CHANGE.s [--pair OLD=NEW ...]

A function is the text from its `_Z...:` label to `.Lfunc_end`. Comments and directives are dropped and local labels
(.LBB, .Ltmp, .LJTI ...) are renumbered in order of appearance, so that a function moved within the file, or one whose
neighbours changed, still compares equal. Functions are matched by demangled name without the parameter list (c++filt);
`--pair OLD=NEW` replaces the substring OLD of a parent's name by NEW first, for a kernel that was renamed or gained a
template argument. One line per function, then the kernels' registers, scratch and LDS from each file's metadata.
Exit status 1 if a function differs or has no partner, or a kernel's resources differ."""
import argparse
import re
import subprocess
import sys

RES_KEYS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
_LOCAL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def split_functions(text: str) -> dict[str, list[str]]:
    """mangled name -> its lines (labels and instructions, comments stripped, directives dropped)"""
    out: dict[str, list[str]] = {}
    cur = None
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].split("//", 1)[0].strip()
        if not line:
            continue
        m = re.match(r"(_Z\w+):$", line)
        if m:  # (a data symbol's label has no .Lfunc_end: the next label ends it)
            cur = m.group(1)
            out[cur] = []
        elif cur is None:
            continue
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif line.endswith(":") or not line.startswith("."):
            out[cur].append(line)
    return {k: v for k, v in out.items() if v}


def normalise(name: str, lines: list[str]) -> list[str]:
    ids: dict[str, str] = {}

    def renumber(m: re.Match) -> str:
        return ids.setdefault(m.group(0), f".L{len(ids)}")

    return [_LOCAL.sub(renumber, " ".join(line.replace(name, "<self>").split())) for line in lines]


def resources(text: str) -> dict[str, dict[str, str]]:
    """mangled kernel name -> RES_KEYS of its entry in amdhsa.kernels"""
    out: dict[str, dict[str, str]] = {}
    entry: dict[str, str] = {}
    for line in text.splitlines():
        m = re.match(r"  (- | {2})(\.\w+):\s*(\S*)", line)
        if not m:
            continue
        if m.group(1) == "- ":
            entry = {}
        entry[m.group(2)] = m.group(3)
        if ".name" in entry and entry[".name"].startswith("_Z"):
            out[entry[".name"]] = entry
    return out


def demangle(names: list[str]) -> list[str]:
    if not names:
        return []
    res = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    return res.stdout.splitlines()


def short(demangled: str) -> str:
    """the name without return type's `void ` and without the parameter list"""
    depth = 0
    for i, ch in enumerate(demangled):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0 and not demangled.startswith("(anonymous namespace)", i):
            demangled = demangled[:i]
            break
    return demangled.removeprefix("void ")


def load(path: str, pairs: list[tuple[str, str]]):
    text = open(path, errors="replace").read()
    funcs = split_functions(text)
    res = resources(text)
    mangled = list(funcs)
    full = demangle(mangled)
    names = [short(d) for d in full]
    # overloads that differ in their parameters only keep the list
    names = [d if names.count(n) > 1 else n for n, d in zip(names, full)]
    out = {}
    for m, n in zip(mangled, names):
        for old, new in pairs:
            n = n.replace(old, new)
        out[n] = (normalise(m, funcs[m]), res.get(m))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("change")
    ap.add_argument("--pair", action="append", default=[], metavar="OLD=NEW",
                    help="replace substring OLD of a parent's demangled name by NEW before matching")
    args = ap.parse_args(argv)
    pairs = [tuple(p.split("=", 1)) for p in args.pair]
    if any(len(p) != 2 for p in pairs):
        ap.error("--pair wants OLD=NEW")
    a, b = load(args.parent, pairs), load(args.change, [])
    bad = 0
    for n in sorted(set(a) | set(b)):
        if n not in a or n not in b:
            print(f"NO PARTNER  {n}  (only in {'parent' if n in a else 'change'})")
            bad += 1
            continue
        la, lb = a[n][0], b[n][0]
        if la == lb:
            print(f"identical   {n}  {len(la)} / {len(lb)} lines")
            continue
        bad += 1
        i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
        print(f"DIFFERS     {n}  {len(la)} / {len(lb)} lines; first at {i}: "
              f"{la[i] if i < len(la) else '<end>'!r} | {lb[i] if i < len(lb) else '<end>'!r}")
    print("\nresources (parent / change): vgpr, sgpr, scratch bytes, LDS bytes")
    res_bad = 0
    for n in sorted(set(a) & set(b)):
        ra, rb = a[n][1], b[n][1]
        if ra is None and rb is None:
            continue  # a device function, not a kernel
        va = [(ra or {}).get(k, "?") for k in RES_KEYS]
        vb = [(rb or {}).get(k, "?") for k in RES_KEYS]
        flag = "" if va == vb else "   <-- UNEQUAL"
        res_bad += va != vb
        print(f"  {n}: " + ", ".join(f"{x} / {y}" for x, y in zip(va, vb)) + flag)
    total = len(set(a) | set(b))
    print(f"\n{total - bad} of {total} functions identical, {bad} differ or have no partner, "
          f"{res_bad} with unequal resources")
    return 1 if bad or res_bad else 0


if __name__ == "__main__":
    sys.exit(main())

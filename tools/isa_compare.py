#!/usr/bin/env python3
"""Compare two trees' gfx950 device assembly, file by file.

usage: tools/isa_compare.py TREE_A TREE_B [-j N] [--keep DIR] [name ...]

For every `hipcc ... -c csrc/X.hip -o build/X.o` line that `make -n -B` prints in
TREE/mast3r-slam_amd (so: with exactly the flags that tree's Makefile gives that file), the same
command is run with `--offload-device-only -S` in place of `-c`, and the two trees' assembly files
are compared line for line.  `__hip_cuid_<hash>` is replaced by a constant first: it is a hash of
the source text and the one thing a neutral edit changes.  Prints one line per file and exits 1
unless every file is `identical`.  Names (`gn_accum chol_df`) restrict the run to those files.
"""
import argparse
import concurrent.futures as cf
import os
import re
import shlex
import subprocess
import sys
import tempfile

CUID = re.compile(rb"__hip_cuid_[0-9a-f]+")


def compile_commands(tree):
    """{name: argv} of the tree's per-file compile commands, from `make -n -B`."""
    pkg = os.path.join(tree, "mast3r-slam_amd")
    out = subprocess.check_output(["make", "-n", "-B", "-C", pkg], text=True)
    cmds = {}
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" not in argv or not argv[0].endswith("hipcc"):
            continue
        src = argv[argv.index("-c") + 1]
        cmds[os.path.splitext(os.path.basename(src))[0]] = argv
    return pkg, cmds


def assemble(pkg, argv, dst):
    i = argv.index("-c")
    o = argv.index("-o")
    argv = list(argv)
    argv[o + 1] = dst
    argv[i:i + 1] = ["--offload-device-only", "-S"]
    subprocess.check_call(argv, cwd=pkg, stderr=subprocess.DEVNULL)
    with open(dst, "rb") as f:
        return CUID.sub(b"__hip_cuid_X", f.read()).splitlines()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("names", nargs="*")
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 4))
    ap.add_argument("--keep", help="keep the assembly files in this folder")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="isa_compare_")
    trees = []
    for side, tree in (("a", a.tree_a), ("b", a.tree_b)):
        os.makedirs(os.path.join(tmp, side), exist_ok=True)
        trees.append((side,) + compile_commands(os.path.abspath(tree)))
    names = sorted(set(trees[0][2]) | set(trees[1][2]))
    if a.names:
        names = [n for n in names if n in a.names]
    jobs = {}
    with cf.ThreadPoolExecutor(a.j) as ex:
        for side, pkg, cmds in trees:
            for n in names:
                if n in cmds:
                    jobs[side, n] = ex.submit(assemble, pkg, cmds[n], os.path.join(tmp, side, n + ".s"))
    bad = 0
    for n in names:
        if ("a", n) not in jobs or ("b", n) not in jobs:
            verdict = "only in " + (a.tree_a if ("a", n) in jobs else a.tree_b)
        else:
            la, lb = jobs["a", n].result(), jobs["b", n].result()
            ndiff = sum(x != y for x, y in zip(la, lb)) + abs(len(la) - len(lb))
            verdict = "identical" if ndiff == 0 else f"DIFFERENT ({ndiff} lines)"
            verdict += f"  {len(la)} / {len(lb)} lines"
        bad += not verdict.startswith("identical")
        print(f"{n:18s} {verdict}", flush=True)
    print(f"{len(names) - bad} of {len(names)} files identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

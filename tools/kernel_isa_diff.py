#!/usr/bin/env python3
"""Compare the gfx950 machine code of every kernel of two checkouts (no GPU needed).

    python tools/kernel_isa_diff.py <old-tree> <new-tree> [--only conv_mfma.hip ...] [--jobs N] [--keep DIR]

Each causal_vae_amd/csrc/*.hip of both trees is compiled with the Makefile's FLAGS plus --offload-device-only -S.  The assembly is split per
kernel symbol: the body from its label to its .Lfunc_end, plus its .amdhsa_kernel ... .end_amdhsa_kernel block.  Before comparing, `;` comments
are dropped, lines stripped and the function-index part of local labels (.LBB<n>_<m>, .Lfunc_end<n>, .Ltmp<n>) is replaced — those renumber
when a neighbouring kernel disappears.  Nothing else is normalised: instructions, register counts, LDS, scratch and accum_offset compare as text.

Reports, per file, (a) kernels in both trees whose text differs, (b) kernels only in the old tree, (c) kernels only in the new tree, by
symbol, with the wall time of each compile.  Exit status 1 if (a) or (c) is non-empty."""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile
import time

CSRC = os.path.join("causal_vae_amd", "csrc")
LOCAL = re.compile(r"\.L(BB|func_end|func_begin|tmp)\d+")


def make_var(tree, name):
    """Value of a `NAME := ...` / `NAME ?= ...` line of the tree's csrc/Makefile, with $(ARCH) expanded and $(EXTRA) empty."""
    vals = {}
    for line in open(os.path.join(tree, CSRC, "Makefile")):
        m = re.match(r"(\w+)\s*[:?]?=\s*(.*)", line)
        if m:
            vals.setdefault(m.group(1), m.group(2).strip())
    out = vals[name]
    for _ in range(4):
        out = re.sub(r"\$\((\w+)\)", lambda m: vals.get(m.group(1), "") if m.group(1) != "EXTRA" else "", out)
    return out


def compile_asm(tree, src, out):
    deps = [os.path.join(tree, CSRC, d) for d in (src, "common.h", "Makefile")]
    if os.path.exists(out) and all(os.path.getmtime(out) > os.path.getmtime(d) for d in deps):
        return 0.0                                                   # --keep DIR from an earlier run: this source has not changed since
    cmd = [make_var(tree, "HIPCC")] + make_var(tree, "FLAGS").split() + ["-w", "--offload-device-only", "-S", src, "-o", out]
    t = time.time()
    subprocess.run(cmd, cwd=os.path.join(tree, CSRC), check=True)
    return time.time() - t


def kernels(asm):
    """{symbol: normalised text} for every .amdhsa_kernel of one assembly file."""
    lines = []
    for line in open(asm):
        line = line.split(";", 1)[0].strip()
        if line:
            lines.append(LOCAL.sub(lambda m: ".L" + m.group(1), line))
    names = {l.split()[1] for l in lines if l.startswith(".amdhsa_kernel ")}
    out, cur, end = {n: [] for n in names}, None, None
    for l in lines:
        if cur is None:
            if l.endswith(":") and l[:-1] in names:
                cur, end = l[:-1], ".Lfunc_end:"
            elif l.startswith(".amdhsa_kernel "):
                cur, end = l.split()[1], ".end_amdhsa_kernel"
        if cur is not None:
            out[cur].append(l)
            if l == end:
                cur = None
    return {n: "\n".join(t) for n, t in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--only", nargs="*", help="file names under csrc/ (default: every *.hip of either tree)")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--keep", help="keep the .s files in this directory")
    a = ap.parse_args()
    trees = {"old": os.path.abspath(a.old), "new": os.path.abspath(a.new)}
    files = a.only or sorted({f for t in trees.values() for f in os.listdir(os.path.join(t, CSRC)) if f.endswith(".hip")})
    tmp = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    os.makedirs(tmp, exist_ok=True)
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        for f in files:
            for side, tree in trees.items():
                if os.path.exists(os.path.join(tree, CSRC, f)):
                    jobs[f, side] = ex.submit(compile_asm, tree, f, os.path.join(tmp, f"{side}_{f[:-4]}.s"))
    bad = 0
    for f in files:
        secs = {side: jobs[f, side].result() for side in trees if (f, side) in jobs}           # a file may exist in one tree only
        k = {side: kernels(os.path.join(tmp, f"{side}_{f[:-4]}.s")) if side in secs else {} for side in trees}
        differ = sorted(n for n in k["old"] if n in k["new"] and k["old"][n] != k["new"][n])
        only_old, only_new = sorted(set(k["old"]) - set(k["new"])), sorted(set(k["new"]) - set(k["old"]))
        print(f"{f}: {len(k['old'])} kernels old ({secs.get('old', 0):.0f} s), {len(k['new'])} new ({secs.get('new', 0):.0f} s): "
              f"(a) {len(differ)} differ, (b) {len(only_old)} only old, (c) {len(only_new)} only new")
        for tag, group in (("a differs ", differ), ("b only old", only_old), ("c only new", only_new)):
            for n in group:
                print(f"  ({tag}) {n}")
        bad += len(differ) + len(only_new)
    if not a.keep:
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

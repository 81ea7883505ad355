#!/usr/bin/env python3
"""Instruction mix of a kernel's largest loop, from gfx950 assembly (no GPU needed).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only causal_vae_amd/csrc/conv_mfma.hip -o conv_mfma.s
    python tools/isa_loop_count.py conv_mfma.s conv_wgrad_kernelIDF16bLi3E

The second argument is a substring of the kernel's (mangled) symbol; it must select one kernel.  A loop is the span from a local label to the
last backward branch that targets it; the largest one (most instructions; inner loops are part of it and count once, as static text) is reported
by instruction class.  Classes go by mnemonic PREFIX only.  The register metadata of the kernel (.vgpr_count, scratch, LDS) is printed with it."""
import re
import sys

CLASSES = (                     # first matching prefix wins
    ("MFMA", ("v_mfma", "v_smfmac")),
    ("VALU", ("v_",)),
    ("waits", ("s_wait", "s_barrier", "s_nop", "s_sleep")),
    ("branches", ("s_cbranch", "s_branch")),
    ("SALU", ("s_",)),
    ("LDS reads", ("ds_read", "ds_load")),
    ("LDS writes", ("ds_write", "ds_store")),
    ("LDS other", ("ds_",)),
    ("global loads", ("global_load", "buffer_load", "flat_load", "scratch_load")),
    ("global stores", ("global_store", "buffer_store", "flat_store", "scratch_store")),
    ("vector memory other", ("global_", "buffer_", "flat_", "scratch_")),
)
ORDER = [c for c, _ in CLASSES] + ["other"]


def classify(mn):
    for c, prefixes in CLASSES:
        if mn.startswith(prefixes):
            return c
    return "other"


def kernel_body(lines, want):
    names = [l.split()[1] for l in lines if l.startswith(".amdhsa_kernel ")]
    hit = [n for n in names if want in n]
    if len(hit) != 1:
        sys.exit(f"{want!r} selects {len(hit)} kernels of {len(names)}:\n  " + "\n  ".join(hit or names))
    sym = hit[0]
    start = lines.index(sym + ":")
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return sym, lines[start + 1:end]


def largest_loop(body):
    label_at = {l[:-1]: i for i, l in enumerate(body) if l.endswith(":")}
    spans = {}
    for i, l in enumerate(body):
        p = l.split()
        if p[0].startswith(("s_cbranch", "s_branch")) and p[-1] in label_at and label_at[p[-1]] < i:
            spans[p[-1]] = (label_at[p[-1]], i)                          # the LAST backward branch to a label closes its loop
    if not spans:
        sys.exit("the kernel has no loop")
    def ninstr(s):
        return sum(1 for l in body[s[0]:s[1] + 1] if not l.endswith(":") and not l.startswith("."))
    lab = max(spans, key=lambda k: ninstr(spans[k]))
    return lab, spans[lab], len(spans)


def metadata(lines, sym):
    out, on = {}, False
    for l in lines:
        if l.startswith("- .agpr_count"):                                 # the first key of a kernel's entry
            blk = {}
            on = True
        if on:
            m = re.match(r"-?\s*\.(\w+):\s*(\S+)$", l)
            if m:
                blk[m.group(1)] = m.group(2)
            if blk.get("name") == sym:
                out = blk
            if l.startswith(".end_amdgpu_metadata"):
                break
    return out


def main():
    asm, want = sys.argv[1], sys.argv[2]
    lines = [l.split(";", 1)[0].strip() for l in open(asm)]
    lines = [l for l in lines if l]
    sym, body = kernel_body(lines, want)
    lab, (a, b), nloops = largest_loop(body)
    counts = dict.fromkeys(ORDER, 0)
    for l in body[a:b + 1]:
        if not l.endswith(":") and not l.startswith("."):
            counts[classify(l.split()[0])] += 1
    print(sym)
    print(f"  largest of {nloops} loops: {lab}, {sum(counts.values())} instructions")
    for c in ORDER:
        if counts[c]:
            print(f"  {c:20s} {counts[c]:5d}")
    if counts["MFMA"]:
        print(f"  {'VALU per MFMA':20s} {counts['VALU'] / counts['MFMA']:5.1f}")
    md = metadata(lines, sym)
    keys = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
    print("  " + ", ".join(f"{k} {md[k]}" for k in keys if k in md))


if __name__ == "__main__":
    main()

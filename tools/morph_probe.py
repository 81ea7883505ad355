"""Time of the morphology kernel on one MI355X, and the A/B over its threads per image (profiles/morphology.md).
    python tools/morph_probe.py [--out profiles/morphology.md] [--rounds 5] [--libs libcvae_hip_m64.so libcvae_hip_m128.so]
        B = 10 000 images of 28 x 28: for the default build and each library named (other builds of the same sources under causal_vae_amd/, e.g.
        make BUILD=build_m64 LIB=../libcvae_hip_m64.so EXTRA="-DCVAE_MORPH_THREADS=64 -DCVAE_MORPH_THREADS_LARGE=64"), `rounds` interleaved rounds of one fresh child process per
        build; the medians over the rounds go into the file, with the same rows' decode time on the default build and the host restatement's time per image
    python tools/morph_probe.py --one       one build (CVAE_HIP_LIB), one JSON line: what a child runs
    python tools/morph_probe.py --once      one launch and nothing else: the run to put under rocprofv3 --kernel-trace --stats
The parent never touches the GPU; every child runs under a time limit, one at a time.  Kernel times are device events around 20 back-to-back launches after a
warm-up, the median of 9 such windows."""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, SIDE = 10000, 28


def digits(n, seed=0):
    """n stroke-like grey images [n, 28, 28] in [0, 1]: smooth noise cut well above its median, so that about a fifth of the pixels are ink, as in MNIST"""
    from scipy import ndimage
    rng = np.random.RandomState(seed)
    s = ndimage.gaussian_filter(rng.rand(n, SIDE, SIDE), sigma=(0, 2.5, 2.5))
    s = (s - s.min(axis=(1, 2), keepdims=True)) / (np.ptp(s, axis=(1, 2), keepdims=True) + 1e-12)
    s[:, :3, :] = s[:, -3:, :] = 0
    s[:, :, :3] = s[:, :, -3:] = 0
    return np.clip(3.0 * (s - 0.55), 0.0, 1.0).astype(np.float32)


def event_ms(fn, inner=20, windows=9):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return statistics.median(out), min(out), max(out)


def one(decode):
    import torch
    from causal_vae_amd import ops, _lib
    x = torch.as_tensor(digits(B)).cuda()
    res = {"threads": int(_lib.lib.cvae_morph12_threads(SIDE, SIDE)), "threads64": int(_lib.lib.cvae_morph12_threads(64, 64)), "lib": os.path.basename(_lib.LIB_PATH)}
    feats, raw = ops.morph_features12(x, return_raw=True)
    res["mean_area"], res["mean_components"] = float(raw[:, 3].float().mean()), float(raw[:, 1].float().mean())
    res["digest"] = int(raw.long().sum())
    res["morph_ms"] = event_ms(lambda: ops.morph_features12(x))
    big = torch.as_tensor(digits(2000, seed=1)).cuda()
    big = torch.nn.functional.interpolate(big[:, None], size=(64, 64), mode="bilinear")[:, 0].contiguous()
    res["morph64_ms"] = event_ms(lambda: ops.morph_features12(big))
    if decode:
        from causal_vae_amd.mnist_baseline import CausalMorphVAE12
        torch.manual_seed(0)
        model = CausalMorphVAE12().cuda().eval()
        z, m = torch.randn(B, 10, device="cuda"), torch.rand(B, 12, device="cuda")
        with torch.no_grad():
            res["decode_fp32_ms"] = event_ms(lambda: model.decode(m, z))
            model.set_compute_dtype(torch.bfloat16)
            res["decode_bf16_ms"] = event_ms(lambda: model.decode(m, z))
    print("MORPH_PROBE " + json.dumps(res), flush=True)


def child(lib, decode):
    env = dict(os.environ)
    if lib:
        env["CVAE_HIP_LIB"] = os.path.join(ROOT, "causal_vae_amd", lib)
    else:
        env.pop("CVAE_HIP_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"] + (["--decode"] if decode else []), env=env, capture_output=True, text=True, timeout=240)
    if p.returncode != 0:
        sys.exit(f"morph_probe: the child for {lib or 'the default build'} ended with {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("MORPH_PROBE ")][-1]
    return json.loads(line[len("MORPH_PROBE "):])


def host_ms_per_image(n=40):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import morphology_reference as mr
    x = digits(n, seed=2)
    t0 = time.perf_counter()
    for im in x:
        mr.measure(im)
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    if "--once" in sys.argv:
        import torch
        from causal_vae_amd import ops
        ops.morph_features12(torch.as_tensor(digits(B)).cuda())
        torch.cuda.synchronize()
        return
    if "--one" in sys.argv:
        one("--decode" in sys.argv)
        return
    arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d          # noqa: E731
    out, rounds = arg("--out", os.path.join(ROOT, "profiles", "morphology.md")), int(arg("--rounds", 5))
    libs = [None]
    if "--libs" in sys.argv:
        i = sys.argv.index("--libs") + 1
        while i < len(sys.argv) and not sys.argv[i].startswith("--"):
            libs.append(sys.argv[i])
            i += 1
    runs = {lib: [] for lib in libs}
    for r in range(rounds):          # interleaved: every build once per round, in turn
        for lib in libs:
            runs[lib].append(child(lib, decode=lib is None))
            print(f"round {r + 1} {lib or 'default'}: {runs[lib][-1]['morph_ms'][0] * 1e3:.1f} us", flush=True)
    digests = {rs[0]["digest"] for rs in runs.values()}
    host = host_ms_per_image()
    med = lambda lib, key: statistics.median(r[key][0] for r in runs[lib])          # noqa: E731
    lo = lambda lib, key: min(r[key][1] for r in runs[lib])          # noqa: E731
    hi = lambda lib, key: max(r[key][2] for r in runs[lib])          # noqa: E731
    d = runs[None][0]
    ms = med(None, "morph_ms")
    lines = ["# The morphology kernel on the MI355X (DESIGN §28)", "",
             "A record, not a claim: no run time is promised for `ops.morph_features12`, and no test asserts one.", "",
             f"How it was taken: `tools/morph_probe.py --rounds {rounds}" + (" --libs " + " ".join(lib for lib in libs if lib) if len(libs) > 1 else "") + "`, one MI355X.  "
             f"Inputs: {B} stroke-like grey images of {SIDE} x {SIDE} from a seed (smooth noise cut above its median: mean area of the measured component "
             f"{d['mean_area']:.0f} pixels, {d['mean_components']:.2f} components per image).  Per build and round one fresh process; in it, after a warm-up, 9 windows "
             "of 20 back-to-back launches between two device events; the figure of a round is the median window, the figure below the median over the rounds "
             "(min - max over every window of every round).  The builds take turns within each round.  Every build returned the same raw records "
             f"({'one digest' if len(digests) == 1 else 'DIGESTS DIFFER: ' + str(digests)}).", "",
             "## The call", "", "| what | time per call, median (min - max) | per image | images/s |", "| --- | --- | --- | --- |",
             f"| `morph_features12`, {B} x {SIDE} x {SIDE}, {d['threads']} threads per image | {ms * 1e3:.1f} us ({lo(None, 'morph_ms') * 1e3:.1f} - {hi(None, 'morph_ms') * 1e3:.1f}) | "
             f"{ms * 1e6 / B:.1f} ns | {B / ms * 1e3 / 1e6:.1f} M |",
             f"| `morph_features12`, 2000 x 64 x 64 (the same images resized), {d['threads64']} threads | {med(None, 'morph64_ms') * 1e3:.1f} us "
             f"({lo(None, 'morph64_ms') * 1e3:.1f} - {hi(None, 'morph64_ms') * 1e3:.1f}) | {med(None, 'morph64_ms') * 1e6 / 2000:.0f} ns | {2000 / med(None, 'morph64_ms') * 1e3 / 1e6:.2f} M |",
             f"| `CausalMorphVAE12.decode` of the same {B} rows, fp32 | {med(None, 'decode_fp32_ms') * 1e3:.1f} us ({lo(None, 'decode_fp32_ms') * 1e3:.1f} - "
             f"{hi(None, 'decode_fp32_ms') * 1e3:.1f}) | {med(None, 'decode_fp32_ms') * 1e6 / B:.1f} ns | {B / med(None, 'decode_fp32_ms') * 1e3 / 1e6:.1f} M |",
             f"| the same decode, bf16 | {med(None, 'decode_bf16_ms') * 1e3:.1f} us ({lo(None, 'decode_bf16_ms') * 1e3:.1f} - {hi(None, 'decode_bf16_ms') * 1e3:.1f}) | "
             f"{med(None, 'decode_bf16_ms') * 1e6 / B:.1f} ns | {B / med(None, 'decode_bf16_ms') * 1e3 / 1e6:.1f} M |",
             f"| the numpy / scipy restatement (`tests/morphology_reference.py`), one host thread | | {host:.2f} ms | {1e3 / host:.0f} |", "",
             f"Measuring costs {ms / med(None, 'decode_fp32_ms'):.2f} of the fp32 decode that made the images and {ms / med(None, 'decode_bf16_ms'):.2f} of the bf16 one; "
             f"the host restatement is {host * 1e6 / (ms * 1e6 / B):.0f} times slower per image.  The call reads {B * SIDE * SIDE * 4 / 1e6:.1f} MB once: "
             f"{B * SIDE * SIDE * 4 / (ms * 1e-3) / 1e12:.2f} TB/s, far from the memory system's rate, as expected of a kernel whose time goes to LDS traffic and its serial sections.", "",
             "## Threads per image (`CVAE_MORPH_THREADS`)", "", "| threads per image (28 x 28 / 64 x 64) | 10 000 x 28 x 28, median (min - max) | 2000 x 64 x 64, median (min - max) |", "| --- | --- | --- |"]
    for lib in sorted(libs, key=lambda k: runs[k][0]["threads"]):
        lines.append(f"| {runs[lib][0]['threads']} / {runs[lib][0]['threads64']}{' (the default build)' if lib is None else ''} | {med(lib, 'morph_ms') * 1e3:.1f} us ({lo(lib, 'morph_ms') * 1e3:.1f} - "
                     f"{hi(lib, 'morph_ms') * 1e3:.1f}) | {med(lib, 'morph64_ms') * 1e3:.1f} us ({lo(lib, 'morph64_ms') * 1e3:.1f} - {hi(lib, 'morph64_ms') * 1e3:.1f}) |")
    lines += ["", "Per round, in the order run (us, 28 x 28): " + "; ".join(
        f"{runs[lib][0]['threads']}: " + " ".join(f"{r['morph_ms'][0] * 1e3:.1f}" for r in runs[lib]) for lib in libs), ""]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()

"""Measurements of DESIGN §24 (the ViT-VAE decoder on batch-statistics BatchNorm2d), three sub-commands:

  kernels --manifest FILE     issue, through `ops`, the BatchNorm launches of the decoder's 11 BatchNorm tensors at --img / --batch in both dtypes: per tensor
                              12 x ops.bn2d_batch_bwd, 12 x ops.bn2d_bwd (the parent's backward) and, for a ResBlock's second layer, 12 x the residual forward.
                              Run it under `rocprofv3 --kernel-trace --stats` in a run of its own; FILE receives the order of the segments.
  parse DIR --manifest FILE   read the run's kernel trace: every call above is three bn2d kernels; per segment the mean us per launch, the first four calls
                              dropped, and the bytes each launch must move.  Prints a markdown table.
  step                        ViTVAE depth 6 as captured steps (GraphedViTTrainStep) in three configurations — eval-mode train_all, stem_batch_stats,
                              stem + decoder batch statistics — alternating rounds of --steps replays, device events; median [min, max] ms per step, ONE JSON line.
Records, not thresholds: profiles/vit_decoder_batchnorm.md."""
import argparse
import copy
import csv
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CALLS, DROP = 12, 4
CHANNELS = (128, 64, 32, 16, 16)


def tensors(img, batch):
    """(label, P, C, act) of the 11 BatchNorm tensors in execution order"""
    out, pos = [], batch * (img[0] // 32) * (img[1] // 32)
    for i, c in enumerate(CHANNELS):
        pos *= 4
        out.append((f"up{i}", pos, c, "leaky001"))
        if i < 3:
            out += [(f"res{i}.bn1", pos, c, "leaky02"), (f"res{i}.bn2", pos, c, None)]
    return out


def kernels(a):
    import torch
    from causal_vae_amd import ops
    if not torch.cuda.is_available():
        sys.exit("vit_decoder_bn_probe: no GPU: nothing is measured without one")
    manifest = []
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        for name, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
            for label, P, C, act in tensors(a.img, a.batch):
                y = torch.randn(P, C, device="cuda", generator=g).to(dtype)
                dy = torch.randn(P, C, device="cuda", generator=g).to(dtype)
                bn = torch.nn.BatchNorm2d(C).to("cuda").eval()
                out, mean, rstd = ops.bn2d_batch_fwd(y, bn, act)
                torch.cuda.synchronize()                               # the set-up call above is one more bn2d triple: it heads the manifest entry
                manifest.append(dict(dtype=name, label=label, P=P, C=C, op="setup_fwd", calls=1))
                for op in ("new_bwd", "old_bwd") + (("res_fwd",) if act is None else ()):
                    for _ in range(CALLS):
                        if op == "new_bwd":
                            ops.bn2d_batch_bwd(y, dy, out if act is not None else None, bn.weight, mean, rstd, act)
                        elif op == "old_bwd":
                            ops.bn2d_bwd(y, dy, out, bn.weight, mean, rstd, act)
                        else:
                            ops.bn2d_batch_fwd(y, bn, None, resid=dy)
                    manifest.append(dict(dtype=name, label=label, P=P, C=C, act=act, op=op, calls=CALLS))
                torch.cuda.synchronize()
                del y, dy, out
    json.dump(manifest, open(a.manifest, "w"))
    print(f"{len(manifest)} segments written to {a.manifest}")


def parse(a):
    f = max(glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = [r for r in csv.DictReader(open(f)) if "bn2d" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    manifest = json.load(open(a.manifest))
    assert len(rows) == 3 * sum(m["calls"] for m in manifest), (len(rows), "bn2d kernels in the trace do not match the manifest")
    i, table = 0, {}
    for m in manifest:
        seg = rows[i:i + 3 * m["calls"]]
        i += 3 * m["calls"]
        if m["op"] == "setup_fwd":
            continue
        per = [[(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in seg[3 * c:3 * c + 3]] for c in range(DROP, m["calls"])]
        table[(m["dtype"], m["label"], m["op"])] = (m, [statistics.mean(col) for col in zip(*per)], [re.search(r"bn2d\w+", r["Kernel_Name"]).group(0) for r in seg[:3]])
    print("| tensor | MB | new: sums, finish, apply = total us | parent: reduce, finalize, apply = total us | new / parent | new apply TB/s | residual forward: moments, finish, apply us |")
    print("|---|---|---|---|---|---|---|")
    for (dt, label, op), (m, new, _names) in table.items():
        if op != "new_bwd":
            continue
        old = table[(dt, label, "old_bwd")][1]
        mb = m["P"] * m["C"] * (2 if dt == "bf16" else 4) / 1e6
        streams = 3 if m["act"] is None else 4                       # apply: y, dy (, a) read, dx written
        res = table.get((dt, label, "res_fwd"))
        fmt = lambda v: ", ".join(f"{x:.1f}" for x in v) + f" = {sum(v):.1f}"
        print(f"| {dt} {label} C {m['C']} P {m['P']} | {mb:.1f} | {fmt(new)} | {fmt(old)} | {sum(new) / sum(old):.2f} | {streams * mb / new[2]:.2f} | "
              f"{fmt(res[1]) if res else ''} |")
    names = {op: t[2] for (_dt, _l, op), t in table.items()}
    print("\nkernel names per op:", json.dumps(names))


def step(a):
    import torch
    import vit_reference as vr
    import vit_decoder_reference as dr
    from causal_vae_amd import FusedAdam
    from causal_vae_amd.vit import GraphedViTTrainStep, ViTVAE
    if not torch.cuda.is_available():
        sys.exit("vit_decoder_bn_probe: no GPU: nothing is measured without one")
    if a.steps < 20:
        sys.exit("vit_decoder_bn_probe: --steps of at least 20 (a round ends in one synchronize)")
    res = {"probe": "vit_decoder_bn_step", "img": list(a.img), "depth": a.depth, "batch": a.batch, "steps_per_round": a.steps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    configs = (("eval", {}), ("stem", dict(stem_batch_stats=True)), ("stem_decoder", dict(stem_batch_stats=True, decoder_batch_stats=True)))
    for name, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        if name not in a.dtypes:
            continue
        torch.manual_seed(0)
        base = ViTVAE(img_size=tuple(a.img), depth=a.depth, latent_dim=128)
        vr.randomize_stem_bn(base.stem, 1)
        dr.randomize_decoder_bn(base.decoder, 2)
        base = base.to("cuda").eval().set_compute_dtype(dtype)
        x = vr.vit_inputs(a.batch, *a.img, seed=3).to("cuda")
        legs = {}
        for cfg, kw in configs:
            model = copy.deepcopy(base)
            model.train_all(**kw)
            opt = FusedAdam(model.parameters(), lr=1e-4, device_step=True)
            graphed = GraphedViTTrainStep(model, opt, (x,), warmup=a.warmup)
            legs[cfg] = (lambda gr: (lambda: gr(x)))(graphed)
        for _ in range(a.warmup):
            for leg in legs.values():
                leg()
        rounds = {k: [] for k in legs}
        for _ in range(a.rounds):                          # interleaved: every leg sees the same minutes of a shared host
            for k, leg in legs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                s.record()
                for _i in range(a.steps):
                    leg()
                e.record()
                torch.cuda.synchronize()
                rounds[k].append(s.elapsed_time(e) / a.steps)
        res[name] = {k: dict(median_ms=round(statistics.median(v), 3), min_max_ms=[round(min(v), 3), round(max(v), 3)]) for k, v in rounds.items()}
        del legs, base
        torch.cuda.empty_cache()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("kernels", "parse", "step"):
        p = sub.add_parser(name)
        p.add_argument("--img", type=int, nargs=2, default=(768, 1280))
        p.add_argument("--batch", type=int, default=8)
        if name != "step":
            p.add_argument("--manifest", required=True)
        if name == "parse":
            p.add_argument("dir")
        if name == "step":
            p.add_argument("--depth", type=int, default=6)
            p.add_argument("--steps", type=int, default=20)
            p.add_argument("--rounds", type=int, default=5)
            p.add_argument("--warmup", type=int, default=3)
            p.add_argument("--dtypes", nargs="*", default=["bf16", "f32"])
    a = ap.parse_args()
    {"kernels": kernels, "parse": parse, "step": step}[a.cmd](a)


if __name__ == "__main__":
    main()

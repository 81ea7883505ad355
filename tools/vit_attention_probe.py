"""What looking inside the encoder costs: ViTVAE at 768 x 1280, depth 6, B = 1 and 8, fp32 and bf16, printed as ONE JSON line.
Five calls on one model and one batch, interleaved in one process after warm-up:
  cls_features(x) ........... the encoder itself, the yardstick
  attention_weights(x) ...... the CLS rows of every block, head-averaged: the same walk with lse saved + one mhsa_weights launch per block
  attention_rollout(x) ...... the same walk + one mhsa_rollout_step launch per block
  gradcam(x) ................ the saving walk + the data-only backward down to dstem + one Grad-CAM launch: the backward attention_relevance rides on
  attention_relevance(x) .... that walk and backward + one mhsa_relevance_step (kernel and, past 64 query rows, its finish launch) per block
A round is `--steps` calls of one of them issued back to back and ended by ONE synchronize; the figure is the host wall time over the round per call, the
median over `--rounds` rounds (minimum and maximum next to it).
`--only NAME [NAME ...]` (of the five) runs a few calls of those, alternating, in bf16 at B = 8: the shape for a separate
`rocprofv3 --kernel-trace --stats` run; two names put both calls' kernels into one trace."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr                            # noqa: E402
from causal_vae_amd.vit import ViTVAE                 # noqa: E402

CALLS = ("cls_features", "attention_weights", "attention_rollout", "gradcam", "attention_relevance")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=CALLS, nargs="+")
    a = ap.parse_args()
    torch.manual_seed(42)
    model = ViTVAE()
    vr.randomize_stem_bn(model.stem, 4242)
    model = model.requires_grad_(False).cuda().eval()
    if a.only:
        model.set_compute_dtype(torch.bfloat16)
        x = vr.vit_inputs(8, 768, 1280, 1302).cuda()
        for _ in range(a.warmup + a.steps):
            for name in a.only:
                getattr(model, name)(x)
        torch.cuda.synchronize()
        return
    out = {"probe": "vit_attention", "img": [768, 1280], "depth": model.depth, "steps_per_round": a.steps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    for dt, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        model.set_compute_dtype(dt)
        out[tag] = []
        for B in (1, 8):
            x = vr.vit_inputs(B, 768, 1280, 1302).cuda()
            fns = {n: (lambda n=n: getattr(model, n)(x)) for n in CALLS}
            for _ in range(a.warmup):
                for f in fns.values():
                    f()
            torch.cuda.synchronize()
            ts = {n: [] for n in CALLS}
            for _ in range(a.rounds):
                for n, f in fns.items():
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        f()
                    torch.cuda.synchronize()
                    ts[n].append((time.perf_counter() - t0) * 1e3 / a.steps)
            row = {"batch": B}
            for n in CALLS:
                row[n + "_ms"] = round(statistics.median(ts[n]), 3)
                row[n + "_min_max_ms"] = [round(min(ts[n]), 3), round(max(ts[n]), 3)]
            for n in CALLS[1:]:
                row[n + "_over_cls_features"] = round(row[n + "_ms"] / row["cls_features_ms"], 3)
            out[tag].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

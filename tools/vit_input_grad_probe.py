"""What the gradient with respect to the image costs: ViTVAE at 768 x 1280, depth 6, B = 1 and 8, fp32 and bf16, printed as ONE JSON line.
Calls on one model and one batch, interleaved in one process after warm-up:
  cls_features(x) .................. the encoder's inference walk, the yardstick
  encode_vjp(x, g_mu, g_lv) ........ the saving walk + the data-only backward down to the image (no weight-gradient launch); the model frozen
  encode_with_grad + backward ...... after train_stem() + train_transformer(), x NOT asking: every parameter's gradient, no image launch — the launches the
                                     parent commit issues for this call, so this figure is the parent's
  the same with x.requires_grad .... the full backward plus the one image launch
  gradcam(x) ....................... the saving walk without the stem's activations + the data-only backward down to dstem + one Grad-CAM launch
A round is `--steps` calls of one of them issued back to back and ended by ONE synchronize; the figure is the host wall time over the round per call, the
median over `--rounds` rounds (minimum and maximum next to it).  Records, not thresholds."""
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

CALLS = ("cls_features", "encode_vjp", "full_backward", "full_backward_with_image", "gradcam")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch.manual_seed(42)
    frozen, live = ViTVAE(), ViTVAE()
    live.load_state_dict(frozen.state_dict())
    for m in (frozen, live):
        vr.randomize_stem_bn(m.stem, 4242)
        m.requires_grad_(False).cuda().eval()
    live.train_stem()
    live.train_transformer()
    out = {"probe": "vit_input_grad", "img": [768, 1280], "depth": frozen.depth, "steps_per_round": a.steps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    for dt, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        frozen.set_compute_dtype(dt)
        live.set_compute_dtype(dt)
        out[tag] = []
        for B in (1, 8):
            x = vr.vit_inputs(B, 768, 1280, 1302).cuda()
            g = torch.Generator().manual_seed(7)
            gm, gl = torch.randn(B, 128, generator=g).cuda(), torch.randn(B, 128, generator=g).cuda()

            def full(asks):
                live.zero_grad(set_to_none=True)
                mu, lv = live.encode_with_grad(x.clone().requires_grad_(asks))
                torch.autograd.backward([mu, lv], [gm, gl])

            fns = {"cls_features": lambda: frozen.cls_features(x), "encode_vjp": lambda: frozen.encode_vjp(x, gm, gl), "full_backward": lambda: full(False),
                   "full_backward_with_image": lambda: full(True), "gradcam": lambda: frozen.gradcam(x)}
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
            row["encode_vjp_over_full_backward"] = round(row["encode_vjp_ms"] / row["full_backward_ms"], 3)
            out[tag].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

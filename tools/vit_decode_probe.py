"""ViTVAE.decode timings at 768 x 1280 (device events, median of --reps after --warmup), printed as ONE JSON line:
  hip_{f32,bf16}_b{B}_ms ..... ViTVAE.decode on the gfx950 kernels
  eager_{f32,bf16}_b{B}_ms ... the baseline: the restatement of the reference decoder (tests/vit_decoder_reference.py:decode_ref, BatchNorm folded per call
                               as the product does) run eagerly by stock torch in that dtype on the same GPU in the same session — the parent of this
                               feature has no decoder to compare with
`--batches 1,8,32` picks the batch sizes; `--only B` runs just batch B in `--dtype` a few times without the baseline: the shape for a separate
`rocprofv3 --kernel-trace --stats` run (launch count, per-kernel time)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr                            # noqa: E402
import vit_decoder_reference as dr                    # noqa: E402
from causal_vae_amd.vit import ViTVAE                 # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--dtype", default="bf16", choices=("f32", "bf16"))
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(42)
    model = ViTVAE(depth=1)
    dr.randomize_decoder_bn(model.decoder, 4343)
    model = model.cuda().eval()
    sd = {k: v.detach() for k, v in model.state_dict().items() if k.startswith("decoder")}
    dts = {"f32": torch.float32, "bf16": torch.bfloat16}
    out = {}
    for B in ([a.only] if a.only else [int(v) for v in a.batches.split(",")]):
        z = dr.dec_inputs(B, 128, 1313).cuda()
        for tag in ([a.dtype] if a.only else ["f32", "bf16"]):
            dt = dts[tag]
            model.set_compute_dtype(dt)
            out[f"hip_{tag}_b{B}_ms"] = round(timed(lambda: model.decode(z), a.reps, a.warmup), 3)
            if not a.only and not a.no_eager:
                sd_dt = {k: v.to(dt) for k, v in sd.items() if v.is_floating_point()}       # cast once, outside the timed region
                with torch.no_grad():
                    out[f"eager_{tag}_b{B}_ms"] = round(timed(lambda: dr.decode_ref(sd_dt, z, (24, 40), dtype=dt)["image"], a.reps, a.warmup), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

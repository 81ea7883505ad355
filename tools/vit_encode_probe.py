"""ViTVAEEncoder.encode timings at 768 x 1280 (device events, median of --reps after --warmup), printed as ONE JSON line:
  hip_{f32,bf16}_b{1,8,32}_ms ..... ViTVAEEncoder.encode on the gfx950 kernels
  eager_{f32,bf16}_b{1,8,32}_ms ... the baseline: the same restatement (tests/vit_reference.py:encode_ref) run eagerly by stock torch in that dtype on
                                    the same GPU in the same session — what a user of this package had before the encoder existed
`--only B` runs just batch B in bf16 a few times: the shape for a separate `rocprofv3 --kernel-trace --stats` run."""
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
from causal_vae_amd.vit import ViTVAEEncoder          # noqa: E402


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
    ap.add_argument("--only", type=int, default=0)
    a = ap.parse_args()
    torch.manual_seed(42)
    model = ViTVAEEncoder()
    vr.randomize_stem_bn(model.stem, 4242)
    model = model.cuda().eval()
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    out = {}
    for B in ([a.only] if a.only else [1, 8, 32]):
        x = vr.vit_inputs(B, 768, 1280, 1302).cuda()
        for dt, tag in ((torch.bfloat16, "bf16"),) if a.only else ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
            model.set_compute_dtype(dt)
            out[f"hip_{tag}_b{B}_ms"] = round(timed(lambda: model.encode(x), a.reps, a.warmup), 3)
            if not a.only:
                sd_dt = {k: v.to(dt) for k, v in sd.items() if v.is_floating_point()}       # cast once, outside the timed region
                with torch.no_grad():
                    out[f"eager_{tag}_b{B}_ms"] = round(timed(lambda: vr.encode_ref(sd_dt, x, 6, dtype=dt, cls_only_last=True), a.reps, a.warmup), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

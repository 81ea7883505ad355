"""Timings of one ViTVAE training step at 768 x 1280 (depth 6), eager against captured, ONE JSON line.
Per case (f32, bf16, f32 with dropout) and batch (1, 8), two legs on two copies of one model, both with FusedAdam(device_step=True):
  eager      vit_vae_train_step issued from Python (with dropout: host keys) — the path train_vit_vae takes without graph=True
  captured   GraphedViTTrainStep replayed (with dropout: device keys, one key-table launch per step inside the graph)
After both are warm, --rounds rounds alternate the legs; a leg's round is --steps steps (at least 20) issued back to back and ended by ONE synchronize.
  *_wall_ms   host wall clock over the round, from before the first step to after the synchronize, per step: what a training loop sees
  *_event_ms  device events around the same round, per step
both as the median over rounds, with the rounds' minimum and maximum next to the wall figure.  Records, not thresholds: profiles/vit_train_graph.md."""
import argparse
import copy
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
import vit_decoder_reference as dr                    # noqa: E402
from causal_vae_amd import FusedAdam                  # noqa: E402
from causal_vae_amd.vit import GraphedViTTrainStep, ViTVAE, vit_vae_train_step   # noqa: E402

CASES = (("f32", torch.float32, False), ("bf16", torch.bfloat16, False), ("f32_dropout", torch.float32, True))


def one_round(step, n):
    """(wall ms, event ms) per step of n steps ended by one synchronize"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.record()
    for _ in range(n):
        step()
    e.record()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n, s.elapsed_time(e) / n


def case(img, depth, dtype, dropout, B, a):
    torch.manual_seed(0)
    model = ViTVAE(img_size=img, depth=depth, latent_dim=128)
    vr.randomize_stem_bn(model.stem, 1)
    dr.randomize_decoder_bn(model.decoder, 2)
    model = model.to("cuda").eval().set_compute_dtype(dtype)
    model.train_all(dropout=dropout)
    x = vr.vit_inputs(B, *img, seed=3).to("cuda")
    eager_model, graph_model = model, copy.deepcopy(model)
    eager_opt = FusedAdam(eager_model.parameters(), lr=1e-4, device_step=True)
    graph_opt = FusedAdam(graph_model.parameters(), lr=1e-4, device_step=True)
    graphed = GraphedViTTrainStep(graph_model, graph_opt, (x,), warmup=a.warmup)
    legs = {"eager": lambda: vit_vae_train_step(eager_model, eager_opt, x), "captured": lambda: graphed(x)}
    for _ in range(a.warmup):
        for leg in legs.values():
            leg()
    rounds = {k: [] for k in legs}
    for _ in range(a.rounds):                          # interleaved: both legs see the same minutes of a shared host
        for k, leg in legs.items():
            rounds[k].append(one_round(leg, a.steps))
    out = {"batch": B}
    for k, r in rounds.items():
        wall, ev = [w for w, _e in r], [e for _w, e in r]
        out[f"{k}_wall_ms"], out[f"{k}_event_ms"] = round(statistics.median(wall), 3), round(statistics.median(ev), 3)
        out[f"{k}_wall_min_max_ms"] = [round(min(wall), 3), round(max(wall), 3)]
    out["captured_over_eager_wall"] = round(out["captured_wall_ms"] / out["eager_wall_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--img", type=int, nargs=2, default=(768, 1280))
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--batches", type=int, nargs="*", default=(1, 8))
    ap.add_argument("--cases", nargs="*", default=[c[0] for c in CASES])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vit_train_graph_probe: no GPU: nothing is measured without one")
    if a.steps < 20:
        sys.exit("vit_train_graph_probe: --steps of at least 20 (a round ends in one synchronize; fewer steps time the synchronize)")
    res = {"probe": "vit_train_graph", "img": list(a.img), "depth": a.depth, "steps_per_round": a.steps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    for name, dtype, dropout in CASES:
        if name in a.cases:
            res[name] = [case(tuple(a.img), a.depth, dtype, dropout, B, a) for B in a.batches]
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""CausalViTVAE adapter training at 768 x 1280, B = 8 (device events, median of --reps after --warmup, the compared forms interleaved in one session),
ONE JSON line per run:
  step_{f32,bf16}_ms               forward_train + the vessel loss + backward (the gradients of the 20 head tensors; no optimizer step)
  heads_{f32,bf16}_ms              the three heads alone, training forward + backward with fixed cotangents (ops.mlp_heads_train): their share of the step
  heads_unfused_ms                 the same three heads composed from the unfused differentiable ops (ops.cat, ops.Linear, ops.BatchNorm1dTrain,
                                   ops.Activation, ops.Clamp, ops.Reparameterize), forward + backward, in the same run
  heads_share_{f32,bf16}           heads / step"""
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
import causal_vit_reference as cr                     # noqa: E402
from causal_vae_amd import ops                        # noqa: E402
from causal_vae_amd.vessel.train import loss_function, total_loss   # noqa: E402
from causal_vae_amd.vit import CausalViTVAE           # noqa: E402


def interleaved(fns, reps, warmup):
    """median device time of each callable, the callables taking turns"""
    for _ in range(warmup):
        for f in fns:
            f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            torch.cuda.synchronize()
            ts[i].append(s.elapsed_time(e))
    return [statistics.median(t) for t in ts]


def unfused_adapter(ad, panels, clamps=None, eps=None):
    bn = ad[1]
    h = ops.Linear.apply(ops.cat(panels), ad[0].weight, ad[0].bias, None)
    h = ops.Activation.apply(ops.BatchNorm1dTrain.apply(h, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps), "leaky02")
    y = ops.Linear.apply(h, ad[3].weight, ad[3].bias, None)
    if clamps is None:
        return (y,)
    mu, lv = (c.contiguous() for c in y.chunk(2, dim=1))
    mu, lv = ops.Clamp.apply(mu, *clamps[0]), ops.Clamp.apply(lv, *clamps[1])
    return mu, lv, ops.Reparameterize.apply(mu, lv, eps)


def unfused_morph(model, t):
    s = model.morph_predictor_shared
    h = ops.Linear.apply(t, s[0].weight, s[0].bias, "leaky02")
    h = ops.Linear.apply(h, s[2].weight, s[2].bias, "leaky02")
    return (ops.Linear.apply(h, model.morph_predictor_mu.weight, model.morph_predictor_mu.bias, None),
            ops.Clamp.apply(ops.Linear.apply(h, model.morph_predictor_logvar.weight, model.morph_predictor_logvar.bias, None), -10.0, 10.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    torch.manual_seed(42)
    model = CausalViTVAE()
    vr.randomize_stem_bn(model.backbone.stem, 4242)
    dr.randomize_decoder_bn(model.backbone.decoder, 4343)
    cr.randomize_head_bn(model, 4444)
    model = model.cuda()
    params = model.train_adapters()
    model.train()
    B = a.batch
    x, m, t, eps = (v.cuda() for v in cr.causal_inputs(B, 768, 1280, 1321))
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()
    cls, c_mu, c_lv, c_z, c_out, c_m = rnd(B, 256), rnd(B, 128), rnd(B, 128), rnd(B, 128), rnd(B, 512), rnd(B, 12)
    clamps = ((-100.0, 100.0), (-10.0, 10.0))

    def step():
        out = model.forward_train(x, m, t, eps)
        total_loss(*loss_function(out[0], x, out[1], m, *out[2:])).backward()
        for p in params:
            p.grad = None

    def heads(fused):
        if fused:
            mu, lv, z = ops.mlp_heads_train([cls, m, t], model.enc_adapter.head_layers(), split=128, clamp0=clamps[0], clamp1=clamps[1], eps=eps)
            m_mu, m_lv, _ = ops.mlp_heads_train([t], model.morph_layers(), clamp1=clamps[1])
            z_vit = ops.mlp_heads_train([m, z], model.dec_adapter.head_layers())[0]
        else:
            mu, lv, z = unfused_adapter(model.enc_adapter, [cls, m, t], clamps, eps)
            m_mu, m_lv = unfused_morph(model, t)
            z_vit = unfused_adapter(model.dec_adapter, [m, z])[0]
        torch.autograd.backward([z_vit, mu, lv, m_mu, m_lv], [c_out, c_mu, c_lv, c_m, c_m])
        for p in params:
            p.grad = None

    out = {"batch": B}
    f, u = interleaved([lambda: heads(True), lambda: heads(False)], a.reps, a.warmup)
    out["heads_unfused_ms"] = round(u, 3)
    for tag, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        model.set_compute_dtype(dt)
        s, h = interleaved([step, lambda: heads(True)], max(3, a.reps // 2), a.warmup)
        out[f"step_{tag}_ms"], out[f"heads_{tag}_ms"], out[f"heads_share_{tag}"] = round(s, 3), round(h, 3), round(h / s, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""CausalViTVAE timings at 768 x 1280 (device events, median of --reps after --warmup, the compared forms interleaved in one session), ONE JSON line:
  heads_{enc,dec,morph}_b{B}_{fused,unfused}_us  one cvae_mlp_heads_fwd launch against the same head composed from the entry points that existed before it
                                                 (ops.cat, ops.Linear, ops.bn1d_eval, ops.Activation, ops.Clamp, chunk copies, ops.Reparameterize)
  forward_{f32,bf16}_b{B}_ms / eager_...         CausalViTVAE.forward against the float restatement of the reference model (tests/causal_vit_reference.py)
                                                 run eagerly by stock torch in that dtype on the same GPU
  decode64_{f32,bf16}_ms                         model.decode of 64 rows (the analysis sweeps' chunk)
  latent_to_grid_k512_b{16,64}_{f32,bf16}_us     cvae_latent_to_grid alone at the production latent width
`--trace forward|decode64` runs just that call three times in --dtype: the shape for a separate `rocprofv3 --kernel-trace --stats` run (launch
counts, per-kernel shares)."""
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
    """the adapter from the library's earlier entry points: what a forward cost before the fused kernel"""
    h = ops.Linear.apply(ops.cat(panels), ad[0].weight, ad[0].bias, None)
    h = ops.Activation.apply(ops.bn1d_eval(h, ad[1].weight, ad[1].bias, ad[1].running_mean, ad[1].running_var, ad[1].eps), "leaky02")
    y = ops.Linear.apply(h, ad[3].weight, ad[3].bias, None)
    if clamps is None:
        return y
    mu, lv = (c.contiguous() for c in y.chunk(2, dim=1))
    mu, lv = ops.Clamp.apply(mu, *clamps[0]), ops.Clamp.apply(lv, *clamps[1])
    return mu, lv, ops.Reparameterize.apply(mu, lv, eps)


def unfused_morph(model, t):
    s = model.morph_predictor_shared
    h = ops.Linear.apply(t, s[0].weight, s[0].bias, "leaky02")
    h = ops.Linear.apply(h, s[2].weight, s[2].bias, "leaky02")
    return (ops.Linear.apply(h, model.morph_predictor_mu.weight, model.morph_predictor_mu.bias, None),
            ops.Clamp.apply(ops.Linear.apply(h, model.morph_predictor_logvar.weight, model.morph_predictor_logvar.bias, None), -10.0, 10.0))


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", default="", choices=("", "forward", "decode64"))
    ap.add_argument("--dtype", default="bf16", choices=("f32", "bf16"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    dts = {"f32": torch.float32, "bf16": torch.bfloat16}
    torch.manual_seed(42)
    model = CausalViTVAE()
    vr.randomize_stem_bn(model.backbone.stem, 4242)
    dr.randomize_decoder_bn(model.backbone.decoder, 4343)
    cr.randomize_head_bn(model, 4444)
    model = model.cuda().eval()
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()
    if a.trace:
        model.set_compute_dtype(dts[a.dtype])
        x, m, t, eps = (v.cuda() for v in cr.causal_inputs(a.batch, 768, 1280, 1321))
        z64, m64 = rnd(64, 128), rnd(64, 12)
        for _ in range(3):
            _ = model(x, m, t, eps) if a.trace == "forward" else model.decode(z64, m64)
        torch.cuda.synchronize()
        return
    out = {}
    clamps = ((-100.0, 100.0), (-10.0, 10.0))
    for B in (1, 8, 64, 768):
        cls, m, t, eps, z = rnd(B, 256), rnd(B, 12), rnd(B, 19), rnd(B, 128), rnd(B, 128)
        pairs = {"enc": (lambda: model.enc_adapter.fused([cls, m, t], split=128, clamp0=clamps[0], clamp1=clamps[1], eps=eps),
                         lambda: unfused_adapter(model.enc_adapter, [cls, m, t], clamps, eps)),
                 "dec": (lambda: model.dec_adapter.fused([m, z]), lambda: unfused_adapter(model.dec_adapter, [m, z])),
                 "morph": (lambda: model.predict_morph(t), lambda: unfused_morph(model, t))}
        for name, fns in pairs.items():
            f, u = interleaved(fns, a.reps, a.warmup)
            out[f"heads_{name}_b{B}_fused_us"], out[f"heads_{name}_b{B}_unfused_us"] = round(1e3 * f, 1), round(1e3 * u, 1)
    W, b = model.backbone.decoder_input.weight, model.backbone.decoder_input.bias
    for B in (16, 64):
        zz = rnd(B, 512)
        for tag, dt in dts.items():
            out[f"latent_to_grid_k512_b{B}_{tag}_us"] = round(1e3 * interleaved([lambda: ops.latent_to_grid(zz, W, b, 256, dt)], a.reps, a.warmup)[0], 1)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    z64, m64 = rnd(64, 128), rnd(64, 12)
    for tag, dt in dts.items():
        model.set_compute_dtype(dt)
        out[f"decode64_{tag}_ms"] = round(interleaved([lambda: model.decode(z64, m64)], max(3, a.reps // 4), 2)[0], 3)
        sd_dt = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}       # cast once, outside the timed region
        for B in (1, 8):
            x, m, t, eps = (v.cuda() for v in cr.causal_inputs(B, 768, 1280, 1321))
            fns = [lambda: model(x, m, t, eps)]
            if not a.no_eager:
                fns.append(lambda: cr.forward_ref(sd_dt, x.to(dt), m, t, eps, 6, dtype=dt)["recon_x"])
            r = interleaved(fns, max(3, a.reps // 2), a.warmup)
            out[f"forward_{tag}_b{B}_ms"] = round(r[0], 3)
            if not a.no_eager:
                out[f"eager_{tag}_b{B}_ms"] = round(r[1], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

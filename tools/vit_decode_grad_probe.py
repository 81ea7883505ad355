"""Timings of the ViT-VAE decoder's latent gradient at 768 x 1280 with latent 512 (decoder_input's weight: 503 MB), device events, median of --reps after
--warmup, ONE JSON line.  Per dtype (f32, bf16) and batch (1, 8):
  decode_ms                  ViTVAE.decode
  backward_ms                ViTVAE._decode_backward on the activations a decode_with_grad forward saved (the whole chain, one event pair)
  launches                   [name, microseconds] of every launch of that chain in order (one event pair per call of the ops layer, median over reps)
  eager_backward_ms          torch.autograd.grad through the float restatement of the same decoder (tests/vit_decoder_reference.decode_ref) run eagerly by stock
                             torch in that dtype on the same GPU, backward only (the graph is built once, outside the timed region), interleaved with backward_ms
  l2g_bwd_us / _tbps         cvae_latent_to_grid_bwd alone and decoder_input's weight bytes over that time
  l2g_fwd_us / _tbps         cvae_latent_to_grid (the forward, unchanged) on the same weight in the same run
`--weights`: the weight-gradient leg instead — per dtype and batch, interleaved in one run:
  backward_dz_ms             the dz-only backward (the frozen path: what the parent runs)
  backward_w_ms              the same chain with every decoder parameter's gradient (ViTVAE._decode_backward(saved, cot, z))
  eager_backward_w_ms        torch.autograd.grad with respect to z AND the 48 live parameters through the eager restatement, backward only
  launches_w                 [name, microseconds] of every launch of the chain with weights, the new entries included
`--trace` runs decode_vjp three times in --dtype at --batch: the shape for a separate `rocprofv3 --kernel-trace --stats` run."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_decoder_reference as dr                    # noqa: E402
from causal_vae_amd import ops                        # noqa: E402
from causal_vae_amd.vit import ViTVAE                 # noqa: E402

TIMED = ("conv_s1_c1_bwd_data", "conv_s1_bwd_data", "_conv_down", "pack_weight", "latent_to_grid_bwd")
TIMED_W = TIMED + ("conv_s1_c1_wgrad", "conv_s1_wgrad", "_conv_wgrad", "latent_to_grid_wgrad", "fold_bn_conv_bwd")


def interleaved(fns, reps, warmup):
    """median device time (ms) of each callable, the callables taking turns"""
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


def per_launch(model, saved, cot, reps, z=None):
    """[name, median us] per ops-layer call of the backward chain: the calls are wrapped with event pairs for the duration of this function"""
    log, originals = [], {n: getattr(ops, n) for n in (TIMED if z is None else TIMED_W)}

    def wrap(name, fn):
        def run(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            shape = tuple(out.shape) if torch.is_tensor(out) else (tuple(out[0].shape) if isinstance(out, tuple) and torch.is_tensor(out[0]) else ())
            log[-1].append((f"{name} -> {shape}", s, e))
            return out
        return run

    try:
        for n, fn in originals.items():
            setattr(ops, n, wrap(n, fn))
        for _ in range(reps):
            log.append([])
            model._decode_backward(saved, cot, z)
        torch.cuda.synchronize()
    finally:
        for n, fn in originals.items():
            setattr(ops, n, fn)
    return [[log[0][i][0], round(1e3 * statistics.median(r[i][1].elapsed_time(r[i][2]) for r in log), 1)] for i in range(len(log[0]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--latent", type=int, default=512)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--weights", action="store_true")
    ap.add_argument("--dtype", default="bf16", choices=("f32", "bf16"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    dts = {"f32": torch.float32, "bf16": torch.bfloat16}
    torch.manual_seed(42)
    model = ViTVAE(latent_dim=a.latent, depth=1)
    dr.randomize_decoder_bn(model.decoder, 4343)
    model = model.cuda().eval().freeze_decoder()
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()
    if a.trace:
        model.set_compute_dtype(dts[a.dtype])
        z, cot = rnd(a.batch, a.latent), rnd(a.batch, 1, 768, 1280)
        for _ in range(3):
            model.decode_vjp(z, cot)
        torch.cuda.synchronize()
        return
    out = {"latent": a.latent}
    if a.weights:
        names = [k for k, _p in model.named_parameters() if k.startswith(("decoder_input.", "decoder."))]
        for tag, dt in dts.items():
            model.set_compute_dtype(dt)
            for B in (1, 8):
                z, cot = rnd(B, a.latent), rnd(B, 1, 768, 1280)
                with torch.no_grad():
                    _img, saved = model._decode_walk(z, save=True, keep_inputs=True)
                fns = [lambda: torch.no_grad()(model._decode_backward)(saved, cot), lambda: torch.no_grad()(model._decode_backward)(saved, cot, z)]
                if not a.no_eager:
                    live = {k: (v.detach().to(dt).requires_grad_(k in names) if v.is_floating_point() else v) for k, v in model.state_dict().items()}
                    zz = z.clone().requires_grad_(True)
                    image = dr.decode_ref(live, zz.to(dt), (24, 40), dtype=dt)["image"]
                    cot_dt = cot.to(dt)
                    fns.append(lambda: torch.autograd.grad(image, [zz] + [live[k] for k in names], cot_dt, retain_graph=True))
                r = interleaved(fns, a.reps, a.warmup)
                out[f"backward_dz_{tag}_b{B}_ms"], out[f"backward_w_{tag}_b{B}_ms"] = round(r[0], 3), round(r[1], 3)
                if not a.no_eager:
                    out[f"eager_backward_w_{tag}_b{B}_ms"] = round(r[2], 3)
                    del image, live
                with torch.no_grad():
                    out[f"launches_w_{tag}_b{B}"] = per_launch(model, saved, cot, a.reps, z)
                del saved
        print(json.dumps(out))
        return
    W, b = model.decoder_input.weight, model.decoder_input.bias
    wbytes = W.numel() * 4
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    for tag, dt in dts.items():
        model.set_compute_dtype(dt)
        sd_dt = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}       # cast once, outside the timed region
        for B in (1, 8):
            z, cot = rnd(B, a.latent), rnd(B, 1, 768, 1280)
            with torch.no_grad():
                _img, saved = model._decode_walk(z, save=True)
                fns = [lambda: model.decode(z), lambda: model._decode_backward(saved, cot)]
                if a.no_eager:
                    r = interleaved(fns, a.reps, a.warmup)
            if not a.no_eager:
                zz = z.clone().requires_grad_(True)
                image = dr.decode_ref(sd_dt, zz.to(dt), (24, 40), dtype=dt)["image"]
                cot_dt = cot.to(dt)
                guarded = [lambda f=f: torch.no_grad()(f)() for f in fns]
                r = interleaved(guarded + [lambda: torch.autograd.grad(image, zz, cot_dt, retain_graph=True)], a.reps, a.warmup)
                out[f"eager_backward_{tag}_b{B}_ms"] = round(r[2], 3)
                del image
            out[f"decode_{tag}_b{B}_ms"], out[f"backward_{tag}_b{B}_ms"] = round(r[0], 3), round(r[1], 3)
            with torch.no_grad():
                out[f"launches_{tag}_b{B}"] = per_launch(model, saved, cot, a.reps)
                grid = rnd(B, 960, 256).to(dt)
                tb, tf = interleaved([lambda: ops.latent_to_grid_bwd(grid, W), lambda: ops.latent_to_grid(z, W, b, 256, dt)], a.reps, a.warmup)
            for name, t in (("l2g_bwd", tb), ("l2g_fwd", tf)):
                out[f"{name}_{tag}_b{B}_us"], out[f"{name}_{tag}_b{B}_tbps"] = round(1e3 * t, 1), round(wbytes / (t * 1e-3) / 1e12, 3)
            del saved
    print(json.dumps(out))


if __name__ == "__main__":
    main()

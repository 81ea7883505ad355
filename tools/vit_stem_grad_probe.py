"""Timings of training the ViT-VAE conv stem at 768 x 1280 (depth 6), device events, median of --reps after --warmup, interleaved, ONE JSON line.
Per dtype (f32, bf16) and batch (1, 8):
  (a) fwd_bwd_frozen_ms          encode_with_grad forward + backward after train_transformer() alone (the parent's path: the stem runs in the forward only)
      fwd_bwd_stem_ms            the same after train_stem() + train_transformer(): the five layer outputs kept, the stem's backward behind the blocks
      stem_launches              [name, microseconds] of every ops-layer call of the stem's backward in order (1 gated token launch, 5 weight gradients, 4 weight
                                 packs, 4 gated data gradients, 1 fold), median over reps
  (b) gated_us / two_launch_us   ONE gated data gradient (cvae_conv_down_bwd_data, leaky001) at the first two stem layers' shapes (64 -> 32 into 384 x 640, 128 -> 64
                                 into 192 x 320) against cvae_conv_up followed by cvae_act_bwd: the two-launch form the parent has
  (c) train_step_ms              one train_vit_vae step (forward_train, vit_vae_loss, backward, Adam) on a depth-6 ViTVAE
      eager_train_step_ms        the same step through the eager torch restatement of the model on the same GPU (tests/vit_reference.encode_ref's modules: the model's
                                 own nn.Sequential stem, nn.MultiheadAttention blocks and decoder stack run by stock torch in eval mode), as profiles/vit_encode.md does
`--trace` runs (a)'s stem leg three times in --dtype at --batch: the shape for a separate `rocprofv3 --kernel-trace --stats` run.  Results: profiles/vit_stem_grad.md."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr                            # noqa: E402
import vit_decoder_reference as dr                    # noqa: E402
from causal_vae_amd import ops                        # noqa: E402
from causal_vae_amd.vit import ViTVAE, vit_vae_loss   # noqa: E402
from vit_decode_grad_probe import interleaved         # noqa: E402

TIMED = ("vit_tokens_bwd", "_conv_wgrad", "pack_weight", "conv_down_bwd_data", "fold_bn_conv_bwd")


def stem_launches(model, x, cot, reps):
    """[name, median us] per ops-layer call from the token backward on.  The calls are wrapped for the duration of this function, and the wrappers record
    only while `on` is set, around the backward: the forward calls pack_weight too."""
    log, originals, on = [], {n: getattr(ops, n) for n in TIMED}, [False]

    def wrap(name, fn):
        def run(*a, **k):
            if not on[0]:
                return fn(*a, **k)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            first = out[0] if isinstance(out, (tuple, list)) else out
            first = first[0] if isinstance(first, (tuple, list)) else first
            log[-1].append((f"{name} -> {tuple(first.shape)}", s, e))
            return out
        return run

    try:
        for n, fn in originals.items():
            setattr(ops, n, wrap(n, fn))
        for _ in range(reps):
            model.zero_grad(set_to_none=True)
            mu, lv = model.encode_with_grad(x)
            log.append([])
            on[0] = True
            torch.autograd.backward([mu, lv], [cot, cot])
            on[0] = False
        torch.cuda.synchronize()
        assert len({len(r) for r in log}) == 1 and len(log[0]) == 15, [len(r) for r in log]
    finally:
        for n, fn in originals.items():
            setattr(ops, n, fn)
    return [[log[0][j][0], round(1e3 * statistics.median(r[j][1].elapsed_time(r[j][2]) for r in log), 1)] for j in range(len(log[0]))]


def eager_model(model, dt):
    """the model's own torch modules, copied into the compute dtype: stock torch runs them in eval mode"""
    m = copy.deepcopy(model).to(dt).eval()
    m.requires_grad_(True)

    def forward(x, eps):
        B = x.shape[0]
        t = m.stem(x.to(dt)).flatten(2).transpose(1, 2)
        t = torch.cat([m.cls_token.expand(B, -1, -1), t], 1) + m.pos_embedding
        for blk in m.transformer:
            y = blk.norm1(t)
            t = t + blk.attn(y, y, y, need_weights=False)[0]
            t = t + blk.mlp(blk.norm2(t))
        c = m.to_latent(t[:, 0])
        mu, lv = m.fc_mu(c), m.fc_var(c)
        z = mu + eps.to(dt) * torch.exp(0.5 * lv)
        h = m.decoder_input(z).view(B, m.embed_dim, m.grid_h, m.grid_w)
        for mod in m.decoder:
            h = h + mod.conv(h) if hasattr(mod, "conv") else mod(h)
        return h, mu, lv
    return m, forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--dtype", default="bf16", choices=("f32", "bf16"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    dts = {"f32": torch.float32, "bf16": torch.bfloat16}
    torch.manual_seed(42)
    model = ViTVAE()
    vr.randomize_stem_bn(model.stem, 4343)
    dr.randomize_decoder_bn(model.decoder, 4344)
    model.requires_grad_(False)
    model = model.cuda().eval()
    g = torch.Generator().manual_seed(1)

    def step(x, cot):
        model.zero_grad(set_to_none=True)
        mu, lv = model.encode_with_grad(x)
        torch.autograd.backward([mu, lv], [cot, cot])

    if a.trace:
        model.set_compute_dtype(dts[a.dtype])
        model.train_stem()
        model.train_transformer()
        x, cot = vr.vit_inputs(a.batch, 768, 1280, seed=2).cuda(), torch.randn(a.batch, model.latent_dim, generator=g).cuda()
        for _ in range(3):
            step(x, cot)
        torch.cuda.synchronize()
        return
    out = {}
    for tag, dt in dts.items():
        model.set_compute_dtype(dt)
        for B in (1, 8):
            x, cot = vr.vit_inputs(B, 768, 1280, seed=2).cuda(), torch.randn(B, model.latent_dim, generator=g).cuda()
            # (a): the two modes cannot be interleaved call by call without flipping flags, so each call sets its own
            def frozen():
                model.freeze_stem()
                step(x, cot)

            def live():
                model.train_stem()
                step(x, cot)

            model.requires_grad_(False)
            model.train_transformer()
            r = interleaved([frozen, live], a.reps, a.warmup)
            out[f"fwd_bwd_frozen_{tag}_b{B}_ms"], out[f"fwd_bwd_stem_{tag}_b{B}_ms"] = round(r[0], 3), round(r[1], 3)
            model.train_stem()
            out[f"stem_launches_{tag}_b{B}"] = stem_launches(model, x, cot, a.reps)
            # (b)
            with torch.no_grad():
                for name, Cs, Cl, sh, sw in (("l1", 64, 32, 192, 320), ("l2", 128, 64, 96, 160)):
                    gg = torch.randn(B, 1, sh, sw, Cs, generator=g).to(dt).cuda()
                    gate = torch.randn(B, 1, 2 * sh, 2 * sw, Cl, generator=g).to(dt).cuda()
                    wp = ops.pack_weight(0.05 * torch.randn(Cs, Cl, 4, 4, generator=g).cuda(), 2, True, dt)
                    r = interleaved([lambda: ops.conv_down_bwd_data(gg, wp, gate, "leaky001"),
                                     lambda: ops._act_bwd(ops._conv_up(gg, wp, None, None, Cl, 2, None), gate, "leaky001")], a.reps, a.warmup)
                    out[f"gated_{name}_{tag}_b{B}_us"], out[f"two_launch_{name}_{tag}_b{B}_us"] = round(1e3 * r[0], 1), round(1e3 * r[1], 1)
                    del gg, gate
            # (c)
            eps = torch.randn(B, model.latent_dim, generator=g).cuda()
            params = model.train_all()
            opt = torch.optim.Adam(params, lr=1e-4)

            def train_step():
                opt.zero_grad()
                vit_vae_loss(*model.forward_train(x, eps)).backward()
                opt.step()

            fns = [train_step]
            if not a.no_eager:
                em, eforward = eager_model(model, dt)
                eopt = torch.optim.Adam(em.parameters(), lr=1e-4)

                def eager_train_step():
                    eopt.zero_grad()
                    rec, mu, lv = eforward(x, eps)
                    (F.mse_loss(rec.float(), x) + -0.5 * torch.mean(1 + lv.float() - lv.float().exp() - mu.float().pow(2))).backward()
                    eopt.step()
                fns.append(eager_train_step)
            r = interleaved(fns, a.reps, a.warmup)
            out[f"train_step_{tag}_b{B}_ms"] = round(r[0], 3)
            if not a.no_eager:
                out[f"eager_train_step_{tag}_b{B}_ms"] = round(r[1], 3)
                del em, eopt
            del opt
            model.requires_grad_(False)
            model.freeze_stem().freeze_transformer().freeze_decoder()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Timings of training the ViT-VAE encoder's transformer at 768 x 1280 (961 tokens, depth 6), device events, median of --reps after --warmup, interleaved,
ONE JSON line.  Per dtype (f32, bf16) and batch (1, 8):
  cls_features_ms            ViTVAEEncoder.cls_features (the inference path: stem + transformer forward)
  fwd_bwd_ms                 cls_features_with_grad forward + backward (every transformer parameter's gradient and dstem; the stem runs in the forward only)
  eager_fwd_bwd_ms           the same transformer through the model's own nn.LayerNorm / nn.MultiheadAttention / nn.Linear modules run eagerly by stock torch in
                             that dtype on the same GPU, forward + torch.autograd backward, from the same stem output (the stem is not part of this leg)
  stem_ms                    the stem alone (what fwd_bwd_ms contains and eager_fwd_bwd_ms does not)
  launches                   [name, microseconds] of every ops-layer call of ONE block's backward chain in order (median over reps)
`--trace` runs forward + backward three times in --dtype at --batch: the shape for a separate `rocprofv3 --kernel-trace --stats` run."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr                            # noqa: E402
from causal_vae_amd import ops                        # noqa: E402
from causal_vae_amd.vit import ViTVAEEncoder          # noqa: E402
from vit_decode_grad_probe import interleaved         # noqa: E402

TIMED = ("token_gemm_bwd_data", "token_gemm_wgrad", "layernorm256_bwd", "mhsa_bwd")


def eager_step(mods, stem, g):
    """forward + backward of the transformer through stock torch modules (a copy of the model's, in the compute dtype)"""
    cls_token, pos, blocks, to_latent = mods
    B = stem.shape[0]
    t = torch.cat([cls_token.expand(B, -1, -1), stem], 1) + pos
    for blk in blocks:
        y = blk.norm1(t)
        t = t + blk.attn(y, y, y, need_weights=False)[0]
        t = t + blk.mlp(blk.norm2(t))
    to_latent(t[:, 0]).backward(g)


def block_launches(model, x, reps):
    """[name, median us] per ops-layer call of the LAST FULL block's backward (from the saving walk's _BlockStep of that block): the calls are wrapped with
    event pairs for the duration of this function"""
    log, originals = [], {n: getattr(ops, n) for n in TIMED}

    def wrap(name, fn):
        def run(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            first = out[0] if isinstance(out, tuple) else out
            log[-1].append((f"{name} -> {tuple(first.shape)}", s, e))
            return out
        return run

    with torch.no_grad():
        _out, saved = model._walk(x, save=True)
        i = model.depth - 2
        try:
            for n, fn in originals.items():
                setattr(ops, n, wrap(n, fn))
            for _ in range(reps):
                log.append([])
                model._block_backward(model.transformer[i], f"transformer.{i}.", saved.steps[i], torch.randn(saved.B * saved.N, 256, device=x.device), {})
            torch.cuda.synchronize()
        finally:
            for n, fn in originals.items():
                setattr(ops, n, fn)
    return [[log[0][j][0], round(1e3 * statistics.median(r[j][1].elapsed_time(r[j][2]) for r in log), 1)] for j in range(len(log[0]))]


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
    model = ViTVAEEncoder()
    vr.randomize_stem_bn(model.stem, 4343)
    model.requires_grad_(False)
    model = model.cuda().eval()
    model.train_transformer()
    g = torch.Generator().manual_seed(1)

    def step(x, cot):
        model.zero_grad(set_to_none=True)
        model.cls_features_with_grad(x).backward(cot)

    if a.trace:
        model.set_compute_dtype(dts[a.dtype])
        x, cot = vr.vit_inputs(a.batch, 768, 1280, seed=2).cuda(), torch.randn(a.batch, 256, generator=g).cuda()
        for _ in range(3):
            step(x, cot)
        torch.cuda.synchronize()
        return
    out = {}
    for tag, dt in dts.items():
        model.set_compute_dtype(dt)
        for B in (1, 8):
            x, cot = vr.vit_inputs(B, 768, 1280, seed=2).cuda(), torch.randn(B, 256, generator=g).cuda()
            fns = [lambda: model.cls_features(x), lambda: step(x, cot), lambda: torch.no_grad()(model._stem_cl)(x)]
            if not a.no_eager:
                mods = (copy.deepcopy(model.cls_token).to(dt), copy.deepcopy(model.pos_embedding).to(dt), copy.deepcopy(model.transformer).to(dt),
                        copy.deepcopy(model.to_latent).to(dt))
                with torch.no_grad():
                    stem = model._stem_cl(x).view(B, -1, 256).to(dt)
                cot_dt = cot.to(dt)
                fns.append(lambda: eager_step(mods, stem, cot_dt))
            r = interleaved(fns, a.reps, a.warmup)
            out[f"cls_features_{tag}_b{B}_ms"], out[f"fwd_bwd_{tag}_b{B}_ms"], out[f"stem_{tag}_b{B}_ms"] = round(r[0], 3), round(r[1], 3), round(r[2], 3)
            if not a.no_eager:
                out[f"eager_fwd_bwd_{tag}_b{B}_ms"] = round(r[3], 3)
                del mods
            out[f"launches_{tag}_b{B}"] = block_launches(model, x, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""CausalVesselVAE inference timings (device events, median of --reps after --warmup), printed as ONE JSON line:
  fwd_eval_b8 / enc_dec_folded_b8 .. eval forward vs encode + reparameterize + decode (folded) at B = 8;
  decode64_{f32,bf16}_{unfolded,folded} .. the decoder alone on 64 rows (dec_fc + dec_conv);
  fold_{enc,dec}_MB, fold_{enc,dec}_call_us .. one cvae_fold_bn_conv call for each stack: bytes moved, and the event time of the call (host-side
      preparation included; the kernel's own time comes from the kernel trace of `--only decode`);
  sweep_fused_ms vs sweep_eager_ms .. the 1,300-row feature-importance sweep (analyze_vessel.py:68-121: N = 100, 12 features) through
      vessel.feature_importance vs an eager per-feature loop of the unfolded eval path with torch norms (the reference's code on this package).
`--only decode` runs just the 64-row decodes (folded and unfolded, fp32) a few times: the shape for a separate `rocprofv3 --kernel-trace --stats` run."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from causal_vae_amd import ops                                            # noqa: E402
from causal_vae_amd.vessel import CausalVesselVAE, feature_importance     # noqa: E402


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


def model_with_stats(seed=42):
    torch.manual_seed(seed)
    model = CausalVesselVAE().cuda()
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0.0, 0.1)
                mod.running_var.uniform_(0.5, 1.5)
    return model.eval()


def fold_tables(model):
    """the cvae_fold_bn_conv tables of the encoder and the decoder, as their folded forwards build them"""
    enc, dec = list(model.enc_conv), list(model.dec_conv)
    enc_tab = [(enc[i].weight, ops.FOLD_CONV_K4, enc[i].bias, enc[i + 1]) for i in range(0, 21, 3)]
    dec_tab, i = [], 0
    while i < len(dec):
        bn = dec[i + 2] if isinstance(dec[i + 2], torch.nn.BatchNorm2d) else None
        dec_tab.append((dec[i + 1].weight, ops.FOLD_UPCONV_K3, dec[i + 1].bias, bn))
        i += 4 if bn is not None else 3
    return {"enc": enc_tab, "dec": dec_tab}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["all", "decode"], default="all")
    a = ap.parse_args()
    model = model_with_stats()
    g = torch.Generator().manual_seed(0)
    z64, m64 = torch.randn(64, 128, generator=g).cuda(), torch.randn(64, 12, generator=g).cuda()
    res = {"what": "vessel_infer_probe", "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        if a.only == "decode":
            for _ in range(3):
                ops.fold_bn_conv(fold_tables(model)["enc"])                # the encoder's fold launch too, for its kernel time
            for folded in (False, True):
                torch.cuda.synchronize()
                res[f"decode64_f32_{'folded' if folded else 'unfolded'}_ms"] = timed(lambda: model.decode(z64, m64, folded=folded), 3, 1)
            print(json.dumps(res))
            return
        x = (torch.rand(8, 1, 768, 1280, generator=g) < 0.08).float().cuda()
        m8 = torch.randn(8, 12, generator=g).cuda()
        t8 = torch.nn.functional.one_hot(torch.randint(0, 19, (8,), generator=g), 19).float().cuda()
        eps8 = torch.randn(8, 128, generator=g).cuda()

        def enc_dec():
            mu, lv = model.encode(x, m8, t8)
            return model.decode(model.reparameterize(mu, lv, eps8), m8)
        res["fwd_eval_b8_ms"] = timed(lambda: model(x, m8, t8, eps=eps8), a.reps, a.warmup)
        res["enc_dec_folded_b8_ms"] = timed(enc_dec, a.reps, a.warmup)
        for dt in (torch.float32, torch.bfloat16):
            model.set_compute_dtype(dt)
            name = "f32" if dt == torch.float32 else "bf16"
            res[f"decode64_{name}_unfolded_ms"] = timed(lambda: model.decode(z64, m64, folded=False), a.reps, a.warmup)
            res[f"decode64_{name}_folded_ms"] = timed(lambda: model.decode(z64, m64), a.reps, a.warmup)
        model.set_compute_dtype(torch.float32)
        for name, tab in fold_tables(model).items():
            # bytes: weight + bias read, folded weight + bias written, the BatchNorm vectors read (4 x Cout floats)
            nb = 0
            for w, kind, b, bn in tab:
                cout, cin = w.shape[0], w.shape[1]
                nb += 4 * (w.numel() + cout + cout * cin * 16 + cout + (4 * cout if bn is not None else 0))
            ms = timed(lambda: ops.fold_bn_conv(tab), 20, 3)
            res[f"fold_{name}_MB"] = nb / 1e6
            res[f"fold_{name}_call_us"] = ms * 1e3                      # one call between two events: the host-side launch preparation included
        # the 1,300-row sweep: N = 100 draws, 12 features (+ the 100 base rows)
        N = 100
        zs, ms_ = torch.randn(N, 128, generator=g).cuda(), torch.randn(N, 12, generator=g).cuda()
        res["sweep_fused_ms"] = timed(lambda: feature_importance(model, zs, ms_, chunk_rows=64), 2, 1)

        def eager():
            x_base = model.dec_conv(model.dec_fc(torch.cat([ms_, zs], 1)).view(-1, 512, 6, 10))
            out = []
            for f in range(12):
                m_p = ms_.clone()
                m_p[:, f] += 1.0
                x_p = model.dec_conv(model.dec_fc(torch.cat([m_p, zs], 1)).view(-1, 512, 6, 10))
                out.append((x_p - x_base).view(N, -1).norm(dim=1).mean())
            return torch.stack(out)
        res["sweep_eager_ms"] = timed(eager, 2, 1)
        res["sweep_rows"] = N * 13
    print(json.dumps(res))


if __name__ == "__main__":
    main()

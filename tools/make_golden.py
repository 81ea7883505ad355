#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE's own classes (build container only).

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden.py

What is imported from /root/reference (read-only, nothing is written there):
  * causal_cascade/models.py  -> CausalBioVAE           (a1-a5)
  * causal_cascade/train.py   -> loss_function          (a6)
  * mnist_test/01_baseline_causal_vae/{config,models}.py -> CausalMorphVAE12, LatentDiscriminator (a8)
  * mnist_test/06_model_experiment/{config,models}.py    -> Gaussian-head CausalMorphVAE12
  * vessel_analysis/00_core/models.py: the text of ``CausalVesselVAE`` is compiled with its two unimportable imports dropped (a11)
  * vessel_analysis/00_core/vit_backbone.py -> ViTVAE (eval mode; encode: `python tools/make_golden.py vitvae`, decode: `... vitvae_dec`; the encoder's
    gradients: `... vitvae_grad` (transformer side), `... vitvae_stem_grad` (the conv stem))
  * vessel_analysis/00_core/models.py: the text of ``CausalViTVAE`` is compiled around that ViTVAE (eval mode; `... causal_vitvae`)
  * vessel_analysis/01_train/train.py: only the text of ``loss_function`` is compiled (the module
    itself cannot be imported: it pulls tifffile/torchvision through ``dataset``) (a10)
The MNIST adversarial loop body (mnist_test/01_baseline_causal_vae/train.py:34-93) cannot be imported
(torchvision at module import); its goldens are produced by driving the *imported reference models*
with the same torch calls the loop makes (F.cross_entropy, F.binary_cross_entropy, F.kl_div,
optim.Adam), in the loop's order, with the loop's six eps draws per step.

The fixtures hold data only: inputs, injected eps, outputs, loss scalars, gradients (full for small
tensors, digests for large ones) and state_dict digests.  /root/reference never travels.
"""
import ast
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
sys.dont_write_bytecode = True
torch.set_num_threads(8)
FULL_LIMIT = 20000          # tensors up to this many elements are stored whole


def digest(t):
    """[sum, abs-sum, sum of squares, first 8 values, last 8 values] in float64."""
    f = t.detach().double().flatten()
    head = torch.zeros(8, dtype=torch.float64); tail = torch.zeros(8, dtype=torch.float64)
    n = min(8, f.numel())
    head[:n] = f[:n]; tail[:n] = f[-n:]
    return torch.cat([torch.stack([f.sum(), f.abs().sum(), (f * f).sum()]), head, tail]).numpy()


def pack(prefix, named, store, full_limit=None):
    for k, v in named.items():
        v = v.detach()
        store[f"{prefix}/{k}#digest"] = digest(v)
        store[f"{prefix}/{k}#shape"] = np.array(v.shape, dtype=np.int64)
        if v.numel() <= (FULL_LIMIT if full_limit is None else full_limit):
            store[f"{prefix}/{k}"] = v.numpy().copy()


def import_from(dirname, *modules):
    """Import bare-named modules (config, models, ...) from one reference directory."""
    for name in ("config", "models", "train", "dataset", "cvae_models"):
        sys.modules.pop(name, None)
    sys.path.insert(0, dirname)
    try:
        return [importlib.import_module(mod) for mod in modules]
    finally:
        sys.path.remove(dirname)


def bio2d_case(name, B, H, W, seed_data):
    models, train = import_from(os.path.join(REF, "causal_cascade"), "models", "train")
    torch.manual_seed(42)                              # causal_cascade/main.py:28
    model = models.CausalBioVAE(img_channels=1, m_dim=12, t_dim=19, latent_dim=64)
    model.train()
    store = {}
    pack("sd0", model.state_dict(), store)
    g = torch.Generator().manual_seed(seed_data)
    x = torch.randn(B, 1, H, W, generator=g)
    m = torch.rand(B, 12, generator=g)
    t = torch.randint(0, 19, (B,), generator=g)
    acts = {}
    hooks = []
    for i in range(4):
        hooks.append(model.enc_conv[2 * i + 1].register_forward_hook(
            lambda _m, _i, o, k=f"enc{i+1}": acts.__setitem__(k, o.detach().clone())))
    for i in range(3):
        hooks.append(model.dec_conv[2 * i + 1].register_forward_hook(
            lambda _m, _i, o, k=f"dec{i+1}": acts.__setitem__(k, o.detach().clone())))
    hooks.append(model.dec_conv[6].register_forward_hook(
        lambda _m, _i, o: acts.__setitem__("dec4", o.detach().clone())))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)          # main.py:50
    opt.zero_grad()
    torch.manual_seed(999)
    recon_x, m_hat, mu, logvar = model(x, m, t)
    torch.manual_seed(999)
    eps = torch.randn(B, 64)                                      # the eps forward() drew
    z = mu + eps * torch.exp(0.5 * logvar)
    for h in hooks:
        h.remove()
    loss, l_recon, l_m = train.loss_function(recon_x, x, m_hat, m, mu, logvar)
    kld = loss - l_recon - 2000.0 * l_m
    loss.backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    opt.step()
    # self-check of the eps recipe: decode by hand from z in eval-free manner
    with torch.no_grad():
        t1h = F.one_hot(t, 19).float()
        chk = model.dec_input(torch.cat([z, m_hat], 1)).view(-1, 256, 4, 4)
    store.update({"in/x": x.numpy(), "in/m": m.numpy(), "in/t": t.numpy(), "in/eps": eps.numpy()})
    pack("out", dict(recon_x=recon_x, m_hat=m_hat, mu=mu, logvar=logvar, z=z), store)
    pack("act", acts, store)
    pack("loss", dict(loss=loss, recon=l_recon, m_loss=l_m, kld=kld), store)
    pack("grad", grads, store)
    pack("sd1", model.state_dict(), store)                        # after one Adam step (+BN running stats)
    # second forward in eval mode with the updated weights (BN running stats path; analyze.py:10-23)
    model.eval()
    with torch.no_grad():
        m_hat_eval = model.mechanism_net(F.one_hot(t, 19).float())
    pack("eval", dict(m_hat=m_hat_eval), store)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)
    print(name, "loss", float(loss), "keys", len(store))


def morph_case(name, B, seed_data, gaussian_head):
    sub = "06_model_experiment" if gaussian_head else "01_baseline_causal_vae"
    config, models = import_from(os.path.join(REF, "mnist_test", sub), "config", "models")
    CONFIG = config.CONFIG
    torch.manual_seed(CONFIG["SEED"])
    vae = models.CausalMorphVAE12(); disc = models.LatentDiscriminator()
    vae.train(); disc.train()
    store = {}
    pack("sd0", vae.state_dict(), store)
    pack("sdd0", disc.state_dict(), store)
    g = torch.Generator().manual_seed(seed_data)
    x = torch.rand(B, 1, 28, 28, generator=g)
    m = torch.rand(B, 12, generator=g)
    t = F.one_hot(torch.randint(0, 10, (B,), generator=g), 10).float()
    store.update({"in/x": x.numpy(), "in/m": m.numpy(), "in/t": t.numpy()})
    # ---- plain forward with a known eps ----
    torch.manual_seed(999)
    outs = vae(x, m, t)
    torch.manual_seed(999)
    eps = torch.randn(B, 10)
    names = ["recon_x", "m_hat", "mu", "logvar", "m_mu", "m_logvar"][:len(outs)]
    fwd = dict(zip(names, outs))
    fwd["z"] = fwd["mu"] + eps * torch.exp(0.5 * fwd["logvar"])
    store["fwd/eps"] = eps.numpy()
    pack("fwd", fwd, store)
    if gaussian_head:
        nll = 0.5 * torch.sum(fwd["m_logvar"] + (m - fwd["m_mu"]) ** 2 / fwd["m_logvar"].exp())   # 06/train.py:79
        pack("fwd", dict(nll=nll), store)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)
        print(name, "keys", len(store))
        return
    # ---- one adversarial step, in the order of 01/train.py:34-93 ----
    opt_vae = torch.optim.Adam(vae.parameters(), lr=CONFIG["LR"])
    opt_d = torch.optim.Adam(disc.parameters(), lr=CONFIG["LR"])
    torch.manual_seed(4321)
    e = [None] * 6
    t_indices = torch.argmax(t, dim=1)
    opt_d.zero_grad()
    with torch.no_grad():
        _, _, mu, logvar = vae(x, m, t)                 # draw #1
        z = vae.reparameterize(mu, logvar).detach()     # draw #2
        _, _, mu, logvar = vae(x, m, t)                 # draw #3
        std = torch.exp(0.5 * logvar)
        eps4 = torch.randn_like(std)                    # draw #4
        z = mu + eps4 * std
    d_logits = disc(z)
    loss_d = F.cross_entropy(d_logits, t_indices)
    loss_d.backward()
    grads_d = {k: p.grad.clone() for k, p in disc.named_parameters()}
    opt_d.step()
    opt_vae.zero_grad()
    recon_x, m_hat, mu, logvar = vae(x, m, t)           # draw #5
    loss_recon = F.binary_cross_entropy(recon_x.view(-1, 784), x.view(-1, 784), reduction='sum')
    loss_kld = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp()) * CONFIG["BETA"]
    loss_morph = F.mse_loss(m_hat, m, reduction='sum') * 100
    z_sample = vae.reparameterize(mu, logvar)           # draw #6
    d_fake = disc(z_sample)
    target_uniform = torch.full_like(d_fake, 1.0 / CONFIG["T_DIM"])
    loss_adv = F.kl_div(F.log_softmax(d_fake, dim=1), target_uniform, reduction='batchmean') * CONFIG["LAMBDA_ADV"] * 100
    loss = loss_recon + loss_kld + loss_morph + loss_adv
    loss.backward()
    grads_v = {k: p.grad.clone() for k, p in vae.named_parameters()}
    opt_vae.step()
    torch.manual_seed(4321)
    for i in range(6):
        e[i] = torch.randn(B, 10)
    assert torch.equal(e[3], eps4), "eps draw-order recipe broken"
    assert torch.allclose(z_sample, mu + e[5] * torch.exp(0.5 * logvar), atol=0, rtol=0)
    store.update({"step/eps_d": e[3].numpy(), "step/eps_vae": e[4].numpy(), "step/eps_adv": e[5].numpy()})
    pack("step", dict(loss_d=loss_d, loss=loss, recon=loss_recon, kld=loss_kld, morph=loss_morph, adv=loss_adv,
                      recon_x=recon_x, mu=mu, logvar=logvar, m_hat=m_hat, d_logits=d_logits), store)
    pack("gradv", grads_v, store)
    pack("gradd", grads_d, store)
    pack("sd1", vae.state_dict(), store)
    pack("sdd1", disc.state_dict(), store)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)
    print(name, "loss", float(loss), "loss_d", float(loss_d), "keys", len(store))


def cvae_case(name, B, seed_data):
    """ConditionalVAE (mnist_test/03_measurement_approach/cvae_models.py:7-85) and one iteration of its loop (cvae_train.py:27-47)."""
    config, models = import_from(os.path.join(REF, "mnist_test", "03_measurement_approach"), "config", "cvae_models")
    CONFIG = config.CONFIG
    torch.manual_seed(CONFIG["SEED"])
    vae = models.ConditionalVAE()
    vae.train()
    store = {}
    pack("sd0", vae.state_dict(), store)
    g = torch.Generator().manual_seed(seed_data)
    x = torch.rand(B, 1, 28, 28, generator=g)
    t = F.one_hot(torch.randint(0, 10, (B,), generator=g), 10).float()
    store.update({"in/x": x.numpy(), "in/t": t.numpy()})
    opt = torch.optim.Adam(vae.parameters(), lr=CONFIG["LR"])
    opt.zero_grad()
    torch.manual_seed(999)
    recon_x, mu, logvar = vae(x, t)
    torch.manual_seed(999)
    eps = torch.randn(B, CONFIG["Z_DIM"])
    store["fwd/eps"] = eps.numpy()
    loss_recon = F.binary_cross_entropy(recon_x.view(-1, 784), x.view(-1, 784), reduction='sum')
    loss_kld = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp()) * 1.0
    loss = loss_recon + loss_kld
    loss.backward()
    grads = {k: p.grad.clone() for k, p in vae.named_parameters()}
    opt.step()
    pack("fwd", dict(recon_x=recon_x, mu=mu, logvar=logvar, z=mu + eps * torch.exp(0.5 * logvar), loss=loss, recon=loss_recon, kld=loss_kld), store)
    pack("grad", grads, store)
    pack("sd1", vae.state_dict(), store)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)
    print(name, "loss", float(loss), "keys", len(store))


def vessel_loss_case(name):
    src = open(os.path.join(REF, "vessel_analysis", "01_train", "train.py")).read()
    fn_node = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "loss_function")
    ns = {"torch": torch, "F": F}
    exec(compile(ast.Module(body=[fn_node], type_ignores=[]), "<reference vessel loss_function>", "exec"), ns)
    ref_loss = ns["loss_function"]
    store = {}
    g = torch.Generator().manual_seed(77)
    for tag, shape, density in (("d10", (2, 1, 48, 80), 0.10), ("d001", (2, 1, 16, 16, 16), 0.004), ("d60", (3, 1, 24, 40), 0.6)):
        x = (torch.rand(*shape, generator=g) < density).float()
        recon_x = torch.rand(*shape, generator=g) * 1.2 - 0.1
        B = shape[0]
        m = torch.randn(B, 12, generator=g); m_mu = torch.randn(B, 12, generator=g); m_logvar = torch.randn(B, 12, generator=g) * 0.5
        mu = torch.randn(B, 128, generator=g); logvar = torch.randn(B, 128, generator=g) * 0.3
        recon_x.requires_grad_(True); m_mu.requires_grad_(True); m_logvar.requires_grad_(True)
        mu.requires_grad_(True); logvar.requires_grad_(True)
        recon, kld, morph, sparsity = ref_loss(recon_x, x, m_mu, m, mu, logvar, m_mu, m_logvar)
        total = recon + 0.5 * kld + morph + 0.3 * sparsity          # train.py:82 (BETA = 0.5, config.py)
        total.backward()
        store.update({f"{tag}/x": x.numpy(), f"{tag}/recon_x": recon_x.detach().numpy(), f"{tag}/m": m.numpy(),
                      f"{tag}/m_mu": m_mu.detach().numpy(), f"{tag}/m_logvar": m_logvar.detach().numpy(),
                      f"{tag}/mu": mu.detach().numpy(), f"{tag}/logvar": logvar.detach().numpy()})
        pack(tag, dict(recon=recon, kld=kld, morph=morph, sparsity=sparsity, total=total,
                       g_recon_x=recon_x.grad, g_m_mu=m_mu.grad, g_m_logvar=m_logvar.grad,
                       g_mu=mu.grad, g_logvar=logvar.grad), store)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)
    print(name, "keys", len(store))


def vessel2d_inputs(B, seed):
    """Deterministic synthetic batch in the vessel dataset's format (dataset.py:192-248): binary sparse image, standardised m, one-hot t."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, 1, 768, 1280, generator=g) < 0.08).float()
    m = torch.randn(B, 12, generator=g)
    t = F.one_hot(torch.randint(0, 19, (B,), generator=g), 19).float()
    eps = torch.randn(B, 128, generator=g)
    return x, m, t, eps


def vessel2d_case(name, B=4, seed_data=4321):
    """CausalVesselVAE (vessel_analysis/00_core/models.py:9-166).  The module imports torchvision and a bare `config`, neither importable
    here, so the class text up to `class CausalViTVAE` is compiled with those two import lines dropped and CONFIG injected; the loss is the
    reference loss_function text as in vessel_loss_case; total as train_one_epoch composes it (01_train/train.py:82)."""
    src = open(os.path.join(REF, "vessel_analysis", "00_core", "models.py")).read()
    src = src.replace("import torchvision\n", "").replace("from config import CONFIG\n", "")
    ns = {"CONFIG": {"M_DIM": 12, "T_DIM": 19, "Z_DIM": 128}}
    exec(compile(src[:src.index("class CausalViTVAE")], "<reference vessel models.py>", "exec"), ns)
    lsrc = open(os.path.join(REF, "vessel_analysis", "01_train", "train.py")).read()
    fn_node = next(n for n in ast.parse(lsrc).body if isinstance(n, ast.FunctionDef) and n.name == "loss_function")
    lns = {"torch": torch, "F": F}
    exec(compile(ast.Module(body=[fn_node], type_ignores=[]), "<reference vessel loss_function>", "exec"), lns)
    torch.manual_seed(42)
    model = ns["CausalVesselVAE"]()
    model.train()
    store = {}
    pack("sd0", model.state_dict(), store)
    x, m, t, eps = vessel2d_inputs(B, seed_data)
    model.reparameterize = lambda mu, logvar: mu + eps * torch.exp(0.5 * logvar)     # :137-140 with the draw injected
    recon_x, m_hat, mu, logvar, m_mu, m_logvar = model(x, m, t)
    recon, kld, morph, sparsity = lns["loss_function"](recon_x, x, m_hat, m, mu, logvar, m_mu, m_logvar)
    total = recon + 0.5 * kld + morph + 0.3 * sparsity
    total.backward()
    store.update({"in/m": m.numpy(), "in/t": t.numpy(), "in/eps": eps.numpy(), "in/seed": np.array([B, seed_data], dtype=np.int64)})
    pack("in", dict(x=x), store)
    pack("fwd", dict(recon_x=recon_x, m_hat=m_hat, mu=mu, logvar=logvar, m_mu=m_mu, m_logvar=m_logvar, recon=recon, kld=kld, morph=morph,
                     sparsity=sparsity, total=total), store)
    pack("grad", {k: p.grad for k, p in model.named_parameters()}, store)
    pack("sd1", {k: v for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}, store)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)
    print(name, "total", float(total), "keys", len(store))
    # eval mode on the same batch, as validate() runs it (vessel_analysis/01_train/train.py:100-133): BatchNorm layers on the running
    # statistics the training forward above has just updated (sd1), no_grad, the same loss composition.  Kept in a file of its own.
    model.eval()
    with torch.no_grad():
        recon_x, m_hat, mu, logvar, m_mu, m_logvar = model(x, m, t)
        recon, kld, morph, sparsity = lns["loss_function"](recon_x, x, m_hat, m, mu, logvar, m_mu, m_logvar)
        total = recon + 0.5 * kld + morph + 0.3 * sparsity
    ev = {"in/seed": np.array([B, seed_data], dtype=np.int64)}
    pack("eval", dict(recon_x=recon_x, m_hat=m_hat, mu=mu, logvar=logvar, m_mu=m_mu, m_logvar=m_logvar, recon=recon, kld=kld, morph=morph,
                      sparsity=sparsity, total=total), ev)
    np.savez_compressed(os.path.join(OUT, name + "_eval.npz"), **ev)
    print(name + "_eval", "total", float(total), "keys", len(ev))


def vitvae_case(name, B, H, W, depth, seed_model, seed_bn, seed_data, full):
    """ViTVAE.encode in eval mode at random init (no pretrained file exists offline).  The encoder weights are the seed's draws (the product class
    constructs the same modules in the same order, so the fixture keeps digests only); the five stem BatchNorm2d layers get non-trivial statistics and
    affine parameters from a second seed (tests/vit_reference.py:randomize_stem_bn; stored whole: 4 x 736 values).  full: keep the stem output and the
    token stream after every block (the LAST block's stream as a digest plus its CLS row: three whole [B, N, 256] tensors would pass the size of the
    largest fixture); otherwise only the CLS row after every block."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    from vit_reference import randomize_stem_bn, vit_inputs
    (vb,) = import_from(os.path.join(REF, "vessel_analysis", "00_core"), "vit_backbone")
    torch.manual_seed(seed_model)
    model = vb.ViTVAE(in_channels=1, latent_dim=128, img_size=(H, W), depth=depth)
    randomize_stem_bn(model.stem, seed_bn)
    model.eval()
    x = vit_inputs(B, H, W, seed_data)
    acts = {}
    hooks = [model.stem.register_forward_hook(lambda _m, _i, o: acts.__setitem__("stem", o.detach().clone())),
             model.to_latent.register_forward_hook(lambda _m, _i, o: acts.__setitem__("cls_out", o.detach().clone()))]
    for i, blk in enumerate(model.transformer):
        hooks.append(blk.register_forward_hook(lambda _m, _i, o, k=i: acts.__setitem__(f"block{k}", o.detach().clone())))
    with torch.no_grad():
        mu, log_var = model.encode(x)
    for h in hooks:
        h.remove()
    store = {"in/seed": np.array([B, H, W, depth, seed_model, seed_bn, seed_data], dtype=np.int64)}
    pack("sd0", {k: v for k, v in model.state_dict().items() if not k.startswith(("decoder_input.", "decoder."))}, store)
    pack("in", dict(x=x), store)
    if full:
        store["in/x_bits"] = np.packbits(x.numpy().astype(np.uint8).reshape(-1))
    named = dict(mu=mu, log_var=log_var, cls_out=acts["cls_out"])
    for i in range(depth):
        named[f"cls_row{i}"] = acts[f"block{i}"][:, 0]
        if full and i < depth - 1:
            named[f"tokens{i}"] = acts[f"block{i}"]
    if full:
        named["stem"] = acts["stem"]
    pack("out", named, store, full_limit=1 << 20)
    if full:
        pack("out", {f"tokens{depth - 1}": acts[f"block{depth - 1}"]}, store)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)
    print(name, "mu[0,:3]", mu[0, :3].tolist(), "keys", len(store), "bytes", os.path.getsize(os.path.join(OUT, name + ".npz")))


GRAD_ROWS = 6               # rows of every weight-matrix gradient kept by vitvae_grad_case: evenly spaced, first and last included


def grad_rows(n):
    """the fixed row subset of an [n, ...] weight gradient that the encoder-gradient fixture stores"""
    return sorted({round(i * (n - 1) / (GRAD_ROWS - 1)) for i in range(GRAD_ROWS)})


def vitvae_grad_case(name, B, H, W, depth, seed_model, seed_bn, seed_data, seed_cot):
    """The gradients of ViTVAE.encode in eval mode at random init, from a seeded cotangent on (mu, log_var): loss = sum(mu g_mu) + sum(log_var g_lv), one
    backward through the reference class (fp32, CPU).  Weights and stem statistics as vitvae_case (digests).  Stored: the cotangents and the stem output
    whole, the fp32 gradients of the small tensors whole (biases, LayerNorm parameters, cls_token, pos_embedding) and rows grad_rows(n) of each weight
    matrix's gradient.  The stem's own gradients are not stored (the product trains the transformer on a frozen stem)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    from vit_reference import randomize_stem_bn, vit_inputs
    (vb,) = import_from(os.path.join(REF, "vessel_analysis", "00_core"), "vit_backbone")
    torch.manual_seed(seed_model)
    model = vb.ViTVAE(in_channels=1, latent_dim=128, img_size=(H, W), depth=depth)
    randomize_stem_bn(model.stem, seed_bn)
    model.eval()
    x = vit_inputs(B, H, W, seed_data)
    g = torch.Generator().manual_seed(seed_cot)
    g_mu, g_lv = torch.randn(B, 128, generator=g), torch.randn(B, 128, generator=g)
    acts = {}
    hook = model.stem.register_forward_hook(lambda _m, _i, o: acts.__setitem__("stem", o.detach().clone()))
    mu, log_var = model.encode(x)
    hook.remove()
    torch.autograd.backward([mu, log_var], [g_mu, g_lv])
    store = {"in/seed": np.array([B, H, W, depth, seed_model, seed_bn, seed_data], dtype=np.int64), "in/seed_cot": np.array([seed_cot], dtype=np.int64)}
    pack("sd0", {k: v for k, v in model.state_dict().items() if not k.startswith(("decoder_input.", "decoder."))}, store)
    pack("in", dict(x=x, g_mu=g_mu, g_lv=g_lv), store)
    pack("out", dict(mu=mu, log_var=log_var, stem=acts["stem"]), store)
    for k, p in model.named_parameters():
        if k.startswith(("stem.", "decoder_input.", "decoder.")):
            continue
        if p.dim() == 2:
            rows = grad_rows(p.shape[0])
            store[f"grad/{k}#rows"] = np.array(rows, dtype=np.int64)
            store[f"grad/{k}"] = p.grad[rows].numpy().copy()
        else:
            store[f"grad/{k}"] = p.grad.numpy().copy()
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)
    print(name, "mu[0,:3]", mu[0, :3].tolist(), "keys", len(store), "bytes", os.path.getsize(os.path.join(OUT, name + ".npz")))


def vitvae_stem_grad_case(name, B, H, W, depth, seed_model, seed_bn, seed_data, seed_cot):
    """The STEM's gradients of ViTVAE.encode in eval mode at random init: the model, image, loss and seeds of vitvae_grad_case (loss = sum(mu g_mu) +
    sum(log_var g_lv), one fp32 CPU backward through the reference class).  Stored: the cotangents, the gradient arriving at the stem's output (`out/dstem`,
    NCHW, from a hook: what the restatement of the stem alone starts from; weights and image as digests: the seeds reproduce them), the fp32 gradients of the 15 small tensors (conv biases, BatchNorm weights and
    biases) whole and rows grad_rows(Cout) of each conv weight's gradient along dimension 0."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    from vit_reference import randomize_stem_bn, vit_inputs
    (vb,) = import_from(os.path.join(REF, "vessel_analysis", "00_core"), "vit_backbone")
    torch.manual_seed(seed_model)
    model = vb.ViTVAE(in_channels=1, latent_dim=128, img_size=(H, W), depth=depth)
    randomize_stem_bn(model.stem, seed_bn)
    model.eval()
    x = vit_inputs(B, H, W, seed_data)
    g = torch.Generator().manual_seed(seed_cot)
    g_mu, g_lv = torch.randn(B, 128, generator=g), torch.randn(B, 128, generator=g)
    acts = {}
    hook = model.stem.register_forward_hook(lambda _m, _i, o: (acts.__setitem__("stem", o.detach().clone()),
                                                               o.register_hook(lambda gg: acts.__setitem__("dstem", gg.detach().clone()))) and None)
    mu, log_var = model.encode(x)
    hook.remove()
    torch.autograd.backward([mu, log_var], [g_mu, g_lv])
    store = {"in/seed": np.array([B, H, W, depth, seed_model, seed_bn, seed_data], dtype=np.int64), "in/seed_cot": np.array([seed_cot], dtype=np.int64)}
    pack("sd0", {k: v for k, v in model.state_dict().items() if not k.startswith(("decoder_input.", "decoder."))}, store, full_limit=0)
    pack("in", dict(x=x), store, full_limit=0)                    # weights and image are the seeds' draws: digests only
    pack("in", dict(g_mu=g_mu, g_lv=g_lv), store)
    pack("out", dict(mu=mu, log_var=log_var, dstem=acts["dstem"]), store)
    for k, p in model.stem.named_parameters():
        if p.dim() == 4:
            rows = grad_rows(p.shape[0])
            store[f"grad/stem.{k}#rows"] = np.array(rows, dtype=np.int64)
            store[f"grad/stem.{k}"] = p.grad[rows].numpy().copy()
        else:
            store[f"grad/stem.{k}"] = p.grad.numpy().copy()
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)
    print(name, "mu[0,:3]", mu[0, :3].tolist(), "keys", len(store), "bytes", os.path.getsize(os.path.join(OUT, name + ".npz")))


def vitvae_dec_case(name, B, H, W, depth, seed_model, seed_bn, seed_dec_bn, seed_z, whole):
    """ViTVAE.decode in eval mode at random init.  The weights are the seed's draws (digests only: the product class draws the same); the stem BatchNorms
    are randomised as in vitvae_case, ALL decoder BatchNorm2d layers (the ones nested in the ResBlocks included) from a further seed
    (tests/vit_decoder_reference.py:randomize_decoder_bn).  Stored: z, the activation after decoder_input (viewed NCHW) and after each of the 8 stages,
    and the image — the names in `whole` as arrays, everything else (the state_dict included) as digests, so that a fixture stays below the largest
    existing one."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    from vit_reference import randomize_stem_bn
    from vit_decoder_reference import randomize_decoder_bn, dec_inputs, STAGES
    (vb,) = import_from(os.path.join(REF, "vessel_analysis", "00_core"), "vit_backbone")
    torch.manual_seed(seed_model)
    model = vb.ViTVAE(in_channels=1, latent_dim=128, img_size=(H, W), depth=depth)
    randomize_stem_bn(model.stem, seed_bn)
    randomize_decoder_bn(model.decoder, seed_dec_bn)
    model.eval()
    z = dec_inputs(B, 128, seed_z)
    acts = {}
    hooks = [model.decoder_input.register_forward_hook(lambda _m, _i, o: acts.__setitem__("grid", o.detach().view(-1, 256, H // 32, W // 32).clone()))]
    for i, (kind, idx) in enumerate(STAGES):
        mod = model.decoder[idx + 2] if kind == "up" else model.decoder[idx]         # the LeakyReLU behind a transposed conv / the ResBlock
        hooks.append(mod.register_forward_hook(lambda _m, _i, o, k=i: acts.__setitem__(f"stage{k}", o.detach().clone())))
    with torch.no_grad():
        acts["image"] = model.decode(z)
    for h in hooks:
        h.remove()
    store = {"in/seed": np.array([B, H, W, depth, seed_model, seed_bn, seed_dec_bn, seed_z], dtype=np.int64)}
    pack("sd0", model.state_dict(), store, full_limit=0)
    pack("in", dict(z=z), store)
    pack("out", {k: v for k, v in acts.items() if k not in whole}, store, full_limit=0)
    pack("out", {k: v for k, v in acts.items() if k in whole}, store, full_limit=1 << 30)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)
    print(name, "image[0,0,0,:3]", acts["image"][0, 0, 0, :3].tolist(), "keys", len(store), "bytes", os.path.getsize(os.path.join(OUT, name + ".npz")))


def causal_vitvae_case(name, B, H, W, seed_model, seed_bn, seed_dec_bn, seed_head_bn, seed_data, crop):
    """CausalViTVAE (vessel_analysis/00_core/models.py:181-307) in eval mode at random init.  The class text (from `class CausalViTVAE` on) is compiled
    with CONFIG and the reference's own ViTVAE injected, as vessel2d_case does for the older model (the module's torchvision / bare `config` imports are
    never executed).  Weights are the seed's draws (digests and the key list only: the product class draws the same); every BatchNorm gets non-trivial
    statistics from recorded seeds — stem and decoder BatchNorm2d as in the ViTVAE cases, the adapters' BatchNorm1d by
    tests/causal_vit_reference.py:randomize_head_bn; eps is injected.  Stored whole: m, t, eps, x as packed bits, cls_out, mu, logvar, z, z_vit, m_mu,
    m_logvar and the crop [y0:y1, x0:x1] of recon_x; recon_x itself as a digest."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    from vit_reference import randomize_stem_bn
    from vit_decoder_reference import randomize_decoder_bn
    from causal_vit_reference import randomize_head_bn, causal_inputs
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
    (vb,) = import_from(os.path.join(REF, "vessel_analysis", "00_core"), "vit_backbone")
    src = open(os.path.join(REF, "vessel_analysis", "00_core", "models.py")).read()
    ns = {"torch": torch, "nn": torch.nn, "F": F, "ViTVAE": vb.ViTVAE,
          "CONFIG": {"M_DIM": 12, "T_DIM": 19, "Z_DIM": 128, "IMG_HEIGHT": H, "IMG_WIDTH": W, "DEVICE": "cpu"}}
    exec(compile(src[src.index("class CausalViTVAE"):], "<reference vessel models.py: CausalViTVAE>", "exec"), ns)
    torch.manual_seed(seed_model)
    model = ns["CausalViTVAE"]()
    randomize_stem_bn(model.backbone.stem, seed_bn)
    randomize_decoder_bn(model.backbone.decoder, seed_dec_bn)
    randomize_head_bn(model, seed_head_bn)
    model.eval()
    x, m, t, eps = causal_inputs(B, H, W, seed_data)
    acts = {}

    def reparam(mu, logvar):                                    # :252-255 with the draw injected
        acts["z"] = mu + eps * torch.exp(0.5 * logvar)
        return acts["z"]
    model.reparameterize = reparam
    hooks = [model.backbone.to_latent.register_forward_hook(lambda _m, _i, o: acts.__setitem__("cls_out", o.detach().clone())),
             model.dec_adapter.register_forward_hook(lambda _m, _i, o: acts.__setitem__("z_vit", o.detach().clone()))]
    with torch.no_grad():
        recon_x, m_hat, mu, logvar, m_mu, m_logvar = model(x, m, t)
    for h in hooks:
        h.remove()
    assert m_hat is m_mu
    y0, y1, x0, x1 = crop
    store = {"in/seed": np.array([B, H, W, seed_model, seed_bn, seed_dec_bn, seed_head_bn, seed_data], dtype=np.int64), "in/m": m.numpy(), "in/t": t.numpy(),
             "in/eps": eps.numpy(), "in/x_bits": np.packbits(x.numpy().astype(np.uint8).reshape(-1)), "in/crop": np.array(crop, dtype=np.int64),
             "sd0_keys": np.array(list(model.state_dict().keys()))}
    pack("sd0", model.state_dict(), store, full_limit=0)
    pack("in", dict(x=x), store, full_limit=0)
    pack("out", dict(cls_out=acts["cls_out"], mu=mu, logvar=logvar, z=acts["z"], z_vit=acts["z_vit"], m_mu=m_mu, m_logvar=m_logvar,
                     recon_crop=recon_x[:, :, y0:y1, x0:x1].contiguous()), store, full_limit=1 << 30)
    pack("out", dict(recon_x=recon_x), store, full_limit=0)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)
    print(name, "mu[0,:3]", mu[0, :3].tolist(), "recon[0,0,0,:3]", recon_x[0, 0, 0, :3].tolist(), "keys", len(store), "bytes",
          os.path.getsize(os.path.join(OUT, name + ".npz")))


def main():
    os.makedirs(OUT, exist_ok=True)
    if len(sys.argv) > 1 and sys.argv[1] == "vitvae_dec":
        # grid 2 x 3: the image and every stage but the last two whole (stage6 / stage7 are 0.3 / 1.2 MB as arrays: digests)
        vitvae_dec_case("vitvae_dec_64x96", 3, 64, 96, 1, 42, 4242, 4343, 1311, whole={"grid", "image"} | {f"stage{i}" for i in range(6)})
        vitvae_dec_case("vitvae_dec_256x320", 2, 256, 320, 1, 42, 4242, 4343, 1312, whole={"image"})       # grid 8 x 10: the image whole
        vitvae_dec_case("vitvae_dec_768x1280", 1, 768, 1280, 1, 42, 4242, 4343, 1313, whole=set())         # digests only
        return
    if len(sys.argv) > 1 and sys.argv[1] == "causal_vitvae":
        causal_vitvae_case("causal_vitvae_768x1280", 2, 768, 1280, 42, 4242, 4343, 4444, 1321, crop=(352, 416, 608, 672))
        return
    if len(sys.argv) > 1 and sys.argv[1] == "vitvae":
        vitvae_case("vitvae_enc_256x320", 3, 256, 320, 2, 42, 4242, 1301, full=True)       # 81 tokens
        vitvae_case("vitvae_enc_768x1280", 2, 768, 1280, 6, 42, 4242, 1302, full=False)    # 961 tokens
        return
    if len(sys.argv) > 1 and sys.argv[1] == "vitvae_grad":
        vitvae_grad_case("vitvae_enc_grad_64x96", 2, 64, 96, 2, 42, 4242, 1303, 1304)      # 7 tokens
        return
    if len(sys.argv) > 1 and sys.argv[1] == "vitvae_stem_grad":
        vitvae_stem_grad_case("vitvae_stem_grad_64x96", 2, 64, 96, 2, 42, 4242, 1303, 1304)  # vitvae_grad's model, image and cotangents
        return
    if len(sys.argv) > 1 and sys.argv[1] == "vessel2d":
        vessel2d_case("vessel2d_b4")
        return
    if len(sys.argv) > 1 and sys.argv[1] == "cvae":
        sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
        cvae_case("mnist_cvae_b8", 8, 1234)
        return
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))   # unused import in some ref files
    bio2d_case("bio2d_b4_64x96", 4, 64, 96, 1234)       # non-identity bilinear + non-divisible adaptive pool (6 -> 4)
    bio2d_case("bio2d_b2_64x64", 2, 64, 64, 1235)       # identity resize, identity pool
    bio2d_case("bio2d_b3_128x160", 3, 128, 160, 1236)   # 8x10 -> 4x4 pool (mixed window sizes), 2x/2.5x upsample
    morph_case("morph12_b8", 8, 1234, gaussian_head=False)
    morph_case("morph12g_b8", 8, 1234, gaussian_head=True)
    cvae_case("mnist_cvae_b8", 8, 1234)
    vessel_loss_case("vessel_loss")
    vessel2d_case("vessel2d_b4")          # B = 4: at B = 2 a train-mode BatchNorm1d backward is (g1 - g2)(1 - xhat^2) ~ eps/var, pure cancellation


if __name__ == "__main__":
    main()

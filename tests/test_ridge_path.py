"""The ridge alpha path on the device (ops.ridge_loo_path, causal_vae_amd.vit.fit_translator_ridge_cv and translate_vit_latents' grid; cvae_centered_gram_f64,
cvae_eigh_f64, cvae_centered_matmul_f64, cvae_ridge_path_f64) against tests/ridge_path_reference.py: per alpha the wide Cholesky closed form of
tests/ridge_translator_reference.py and its bounds c (N + d) 2^-53 kappa s with c = C_PATH = 8 (tests/test_ridge_path_cpu.py shows where it comes from).

Inputs: the cases of the latent translator's tests and the long one, N over 4096; the grid {1e-3, 1e-1, 1, 10, 1e3}.
  accuracy     for every alpha: leverage, loo, r2, corr and sse within their bounds; the eigenvalues ascending and not negative
  consistency  the path at alpha_g against ops.ridge_fit_loo(Z, M, alpha_g), the Cholesky route: within the sum of the two routes' bounds
  selection    fit_translator_ridge_cv on {1, 100, 1e4} chooses the wide reference's alpha under "mse" and under "r2" (whose margin over the runner-up is
               asserted above 1e-6 on the reference alone); the first four outputs are bit for bit fit_translator_ridge(alpha=chosen)'s; path holds Python floats
  bits         two runs, and float32 / float64 / device-tensor inputs, give equal bits
  pieces       cvae_centered_matmul_f64 with either operand transposed in place and ragged sizes against numpy.longdouble; cvae_centered_gram_f64 without M
  from a model translate_vit_latents(alphas=None) is the five-tuple it was, bit for bit fit_translator_ridge's; with a grid the path is appended

Measured on the MI355X with c = 8, the largest over the grid (the RATIO lines of the run):
  N2-d1-F1          sweeps 1   leverage 0.018   loo 0.157   r2 0.0366   corr 0        sse 0.0333
  N16-d512-F7       sweeps 13  leverage 0.0316  loo 0.00593 r2 0.000767 corr 0.000424 sse 0.000737
  N40-d8-F5-const   sweeps 6   leverage 0.00246 loo 0.00716 r2 0.000381 corr 8.9e-05  sse 0.000358
  N97-d64-F12       sweeps 9   leverage 0.00397 loo 0.00658 r2 0.00103  corr 8.7e-05  sse 0.000995
  N300-d130-F3      sweeps 10  leverage 0.00405 loo 0.00738 r2 0.000931 corr 4.5e-06  sse 0.000935
  N40-d8-F5         sweeps 6   leverage 0.00246 loo 0.00889 r2 0.000381 corr 8.9e-05  sse 0.000358
  N4500-d8-F2       sweeps 6   leverage 2.5e-06 loo 0.00033 r2 1.1e-05  corr 2.3e-06  sse 1.2e-05
  path against the Cholesky route, of the sum of the two bounds: N16-d512-F7 0.0158, N97-d64-F12 0.00341, N300-d130-F3 0.00368
No ratio is above 0.16 (loo at N = 2, d = 1, where one rounding is most of the bound)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ridge_path_reference as rp  # noqa: E402
import ridge_translator_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL_CASES = rr.CASES + [rr.LONG_CASE]
_PATH = {}


def path_of(case):
    """ops.ridge_loo_path of a case on GRID as numpy, once"""
    if case not in _PATH:
        from causal_vae_amd import ops
        Z, M, _ = rp.wide(case)
        p = ops.ridge_loo_path(torch.as_tensor(Z).to(DEV), torch.as_tensor(M).to(DEV), rp.GRID)
        _PATH[case] = {k: getattr(p, k).cpu().numpy() for k in ("alphas", "eigenvalues", "leverage", "loo", "sse", "r2", "corr")}
        _PATH[case]["sweeps"] = p.sweeps
    return _PATH[case]


def at(path, g):
    return {k: path[k][g] for k in rp.KEYS}


def names_of(F):
    return [f"feat{j}" for j in range(F)]


@pytest.mark.parametrize("case", ALL_CASES, ids=rr.case_id)
def test_path_against_the_wide_closed_form(case):
    N, d, F = case[:3]
    Z, M, refs = rp.wide(case)
    path = path_of(case)
    G = len(rp.GRID)
    assert path["leverage"].shape == (G, N) and path["loo"].shape == (G, N, F) and path["sse"].shape == (G, F) and path["r2"].shape == (G, F)
    assert path["alphas"].tolist() == list(rp.GRID) and path["eigenvalues"].shape == (d,)
    assert (path["eigenvalues"] >= 0).all() and (np.diff(path["eigenvalues"]) >= 0).all() and path["sweeps"] >= 1
    worst = {k: 0.0 for k in rp.KEYS}
    for g, ref in enumerate(refs):
        for k, v in rp.ratios(at(path, g), ref, rp.bounds(ref, M)).items():
            worst[k] = max(worst[k], v)
    print(f"RATIO path {rr.case_id(case)} sweeps {path['sweeps']} " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (rr.case_id(case), k, v)
    if case[4]:          # the constant column: the rules, not arithmetic, at every alpha
        assert (path["r2"][:, -1] == 1.0).all() and (path["corr"][:, -1] == 0.0).all()


@pytest.mark.parametrize("case", [rr.CASES[1], rr.CASES[3], rr.CASES[4]], ids=rr.case_id)
def test_path_is_consistent_with_the_cholesky_route(case):
    from causal_vae_amd import ops
    Z, M, refs = rp.wide(case)
    path = path_of(case)
    Zd, Md = torch.as_tensor(Z).to(DEV), torch.as_tensor(M).to(DEV)
    worst = 0.0
    for g, (alpha, ref) in enumerate(zip(rp.GRID, refs)):
        fit = ops.ridge_fit_loo(Zd, Md, alpha)
        b_path, b_chol = rp.bounds(ref, M), rr.bounds(ref, M)
        for k in ("leverage", "loo", "r2", "corr"):
            worst = max(worst, rr.max_ratio(path[k][g], getattr(fit, k).cpu().numpy(), np.asarray(b_path[k]) + np.asarray(b_chol[k])))
    print(f"RATIO path-vs-cholesky {rr.case_id(case)} {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("case", rp.SELECT_CASES, ids=rr.case_id)
def test_selection_and_the_fit_of_the_chosen_alpha(case):
    from causal_vae_amd.vit import fit_translator_ridge, fit_translator_ridge_cv
    Z, M, refs = rp.wide(case, rp.SELECT_GRID)
    names = names_of(case[2])
    for criterion in ("mse", "r2"):
        best, margin = rp.select(refs, M, criterion)
        assert margin > 1e-6          # on the reference alone
        translator, ranking, mhat, W, path = fit_translator_ridge_cv(Z, M, alphas=rp.SELECT_GRID, feature_names=names, select=criterion, device=DEV)
        assert translator.alpha == rp.SELECT_GRID[best], (criterion, [(r["alpha"], r["mse"], r["mean_r2"]) for r in path])
        assert [r["alpha"] for r in path] == list(rp.SELECT_GRID) and all(set(r) == {"alpha", "mse", "mean_r2", "max_leverage", "r2"} for r in path)
        assert all(type(r[k]) is float for r in path for k in ("alpha", "mse", "mean_r2", "max_leverage")) and all(type(v) is float for r in path for v in r["r2"].values())
        assert all(list(r["r2"]) == names for r in path)
        t2, ranking2, mhat2, W2 = fit_translator_ridge(Z, M, feature_names=names, alpha=translator.alpha, device=DEV)
        assert np.array_equal(translator.coef_, t2.coef_) and np.array_equal(translator.intercept_, t2.intercept_) and np.array_equal(mhat, mhat2)
        assert np.array_equal(translator.loo_pred_, t2.loo_pred_) and np.array_equal(translator.leverage_, t2.leverage_) and ranking == ranking2
        assert W is translator.coef_ and np.array_equal(W, W2)


def test_a_tie_takes_the_first_alpha():
    from causal_vae_amd.vit import fit_translator_ridge_cv
    Z, M, _ = rp.wide(rr.CASES[3])
    for grid in [(10.0, 10.0, 1e4), (1e4, 10.0, 10.0)]:
        translator, _r, _m, _w, path = fit_translator_ridge_cv(Z, M, alphas=grid, device=DEV)
        assert translator.alpha == 10.0 and [r["mse"] for r in path].index(min(r["mse"] for r in path)) == grid.index(10.0)
        assert path[grid.index(10.0)]["mse"] == path[2 if grid[0] == 1e4 else 1]["mse"]          # equal alphas, equal bits


@pytest.mark.parametrize("case", [rr.CASES[1], rr.CASES[4]], ids=rr.case_id)
def test_input_forms_and_runs_give_equal_bits(case):
    from causal_vae_amd import ops
    Z, M, _ = rp.wide(case)
    base = path_of(case)
    forms = {"float64": (torch.as_tensor(Z.astype(np.float64)), torch.as_tensor(M)), "float32 again": (torch.as_tensor(Z), torch.as_tensor(M)),
             "float32 M": (torch.as_tensor(Z), torch.as_tensor(M.astype(np.float32).astype(np.float64)))}
    for label, (z, m) in forms.items():
        p = ops.ridge_loo_path(z.to(DEV), m.to(DEV), list(rp.GRID))
        if label == "float32 M":
            continue          # other inputs: only that it runs on a grid given as a list
        for k in ("eigenvalues", "leverage", "loo", "sse", "r2", "corr"):
            assert np.array_equal(getattr(p, k).cpu().numpy(), base[k]), (label, k)
        assert p.sweeps == base["sweeps"]


def test_centered_matmul_and_gram_pieces():
    from causal_vae_amd import ops
    rng = np.random.RandomState(11)
    x, b, mean = rng.standard_normal((70, 37)), rng.standard_normal((37, 33)), rng.standard_normal(37)
    xd, bd, md = (torch.as_tensor(a).to(DEV) for a in (x, b, mean))
    W = rr.WIDE
    bound = lambda A, B: 8 * 37 * rr.U * (np.abs(A) @ np.abs(B))          # noqa: E731  a dot product of 37 terms, fma or not, with room
    want = (x.astype(W) - mean.astype(W)) @ b.astype(W)
    assert rr.max_ratio(ops.centered_matmul_f64(xd, md, bd).cpu().numpy(), want, bound(np.abs(x) + np.abs(mean), b)) <= 1.0
    xt, bt = torch.as_tensor(np.ascontiguousarray(x.T)).to(DEV), torch.as_tensor(np.ascontiguousarray(b.T)).to(DEV)
    plain = ops.centered_matmul_f64(xd, md, bd)
    assert torch.equal(ops.centered_matmul_f64(xt, md, bd, x_t=True), plain) and torch.equal(ops.centered_matmul_f64(xd, md, bt, b_t=True), plain)
    assert rr.max_ratio(ops.centered_matmul_f64(xd, None, bd).cpu().numpy(), x.astype(W) @ b.astype(W), bound(x, b)) <= 1.0
    gram, none = ops.centered_gram_f64(xd, ops.col_means_f64(xd))
    xc = x.astype(W) - x.astype(W).sum(axis=0) / 70
    assert none is None and rr.max_ratio(gram.cpu().numpy(), xc.T @ xc, 8 * 70 * rr.U * (np.abs(xc).T @ np.abs(xc)).astype(np.float64)) <= 1.0
    assert torch.equal(gram, gram.T)


def test_translate_vit_latents_with_and_without_a_grid():
    from causal_vae_amd.vit import ViTVAEEncoder, fit_translator_ridge, fit_translator_ridge_cv, translate_vit_latents
    torch.manual_seed(3)
    model = ViTVAEEncoder(img_size=(64, 96), depth=1, latent_dim=16).to(DEV).eval()
    loader = [{"x": torch.randn(2, 1, 64, 96)} for _ in range(3)]
    M = np.random.RandomState(1).standard_normal((6, 4))
    names = names_of(4)
    out = translate_vit_latents(model, loader, M, DEV, feature_names=names, alpha=0.5, alphas=None)
    assert len(out) == 5
    Z, translator, ranking, mhat, W = out
    t2, ranking2, mhat2, _ = fit_translator_ridge(Z, M, feature_names=names, alpha=0.5, device=DEV)
    assert np.array_equal(translator.coef_, t2.coef_) and np.array_equal(translator.intercept_, t2.intercept_) and np.array_equal(mhat, mhat2)
    assert np.array_equal(translator.loo_pred_, t2.loo_pred_) and ranking == ranking2 and translator.alpha == 0.5
    out = translate_vit_latents(model, loader, M, DEV, feature_names=names, alphas=(0.1, 1.0, 10.0))
    assert len(out) == 6 and np.array_equal(out[0], Z)
    t3, ranking3, mhat3, _w, path3 = fit_translator_ridge_cv(Z, M, alphas=(0.1, 1.0, 10.0), feature_names=names, device=DEV)
    assert out[1].alpha == t3.alpha and np.array_equal(out[1].coef_, t3.coef_) and out[2] == ranking3 and np.array_equal(out[3], mhat3) and out[5] == path3

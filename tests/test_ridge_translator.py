"""The latent translator on the device (csrc/ridge.hip through ops.ridge_fit_loo and causal_vae_amd.vit's fit_translator_ridge, translate_vit_latents and
bootstrap_feature_stability) against tests/ridge_translator_reference.py: the closed form in numpy.longdouble and the bounds
c (N + d) 2^-53 kappa s derived there (c = 8; tests/test_ridge_translator_cpu.py shows where it comes from and that float32 misses these bounds by orders
of magnitude).

Cases (N, d, F), alpha = 1 unless said: (2, 1, 1) the smallest legal one; (16, 512, 7) the reference's own regime: N < d, leverage 0.998, eight 64-wide
Cholesky blocks; (40, 8, 5) with a constant column (the R² and correlation rules); (97, 64, 12) N and F ragged against every tile; (300, 130, 3) d ragged with a
partial last Cholesky block, N over one 256-row chunk; (40, 8, 5) at alpha = 1e-3; and, beyond the issue's list, (4500, 8, 2): N over 4096, where a row chunk
grows to 512 rows (9 chunks, the last one ragged).  Z is float32 standard normal, M = Z B + noise growing from 0.3 over the
columns, column 0 scaled by 1000.
  fit          coef_, intercept_, Mhat_full, loo_pred_, leverage_, r2, corr within their bounds; the ranking order is the reference's (whose smallest adjacent
               r2 gap is asserted to exceed 1e-6)
  bits         Z as float32 numpy, float64 numpy and a device tensor, and a second run, all give equal bits
  predict      new rows within the bound, numpy in numpy out, tensor in tensor out
  info         a NaN in Z is a CvaeError from the Cholesky's info; nothing faults
  rules        cvae_ranking_stats_f64 on a constant truth and a constant prediction
  bootstrap    N = 24, three groups of 8, d = 16, F = 12, n_boot = 20, top_k = 3: topk_count equals the restatement's exactly and nothing is skipped (the
               restatement's top-k margin above 1e-9 and every group present in every draw are asserted on it alone); with a group of one sample the number of
               skipped (bootstrap, pair) combinations equals the restatement's
  from a model translate_vit_latents on a ViTVAEEncoder at 64 x 96 and a loader of three batches of two: Z is extract_vit_latents' bits, the rest
               fit_translator_ridge(Z, M)'s

Measured on the MI355X, max |got - ref| / bound with c = 8 (the RATIO lines of the run):
  N2-d1-F1        coef 0.086 intercept 0.025 fitted 0.026 loo 0.14 leverage 0.024 r2 0.017 corr 0
  N16-d512-F7     coef 0.00076 intercept 0.00012 fitted 3.9e-06 loo 6.9e-06 leverage 6.7e-06 r2 7.9e-07 corr 3.6e-07    (kappa 672, max h 0.998296)
  N40-d8-F5       coef 0.0054 intercept 0.042 fitted 0.0034 loo 0.0028 leverage 0.00063 r2 8.0e-05 corr 5.3e-05   (alpha 1e-3: 0.0050 0.019 0.0031 0.0024 0.00076 6.7e-05 3.2e-05)
  N97-d64-F12     coef 0.00042 intercept 0.0034 fitted 0.00021 loo 0.00016 leverage 8.3e-05 r2 3.5e-06 corr 4.2e-06
  N300-d130-F3    coef 0.00056 intercept 0.0049 fitted 0.00019 loo 0.00017 leverage 7.3e-05 r2 1.1e-06 corr 4.6e-07
  N4500-d8-F2     coef 9.8e-05 intercept 0.00067 fitted 0.00013 loo 0.00013 leverage 6.5e-07 r2 8.4e-07 corr 1.2e-06
  predict         N16-d512-F7 0.00041, N97-d64-F12 0.00037
  bootstrap       the restatement's smallest top-3 margin 0.0087 (three groups of 8; 0 skipped, 180 slots) and 0.057 (a group of one; 8 skipped, 156 slots)
No ratio is above 0.15; the float32 evaluation of the same algebra is at 3e3 (loo) to 4e5 (coef) bounds at N = 16, d = 512 (tests/test_ridge_translator_cpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ridge_translator_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_REF, _FIT = {}, {}


def reference(case):
    """the inputs and the wide closed form of a case, computed once and shared"""
    if case not in _REF:
        Z, M = rr.inputs(case)
        _REF[case] = (Z, M, rr.closed_form(Z, M, case[3]))
    return _REF[case]


def names_of(F):
    return [f"feat{j}" for j in range(F)]


def fitted(case):
    """fit_translator_ridge of a case on the device, once"""
    if case not in _FIT:
        from causal_vae_amd.vit import fit_translator_ridge
        Z, M, _ = reference(case)
        _FIT[case] = fit_translator_ridge(Z, M, feature_names=names_of(case[2]), alpha=case[3], device=DEV)
    return _FIT[case]


def got_outputs(case):
    translator, ranking, mhat, W = fitted(case)
    by_name = {r["feature"]: r for r in ranking}
    order = names_of(case[2])
    return {"coef": translator.coef_, "intercept": translator.intercept_, "fitted": mhat, "loo": translator.loo_pred_, "leverage": translator.leverage_,
            "r2": np.array([by_name[n]["r2"] for n in order]), "corr": np.array([by_name[n]["corr"] for n in order])}


@pytest.mark.parametrize("case", rr.CASES + [rr.LONG_CASE], ids=rr.case_id)
def test_fit_against_the_wide_closed_form(case):
    Z, M, ref = reference(case)
    translator, ranking, mhat, W = fitted(case)
    N, d, F = case[:3]
    assert translator.coef_.shape == (F, d) and translator.coef_.dtype == np.float64 and W is translator.coef_ and translator.alpha == case[3]
    assert translator.intercept_.shape == (F,) and mhat.shape == (N, F) and mhat.dtype == np.float64
    assert translator.loo_pred_.shape == (N, F) and translator.leverage_.shape == (N,)
    assert all(type(r["r2"]) is float and type(r["corr"]) is float for r in ranking)
    got, b = got_outputs(case), rr.bounds(ref, M)
    ratios = {k: rr.max_ratio(got[k], ref[k], b[k]) for k in rr.KEYS}
    print(f"RATIO fit {rr.case_id(case)} kappa {ref['kappa']:.3g} max h {float(ref['leverage'].max()):.6f} " + " ".join(f"{k} {v:.4g}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (rr.case_id(case), k, v)
    assert rr.min_adjacent_gap(ref["r2"]) > 1e-6          # on the reference alone: its order is no coin toss
    assert [r["feature"] for r in ranking] == [names_of(F)[j] for j in rr.ranking_order(ref["r2"])]
    assert [r["r2"] for r in ranking] == sorted((r["r2"] for r in ranking), reverse=True)
    if case[4]:          # the constant column: the rules, not arithmetic
        const = {r["feature"]: r for r in ranking}[names_of(F)[-1]]
        assert const["r2"] == 1.0 and const["corr"] == 0.0


@pytest.mark.parametrize("case", [rr.CASES[1], rr.CASES[4]], ids=rr.case_id)
def test_input_forms_and_runs_give_equal_bits(case):
    from causal_vae_amd.vit import fit_translator_ridge
    Z, M, _ = reference(case)
    base = got_outputs(case)
    forms = {"float64 numpy": (Z.astype(np.float64), M), "device tensors": (torch.as_tensor(Z).to(DEV), torch.as_tensor(M).to(DEV)),
             "float32 numpy again": (Z, M), "default names": (Z, M)}
    for label, (z, m) in forms.items():
        names = () if label == "default names" else names_of(case[2])
        t, ranking, mhat, _ = fit_translator_ridge(z, m, feature_names=names, alpha=case[3], device=DEV)
        again = {"coef": t.coef_, "intercept": t.intercept_, "fitted": mhat, "loo": t.loo_pred_, "leverage": t.leverage_}
        for k, v in again.items():
            assert np.array_equal(v, base[k]), (label, k)
        assert sorted(r["r2"] for r in ranking) == sorted(base["r2"].tolist()), label
        if label == "default names":
            assert sorted(r["feature"] for r in ranking) == sorted(f"m{j}" for j in range(case[2]))


@pytest.mark.parametrize("case", [rr.CASES[1], rr.CASES[3]], ids=rr.case_id)
def test_predict_on_new_rows(case):
    Z, M, ref = reference(case)
    translator = fitted(case)[0]
    Znew = np.random.RandomState(5).standard_normal((11, case[1])).astype(np.float32)
    want = rr.predict_wide(ref, Znew)
    got = translator.predict(Znew)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (11, case[2])
    ratio = rr.max_ratio(got, want, rr.predict_bound(ref, M, want))
    print(f"RATIO predict {rr.case_id(case)} {ratio:.4g}")
    assert ratio <= 1.0
    on_dev = translator.predict(torch.as_tensor(Znew).to(DEV))
    assert torch.is_tensor(on_dev) and on_dev.is_cuda and on_dev.dtype == torch.float64 and np.array_equal(on_dev.cpu().numpy(), got)
    on_cpu = translator.predict(torch.as_tensor(Znew.astype(np.float64)))
    assert torch.is_tensor(on_cpu) and not on_cpu.is_cuda and np.array_equal(on_cpu.numpy(), got)


@pytest.mark.parametrize("case,where", [(rr.CASES[2], (3, 2)), (rr.CASES[4], (299, 129))], ids=["N40-d8", "N300-d130"])
def test_nan_in_z_is_reported_through_info(case, where):
    from causal_vae_amd import ops
    from causal_vae_amd._lib import CvaeError
    Z, M, _ = reference(case)
    Z = Z.copy()
    Z[where] = np.nan
    with pytest.raises(CvaeError, match=r"Cholesky factorisation .* failed at column \d+ \(info = \d+\)"):
        ops.ridge_fit_loo(torch.as_tensor(Z).to(DEV), torch.as_tensor(M).to(DEV), case[3])
    torch.cuda.synchronize()          # nothing faulted: the device still answers
    good = ops.ridge_fit_loo(torch.as_tensor(reference(case)[0]).to(DEV), torch.as_tensor(M).to(DEV), case[3])
    assert good.info == 0 and bool(torch.isfinite(good.loo).all())


def test_ranking_rules_on_constant_columns():
    from causal_vae_amd import ops
    rng = np.random.RandomState(2)
    Y, P = rng.standard_normal((33, 4)), rng.standard_normal((33, 4))
    Y[:, 0] = 2.0                      # constant truth, imperfect prediction: r2 0 (sklearn), corr 0
    Y[:, 1] = 0.5
    P[:, 1] = 0.5                      # constant truth, perfect prediction: r2 1, corr 0
    P[:, 2] = 4.0                      # constant prediction: corr 0, r2 by the formula
    r2, corr = (t.cpu().numpy() for t in ops.ranking_stats_f64(torch.as_tensor(Y).to(DEV), torch.as_tensor(P).to(DEV)))
    want_r2, want_corr = rr.ranking_stats(Y.astype(rr.WIDE), P.astype(rr.WIDE))
    assert r2[0] == 0.0 and corr[0] == 0.0 and r2[1] == 1.0 and corr[1] == 0.0 and corr[2] == 0.0
    assert np.allclose(r2[2:], want_r2[2:].astype(np.float64), rtol=1e-13, atol=0) and abs(corr[3] - float(want_corr[3])) < 1e-14


def bootstrap_inputs(lonely):
    """N = 24, d = 16, F = 12: three groups of 8 (or 12, 11 and 1 with `lonely`) whose latents differ by a group offset; M linear in Z plus noise, its columns on
    scales 1 .. 12 so that the predicted differences are well apart"""
    rng = np.random.RandomState(77)
    groups = np.array((["g0"] * 12 + ["g1"] * 11 + ["g2"]) if lonely else (["g0", "g1", "g2"] * 8))
    offsets = {g: rng.standard_normal(16) for g in ("g0", "g1", "g2")}
    Z = (np.stack([offsets[g] for g in groups]) + 0.3 * rng.standard_normal((24, 16))).astype(np.float32)
    M = (Z.astype(np.float64) @ (rng.standard_normal((16, 12)) / 4.0) + 0.1 * rng.standard_normal((24, 12))) * (1.0 + np.arange(12))
    return groups, Z, M


@pytest.mark.parametrize("lonely", [False, True], ids=["three-groups-of-8", "a-group-of-one"])
def test_bootstrap_counts_equal_the_restatement(lonely):
    from causal_vae_amd.vit import bootstrap_feature_stability, fit_translator_ridge
    groups, Z, M = bootstrap_inputs(lonely)
    names = names_of(12)
    ref = rr.closed_form(Z, M, 1.0)
    scale = M.std(axis=0)
    want = rr.bootstrap(groups, Z, ref["coef"].astype(np.float64), ref["intercept"].astype(np.float64), names, scale=scale, n_boot=20, top_k=3, seed=4)
    assert want["min_margin"] > 1e-9          # on the restatement alone: no top-3 set is near a tie
    if lonely:
        assert 0 < want["skipped"] < 20 * 3
    else:
        assert want["all_present"] and want["skipped"] == 0
    translator = fit_translator_ridge(Z, M, feature_names=names, device=DEV)[0]
    rows, skipped = bootstrap_feature_stability(groups, Z, translator, names, scale=scale, n_boot=20, top_k=3, seed=4)
    print(f"bootstrap lonely={lonely}: margin {want['min_margin']:.3g}, skipped {skipped}, slots {want['total_slots']}")
    assert skipped == want["skipped"]
    assert {r["feature"]: r["topk_count"] for r in rows} == want["counts"]
    assert [r["stability_freq"] for r in rows] == sorted((r["stability_freq"] for r in rows), reverse=True)
    for r in rows:
        assert r["stability_freq"] == want["freq"][r["feature"]]


def test_group_means_resampled_against_numpy():
    from causal_vae_amd import ops
    rng = np.random.RandomState(9)
    Z = rng.standard_normal((37, 70))          # d over one 64-wide workgroup
    codes = rng.randint(0, 4, size=37)
    codes[codes == 3] = 0                      # G = 5 with groups 3 and 4 empty
    idx = rng.randint(0, 37, size=(6, 37))
    means, counts = ops.group_means_resampled(torch.as_tensor(Z).to(DEV), torch.as_tensor(codes).to(DEV), torch.as_tensor(idx).to(DEV), 5)
    means, counts = means.cpu().numpy(), counts.cpu().numpy()
    assert means.shape == (6, 5, 70) and counts.shape == (6, 5) and counts.dtype == np.int32
    for b in range(6):
        for g in range(5):
            rows = Z[idx[b]][codes[idx[b]] == g]
            assert counts[b, g] == len(rows)
            if len(rows):
                assert np.abs(means[b, g] - rows.astype(rr.WIDE).mean(axis=0).astype(np.float64)).max() <= 37 * rr.U * np.abs(rows).max()
            else:
                assert not means[b, g].any()


def test_translate_vit_latents_is_extract_then_fit():
    from causal_vae_amd.vit import ViTVAEEncoder, extract_vit_latents, fit_translator_ridge, translate_vit_latents
    torch.manual_seed(3)
    model = ViTVAEEncoder(img_size=(64, 96), depth=1, latent_dim=16).to(DEV).eval()
    loader = [{"x": torch.randn(2, 1, 64, 96)} for _ in range(3)]
    M = np.random.RandomState(1).standard_normal((6, 4))
    names = names_of(4)
    Z, translator, ranking, mhat, W = translate_vit_latents(model, loader, M, DEV, feature_names=names, alpha=0.5)
    assert Z.dtype == np.float32 and Z.shape == (6, 16) and np.array_equal(Z, extract_vit_latents(model, loader, DEV))
    t2, ranking2, mhat2, W2 = fit_translator_ridge(Z, M, feature_names=names, alpha=0.5, device=DEV)
    assert np.array_equal(translator.coef_, t2.coef_) and np.array_equal(translator.intercept_, t2.intercept_) and np.array_equal(mhat, mhat2)
    assert np.array_equal(translator.loo_pred_, t2.loo_pred_) and np.array_equal(translator.leverage_, t2.leverage_) and ranking == ranking2
    assert W is translator.coef_ and translator.alpha == 0.5

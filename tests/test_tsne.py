"""The exact t-SNE on the device (causal_vae_amd.vit.latent_tsne and the ops behind it; csrc/tsne.hip) against tests/tsne_reference.py: the
same definitions in numpy.longdouble, with the bounds derived there (C_TSNE_D = C_TSNE_AFF = C_TSNE_FORCE = 1, C_TSNE_STEP = 4, C_TSNE_TRAJ = 256;
tests/test_tsne_cpu.py shows where they come from and that the inputs decide every branch clearly).

Cases (N, d, perplexity): (33, 7, 5), (96, 20, 30), (130, 512, 10) the ViT latent width, (300, 10, 50) the MNIST width and more than 256 columns; float32 blobs;
and (40, 6, 8) with every row doubled.
  distances     D within its bound, bitwise symmetric, a zero diagonal
  affinities    beta, Pc, P at tol = 1e-5 and tol = 0 from the reference's float64 D; steps equal at 1e-5; P bitwise symmetric, its sum within bound of 1;
                the doubled rows stay finite; distances= gives the bits of the Z path
  forces, step  at the reference's own states before iterations 0, 200 and 400: (kl, grad), then every output of one step and the same gain decisions
  trajectory    8 iterations through the fit, pointwise
  end to end    N = 96 and N = 300, init="random", random_state=42, 1000 iterations: kl_divergence_ is the KL of the returned embedding; every nearest
                embedded neighbour has its point's label; the KL is at most 1.25 times the largest of the float64 reference's runs from the init moved by one
                ulp in 5 random directions; n_iter_ and the stop reason agree with the record
  schedule      max_iter = 0; a high min_grad_norm stops at the first check; a NaN in Z is a CvaeError naming the entry; two fits give equal bits; init="pca"

Measured on the MI355X with these constants (the RATIO lines of the run; per case D | the largest of beta, Pc, P over both tolerances | the largest over
the three states of kl, grad | of Y, update, gains, grad_norm | the 8-step trajectory | the end-to-end KL against its recomputation):
  N33-d7-p5       0.218  | 0.0915 | 0.0364 0.165  | 0.187 0.0944 0.119 0.011   | 0.0335
  N96-d20-p30     0.255  | 0.173  | 0.0253 0.137  | 0.0995 0.108 0.124 0.00797 | 0.0227  | 0.0243
  N130-d512-p10   0.0555 | 0.171  | 0.00876 0.209 | 0.213 0.189 0.125 0.0203   | 0.148
  N300-d10-p50    0.25   | 0.11   | 0.0265 0.162  | 0.181 0.14 0.123 0.00671   | 0.00459 | 0.0219
  N40-d6-p8 (doubled rows): D 0.22, beta 0, Pc 0.0779, P 0.055
No ratio is above 0.26, the sum of P aside: 0.999 at N = 130 and 0.986 at N = 300, where 2^-52 for every clamped entry is nearly all of both the difference
and its bound.  beta at tol = 1e-5 is bit-equal to the reference's, and steps equal.  End to end the KL was 0.005541 at N = 96 and 0.203901 at N = 300, inside
the float64 reference's own runs (0.005491 .. 0.005604 and 0.203703 .. 0.205491)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tsne_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_FIT = {}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(DEV)


def host(t):
    return t.cpu().numpy()


def e2e_fit(case):
    """the full fit of an end-to-end case, once"""
    if case not in _FIT:
        from causal_vae_amd.vit import latent_tsne
        ref = tr.wide(case)
        _FIT[case] = latent_tsne(ref["Z"], perplexity=case[2], init="random", random_state=42, device=DEV, keep_affinities=True)
    return _FIT[case]


@pytest.mark.parametrize("case", tr.CASES + [tr.DUPLICATE_CASE], ids=tr.case_id)
def test_distances(case):
    from causal_vae_amd import ops
    ref = tr.wide(case, duplicate=case == tr.DUPLICATE_CASE)
    D = host(ops.tsne_sqdist_f64(torch.as_tensor(ref["Z"]).to(DEV)))
    ratio = tr.max_ratio(D, ref["D"], tr.bound_D(case, ref["D"]))
    print(f"RATIO tsne D {tr.case_id(case)} {ratio:.3g}")
    assert ratio <= 1.0
    assert np.array_equal(D, D.T) and (np.diag(D) == 0).all()
    D64 = host(ops.tsne_sqdist_f64(torch.as_tensor(ref["Z"].astype(np.float64)).to(DEV)))
    assert np.array_equal(D, D64)          # float32 rows are converted on load: the same bits as from their float64 copy


@pytest.mark.parametrize("tol_name", ["tol", "tol0"])
@pytest.mark.parametrize("case", tr.CASES, ids=tr.case_id)
def test_affinities(case, tol_name):
    from causal_vae_amd import ops
    ref = tr.wide(case)
    a = ref[tol_name]
    P, Pc, beta, steps = (host(t) for t in ops.tsne_affinities_f64(dev(ref["D64"]), case[2], 1e-5 if tol_name == "tol" else 0.0))
    b = tr.bounds_affinities(case, a)
    r = {k: tr.max_ratio(v, a[k], b[k]) for k, v in (("beta", beta), ("Pc", Pc), ("P", P))}
    r["sumP"] = abs(float(P.astype(tr.WIDE).sum() - 1)) / b["sumP"]
    print(f"RATIO tsne affinities {tr.case_id(case)} {tol_name} " + " ".join(f"{k} {v:.3g}" for k, v in r.items()) + f" steps {steps.min()}..{steps.max()}")
    for k, v in r.items():
        assert v <= 1.0, (k, v)
    if tol_name == "tol":
        assert np.array_equal(steps, a["steps"])
    else:
        assert (steps <= tr.SEARCH_STEPS).all() and steps.max() == tr.SEARCH_STEPS
    assert np.array_equal(P, P.T) and (np.diag(P) == 0).all() and (np.diag(Pc) == 0).all() and (P[~np.eye(len(P), dtype=bool)] >= tr.EPS).all()


def test_doubled_rows_stay_finite():
    from causal_vae_amd import ops
    case = tr.DUPLICATE_CASE
    ref = tr.wide(case, duplicate=True)
    assert (ref["D64"][np.arange(0, case[0], 2), np.arange(1, case[0], 2)] == 0).all()
    P, Pc, beta, steps = (host(t) for t in ops.tsne_affinities_f64(ops.tsne_sqdist_f64(torch.as_tensor(ref["Z"]).to(DEV)), case[2]))
    assert np.isfinite(P).all() and np.isfinite(Pc).all() and np.isfinite(beta).all() and (beta > 0).all()
    a = ref["tol"]
    b = tr.bounds_affinities(case, a)
    r = {k: tr.max_ratio(v, a[k], b[k]) for k, v in (("beta", beta), ("Pc", Pc), ("P", P))}
    print(f"RATIO tsne affinities doubled {tr.case_id(case)} " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0 and np.array_equal(steps, a["steps"])


def test_precomputed_distances_give_the_same_bits():
    from causal_vae_amd import ops
    from causal_vae_amd.vit import latent_tsne
    case = tr.CASES[0]
    ref = tr.wide(case)
    Y0 = tr.random_init(case[0])
    by_z = latent_tsne(ref["Z"], perplexity=case[2], init=Y0, max_iter=60, device=DEV, keep_affinities=True)
    D = ops.tsne_sqdist_f64(torch.as_tensor(ref["Z"]).to(DEV))
    by_d = latent_tsne(None, distances=D, perplexity=case[2], init=Y0, max_iter=60, device=DEV, keep_affinities=True)
    assert np.array_equal(by_z.affinities_, by_d.affinities_) and np.array_equal(by_z.betas_, by_d.betas_)
    assert np.array_equal(by_z.embedding_, by_d.embedding_) and by_z.kl_divergence_ == by_d.kl_divergence_ and by_z.n_iter_ == 59


@pytest.mark.parametrize("case", tr.CASES, ids=tr.case_id)
def test_forces_and_one_step_at_the_reference_states(case):
    from causal_vae_amd import ops
    ref = tr.wide(case)
    states = tr.trajectory(case)["states"]
    P = dev(ref["P64"])
    lr = tr.auto_learning_rate(case[0])
    for i in tr.STATE_ITERS:
        Y, update, gains = states[i]
        ex, momentum = tr.phase_of(i)
        kl_w, grad_w, kl_scale, grad_scale = tr.forces(Y, ref["P64"], ex, scales=True)
        bf = tr.bounds_forces(case, kl_scale, grad_scale)
        kl, grad = ops.tsne_forces_f64(dev(Y), P, ex)
        r = {"kl": tr.max_ratio(host(kl)[0], kl_w, bf["kl"]), "grad": tr.max_ratio(host(grad), grad_w, bf["grad"])}
        s = tr.step(Y, update, gains, ref["P64"], ex, momentum, lr)
        bs = tr.bounds_step(case, s, update, momentum, lr, bf["grad"])
        Yn, un, gn, (kl1, norm) = ops.tsne_step_f64(dev(Y), dev(update), dev(gains), P, ex, momentum, lr)
        r.update({"Y": tr.max_ratio(host(Yn), s["Y"], bs["Y"]), "update": tr.max_ratio(host(un), s["update"], bs["update"]),
                  "gains": tr.max_ratio(host(gn), s["gains"], bs["gains"]), "grad_norm": tr.max_ratio(host(norm)[0], s["grad_norm"], bs["grad_norm"]),
                  "step kl": tr.max_ratio(host(kl1)[0], kl_w, bf["kl"])})
        print(f"RATIO tsne state {tr.case_id(case)} iteration {i} " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
        for k, v in r.items():
            assert v <= 1.0, (i, k, v)
        assert np.array_equal(host(gn) > np.asarray(gains), s["inc"]), i          # + 0.2 grows a gain, * 0.8 (or the floor of 0.01) does not: the decisions
        assert host(kl1)[0] == host(kl)[0]


@pytest.mark.parametrize("case", tr.CASES, ids=tr.case_id)
def test_short_trajectory(case):
    from causal_vae_amd import ops
    ref = tr.wide(case)
    want = tr.trajectory(case)["short"]
    fit = ops.tsne_fit_f64(dev(ref["P64"]), dev(tr.random_init(case[0])), max_iter=tr.TRAJ_STEPS)
    ratio = tr.max_ratio(host(fit.Y), want["Y"], tr.bound_trajectory(want["Y"]))
    print(f"RATIO tsne trajectory {tr.case_id(case)} {tr.TRAJ_STEPS} steps {ratio:.3g}")
    assert ratio <= 1.0 and fit.n_iter == tr.TRAJ_STEPS - 1 and fit.reason == 0 and fit.checks == 0


@pytest.mark.parametrize("case", tr.E2E_CASES, ids=tr.case_id)
def test_end_to_end(case):
    ref = tr.wide(case)
    fit = e2e_fit(case)
    assert fit.embedding_.shape == (case[0], 2) and fit.embedding_.dtype == np.float64 and fit.learning_rate_ == tr.auto_learning_rate(case[0])
    kl_w, _g, kl_scale, grad_scale = tr.forces(fit.embedding_, fit.affinities_, 1.0, scales=True)
    ratio = tr.max_ratio(fit.kl_divergence_, kl_w, tr.bounds_forces(case, kl_scale, grad_scale)["kl"])
    runs = tr.e2e_reference(case)
    kls = [float(r["kl"]) for r in runs]
    print(f"RATIO tsne end-to-end {tr.case_id(case)} kl {ratio:.3g}; KL {fit.kl_divergence_:.6g} against the reference's {min(kls):.6g} .. {max(kls):.6g}, "
          f"n_iter_ {fit.n_iter_} ({fit.stop_reason_})")
    assert ratio <= 1.0
    assert tr.nearest_neighbour_labels_agree(fit.embedding_, ref["labels"])
    assert fit.kl_divergence_ <= tr.E2E_MARGIN * max(kls[1:])
    from causal_vae_amd import ops
    reason = ops.TSNE_STOP_REASONS.index(fit.stop_reason_)
    if reason == 0:
        assert fit.n_iter_ == 999 and fit.n_checks_ == 20
    else:          # a stop is decided at a check: after an iteration i with (i + 1) % 50 == 0, and one record per 50 iterations was read
        assert (fit.n_iter_ + 1) % tr.CHECK == 0 and fit.n_checks_ == (fit.n_iter_ + 1) // tr.CHECK and fit.n_iter_ < 999


def test_schedule_and_status():
    from causal_vae_amd import ops
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import latent_tsne
    case = tr.CASES[0]
    ref = tr.wide(case)
    Y0 = tr.random_init(case[0])
    none = latent_tsne(ref["Z"], perplexity=case[2], init=Y0, max_iter=0, device=DEV, keep_affinities=True)
    kl, _grad = ops.tsne_forces_f64(dev(Y0), dev(none.affinities_), 1.0)
    assert np.array_equal(none.embedding_, Y0) and none.kl_divergence_ == float(kl.item()) and none.n_iter_ == 0
    early = latent_tsne(ref["Z"], perplexity=case[2], init=Y0, min_grad_norm=1e3, device=DEV)
    assert early.n_iter_ == 49 and early.stop_reason_ == ops.TSNE_STOP_REASONS[1] and early.n_checks_ == 1
    Zbad = ref["Z"].copy()
    Zbad[3, 2] = np.nan
    with pytest.raises(CvaeError, match=r"cvae_tsne_joint_f64.*info = 2"):
        latent_tsne(Zbad, perplexity=case[2], init=Y0, device=DEV)
    with pytest.raises(CvaeError, match=r"cvae_tsne_fit_f64.*info = 2"):
        Ynan = Y0.copy()
        Ynan[0, 0] = np.nan
        ops.tsne_fit_f64(dev(ref["P64"]), dev(Ynan), max_iter=60)


def test_two_fits_give_equal_bits():
    from causal_vae_amd.vit import latent_tsne
    case = tr.E2E_CASES[0]
    ref = tr.wide(case)
    first = e2e_fit(case)
    again = latent_tsne(ref["Z"], perplexity=case[2], init="random", random_state=42, device=DEV)
    assert np.array_equal(first.embedding_, again.embedding_) and first.kl_divergence_ == again.kl_divergence_ and first.n_iter_ == again.n_iter_


def test_pca_init():
    from causal_vae_amd.vit import latent_pca, latent_tsne
    import latent_pca_reference as pr
    case = tr.CASES[1]
    ref = tr.wide(case)
    Z = ref["Z"]
    start = latent_tsne(Z, perplexity=case[2], max_iter=0, device=DEV)          # init="pca" is the default
    scores = latent_pca(Z, 2, device=DEV).transform(Z)
    want = scores / scores[:, 0].std() * 1e-4
    assert np.abs(start.embedding_[:, 0].std() - 1e-4) < 1e-4 * 32 * tr.U          # the scaling's roundings and the deviation's own sum
    # the PCA bound on the scores (tests/latent_pca_reference.py's form with c = C_PCA), carried through the scaling: relative to the first column's deviation
    Zw = Z.astype(tr.WIDE)
    Xc = Zw - Zw.mean(axis=0)
    lam = np.sort(np.linalg.eigvalsh((Xc.T @ Xc).astype(np.float64)))[::-1]
    gap = min(lam[0] - lam[1], lam[1] - lam[2])
    N, d = Z.shape
    bound = pr.C_PCA * (N + d) * tr.U * (lam[0] / gap + 1) * np.sqrt((Xc.astype(np.float64) ** 2).sum(axis=1))[:, None] / scores[:, 0].std() * 1e-4 * 2
    assert (np.abs(start.embedding_ - want) <= bound).all()
    full = latent_tsne(Z, perplexity=case[2], device=DEV)
    assert np.isfinite(full.embedding_).all() and full.n_iter_ >= 249 and tr.nearest_neighbour_labels_agree(full.embedding_, ref["labels"])


def test_tsne_vit_latents_is_extract_then_tsne():
    from causal_vae_amd.vit import ViTVAEEncoder, extract_vit_latents, latent_tsne, tsne_vit_latents
    torch.manual_seed(3)
    model = ViTVAEEncoder(img_size=(64, 96), depth=1, latent_dim=16).to(DEV).eval()
    loader = [{"x": torch.randn(2, 1, 64, 96)} for _ in range(3)]
    Z, tsne = tsne_vit_latents(model, loader, DEV, perplexity=2.0, max_iter=100)
    assert Z.dtype == np.float32 and Z.shape == (6, 16) and np.array_equal(Z, extract_vit_latents(model, loader, DEV))
    again = latent_tsne(Z, perplexity=2.0, max_iter=100, device=DEV)
    assert np.array_equal(tsne.embedding_, again.embedding_) and tsne.kl_divergence_ == again.kl_divergence_ and tsne.n_iter_ == 99

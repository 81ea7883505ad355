"""The latent translator: steps 3 and 4 of the reference's latent_translator pipeline (main.py:129-150 on analysis.py:11-82, 91-165) on the float64 kernels of
csrc/ridge.hip.  fit_translator_ridge: a Ridge regression from the latents Z to the morphology table M, the features ranked by leave-one-out R²
(the exact closed form on one factorisation; the reference refits N times); translate_vit_latents: the same straight from a model and a loader, the latents
never leaving the device; compute_group_means / pairwise_contrasts / contrast_delta / topk_features / bootstrap_feature_stability: the group-contrast
bootstrap.  Where the reference returns a pandas DataFrame, a list of dicts stands in (there is no pandas here)."""
import numpy as np
import torch

from .. import ops
from .._lib import CvaeError


def _matrix(a, what):
    """a numpy array or a tensor on any device -> (a float32 / float64 matrix where it is, whether the caller gave numpy)"""
    was_numpy = not torch.is_tensor(a)
    t = torch.as_tensor(np.asarray(a)) if was_numpy else a.detach()
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    if t.dim() != 2:
        raise CvaeError(f"{what} must be a matrix, got {tuple(t.shape)}")
    return t, was_numpy


def _to_device(a, device, what):
    t, was_numpy = _matrix(a, what)
    return t.to(device), was_numpy


class RidgeTranslator:
    """What sklearn's fitted Ridge is to the reference: coef_ [F, d] and intercept_ [F] (float64 numpy, sklearn's names), alpha, and the by-products of the fit,
    loo_pred_ [N, F] (the leave-one-out predictions) and leverage_ [N].  predict(Z) = intercept_ + Z coef_^T on the device in float64: numpy in, numpy out;
    a tensor in, a tensor (on its device) out."""

    def __init__(self, coef, intercept, alpha, loo_pred, leverage, device="cuda"):
        self.coef_, self.intercept_, self.alpha = coef, intercept, float(alpha)
        self.loo_pred_, self.leverage_ = loo_pred, leverage
        self.device = device
        self._dev = None

    def _params(self, device):
        if self._dev is None or self._dev[0].device != torch.device(device):
            self._dev = (torch.as_tensor(self.coef_).to(device), torch.as_tensor(self.intercept_).to(device))
        return self._dev

    def predict(self, Z):
        if torch.is_tensor(Z) and Z.is_cuda:
            return ops.ridge_predict(Z, *self._params(Z.device))
        z, was_numpy = _to_device(Z, self.device, "Z")
        out = ops.ridge_predict(z, *self._params(z.device))
        return out.cpu().numpy() if was_numpy else out.to(Z.device)


def _feature_names(feature_names, F):
    names = list(feature_names)
    if not names:
        return [f"m{j}" for j in range(F)]
    if len(names) != F:
        raise CvaeError(f"feature_names has {len(names)} entries for {F} feature columns")
    return names


def _ranking(names, r2, corr):
    rows = [{"feature": n, "r2": float(a), "corr": float(b)} for n, a, b in zip(names, r2, corr)]
    return sorted(rows, key=lambda r: -r["r2"])          # sorted() is stable: ties stay in input order


def _fit(Zd, Md, names, alpha, device):
    fit = ops.ridge_fit_loo(Zd, Md, alpha)
    host = {k: getattr(fit, k).cpu().numpy() for k in ("coef", "intercept", "fitted", "loo", "leverage", "r2", "corr")}
    translator = RidgeTranslator(host["coef"], host["intercept"], alpha, host["loo"], host["leverage"], device=device)
    return translator, _ranking(names, host["r2"], host["corr"]), host["fitted"], translator.coef_


def fit_translator_ridge(Z, M, Z_test=None, M_test=None, feature_names=(), alpha=1.0, device="cuda"):
    """latent_translator/analysis.py:11-82: (translator, ranking, Mhat_full, W).  Z [N, d] and M [N, F]: numpy arrays or tensors on any device (Z_test and M_test
    are accepted and ignored, as there).  translator: a RidgeTranslator fitted on all of (Z, M); ranking: a list of {"feature", "r2", "corr"} dicts (Python
    floats) of the leave-one-out predictions against M, sorted by r2 descending with ties in input order (the reference's DataFrame); Mhat_full [N, F]: the
    fit's own predictions, float64 numpy; W: translator.coef_.  Empty feature_names: m0, m1, ...; any other length than F: CvaeError."""
    Zh, Mh = _matrix(Z, "Z")[0], _matrix(M, "M")[0]
    if Mh.shape[0] != Zh.shape[0]:
        raise CvaeError(f"fit_translator_ridge: Z has {Zh.shape[0]} rows, M has {Mh.shape[0]}")
    names = _feature_names(feature_names, Mh.shape[1])          # every refusal that needs no device comes before the first copy to it
    return _fit(Zh.to(device), Mh.to(device), names, alpha, device)


def _select_alpha(path, Md, names, select):
    """the rows of `path` (one dict per alpha, Python floats) and the index of the chosen alpha, from ONE host read: the mean squared leave-one-out residual over
    all rows and features ("mse", RidgeCV's criterion) or the mean leave-one-out R² over the features that are not constant ("r2"); a tie takes the first"""
    G, N = path.leverage.shape
    F = len(names)
    varies = (Md.max(dim=0).values != Md.min(dim=0).values).to(torch.float64)
    host = torch.cat([path.alphas[:, None], path.leverage.max(dim=1).values[:, None], path.sse, path.r2, varies[None, :].expand(G, F)], dim=1).cpu().numpy()
    alphas, max_h, sse, r2, keep = host[:, 0], host[:, 1], host[:, 2:2 + F], host[:, 2 + F:2 + 2 * F], host[0, 2 + 2 * F:] != 0
    rows = []
    for g in range(G):
        mean_r2 = float(np.sum(r2[g][keep]) / keep.sum()) if keep.any() else 0.0
        rows.append({"alpha": float(alphas[g]), "mse": float(np.sum(sse[g]) / (N * F)), "mean_r2": mean_r2, "max_leverage": float(max_h[g]),
                     "r2": {n: float(v) for n, v in zip(names, r2[g])}})
    score = [r["mse"] for r in rows] if select == "mse" else [-r["mean_r2"] for r in rows]
    return rows, min(range(G), key=lambda g: score[g])          # min() keeps the first of equals


def _fit_cv(Zd, Md, names, grid, select, device):
    rows, best = _select_alpha(ops.ridge_loo_path(Zd, Md, grid), Md.double(), names, select)
    return _fit(Zd, Md, names, grid[best], device) + (rows,)


def _cv_args(what, Zh, Mh, alphas, feature_names, select):
    """every refusal that needs no device -> (names, the grid as Python floats)"""
    if select not in ("mse", "r2"):
        raise CvaeError(f'{what}: select must be "mse" or "r2", got {select!r}')
    grid = ops.ridge_path_args(what, Zh, Mh, alphas)
    return _feature_names(feature_names, Mh.shape[1]), grid


def fit_translator_ridge_cv(Z, M, alphas=(0.1, 1.0, 10.0), feature_names=(), select="mse", device="cuda"):
    """fit_translator_ridge with alpha chosen from a grid by exact leave-one-out (sklearn's RidgeCV, whose default grid and criterion these are):
    (translator, ranking, Mhat_full, W, path).  The leave-one-out predictions of every alpha come from one eigendecomposition of the centred Gram matrix
    (ops.ridge_loo_path).  select="mse": the alpha with the smallest mean squared leave-one-out residual over all rows and features; select="r2": the largest
    mean leave-one-out R² over the features that are not constant (scale-free; what the ranking is by).  A tie takes the first alpha in the order given.  The
    chosen alpha is then fitted by fit_translator_ridge's own route, so the first four values are bit for bit fit_translator_ridge(..., alpha=chosen)'s and
    translator.alpha is the choice.  path: one dict per alpha, in the order given: "alpha", "mse", "mean_r2", "max_leverage" and "r2" (a dict by feature name),
    all Python floats."""
    what = "fit_translator_ridge_cv"
    Zh, Mh = _matrix(Z, "Z")[0], _matrix(M, "M")[0]
    names, grid = _cv_args(what, Zh, Mh, alphas, feature_names, select)
    return _fit_cv(Zh.to(device), Mh.to(device), names, grid, select, device)


@torch.no_grad()
def translate_vit_latents(model, loader, M, device, feature_names=(), alpha=1.0, alphas=None, select="mse"):
    """Steps 2 and 3 of the pipeline in one: (Z, translator, ranking, Mhat_full, W).  extract_vit_latents' protocol (eval mode, mu of every batch["x"]), but the
    per-batch mu stay on the device and go straight into the fit; Z [N, latent_dim] float32 numpy is copied to the host once, for the return value.
    model: a ViTVAE or a ViTVAEEncoder.  With a grid `alphas`, alpha is chosen from it as fit_translator_ridge_cv does (`alpha` is then not used) and the
    path is appended: (Z, translator, ranking, Mhat_full, W, path)."""
    model.eval()
    zs = [model.encode(batch["x"].to(device))[0] for batch in loader]
    if not zs:
        raise CvaeError("translate_vit_latents: the loader gave no batch")
    Zd = torch.cat(zs, dim=0)
    Md, _ = _to_device(M, device, "M")
    if Md.shape[0] != Zd.shape[0]:
        raise CvaeError(f"translate_vit_latents: the loader gave {Zd.shape[0]} samples, M has {Md.shape[0]} rows")
    if alphas is None:
        return (Zd.cpu().numpy(),) + _fit(Zd, Md, _feature_names(feature_names, Md.shape[1]), alpha, device)
    names, grid = _cv_args("translate_vit_latents", Zd, Md, alphas, feature_names, select)
    return (Zd.cpu().numpy(),) + _fit_cv(Zd, Md, names, grid, select, device)


def _unique_in_order(groups):
    seen = {}
    for g in groups:
        seen.setdefault(g, len(seen))
    return list(seen)


def compute_group_means(arr, groups):
    """analysis.py:91-98: (unique_groups, means [G, C]) with the groups in order of first appearance (pd.unique's order); host-side, in arr's precision."""
    arr, groups = np.asarray(arr), np.asarray(groups)
    uniq = _unique_in_order(groups.tolist())
    return uniq, np.stack([arr[groups == g].mean(axis=0) for g in uniq]) if uniq else np.zeros((0, arr.shape[1]), dtype=arr.dtype)


def pairwise_contrasts(groups):
    """analysis.py:100-105"""
    groups = list(groups)
    return [(groups[i], groups[j]) for i in range(len(groups)) for j in range(i + 1, len(groups))]


def contrast_delta(groups, means, g1, g2):
    """analysis.py:107-111 on compute_group_means' pair of values: the row of g2 minus the row of g1, each rounded to float32 first, as there."""
    groups = list(groups)
    means = np.asarray(means)
    return means[groups.index(g2)].astype(np.float32) - means[groups.index(g1)].astype(np.float32)


def topk_features(delta_m, feature_names, k=10):
    """analysis.py:113-116"""
    delta_m = np.asarray(delta_m)
    idx = np.argsort(-np.abs(delta_m))[:k]
    return [(feature_names[i], float(delta_m[i])) for i in idx]


def bootstrap_feature_stability(groups, Z, translator, feature_names, scale=None, n_boot=200, top_k=10, seed=0):
    """analysis.py:118-165: (rows, skipped).  rows: a list of {"feature", "topk_count", "stability_freq"} dicts sorted by frequency descending (ties in input
    order): how often a feature is among the top_k by |predicted difference| over every bootstrap and every pair of groups.  The resample indices are the
    reference's draws, np.random.RandomState(seed).randint(0, N, size=N) once per bootstrap in order; the groups are sorted(unique) with every pair i < j.
    Per bootstrap: the resampled group means (one kernel launch for all bootstraps), translator.predict of all of them (one launch), m2 - m1 (times `scale`,
    the reference's scaler_m.scale_, if given), the top_k by absolute value.  A group absent from a bootstrap sample crashes the reference; here its pairs are
    skipped for that bootstrap and not counted in the slots, and `skipped` is the number of such (bootstrap, pair) combinations."""
    groups = np.asarray([str(g) for g in np.asarray(groups).tolist()])
    names = list(feature_names)
    Zh = _matrix(Z, "Z")[0]
    N = Zh.shape[0]
    if groups.shape[0] != N:
        raise CvaeError(f"bootstrap_feature_stability: {groups.shape[0]} group labels for {N} rows of Z")
    if len(names) != translator.coef_.shape[0]:
        raise CvaeError(f"bootstrap_feature_stability: feature_names has {len(names)} entries for {translator.coef_.shape[0]} features")
    Zd = Zh.to(translator.device)
    uniq = sorted(_unique_in_order(groups.tolist()))
    code_of = {g: i for i, g in enumerate(uniq)}
    pairs = pairwise_contrasts(range(len(uniq)))
    rng = np.random.RandomState(seed)
    idx = np.stack([rng.randint(0, N, size=N) for _ in range(n_boot)]) if n_boot > 0 else np.zeros((0, N), dtype=np.int64)
    counts = {fn: 0 for fn in names}
    total_slots = skipped = 0
    if n_boot > 0 and pairs:
        codes = torch.as_tensor(np.array([code_of[g] for g in groups], dtype=np.int32)).to(Zd.device)
        means, present = ops.group_means_resampled(Zd, codes, torch.as_tensor(idx.astype(np.int32)).to(Zd.device), len(uniq))
        pred = translator.predict(means.reshape(n_boot * len(uniq), -1)).reshape(n_boot, len(uniq), -1).cpu().numpy()
        present = present.cpu().numpy() > 0
        scale = None if scale is None else np.asarray(scale, dtype=np.float64)
        for b in range(n_boot):
            for i, j in pairs:
                if not (present[b, i] and present[b, j]):
                    skipped += 1
                    continue
                dm = pred[b, j] - pred[b, i]
                if scale is not None:
                    dm = dm * scale
                for fn, _val in topk_features(dm, names, k=top_k):
                    counts[fn] += 1
                total_slots += top_k
    rows = [{"feature": fn, "topk_count": c, "stability_freq": c / max(total_slots, 1)} for fn, c in counts.items()]
    return sorted(rows, key=lambda r: -r["stability_freq"]), skipped

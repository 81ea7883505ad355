"""What the t-SNE tests (causal_vae_amd.vit.latent_tsne) rest on, checked without a GPU on tests/tsne_reference.py:
  the inputs    on the wide reference alone: at tol = 1e-5 no step of any row's search lands within 1e-9 of the tolerance while above it (nor, being above it,
                within 1e-9 of 0), so the stopping step is not a coin toss; in the trajectories no gradient entry is within 1e-12 of zero relative to the sum
                of |terms| behind it, and no update within 1e-12 of zero relative to its two terms, so no gain decision is one either
  the constants C_TSNE_* follow the rule from the ratios the same algebra in float64 numpy reaches with c = 1
  sklearn       (1.7.2 where it imports) _joint_probabilities on integer-valued rows, _kl_divergence at the reference's states, TSNE(method="exact") for the record
  end to end    the float64 reference meets the nearest-neighbour condition on the end-to-end inputs, and the spread of its final KL over one-ulp moves of the
                init stays below the 1.25 margin
  refusals      every tsne_args refusal is a CvaeError raised without a device

Measured here with c = 1 (the RATIO lines; D | beta, Pc, P at tol 1e-5 | the same at tol 0 | the largest over the three states of kl, grad | of gains, update,
Y, grad_norm | the 8-step trajectory in units of 8 * 2^-53 max |Y|):
  N33-d7-p5       0.218 | 0 0.107 0.0431 | 0.0676 0.0965 0.0713 | 0.0105 0.195 | 0.476 0.186 0.637 0.041  | 11.1
  N96-d20-p30     0.208 | 0 0.157 0.0844 | 0.0823 0.19   0.0893 | 0.00275 0.17 | 0.48  0.148 0.489 0.0175 | 3.89
  N130-d512-p10   0.00633 | 0 0.107 0.0633 | 0.153 0.133 0.0927 | 0.00464 0.217 | 0.498 0.173 0.718 0.0494 | 39.9
  N300-d10-p50    0.232 | 0 0.11  0.062  | 0.0585 0.121  0.0618 | 0.00909 0.161 | 0.494 0.16  0.621 0.0324 | 1.36
So C_TSNE_D = 1 (0.232), C_TSNE_AFF = 1 (0.19), C_TSNE_FORCE = 1 (0.217), C_TSNE_STEP = 4 (0.718: four times it is 2.9) and C_TSNE_TRAJ = 256 (39.9: the
descent stretches errors from the first step on, which is why 8 steps is the length compared pointwise).  beta at tol = 1e-5 is exact: the search only doubles,
halves and takes midpoints of dyadic numbers, and takes the same branches.
Margins: the closest a visited step comes to the tolerance is 1.2e-8 (N300); the smallest relative gradient entry over 401 steps is 2.2e-8, the smallest
relative update 4.9e-6.
sklearn: _joint_probabilities on integer rows (its search runs on float32 distances, which are exact there, and takes the same steps) is within 0.018 of
four times the float64 bound on P; _kl_divergence at the reference's states is within 0.068 of four times the float64 bound, the clamp of Q included.
End to end, final KL of the float64 reference from the init and from five one-ulp moves of it: N = 96: 0.00547 .. 0.00561, a spread of 1.025; N = 300:
0.2037 .. 0.2055, a spread of 1.009."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tsne_reference as tr  # noqa: E402

_RATIOS = {}


def float64_ratios(case):
    """the ratios with c = 1 of the float64 algebra against the wide reference, per constant, once"""
    if case not in _RATIOS:
        ref, N = tr.wide(case), case[0]
        r = {"D": {"D": tr.max_ratio(tr.sqdist(ref["Z"], np.float64), ref["D"], tr.bound_D(case, ref["D"], 1.0))}, "AFF": {}, "FORCE": {}, "STEP": {}, "TRAJ": {}}
        for name, tol in (("tol", 1e-5), ("tol0", 0.0)):
            a, b = ref[name], tr.bounds_affinities(case, ref[name], 1.0)
            g = tr.affinities(ref["D64"], case[2], tol, np.float64)
            g["P"] = tr.joint(g["Pc"])
            r["AFF"].update({f"{name} {k}": tr.max_ratio(g[k], a[k], b[k]) for k in ("beta", "Pc", "P")})
            if name == "tol":
                assert np.array_equal(g["steps"], a["steps"])
            assert abs(float(g["P"].sum()) - 1) <= b["sumP"]
        tj = tr.trajectory(case, margins=True)
        lr = tr.auto_learning_rate(N)
        for i in tr.STATE_ITERS:
            Y, u, g = tj["states"][i]
            ex, mom = tr.phase_of(i)
            kl, grad, kls, gs = tr.forces(Y, ref["P64"], ex, scales=True)
            bf = tr.bounds_forces(case, kls, gs, 1.0)
            k64, g64 = tr.forces(Y, ref["P64"], ex, np.float64)
            r["FORCE"].update({f"kl {i}": tr.max_ratio(k64, kl, bf["kl"]), f"grad {i}": tr.max_ratio(g64, grad, bf["grad"])})
            s, s64 = tr.step(Y, u, g, ref["P64"], ex, mom, lr), tr.step(Y, u, g, ref["P64"], ex, mom, lr, np.float64)
            bs = tr.bounds_step(case, s, u, mom, lr, bf["grad"], 1.0)
            r["STEP"].update({f"{k} {i}": tr.max_ratio(s64[k], s[k], bs[k]) for k in ("gains", "update", "Y", "grad_norm")})
            assert np.array_equal(s64["inc"], s["inc"])
        short = tr.fit(ref["P64"], tr.random_init(N), max_iter=tr.TRAJ_STEPS, dtype=np.float64)
        r["TRAJ"]["Y"] = tr.max_ratio(short["Y"], tj["short"]["Y"], tr.bound_trajectory(tj["short"]["Y"], 1.0))
        _RATIOS[case] = r
    return _RATIOS[case]


@pytest.mark.parametrize("case", tr.CASES + [tr.DUPLICATE_CASE], ids=tr.case_id)
def test_no_search_step_lands_on_the_tolerance(case):
    ref = tr.wide(case, duplicate=case == tr.DUPLICATE_CASE)
    v = ref["tol"]["visited"]
    v = v[~np.isnan(v)]
    above = v[v > 1e-5]
    print(f"TSNE search {tr.case_id(case)} steps {ref['tol']['steps'].min()}..{ref['tol']['steps'].max()} closest to tol {np.abs(above - 1e-5).min():.3g}")
    assert (np.abs(above - 1e-5) > 1e-9).all() and (above > 1e-9).all()
    assert (ref["tol"]["steps"] < tr.SEARCH_STEPS).all() and np.isfinite(ref["tol"]["P"].astype(np.float64)).all()
    P = ref["tol"]["P"]
    assert np.array_equal(P, P.T) and (P[~np.eye(len(P), dtype=bool)] >= tr.EPS).all()


@pytest.mark.parametrize("case", tr.CASES, ids=tr.case_id)
def test_no_gain_decision_is_a_coin_toss(case):
    float64_ratios(case)
    m = np.array(tr.trajectory(case, margins=True)["margins"])
    print(f"TSNE margins {tr.case_id(case)} over {len(m)} steps: gradient {m[:, 0].min():.3g} update {m[:, 1].min():.3g}")
    assert (m > 1e-12).all()


@pytest.mark.parametrize("name", ["D", "AFF", "FORCE", "STEP", "TRAJ"])
def test_bound_constants_follow_their_rule(name):
    worst = 0.0
    for case in tr.CASES:
        r = float64_ratios(case)[name]
        print(f"RATIO numpy-float64 c=1 {name} {tr.case_id(case)} " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
        worst = max(worst, max(r.values()))
    rule = max(1.0, 2.0 ** math.ceil(math.log2(4.0 * worst)))
    print(f"largest ratio {worst:.4g}: c = {rule:g}")
    assert getattr(tr, "C_TSNE_" + name) == rule


def test_sklearn_joint_probabilities_agree():
    tsne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    rng = np.random.RandomState(5)
    labels = np.arange(60) % 4
    Z = (rng.randint(-3, 4, size=(60, 6)) + 6 * np.eye(4, 6, dtype=np.int64)[labels] * 3).astype(np.float32)          # small integers: float32 distances are exact
    Z[1] = Z[0] + 1
    D = tr.sqdist(Z).astype(np.float64)
    assert np.array_equal(D, D.astype(np.float32))
    a = tr.affinities(D, 10.0)
    a["P"] = tr.joint(a["Pc"])
    got = squareform(tsne._joint_probabilities(D.astype(np.float32), 10.0, 0))
    ratio = tr.max_ratio(got, a["P"], tr.bounds_affinities((60, 6, 10.0), a, 4.0 * tr.C_TSNE_AFF)["P"])          # another route (no shift of the row): the rule's four on top
    print(f"RATIO sklearn _joint_probabilities {ratio:.3g}")
    assert ratio <= 1.0


@pytest.mark.parametrize("case", tr.CASES, ids=tr.case_id)
def test_sklearn_kl_divergence_agrees(case):
    tsne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    ref, N = tr.wide(case), case[0]
    states = tr.trajectory(case, margins=True)["states"]
    for i in tr.STATE_ITERS:
        Y = states[i][0]
        kl, grad, kls, gs = tr.forces(Y, ref["P64"], 1.0, scales=True)
        b = tr.bounds_forces(case, kls, gs, 4.0 * tr.C_TSNE_FORCE)
        kl_s, grad_s = tsne._kl_divergence(Y.ravel().copy(), squareform(ref["P64"]), 1, N, 2)          # the clamp of Q at 2^-52 included
        r = (tr.max_ratio(kl_s, kl, b["kl"]), tr.max_ratio(grad_s.reshape(N, 2), grad, b["grad"]))
        print(f"RATIO sklearn _kl_divergence {tr.case_id(case)} iteration {i} kl {r[0]:.3g} grad {r[1]:.3g}")
        assert max(r) <= 1.0


@pytest.mark.parametrize("case", tr.E2E_CASES, ids=tr.case_id)
def test_end_to_end_conditions_hold_for_the_float64_reference(case):
    ref = tr.wide(case)
    runs = tr.e2e_reference(case)
    kls = [float(r["kl"]) for r in runs]
    print(f"TSNE end-to-end {tr.case_id(case)} final KL {min(kls):.6g} .. {max(kls):.6g} spread {max(kls) / min(kls):.4g} n_iter {[r['n_iter'] for r in runs]}")
    assert all(tr.nearest_neighbour_labels_agree(r["Y"], ref["labels"]) for r in runs)
    assert max(kls) / min(kls) < tr.E2E_MARGIN
    try:
        from sklearn.manifold import TSNE
    except ImportError:
        return
    model = TSNE(method="exact", init=tr.random_init(case[0]), perplexity=case[2], random_state=0).fit(ref["Z"])
    print(f"TSNE sklearn method='exact' from the same init: final KL {model.kl_divergence_:.6g}, n_iter_ {model.n_iter_} (for the record)")


def test_refusals_need_no_device():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import latent_tsne
    Z = np.zeros((6, 4), dtype=np.float32)
    ok = dict(perplexity=2.0)
    for kw, match in [(dict(Z=np.zeros(6)), "matrix expected"), (dict(Z=np.zeros((6, 4), dtype=np.int64)), "float32 or float64"),
                      (dict(Z=np.zeros((6, 4), dtype=np.float16)), "float32 or float64"), (dict(Z=np.zeros((2, 4))), "3 <= N <= 4096"),
                      (dict(Z=np.zeros((4097, 1), dtype=np.float32)), "3 <= N <= 4096"), (dict(Z=Z, perplexity=6.0), r"perplexity must be in \(0, N\) = \(0, 6\)"),
                      (dict(Z=Z, perplexity=0.0), "perplexity must be in"), (dict(Z=Z), "perplexity must be in"), (dict(Z=Z, n_components=3, **ok), "n_components must be 2"),
                      (dict(Z=Z, early_exaggeration=0.0, **ok), "early_exaggeration must be positive"), (dict(Z=Z, learning_rate=0.0, **ok), "learning_rate must be positive"),
                      (dict(Z=Z, learning_rate="fast", **ok), "or 'auto'"), (dict(Z=Z, max_iter=-1, **ok), "max_iter must be a non-negative integer"),
                      (dict(Z=Z, init=np.zeros((5, 2)), **ok), r"shape \[N, 2\] = \[6, 2\]"), (dict(Z=Z, init="spectral", **ok), "'pca', 'random' or an array"),
                      (dict(Z=Z, tol=-1.0, **ok), "tol must be >= 0"), (dict(Z=None, distances=np.zeros((6, 6)), **ok), "init='pca' cannot be used with precomputed"),
                      (dict(Z=None, distances=np.zeros((6, 5)), init="random", **ok), "square matrix of squared distances"),
                      (dict(Z=Z, distances=np.zeros((6, 6)), **ok), "not both"), (dict(Z=np.zeros((6, 1025)), **ok), "1 <= d <= 1024"),
                      (dict(Z=np.zeros((5, 1)), **ok), r"n_components <= min\(N - 1, d\) = 1")]:
        with pytest.raises(CvaeError, match=match):
            latent_tsne(**kw)
    from causal_vae_amd import ops
    with pytest.raises(CvaeError, match="D must be a float64 tensor"):
        ops.tsne_affinities_f64(torch.zeros(6, 6), 2.0)
    with pytest.raises(CvaeError, match="Y must be a float64 tensor"):
        ops.tsne_forces_f64(torch.zeros(5, 2, dtype=torch.float64), torch.zeros(6, 6, dtype=torch.float64))
    with pytest.raises(CvaeError, match="MI355X only"):          # everything in order: the CPU tensor itself is refused, there is no fallback
        latent_tsne(torch.zeros(6, 4), device="cpu", init="random", **ok)
    with pytest.raises(CvaeError, match="MI355X only"):
        latent_tsne(torch.zeros(6, 4), device="cpu", **ok)

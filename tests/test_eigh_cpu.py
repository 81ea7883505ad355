"""What the symmetric eigensolver's tests (cvae_eigh_f64, csrc/eigh.hip) rest on, checked without a GPU on tests/eigh_reference.py:
  order         the round-robin order visits every pair exactly once per sweep, its rounds are disjoint, an odd n has one index sitting out per round
  reference     the wide Jacobi's spectrum equals numpy.linalg.eigvalsh within the bound (two independent methods); it handles the cases by design: a bye, a
                four-fold eigenvalue, a diagonal matrix in one sweep, a rotation angle that underflows
  the constant  C_EIGH follows the rule from the ratios two float64 evaluations reach with c = 1: numpy.linalg.eigh, and the reference's own Jacobi in float64
  refusals      the argument checks of ops.eigh_f64 that need no device

Measured here with c = 1 (the RATIO lines; residual, orth, trace, eig):
  case                         numpy.linalg.eigh              jacobi_eigh in float64 (sweeps)
  n1                           0     0     0      0           0     0     0     0      (1)
  n2                           0.26  1.12  0.24   0.22        0.51  1.32  0.24  0.22   (2)
  n3-bye                       0.43  1.17  0.089  0.27        0.21  2.54  0.17  0.11   (4)
  n5-identity-plus-rank-one    1.05  0.92  0.21   0.73        0.26  1.17  0.10  0.11   (2)
  n7-diagonal                  0     0     0      0           0     0     0     0      (1)
  n2-angle-underflows          0     0     0      0           0     0     0     0      (1)
  n64                          0.19  0.21  0.009  0.061       0.52  1.91  0.16  0.33   (9)
  n65                          0.25  0.25  0.009  0.065       0.55  1.91  0.097 0.24   (9)
  n130                         0.13  0.13  0.022  0.021       0.39  2.03  0.086 0.12   (10)
  gram-16x512                  0.098 0.038 0.002  -           0.69  5.52  0.037 -      (12)
The largest is 5.52 (the orthogonality of 12 sweeps of 511 rounds of rotations at n = 512): four times that, rounded up to a power of two, is C_EIGH = 32.
The float64 Jacobi run at n = 512 is most of this file's run time (about half a minute)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eigh_reference as er  # noqa: E402

_WIDE = {}


def wide_spectrum(name):
    if name not in _WIDE:
        _WIDE[name] = er.jacobi_eigh(er.matrix(name))
    return _WIDE[name]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 64, 65])
def test_round_robin_visits_every_pair_once(n):
    m = n + (n & 1)
    seen = set()
    for r in range(m - 1):
        p, q = er.round_pairs(n, r)
        idx = np.concatenate([p, q])
        assert len(set(idx.tolist())) == len(idx) and (p < q).all() and (q < n).all()          # disjoint
        assert len(idx) == n - (n & 1)                                                            # an odd n: exactly one index sits out
        seen.update(zip(p.tolist(), q.tolist()))
    assert seen == {(i, j) for i in range(n) for j in range(i + 1, n)}


@pytest.mark.parametrize("name", er.WIDE_AFFORDABLE)
def test_wide_jacobi_against_lapack(name):
    print(er.PRECISION)
    A = er.matrix(name)
    w, V, sweeps = wide_spectrum(name)
    n = A.shape[0]
    ev = np.linalg.eigvalsh(A)
    assert sweeps < er.MAX_SWEEPS and np.abs(w.astype(np.float64) - ev).max() <= er.C_EIGH * n * er.U * np.abs(ev).max()
    m = er.measures(A, w.astype(np.float64), V.astype(np.float64), w)          # rounded to float64: half an ulp per entry
    assert max(m.values()) <= er.C_EIGH, m
    if name == "n7-diagonal":
        assert sweeps == 1 and w.tolist() == sorted(np.diag(A).tolist())
    if name == "n2-angle-underflows":
        assert sweeps == 1 and w.tolist() == [1.0, 2.0]
    if name == "n5-identity-plus-rank-one":
        assert np.abs(w[:4].astype(np.float64) - 1.0).max() <= er.C_EIGH * 5 * er.U * float(w[4])


def test_bound_constant_follows_its_rule():
    worst = 0.0
    for name in er.CASES:
        A = er.matrix(name)
        w_ref = wide_spectrum(name)[0] if name in er.WIDE_AFFORDABLE else None
        w, V = np.linalg.eigh(A)
        lapack = er.measures(A, w, V, w_ref)
        wj, Vj, sweeps = er.jacobi_eigh(A, np.float64)
        jacobi = er.measures(A, wj, Vj, w_ref)
        assert sweeps < er.MAX_SWEEPS
        print(f"RATIO c=1 {name} numpy.linalg.eigh " + " ".join(f"{k} {v:.3g}" for k, v in lapack.items()) + f" | jacobi float64 ({sweeps} sweeps) " +
              " ".join(f"{k} {v:.3g}" for k, v in jacobi.items()))
        worst = max([worst] + list(lapack.values()) + list(jacobi.values()))
    rule = max(1.0, 2.0 ** math.ceil(math.log2(4.0 * worst)))
    print(f"largest ratio {worst:.4g}: c = {rule:g}")
    assert er.C_EIGH == rule


def test_refusals_need_no_device():
    from causal_vae_amd import ops
    from causal_vae_amd._lib import CvaeError
    for bad, pattern in [(torch.zeros(3, 4, dtype=torch.float64), "square float64 matrix"), (torch.zeros(3, 3), "square float64 matrix"),
                         (torch.zeros(3, dtype=torch.float64), "square float64 matrix"), (torch.zeros(0, 0, dtype=torch.float64), "1 <= n <= 1024"),
                         (torch.zeros(1025, 1025, dtype=torch.float64), "1 <= n <= 1024"), (torch.eye(3, dtype=torch.float64), "MI355X only")]:
        with pytest.raises(CvaeError, match=pattern):
            ops.eigh_f64(bad)

"""cvae_eigh_f64 on the device (csrc/eigh.hip through ops.eigh_f64) against tests/eigh_reference.py: the device's (w, V) evaluated in
numpy.longdouble under the bounds c n 2^-53 (scale) with c = C_EIGH = 32 (tests/test_eigh_cpu.py shows where it comes from).

Cases: n = 1; 2; 3 (a bye); 5 as I + a rank-one matrix (a four-fold eigenvalue); an already diagonal 7 x 7 with a repeated entry (one sweep, the tie in
original order); [[1, 1e-200], [1e-200, 2]] (the rotation angle underflows); 64 and 65 (a tile edge of the 16-pair workgroup tiles: 32 and 33 pairs); 130; and
the centred Gram matrix of a 16 x 512 float32 standard normal Z (rank 15, 497 zero eigenvalues).
  accuracy     residual max |A V - V diag(w)| <= c n 2^-53 max |A|; orthogonality max |V^T V - I| <= c n 2^-53; trace |sum w - tr A| <= c n 2^-53 sum |a_ii|;
               w ascending; |w - w_wide| <= c n 2^-53 ||A||_2 for n <= 130, |w - eigvalsh(A)| <= 2 c n 2^-53 ||A||_2 at n = 512; the sweeps used are reported
               and below the cap
  bits         two runs give equal bits
  info         a NaN or an infinity in A is a CvaeError with info 2 and a valid call right after it succeeds; nothing hangs, nothing faults
  layout       the lower triangle is what is read; ties keep their original order

Measured on the MI355X, the ratios with c = 32 (the RATIO lines of the run):
  n1                          sweeps 1   residual 0        orth 0       trace 0        eig 0
  n2                          sweeps 2   residual 0.0158   orth 0.0411  trace 0.0076   eig 0.00698
  n3-bye                      sweeps 4   residual 0.0151   orth 0.074   trace 0.000926 eig 0.0035
  n5-identity-plus-rank-one   sweeps 2   residual 0.00943  orth 0.0202  trace 0.00262  eig 0.00214
  n7-diagonal                 sweeps 1   residual 0        orth 0       trace 0        eig 0
  n2-angle-underflows         sweeps 1   residual 7.0e-187 orth 0       trace 0        eig 0
  n64                         sweeps 9   residual 0.0186   orth 0.065   trace 0.00169  eig 0.00865
  n65                         sweeps 9   residual 0.0171   orth 0.0711  trace 0.00281  eig 0.00735
  n130                        sweeps 10  residual 0.00948  orth 0.0652  trace 0.00327  eig 0.00306
  gram-16x512                 sweeps 12  residual 0.0206   orth 0.172   trace 0.000892 eig 0.00277 (against eigvalsh, at twice the bound)
No ratio is above 0.18 (orthogonality at n = 512, 5.5 with c = 1: what the float64 run of the reference's Jacobi reaches there); the cap is 48 sweeps."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eigh_reference as er  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_GOT = {}


def solved(name):
    """the device's (w, V, sweeps) of a case as numpy, once"""
    if name not in _GOT:
        from causal_vae_amd import ops
        w, V, sweeps = ops.eigh_f64(torch.as_tensor(er.matrix(name)).to(DEV))
        _GOT[name] = (w.cpu().numpy(), V.cpu().numpy(), sweeps)
    return _GOT[name]


@pytest.mark.parametrize("name", er.CASES)
def test_against_the_wide_reference(name):
    from causal_vae_amd._lib import lib
    A = er.matrix(name)
    n = A.shape[0]
    w, V, sweeps = solved(name)
    assert w.shape == (n,) and V.shape == (n, n) and w.dtype == np.float64 and type(sweeps) is int
    assert (np.diff(w) >= 0).all()
    assert 1 <= sweeps < lib.cvae_eigh_max_sweeps()
    affordable = name in er.WIDE_AFFORDABLE
    w_ref = er.jacobi_eigh(A)[0] if affordable else np.linalg.eigvalsh(A)
    m = er.measures(A, w, V, w_ref)
    if not affordable:
        m["eig"] /= 2.0          # both sides carry an error of the bound's order
    ratios = {k: v / er.C_EIGH for k, v in m.items()}
    print(f"RATIO eigh {name} sweeps {sweeps} " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (name, k, v)


def test_special_cases_by_value():
    w, V, sweeps = solved("n7-diagonal")
    A = er.matrix("n7-diagonal")
    assert sweeps == 1 and w.tolist() == sorted(np.diag(A).tolist())
    order = np.argsort(np.diag(A), kind="stable")          # ties by original index: the two entries 2.0 keep their order
    assert np.array_equal(V, np.eye(7)[:, order])
    w, V, sweeps = solved("n2-angle-underflows")
    assert w.tolist() == [1.0, 2.0] and np.array_equal(np.abs(V), np.eye(2))
    w, V, sweeps = solved("n1")
    assert w.tolist() == [-3.25] and V.tolist() == [[1.0]]
    w, V, sweeps = solved("n5-identity-plus-rank-one")
    assert np.abs(w[:4] - 1.0).max() <= er.C_EIGH * 5 * er.U * w[4]


def test_the_lower_triangle_is_read():
    from causal_vae_amd import ops
    A = er.matrix("n65")
    spoiled = np.tril(A) + np.triu(np.full_like(A, 7.0), 1)
    w, V, _ = ops.eigh_f64(torch.as_tensor(spoiled).to(DEV))
    assert np.array_equal(w.cpu().numpy(), solved("n65")[0]) and np.array_equal(V.cpu().numpy(), solved("n65")[1])


@pytest.mark.parametrize("name", ["n65", "gram-16x512"])
def test_two_runs_give_equal_bits(name):
    from causal_vae_amd import ops
    w, V, sweeps = ops.eigh_f64(torch.as_tensor(er.matrix(name)).to(DEV))
    assert np.array_equal(w.cpu().numpy(), solved(name)[0]) and np.array_equal(V.cpu().numpy(), solved(name)[1]) and sweeps == solved(name)[2]


@pytest.mark.parametrize("poison", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_entry_is_reported_through_info(poison):
    from causal_vae_amd import ops
    from causal_vae_amd._lib import CvaeError
    A = er.matrix("n65").copy()
    A[40, 7] = poison          # in the lower triangle
    with pytest.raises(CvaeError, match=r"non-finite entry was met \(info = 2\)"):
        ops.eigh_f64(torch.as_tensor(A).to(DEV))
    torch.cuda.synchronize()          # nothing faulted: the device still answers
    w, V, _ = ops.eigh_f64(torch.as_tensor(er.matrix("n65")).to(DEV))
    assert np.array_equal(w.cpu().numpy(), solved("n65")[0]) and bool(torch.isfinite(V).all())

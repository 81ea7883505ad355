"""CPU self-tests of oracle/loss64.py, the float64 references and bounds that tests/test_loss_reference.py holds csrc/losses.hip to.

  1. WITHIN THE BOUNDS: every reference evaluated in fp32 on the CPU (the stand-in for a correct kernel) lies within its bound; the ratio
     max |fp32 - float64| / bound is printed per operation (`RATIO <family> <value>`, the bracketed figures of the GPU file's docstring).
  2. ONE WRONG TERM FAILS: nine subtly wrong kernels, each a named restatement of the fp32 stand-in, are rejected by the same comparison.
  3. ARGUMENT CHECKS of the C entry points that return before any launch, each against what include/cvae_hip.h says.  Valid arguments get past every
     check, which without a device ends as CVAE_E_LAUNCH.  These tests are skipped where a device exists (host buffers stand in for device memory, so a
     missed check may only ever end as CVAE_E_LAUNCH).
     Header and behaviour disagreed twice; fixed with this file: cvae_bn1d_bwd_apply accepted any inv_n > 0 where cvae_bn1d_apply_stats (whose saved
     statistics it reads) demands a global batch of at least 2, inv_n in (0, 0.5] (the kernel's check was wrong, and the header now states the range for
     both); cvae_sqnorm_multi needs scratch for one float more than the tensors of ONE launch table (64 at the most), not `count + 1` as the header said
     (the header was wrong).
The float64 Adam reference takes the betas as the fp32 values the ABI receives; its distance to torch.optim.Adam in float64 with the unrounded 0.9 / 0.999
is printed (`ADAM_RECIPE_DISTANCE t <relative distance>`), not asserted."""
import ctypes as C

import pytest
import torch

from oracle import loss64 as l64

F32, F64 = torch.float32, torch.float64
BIG = (1 << 20) + 3075


def rnd(seed, *shape):
    return torch.randn(*shape, generator=l64.gen(seed))


def ratio(name, fn, *args, keys=None, **kw):
    """the fp32 evaluation of fn against its float64 reference: asserts it within the bounds, prints and returns the largest ratio"""
    ref, err = fn(*args, **kw)
    got, _ = fn(*args, dtype=F32, **kw)
    keys = keys or list(ref.keys())
    bad = l64.compare(got, ref, err, keys)
    worst = max(l64.max_ratio(got[k], ref[k], err[k]) for k in keys)
    print(f"RATIO {name} {worst:.4f}")
    assert not bad, "\n".join(bad)
    return worst


def rejected(got, ref, err, keys):
    bad = l64.compare(got, ref, err, keys)
    assert bad, f"the wrong result passed the comparison of {keys}"
    return bad


# ------------------------------------------------------------------------------------------------ 1. the fp32 stand-in lies within the bounds
@pytest.mark.parametrize("kind", ["sse", "sum", "sqnorm", "bce"])
@pytest.mark.parametrize("n", [1, 5, 1025, BIG])
def test_reductions_fp32_within_bounds(kind, n):
    a, b = (l64.bce_inputs(n, n) if kind == "bce" else (rnd(n, n), rnd(n + 1, n)))
    ratio(f"{kind}[n={n}]", l64.reduce2, kind, a, b, prefill=3.25)
    if kind == "sse":
        ratio("sse_bwd", l64.sse_bwd, a, b, torch.tensor(0.7), 0.25)
    if kind == "bce":
        ratio("bce_bwd", l64.bce_bwd, a, b, torch.tensor(-1.3))


def vessel_case(seed, n, kind, n_pos=None):
    r, x = l64.vessel_inputs(seed, n, kind)
    sum_x = x.double().sum().float()
    return r, x, sum_x, (n if n_pos is None else n_pos)


@pytest.mark.parametrize("kind,npm", [("general", 1), ("general", 3), ("zeros", 1), ("ones", 1), ("sparse", 1)])
def test_wmse_sparsity_fp32_within_bounds(kind, npm):
    n = (1 << 18) + 5
    r, x, sum_x, n_pos = vessel_case(7, n, kind, n * npm)
    pw, _, inside = l64.pos_weight(sum_x, n_pos)
    assert inside == (kind == "general") and float(pw) == {"zeros": 50.0, "ones": 1.0, "sparse": 50.0}.get(kind, float(pw))
    ratio(f"wmse_sparsity[{kind}, n_pos={npm}n]", l64.wmse_sparsity, r, x, sum_x, n_pos, prefill=(3.25, -1.5), g_recon=torch.tensor(0.3), g_sp=torch.tensor(-2.0))


def test_latent_and_nll_fp32_within_bounds():
    n = 65536 + 300
    mu, lv, eps, dz = rnd(1, n), 0.5 * rnd(2, n), rnd(3, n), rnd(4, n)
    ratio("reparam_kld", l64.reparam_kld, mu, lv, eps, prefill=3.25, dz=dz, gkld=torch.tensor(0.8), gk_scale=0.5)
    ratio("gauss_nll", l64.gauss_nll, rnd(5, n), mu, lv, prefill=3.25, gout=torch.tensor(1.7))
    for B, Z in ((1, 1), (17, 241), (9001, 1)):
        h = torch.cat([rnd(6, B, Z), 0.5 * rnd(7, B, Z)], 1)
        ratio(f"latent_head[{B}x{Z}]", l64.latent_head, h, rnd(8, B, Z), rnd(9, B, Z), rnd(10, B, Z), rnd(11, B, Z), torch.tensor(0.6))


@pytest.mark.parametrize("Cn", [1, 2, 10, 64])
@pytest.mark.parametrize("B", [1, 37, 1061])
def test_row_losses_fp32_within_bounds(B, Cn):
    logits = 30.0 * rnd(B * 100 + Cn, B, Cn)
    target = torch.randint(0, Cn, (B,), generator=l64.gen(B + Cn))
    target[0], target[-1] = 0, Cn - 1
    ratio(f"softmax_ce[{B}x{Cn}]", l64.softmax_ce, logits, target, prefill=3.25, gout=torch.tensor(0.9))
    ratio(f"uniform_kl[{B}x{Cn}]", l64.uniform_kl, logits, prefill=3.25, gout=torch.tensor(0.9))


def bn_case(seed, B, Fn, const_col=True):
    x = 1.5 + 2.0 * rnd(seed, B, Fn)
    if const_col:
        x[:, 0] = 1.5                                             # variance exactly 0
    return dict(x=x, w=1.0 + 0.5 * rnd(seed + 1, Fn), b=rnd(seed + 2, Fn), dy=rnd(seed + 3, B, Fn), rm=0.1 * rnd(seed + 4, Fn),
                rv=1.0 + torch.rand(Fn, generator=l64.gen(seed + 5)))


@pytest.mark.parametrize("B,Fn", [(2, 1), (63, 3), (65, 64), (129, 257)])
def test_bn1d_fp32_within_bounds(B, Fn):
    c = bn_case(B + Fn, B, Fn)
    ratio(f"bn1d[{B}x{Fn}]", l64.bn1d, c["x"], c["w"], c["b"], c["dy"], c["rm"], c["rv"], 0.1, 1e-5)
    ratio(f"bn1d[{B}x{Fn}, no affine]", l64.bn1d, c["x"], None, None, c["dy"], None, None, 0.1, 1e-5)
    ratio(f"bn1d_eval[{B}x{Fn}]", l64.bn1d_eval, c["x"], c["w"], c["b"], c["rm"], c["rv"], 1e-5)


SIZES = [1, 1023, 1024, 1025, 4097, 0, 7]


@pytest.mark.parametrize("device_step", [False, True])
@pytest.mark.parametrize("t0,steps", [(1, 3), (1000, 1), (100000, 1)])
def test_adam_fp32_within_bounds(device_step, t0, steps):
    n = 4099
    p, m, v = rnd(1, n), 0.1 * rnd(2, n), 0.01 * rnd(3, n).abs()
    if t0 == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    grads = [rnd(10 + k, n) for k in range(steps)]
    ratio(f"adam[t0={t0}, {steps} steps, device_step={device_step}]", l64.adam, p, m, v, grads, 1e-3, 0.9, 0.999, 1e-8, t0=t0, device_step=device_step,
          gscale=torch.tensor(0.37))


def test_adam_distance_to_the_unrounded_recipe():
    p = rnd(1, 4099)
    for t in (1, 2, 10):
        d = l64.adam_recipe_distance(p, [rnd(10 + k, 4099) for k in range(t)])
        print(f"ADAM_RECIPE_DISTANCE {t} {d:.3e}")


def test_scalars_fp32_within_bounds():
    tensors = [rnd(20 + i, s) for i, s in enumerate(SIZES)]
    ref, _ = l64.sqnorm_multi(tensors)
    ratio("sqnorm_multi", l64.sqnorm_multi, tensors, prefill=3.25)
    for max_norm in (0.5 * float(ref["out"].sqrt()), 2.0 * float(ref["out"].sqrt())):
        ratio("clip_coef", l64.clip_coef, ref["out"].float(), max_norm)
    ratio("scale", l64.scale, tensors[4], torch.tensor(0.123))
    terms = [rnd(40 + i, 1)[0] for i in range(8)]
    ratio("weighted_sum", l64.weighted_sum, terms, [0.5, 1.0, -2.0, 1e-3, 3.0, 0.1, 7.0, 1.5], torch.tensor(0.77))
    ratio("combine3", l64.combine3, rnd(50, 4), 0.1, 1e-4)


# ------------------------------------------------------------------------------------------------ 2. one wrong term fails the comparison
def fp32_sse(a, b, keep):
    d = (a.float() - b.float())[keep]
    return dict(out=(d * d).sum())


def test_fault_last_element_of_a_sum_dropped():
    n = 1025
    a, b = rnd(1, n), rnd(2, n)
    ref, err = l64.reduce2("sse", a, b)
    keep = torch.ones(n, dtype=torch.bool)
    assert not l64.compare(fp32_sse(a, b, keep), ref, err)
    keep[-1] = False
    rejected(fp32_sse(a, b, keep), ref, err, ["out"])


def test_fault_tail_of_the_float4_path_dropped():
    n = 1027
    a, b = rnd(3, n), rnd(4, n)
    ref, err = l64.reduce2("sse", a, b)
    keep = torch.ones(n, dtype=torch.bool)
    keep[n - n % 4:] = False
    rejected(fp32_sse(a, b, keep), ref, err, ["out"])


def test_fault_one_partial_sum_slot_dropped():
    """n = 2^20 + 3075 in 1024 blocks of 256 float4 lanes: block j owns the float4s i with (i // 256) % 1024 == j"""
    n = BIG
    a, b = rnd(5, n), rnd(6, n)
    ref, err = l64.reduce2("sse", a, b)
    slot = (torch.arange(n) // 4 // 256) % 1024
    rejected(fp32_sse(a, b, slot != 5), ref, err, ["out"])
    assert not l64.compare(fp32_sse(a, b, slot >= 0), ref, err)


def test_fault_biased_running_variance_and_local_batch():
    c = bn_case(11, 64, 5)
    args = (c["x"], c["w"], c["b"], c["dy"], c["rm"], c["rv"], 0.1, 1e-5)
    ref, err = l64.bn1d(*args, split=2)
    good, _ = l64.bn1d(*args, dtype=F32)
    assert not l64.compare(good, ref, err)
    b_for_bm1, _ = l64.bn1d(*args, dtype=F32, var_div=64)                  # B where B - 1 belongs
    assert rejected(b_for_bm1, ref, err, ["running_var"]) and not l64.compare(b_for_bm1, ref, err, ["y", "dx", "running_mean"])
    local_n, _ = l64.bn1d(*args, dtype=F32, n_stat=32)                     # the local B of 2 ranks where the global N belongs
    rejected(local_n, ref, err, ["save_mean"])
    rejected(local_n, ref, err, ["y"])
    rejected(local_n, ref, err, ["dx"])


def test_fault_onehot_missing_in_the_ce_gradient():
    logits, target = 3.0 * rnd(1, 37, 10), torch.randint(0, 10, (37,), generator=l64.gen(2))
    ref, err = l64.softmax_ce(logits, target)
    got, _ = l64.softmax_ce(logits, target, dtype=F32, no_onehot=True)
    rejected(got, ref, err, ["dlogits"])
    assert not l64.compare(got, ref, err, ["out"])


def test_fault_positive_weight_clamped_at_49():
    r, x, sum_x, n = vessel_case(3, 4096, "sparse")
    args = (r, x, sum_x, n)
    ref, err = l64.wmse_sparsity(*args, g_recon=torch.tensor(1.0))
    assert float(ref["pw"]) == 50.0
    got, _ = l64.wmse_sparsity(*args, g_recon=torch.tensor(1.0), dtype=F32, pw_cap=49.0)
    rejected(got, ref, err, ["out"])
    rejected(got, ref, err, ["dr"])


def test_fault_adam_with_bc2_of_the_step_before():
    n = 1025
    p, z = rnd(1, n), torch.zeros(n)
    grads = [rnd(10 + k, n) for k in range(3)]
    ref, err = l64.adam(p, z, z, grads, 1e-3, 0.9, 0.999, 1e-8, device_step=True)
    two, _ = l64.adam(p, z, z, grads[:2], 1e-3, 0.9, 0.999, 1e-8, dtype=F32)
    got, _ = l64.adam(two["p"], two["m"], two["v"], grads[2:], 1e-3, 0.9, 0.999, 1e-8, t0=3, dtype=F32, bc2_lag=1)
    rejected(got, ref, err, ["p"])
    assert not l64.compare(got, ref, err, ["m", "v"])


def test_fault_zero_length_tensor_shifts_the_table():
    """a list [a, empty, b, c]: the wrong kernel pairs every parameter after the empty entry with the NEXT tensor's gradient"""
    ps = [rnd(i, 7) for i in range(3)]
    gs = [rnd(10 + i, 7) for i in range(3)] + [rnd(99, 7)]
    z = torch.zeros(7)
    for i in range(3):
        ref, err = l64.adam(ps[i], z, z, [gs[i]], 1e-3, 0.9, 0.999, 1e-8)
        good, _ = l64.adam(ps[i], z, z, [gs[i]], 1e-3, 0.9, 0.999, 1e-8, dtype=F32)
        assert not l64.compare(good, ref, err)
        if i >= 1:
            shifted, _ = l64.adam(ps[i], z, z, [gs[i + 1]], 1e-3, 0.9, 0.999, 1e-8, dtype=F32)
            rejected(shifted, ref, err, ["p"])


def test_branch_margins_are_asserted():
    with pytest.raises(AssertionError):
        l64.wmse_sparsity(torch.ones(4), torch.tensor([0.0, 1.0, 0.1, 0.0]), torch.tensor(1.1), 4)
    with pytest.raises(AssertionError):
        l64.pos_weight(torch.tensor(50.0), 100)                       # pf = 0.5: the weight is 1 to within rounding
    with pytest.raises(AssertionError):
        l64.clip_coef(torch.tensor(4.0), 2.0 + 2e-6)


# ------------------------------------------------------------------------------------------------ 3. argument checks before any launch
HAS_DEVICE = torch.cuda.is_available()
needs_no_device = pytest.mark.skipif(HAS_DEVICE, reason="host pointers stand in for device memory: only where no launch can succeed")
OK, BADSHAPE, UNSUPPORTED, WORKSPACE, LAUNCH, NULLPTR = 0, -1, -3, -4, -5, -6

_buf = (C.c_float * (1 << 14))(*([3.25] * (1 << 14)))           # never read or written through: no launch succeeds here
P = (C.addressof(_buf) + 15) & ~15
NAN = float("nan")


def ptrs(*v):
    return C.cast((C.c_void_p * len(v))(*v), C.c_void_p)


def i64s(*v):
    return C.cast((C.c_int64 * len(v))(*v), C.c_void_p)


def f32s(*v):
    return C.cast((C.c_float * len(v))(*v), C.c_void_p)


T3, N3 = ptrs(P, P, P), i64s(4, 0, 9)
# entry point -> (valid arguments, [({position: value}, expected code)]); R(...) = every listed pointer is required
def R(*pos):
    return [({i: None}, NULLPTR) for i in pos]


def NZ(i):
    return [({i: -1}, BADSHAPE), ({i: 0}, OK)]


CHECKS = {
    "cvae_sse_fwd": ((P, P, P, 4, None, 0, None), NZ(3) + R(0, 1, 2)),
    "cvae_bce_fwd": ((P, P, P, 4, None, 0, None), NZ(3) + R(0, 1, 2)),
    "cvae_sum_fwd": ((P, P, 4, None, 0, None), NZ(2) + R(0, 1)),
    "cvae_sqnorm": ((P, P, 4, None, 0, None), NZ(2) + R(0, 1)),
    "cvae_sse_bwd": ((P, P, None, 1.0, P, 4, None), NZ(5) + R(0, 1, 4)),
    "cvae_bce_bwd": ((P, P, None, P, 4, None), NZ(4) + R(0, 1, 3)),
    "cvae_wmse_sparsity_fwd": ((P, P, P, P, 4, 4, None, 0, None), NZ(4) + R(0, 1, 2, 3) + [({5: 3}, BADSHAPE), ({5: 12}, LAUNCH)]),
    "cvae_wmse_sparsity_bwd": ((P, P, P, None, None, P, 4, 4, None), NZ(6) + R(0, 1, 2, 5) + [({7: 3}, BADSHAPE), ({7: 12}, LAUNCH)]),
    "cvae_reparam_kld_fwd": ((P, P, P, P, P, 4, None, 0, None), NZ(5) + R(0, 1) + [({2: None}, NULLPTR), ({3: None, 4: None}, NULLPTR),
                                                                                  ({2: None, 3: None}, LAUNCH), ({4: None}, LAUNCH)]),
    "cvae_reparam_kld_bwd": ((P, P, 1.0, P, P, P, P, P, 4, None), NZ(8) + R(3, 4, 6, 7) + [({5: None}, NULLPTR), ({0: None, 1: None, 5: None}, LAUNCH)]),
    "cvae_latent_head_fwd": ((P, P, P, P, P, P, 2, 3, None), [({6: -1}, BADSHAPE), ({6: 0}, OK), ({7: 0}, BADSHAPE), ({6: 1 << 12, 7: (1 << 12) + 1}, BADSHAPE),
                                                              ({6: 1 << 12, 7: 1 << 12}, LAUNCH)] + R(0, 1, 2) + [({3: None, 4: None, 5: None}, NULLPTR),
                                                              ({1: None, 2: None, 3: None, 4: None}, LAUNCH)]),
    "cvae_latent_head_bwd": ((P, P, P, P, P, P, P, 2, 3, None), [({7: -1}, BADSHAPE), ({7: 0}, OK), ({8: 0}, BADSHAPE)] + R(3, 4, 5, 6)
                             + [({0: None, 1: None, 2: None, 4: None, 5: None}, LAUNCH)]),
    "cvae_combine3": ((P, 1.0, 1.0, None), R(0)),
    "cvae_gauss_nll_fwd": ((P, P, P, P, 4, None, 0, None), NZ(4) + R(0, 1, 2, 3)),
    "cvae_gauss_nll_bwd": ((P, P, P, None, P, P, 4, None), NZ(6) + R(0, 1, 2, 4, 5)),
    "cvae_softmax_ce_fwd": ((P, P, P, 3, 10, None, 0, None), NZ(3) + R(0, 1, 2) + [({4: 65}, UNSUPPORTED), ({4: 64}, LAUNCH), ({4: 0}, BADSHAPE)]),
    "cvae_softmax_ce_bwd": ((P, P, None, P, 3, 10, None), NZ(4) + R(0, 1, 3) + [({5: 65}, UNSUPPORTED), ({5: 64}, LAUNCH), ({5: 0}, BADSHAPE)]),
    "cvae_uniform_kl_fwd": ((P, P, 3, 10, None, 0, None), NZ(2) + R(0, 1) + [({3: 65}, UNSUPPORTED), ({3: 64}, LAUNCH), ({3: 0}, BADSHAPE)]),
    "cvae_uniform_kl_bwd": ((P, None, P, 3, 10, None), NZ(3) + R(0, 2) + [({4: 65}, UNSUPPORTED), ({4: 64}, LAUNCH), ({4: 0}, BADSHAPE)]),
    "cvae_bn1d_train_fwd": ((P, None, None, P, P, P, None, None, 2, 3, 0.1, 1e-5, None), [({8: 1}, BADSHAPE), ({8: 0}, BADSHAPE), ({9: 0}, BADSHAPE)] + R(0, 3, 4, 5)),
    "cvae_bn1d_train_bwd": ((P, P, None, P, P, P, None, None, 2, 3, None), [({8: 1}, BADSHAPE), ({9: 0}, BADSHAPE)] + R(0, 1, 3, 4, 5)),
    "cvae_bn1d_eval_fwd": ((P, None, None, P, P, P, 1, 3, 1e-5, None), NZ(6) + [({7: 0}, BADSHAPE)] + R(0, 3, 4, 5)),
    "cvae_bn1d_stats": ((P, None, 0.0, P, 1, 3, None), [({4: 0}, BADSHAPE), ({5: 0}, BADSHAPE)] + R(0, 3) + [({1: P, 2: 0.5}, LAUNCH)]),
    "cvae_bn1d_apply_stats": ((P, None, None, P, P, 0.5, P, P, P, None, None, 1, 3, 0.1, 1e-5, None),
                              [({11: 0}, BADSHAPE), ({12: 0}, BADSHAPE), ({5: 0.0}, BADSHAPE), ({5: -0.25}, BADSHAPE), ({5: 0.75}, BADSHAPE), ({5: 1.0}, BADSHAPE),
                               ({5: NAN}, BADSHAPE), ({5: 1.0 / 96}, LAUNCH)] + R(0, 3, 4, 6, 7, 8)),
    "cvae_bn1d_bwd_sums": ((P, P, P, P, P, 1, 3, None), [({5: 0}, BADSHAPE), ({6: 0}, BADSHAPE)] + R(0, 1, 2, 3, 4)),
    "cvae_bn1d_bwd_apply": ((P, P, None, P, P, P, 0.5, P, 1, 3, None),
                            [({8: 0}, BADSHAPE), ({9: 0}, BADSHAPE), ({6: 0.0}, BADSHAPE), ({6: -0.25}, BADSHAPE), ({6: 0.75}, BADSHAPE), ({6: 1.0}, BADSHAPE),
                             ({6: NAN}, BADSHAPE), ({6: 1.0 / 96}, LAUNCH)] + R(0, 1, 3, 4, 5, 7)),
    "cvae_adam_step": ((P, P, P, P, 4, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, None, None),
                       NZ(4) + R(0, 1, 2, 3) + [({9: 0.0}, BADSHAPE), ({10: 0.0}, BADSHAPE), ({9: -0.1}, BADSHAPE), ({10: -1.0}, BADSHAPE)]),
    "cvae_adam_multi": ((T3, T3, T3, T3, N3, 3, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, None, None, None),
                        [({5: -1}, BADSHAPE), ({5: 0}, OK)] + R(0, 1, 2, 3, 4)
                        + [({10: 0.0}, BADSHAPE), ({11: 0.0}, BADSHAPE), ({10: -0.1}, BADSHAPE), ({10: 0.0, 11: 0.0, 12: P}, LAUNCH),      # bc ignored with a device step
                           ({4: i64s(4, -1, 9)}, BADSHAPE), ({4: i64s(0, 0, 0)}, OK), ({1: ptrs(P, None, P)}, LAUNCH),                       # NULL with n == 0: skipped
                           ({1: ptrs(P, P, None)}, NULLPTR), ({0: ptrs(None, P, P)}, NULLPTR), ({2: ptrs(P, P, None)}, NULLPTR), ({3: ptrs(None, P, P)}, NULLPTR)]),
    "cvae_multi_copy": ((T3, T3, N3, 3, None), [({3: -1}, BADSHAPE), ({3: 0}, OK)] + R(0, 1, 2) + [({2: i64s(4, -1, 9)}, BADSHAPE), ({0: ptrs(P, P, None)}, NULLPTR)]),
    "cvae_counter_add": ((P, 1, None), R(0)),
    "cvae_sqnorm_multi": ((T3, N3, 3, P, P, 16, None),
                          [({2: -1}, BADSHAPE), ({2: 0}, OK)] + R(0, 1, 3)
                          + [({4: None, 5: 0}, WORKSPACE), ({5: 12}, WORKSPACE), ({5: 15}, WORKSPACE), ({5: 4}, WORKSPACE), ({5: 0}, WORKSPACE),   # 3 tensors: 4 floats
                             ({1: i64s(4, -1, 9)}, BADSHAPE), ({1: i64s(0, 0, 0), 5: 0}, OK), ({0: ptrs(P, None, P)}, LAUNCH), ({0: ptrs(P, P, None)}, NULLPTR)]),
    "cvae_weighted_sum": ((T3, f32s(1.0, 2.0, 3.0), 3, None, P, 0, None),
                          [({2: 0}, BADSHAPE), ({2: 9}, BADSHAPE), ({2: -1}, BADSHAPE), ({1: None}, NULLPTR), ({4: None}, NULLPTR), ({0: None}, NULLPTR),
                           ({0: ptrs(P, None, P)}, NULLPTR), ({0: None, 5: 1}, LAUNCH), ({2: 1}, LAUNCH),
                           ({0: ptrs(*([P] * 8)), 1: f32s(*([1.0] * 8)), 2: 8}, LAUNCH)]),
    "cvae_scale": ((P, 4, P, None), NZ(1) + R(0, 2)),
    "cvae_clip_coef": ((P, P, 1.0, None), R(0, 1)),
}
FLAT = [(name, k) for name, (_a, muts) in CHECKS.items() for k in range(len(muts))]


@needs_no_device
@pytest.mark.parametrize("name", list(CHECKS))
def test_valid_arguments_reach_the_launch(name):
    from causal_vae_amd import _lib
    args, _ = CHECKS[name]
    assert len(args) == len(_lib.SIGNATURES[name])
    assert getattr(_lib.lib, name)(*args) == LAUNCH, f"{name}: the arguments are not otherwise valid"


@needs_no_device
@pytest.mark.parametrize("name,k", FLAT, ids=[f"{n}-{k}" for n, k in FLAT])
def test_argument_check(name, k):
    from causal_vae_amd import _lib
    args, muts = CHECKS[name]
    change, want = muts[k]
    bad = list(args)
    for i, v in change.items():
        bad[i] = v
    before = bytes(_buf)
    assert getattr(_lib.lib, name)(*bad) == want, f"{name} with {change}"
    assert bytes(_buf) == before                                  # no output written (n == 0 returns OK and leaves them alone)


@needs_no_device
def test_sqnorm_multi_scratch_is_per_launch_table():
    """70 tensors go as tables of 64 and 6: scratch for 65 floats is enough for both (the header said count + 1 = 71); 64 floats is not"""
    from causal_vae_amd import _lib
    tb, n = ptrs(*([P] * 70)), i64s(*([4] * 70))
    assert _lib.lib.cvae_sqnorm_multi(tb, n, 70, P, P, 65 * 4, None) == LAUNCH
    assert _lib.lib.cvae_sqnorm_multi(tb, n, 70, P, P, 64 * 4, None) == WORKSPACE


def test_the_table_names_every_entry_point_of_losses_hip():
    import os
    import re
    from causal_vae_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "losses.hip")).read()
    entries = set(re.findall(r'extern "C" int (cvae_\w+)\(', src))
    assert len(entries) >= 36 and entries - set(CHECKS) == {"cvae_philox_normal", "cvae_philox_normal_advance"}

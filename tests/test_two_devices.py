"""One process, two devices: a kernel's large-LDS limit is a property of one device's copy of that kernel (csrc/common.h, cvae_allow_lds), so the second
device a process drives has to get it as well.  Both ops launch with more than 64 KiB of dynamic LDS:

  ops.Linear, small-dense path   M = 32, K = N = 128, fp32: sd_fwd_kernel holds the weight and 16 rows of x, about 74 KB
  ops.conv_s1, K3                C = 128, bf16: about 67 KB

Each result is compared with the fp32 product of the same operands on the CPU, under the tolerance of the op's own test (test_hip_ops.py::
test_linear_forward_backward; test_vit_decoder.py::test_conv_s1_k3_against_float64, whose bf16 bound is led by half an ulp of the bf16 result).  Within
one process only the first order meets two untouched devices; the other still runs, since the suite may have used cuda:0 long before."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_decoder_reference as dr  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices in one process")]


def linear_small_dense(dev):
    from causal_vae_amd import _lib as L, ops
    M, K, N = 32, 128, 128
    assert ops.SMALL_DENSE and L.lib.cvae_small_dense_supported(M, K, N)
    g = torch.Generator().manual_seed(7)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    y = ops.Linear.apply(x.to(dev), w.to(dev), b.to(dev), None)
    ref = F.linear(x, w, b)
    torch.testing.assert_close(y.cpu(), ref, rtol=1e-4, atol=1e-4 * float(ref.abs().max()), msg=lambda s: f"small-dense Linear on {dev}: {s}")


def conv_s1_k3_bf16(dev):
    from causal_vae_amd import ops
    C, B, H, W = 128, 1, 8, 16
    rnd = lambda *shape, seed, scale=1.0: vr.round_bf16(scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed)))
    x, w, b = rnd(B, C, H, W, seed=1), rnd(C, C, 3, 3, seed=2, scale=0.1), torch.randn(C, generator=torch.Generator().manual_seed(3))
    (m, _b), = ops.fold_bn_conv([(w.to(dev), ops.FOLD_CONV_K3S1, None, None)])
    x_cl = x.permute(0, 2, 3, 1).contiguous().to(device=dev, dtype=torch.bfloat16)
    y = ops.conv_s1(x_cl, ops.conv_s1_pack_weights([m])[0], b.to(dev), ops.CONV_S1_K3, None)
    ref = F.conv2d(x, w, b, padding=1)
    terms = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1)
    err = (dr.kernel_terms("res", C) + 6) * vr.U32 * terms + vr.UBF * ref.double().abs()
    ratio = float(((y.permute(0, 3, 1, 2).cpu().double() - ref.double()).abs() / err).max())
    print(f"conv_s1 k3 bf16 on {dev}: max |got - ref| / bound = {ratio:.4f}")
    assert ratio <= 1.0, (dev, ratio)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["0_then_1", "1_then_0"])
def test_large_lds_kernels_run_on_both_devices_of_one_process(order):
    for i in order:
        with torch.cuda.device(i):
            linear_small_dense(f"cuda:{i}")
            conv_s1_k3_bf16(f"cuda:{i}")
            torch.cuda.synchronize()

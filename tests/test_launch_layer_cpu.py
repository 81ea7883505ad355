"""CPU check of the launch layer's dtype contract (include/cvae_hip.h: a dtype argument that is neither CVAE_F32 nor CVAE_BF16 is CVAE_E_DTYPE).

Every C entry point whose host code goes through common.h's with_dtype / dtype_ok and that takes a dtype code is called with arguments that are otherwise
valid: its smallest supported shape, 16-byte-aligned host buffers, the workspace size its own *_workspace_bytes names.  Each dtype argument in turn is set
to the code 7; the answer must be CVAE_E_DTYPE.  The same arguments with valid codes must get past every argument check, which on a machine without a
device ends as CVAE_E_LAUNCH: that is what shows the arguments to be "otherwise valid".  The whole file is skipped where a device exists, so that a missed
check can only end as CVAE_E_LAUNCH, never as a launch on host pointers."""
import ctypes as C

import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("host pointers stand in for device memory: only where no launch can succeed", allow_module_level=True)

from causal_vae_amd import _lib  # noqa: E402

lib = _lib.lib
F, BF = _lib.F32, _lib.BF16
OK, E_DTYPE, E_LAUNCH = 0, -2, -5
BAD = 7

_buf = (C.c_char * (1 << 16))()                     # never read or written through: no launch succeeds here
P = (C.addressof(_buf) + 15) & ~15


def ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def i64s(*v):
    return (C.c_int64 * len(v))(*v)


# ---- the bottleneck's host-side structs (read before the first launch) ----
_dims = _lib.BottleneckDims(M=2, D=1, H=1, W=1, C=64, OD=1, OH=1, OW=1, m_dim=4, t_dim=4, N1=4, N2=1, Z=1, HM=1)
_ptrs18 = _lib.BottleneckPtrs18(*([P] * 18))
_saved = _lib.BottleneckSaved(*([P] * 10))
DIMS, P18, SAVED = C.addressof(_dims), C.addressof(_ptrs18), C.addressof(_saved)

# 2D conv shapes: S (1 x 1 x 1) <-> L (1 x 2 x 2); the image forms read a 2 x 4 image (fp32 rows of whole 16-byte vectors)
S2, L2, L2W = (1, 1, 1), (1, 2, 2), (1, 2, 4)
WS_DOWN = lib.cvae_conv_data_workspace_bytes(1, *S2, 64, *L2, 16, 2, 0)
WS_UP = lib.cvae_conv_data_workspace_bytes(1, *S2, 16, *L2, 32, 2, 1)
WS_WG, WS_WG1 = lib.cvae_conv_wgrad_workspace_bytes(64, 32, 2), lib.cvae_conv_wgrad_workspace_bytes(32, 1, 2)
_multi = dict(S=ptrs(P), L=ptrs(P), dW=ptrs(P), db=ptrs(None), side=(C.c_int * 1)(0), ws=ptrs(P), wsb=(C.c_size_t * 1)(WS_WG), dims=i64s(1, *S2, 64, *L2, 32))
_pairs = dict(w=ptrs(P), down=ptrs(P), up=ptrs(P), Cs=i64s(16), Cl=i64s(16))

# (entry point, arguments with valid dtype codes, positions of its dtype arguments)
CASES = [
    ("cvae_cast", (P, P, 1, F, BF, None), (3, 4)),
    ("cvae_ncs_to_nsc", (P, P, 1, 2, 1, F, BF, None), (5, 6)),
    ("cvae_nsc_to_ncs", (P, P, 1, 2, 1, BF, F, None), (5, 6)),
    ("cvae_act_fwd", (P, P, 1, 0, F, None), (4,)),
    ("cvae_act_bwd", (P, P, P, 1, 0, BF, None), (5,)),
    ("cvae_channel_sum", (P, P, 1, 1, F, P, lib.cvae_channel_sum_workspace_bytes(1, 1, F), None), (4,)),
    ("cvae_adaptive_avgpool_fwd", (P, P, 1, 1, 1, 1, 1, 1, 1, 1, 1, F, None), (11,)),                       # bare Flatten
    ("cvae_adaptive_avgpool_fwd", (P, P, 1, 1, 2, 2, 1, 1, 1, 1, 1, BF, None), (11,)),                      # pooling
    ("cvae_adaptive_avgpool_bwd", (P, None, P, 1, 1, 1, 1, 1, 1, 1, 1, 1, F, None), (12,)),
    ("cvae_adaptive_avgpool_bwd", (P, None, P, 1, 1, 2, 2, 1, 1, 1, 1, 1, BF, None), (12,)),
    ("cvae_upsample_linear_fwd", (P, P, 1, 1, 1, 2, 1, 2, 4, 1, F, None), (10,)),                           # exact 2x
    ("cvae_upsample_linear_fwd", (P, P, 1, 1, 1, 1, 1, 1, 1, 1, BF, None), (10,)),                          # general
    ("cvae_upsample_linear_bwd", (P, P, 1, 1, 1, 2, 1, 2, 4, 1, F, None), (10,)),
    ("cvae_upsample_linear_bwd", (P, P, 1, 1, 1, 1, 1, 1, 1, 1, BF, None), (10,)),
    ("cvae_up2x_fwd", (P, P, 1, 1, 1, 4, 1, 2, 8, F, None), (9,)),                                          # block form
    ("cvae_up2x_fwd", (P, P, 1, 2, 8, 64, 4, 16, 128, BF, None), (9,)),                                     # LDS-tiled form
    ("cvae_elbo_up2x_fwd", (P, P, P, P, P, P, 1.0, P, P, None, None, None, 1, 1, 1, 4, 1, 2, 8, 1, 1, F, None), (21,)),
    ("cvae_elbo_up2x_bwd", (P, P, P, P, P, 1.0, P, P, P, P, P, 1, 1, 1, 4, 1, 2, 8, 1, 1, BF, None), (20,)),
    ("cvae_bn2d_fwd", (P, P, P, P, P, P, P, P, 2, 8, 0.1, 1e-5, 1, 0, F, P, lib.cvae_bn2d_workspace_bytes(2, 8), None), (14,)),
    ("cvae_bn2d_bwd", (P, P, P, P, P, P, P, P, P, 1, 8, 0, BF, P, lib.cvae_bn2d_workspace_bytes(1, 8), None), (12,)),
    ("cvae_row_diff_norms", (P, P, None, P, None, 1, 1, 1, F, P, lib.cvae_row_diff_norms_workspace_bytes(1, 1, F), None), (8,)),
    ("cvae_vit_tokens", (P, F, P, P, P, 1, 1, None), (1,)),
    ("cvae_layernorm256", (P, 256, P, P, P, 1, 1e-5, BF, None), (7,)),
    ("cvae_token_gemm", (P, 256, P, P, None, 0, P, 256, 1, 256, 256, 0, F, None), (12,)),
    ("cvae_token_gemm_gelu_train", (P, 256, P, P, P, 256, P, 256, 1, 256, 256, BF, None), (11,)),
    ("cvae_mhsa_fwd", (P, P, P, P, 256, 256, 256, 0, 0, 0, 1, 1, 1, F, None), (13,)),
    ("cvae_mhsa_fwd_train", (P, P, P, P, P, 256, 256, 256, 0, 0, 0, 1, 1, 1, BF, None), (14,)),
    ("cvae_vit_tokens_bwd", (P, P, P, P, F, None, 0, 1, 1, None), (4,)),
    ("cvae_layernorm256_bwd", (P, 256, BF, P, 256, P, P, 256, 0, P, P, 1, 1e-5, P, lib.cvae_layernorm256_bwd_workspace_bytes(1), None), (2,)),
    ("cvae_token_gemm_bwd_data", (P, 256, BF, P, None, 0, None, 0, P, 256, F, 1, 256, 256, BF, None), (2, 10, 14)),
    ("cvae_token_gemm_wgrad", (P, 256, F, P, 256, P, P, 1, 256, 256, BF, P, lib.cvae_token_gemm_wgrad_workspace_bytes(1, 256, 256), None), (2, 10)),
    ("cvae_mhsa_bwd", (P,) * 9 + ((256,) * 3 + (0,) * 3) * 2 + (1, 1, 1, F, P, lib.cvae_mhsa_bwd_workspace_bytes(1, 1), None), (24,)),
    ("cvae_conv_pack_weight", (P, P, 1, 16, 2, 0, F, None), (6,)),
    ("cvae_conv_pack_weight_pairs", (_pairs["w"], _pairs["down"], _pairs["up"], _pairs["Cs"], _pairs["Cl"], None, None, None, None, 1, 2, BF, None), (11,)),
    ("cvae_conv_down", (P, P, P, None, None, P, None, 1, *S2, 64, *L2, 16, 2, BF, 0, P, WS_DOWN, 0, None), (17,)),
    ("cvae_conv_down", (P, P, P, None, None, P, None, 1, *S2, 32, *L2, 1, 2, F, 0, None, 0, 0, None), (17,)),          # one image channel: conv_c1.hip
    ("cvae_conv_down_image", (P, F, P, P, None, P, 1, *S2[:2], 2, 32, *L2W, 2, BF, 0, None), (1, 15)),
    ("cvae_conv_down_image_f8", (P, F, P, P, P, None, None, None, None, 1, *S2[:2], 2, 32, *L2W, 2, 0, None), (1,)),
    ("cvae_conv_wgrad_image", (P, P, F, P, P, P, WS_WG1, 1, *S2[:2], 2, 32, *L2W, 2, BF, None), (2, 16)),
    ("cvae_conv_up", (P, P, P, None, None, P, None, 1, *S2, 16, *L2, 32, 2, BF, 0, P, WS_UP, 0, 0, 0, None), (17,)),
    ("cvae_conv_up", (P, P, P, None, None, P, None, 1, *S2, 32, *L2, 1, 2, F, 0, None, 0, 0, 0, 0, None), (17,)),
    ("cvae_conv_down_bwd_data", (P, P, P, P, 1, 1, 1, 16, 2, 2, 32, 2, BF, _lib.ACT_LEAKY02, P, WS_UP, 0, 0, None), (12,)),   # its own gated launch
    ("cvae_conv_down_bwd_data", (P, P, None, P, 1, 1, 1, 16, 2, 2, 32, 2, F, _lib.ACT_NONE, P, WS_UP, 0, 0, None), (12,)),    # through cvae_conv_up
    ("cvae_conv_wgrad", (P, P, P, None, 0, P, WS_WG, 1, *S2, 64, *L2, 32, 2, BF, None), (17,)),
    ("cvae_conv_wgrad", (P, P, P, P, 1, P, WS_WG1, 1, *S2, 32, *L2, 1, 2, F, None), (17,)),
    ("cvae_conv_wgrad_multi", (1, _multi["S"], _multi["L"], _multi["dW"], _multi["db"], _multi["side"], _multi["ws"], _multi["wsb"], _multi["dims"], 2, BF, None), (10,)),
    ("cvae_quantize_fp8", (P, F, P, 1, 1.0, None, None, None), (1,)),
    ("cvae_absmax", (P, BF, 1, P, None), (1,)),
    ("cvae_bottleneck_fwd", (DIMS, P18, P, P, P, None, P, P, P, None, 0.1, 1e-5, 1, P, P, None, SAVED, P, F, None, 0, None, None), (18,)),
    ("cvae_bottleneck_bwd", (DIMS, P18, P18, SAVED, P, P, P, P, P, P, P, P, 0, P, P, P, P, BF, None, None, None), (17,)),
    ("cvae_conv_s1", (P, P, P, None, P, 1, 1, 1, 32, 32, 0, F, 0, None), (11,)),
    ("cvae_conv_s1_c1", (P, P, P, P, 1, 1, 1, 16, BF, 0, None), (8,)),
    ("cvae_latent_to_grid", (P, P, P, P, 1, 4, 1, 32, F, None), (8,)),
    ("cvae_conv_s1_bwd_data", (P, P, None, None, P, 1, 1, 1, 32, 0, BF, 0, None), (10,)),
    ("cvae_conv_s1_c1_bwd_data", (P, P, None, P, 1, 1, 1, 16, F, 0, None), (8,)),
    ("cvae_latent_to_grid_bwd", (P, P, P, 1, 4, 1, 32, BF, P, lib.cvae_latent_to_grid_bwd_workspace_bytes(1, 4, 1, 32), None), (7,)),
    ("cvae_conv_s1_wgrad", (P, P, P, P, 1, 1, 1, 16, 0, F, P, lib.cvae_conv_s1_wgrad_workspace_bytes(1, 1, 1, 16, 0), None), (9,)),
    ("cvae_conv_s1_c1_wgrad", (P, P, P, P, 1, 1, 1, 16, BF, P, lib.cvae_conv_s1_c1_wgrad_workspace_bytes(1, 1, 1), None), (8,)),
    ("cvae_latent_to_grid_wgrad", (P, P, P, P, 1, 4, 1, 32, F, None), (8,)),
]
IDS = [f"{name}-{k}" for k, (name, _a, _d) in enumerate(CASES)]


@pytest.mark.parametrize("name,args,dtype_at", CASES, ids=IDS)
def test_unknown_dtype_code_is_e_dtype(name, args, dtype_at):
    fn = getattr(lib, name)
    assert len(args) == len(_lib.SIGNATURES[name]) and all(_lib.SIGNATURES[name][i] is C.c_int for i in dtype_at)
    assert fn(*args) == E_LAUNCH, f"{name}: the arguments are not otherwise valid"
    for i in dtype_at:
        bad = list(args)
        bad[i] = BAD
        assert fn(*bad) == E_DTYPE, f"{name}: argument {i} = {BAD}"


def test_the_table_covers_every_entry_that_lifts_a_dtype():
    """every extern "C" function of csrc/*.hip whose body (or a static helper it returns through) names with_dtype / with_dtype2 / dtype_ok"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    helpers = {"token_gemm": ("cvae_token_gemm", "cvae_token_gemm_gelu_train"), "mhsa_fwd": ("cvae_mhsa_fwd", "cvae_mhsa_fwd_train"),
               "mhsa_bwd": ("cvae_mhsa_bwd",), "token_gemm_bwd_data": ("cvae_token_gemm_bwd_data",), "transpose_cs": ("cvae_ncs_to_nsc", "cvae_nsc_to_ncs")}
    want = set()
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(".hip"):
            continue
        src = open(os.path.join(csrc, f)).read()
        starts = [m.start() for m in re.finditer(r'^(?:extern "C" |static |template |int |size_t |bool |namespace )', src, flags=re.M)] + [len(src)]
        for a, b in zip(starts, starts[1:]):                    # one top-level definition each
            m = re.match(r'(?:extern "C" |static )?int (\w+)\(', src[a:b])
            if m and re.search(r"\b(with_dtype2?|dtype_ok)\(", src[a:b]):
                want.update(helpers.get(m.group(1), (m.group(1),)))
    want = {n for n in want if n in _lib.SIGNATURES}
    assert len(want) >= 45 and want == {name for name, _a, _d in CASES}

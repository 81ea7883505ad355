"""ctypes binding of libcvae_hip.so — the C ABI declared in include/cvae_hip.h.

There is NO fallback: importing this module without the built library raises, and every op checks the
device of its tensors — the product path either runs the gfx950 kernels or fails loudly.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# CVAE_HIP_LIB (development only): another build of the same sources, e.g. with different tuning constants (make BUILD=build_x LIB=... EXTRA=-D...),
# for A/B runs in one GPU session; it must export the same C ABI (checked symbol by symbol below).
LIB_PATH = os.environ.get("CVAE_HIP_LIB") or os.path.join(_HERE, "libcvae_hip.so")

F32, BF16, FP8 = 0, 1, 2
U16 = 3          # CVAE_U16: cvae_mip_max's source only
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_LEAKY02, ACT_LEAKY001 = 0, 1, 2, 3, 4
_ACT = {None: ACT_NONE, "none": ACT_NONE, "relu": ACT_RELU, "sigmoid": ACT_SIGMOID, "leaky02": ACT_LEAKY02, "leaky001": ACT_LEAKY001}


class CvaeError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(or `make -C causal_vae_amd/csrc`).  causal_vae_amd has no CPU / eager fallback.")
lib = C.CDLL(LIB_PATH)

_p, _i64, _i, _f, _sz, _u64, _d = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_size_t, C.c_uint64, C.c_double

# name -> argtypes (restype is int unless listed in _RESTYPE); mirrors include/cvae_hip.h one to one.
SIGNATURES = {
    "cvae_version": [],
    "cvae_strerror": [_i],
    "cvae_ncs_to_nsc": [_p, _p, _i64, _i64, _i64, _i, _i, _p],
    "cvae_nsc_to_ncs": [_p, _p, _i64, _i64, _i64, _i, _i, _p],
    "cvae_cast": [_p, _p, _i64, _i, _i, _p],
    "cvae_copy_panels": [_p, _p, _p, _i, _p, _i64, _i64, _i64, _i, _p],
    "cvae_onehot_panel": [_p, _p, _i64, _i64, _i64, _i64, _p],
    "cvae_conv_pack_weight": [_p, _p, _i64, _i64, _i, _i, _i, _p],
    "cvae_conv_pack_weight_pairs": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p],
    "cvae_conv_data_workspace_bytes": [_i64] * 9 + [_i, _i],
    "cvae_conv_down": [_p] * 7 + [_i64] * 9 + [_i, _i, _i, _p, _sz, _i, _p],
    "cvae_conv_up": [_p] * 7 + [_i64] * 9 + [_i, _i, _i, _p, _sz, _i, _i, _i64, _p],
    "cvae_conv_down_bwd_data": [_p] * 4 + [_i64] * 7 + [_i, _i, _i, _p, _sz, _i, _i, _p],
    "cvae_conv_down_image_bwd_data": [_p, _p, _p] + [_i64] * 6 + [_i, _i, _f, _i, _p],
    "cvae_quantize_fp8": [_p, _i, _p, _i64, _f, _p, _p, _p],
    "cvae_conv_pack_weight_fp8": [_p, _p, _i64, _i64, _i, _i, _f, _p],
    "cvae_conv_up_c1_fp8in": [_p, _p, _p, _p, _f, _i64, _i64, _i64, _i64, _i64, _i, _i, _p],
    "cvae_absmax": [_p, _i, _i64, _p, _p],
    "cvae_conv_pack_weights_fp8": [_p, _p, _p, _p, _p, _p, _p, _i, _i, _p],
    "cvae_conv_fp8": [_i, _p, _p, _p, _p, _i, _p, _p, _f, _f, _p] + [_i64] * 9 + [_i, _i, _p, _sz, _i, _p, _p],
    "cvae_fp8_scale_update": [_p, _p, _p, _i, _f, _p, _p, _p, _i, _p, _p, _p],
    "cvae_conv_down_image_f8": [_p, _i, _p, _p, _p, _p, _p, _p, _p] + [_i64] * 8 + [_i, _i, _p],
    "cvae_conv_image_supported": [_p, _i64, _i, _i],
    "cvae_conv_down_image": [_p, _i, _p, _p, _p, _p] + [_i64] * 8 + [_i, _i, _i, _p],
    "cvae_conv_wgrad_image": [_p, _p, _i, _p, _p, _p, _sz] + [_i64] * 8 + [_i, _i, _p],
    "cvae_conv_wgrad_workspace_bytes": [_i64, _i64, _i],
    "cvae_conv_wgrad": [_p, _p, _p, _p, _i, _p, _sz] + [_i64] * 9 + [_i, _i, _p],
    "cvae_conv_wgrad_multi": [_i, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _p],
    "cvae_channel_sum_workspace_bytes": [_i64, _i64, _i],
    "cvae_channel_sum": [_p, _p, _i64, _i64, _i, _p, _sz, _p],
    "cvae_act_fwd": [_p, _p, _i64, _i, _i, _p],
    "cvae_act_bwd": [_p, _p, _p, _i64, _i, _i, _p],
    "cvae_adaptive_avgpool_fwd": [_p, _p] + [_i64] * 9 + [_i, _p],
    "cvae_adaptive_avgpool_bwd": [_p, _p, _p] + [_i64] * 9 + [_i, _p],
    "cvae_upsample_linear_fwd": [_p, _p] + [_i64] * 8 + [_i, _p],
    "cvae_upsample_linear_bwd": [_p, _p] + [_i64] * 8 + [_i, _p],
    "cvae_linear_workspace_bytes": [_i64, _i64, _i64, _i],
    "cvae_linear_fwd": [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i, _i, _p, _sz, _p],
    "cvae_linear_bwd_data": [_p, _p, _p, _i64, _i64, _i64, _i64, _i64, _p, _i, _p, _i64, _i, _i, _p, _sz, _p],
    "cvae_linear_bwd_weight": [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _p, _i, _i, _p, _sz, _p],
    "cvae_small_dense_supported": [_i64, _i64, _i64],
    "cvae_small_dense_workspace_bytes": [_i64, _i64, _i64],
    "cvae_small_dense_fwd": [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i, _p],
    "cvae_small_dense_bwd_data": [_p, _p, _p, _p, _i, _p, _i, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p],
    "cvae_small_dense_bwd_weight": [_p, _p, _p, _p, _p, _i, _i64, _i64, _i64, _i64, _i64, _i64, _p, _sz, _p],
    "cvae_bn1d_train_fwd": [_p] * 8 + [_i64, _i64, _f, _f, _p],
    "cvae_bn1d_train_bwd": [_p] * 8 + [_i64, _i64, _p],
    "cvae_bn1d_eval_fwd": [_p] * 6 + [_i64, _i64, _f, _p],
    "cvae_bn1d_stats": [_p, _p, _f, _p, _i64, _i64, _p],
    "cvae_bn1d_apply_stats": [_p] * 5 + [_f] + [_p] * 5 + [_i64, _i64, _f, _f, _p],
    "cvae_bn1d_bwd_sums": [_p] * 5 + [_i64, _i64, _p],
    "cvae_bn1d_bwd_apply": [_p] * 6 + [_f, _p, _i64, _i64, _p],
    "cvae_philox_normal": [_p, _i64, _u64, _u64, _u64, _p, _p],
    "cvae_philox_normal_advance": [_p, _i64, _u64, _u64, _u64, _p, _p],
    "cvae_reduce_workspace_bytes": [],
    "cvae_reparam_kld_fwd": [_p, _p, _p, _p, _p, _i64, _p, _sz, _p],
    "cvae_reparam_kld_bwd": [_p, _p, _f] + [_p] * 5 + [_i64, _p],
    "cvae_latent_head_fwd": [_p, _p, _p, _p, _p, _p, _i64, _i64, _p],
    "cvae_latent_head_bwd": [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _p],
    "cvae_sse_fwd": [_p, _p, _p, _i64, _p, _sz, _p],
    "cvae_sse_bwd": [_p, _p, _p, _f, _p, _i64, _p],
    "cvae_combine3": [_p, _f, _f, _p],
    "cvae_bce_fwd": [_p, _p, _p, _i64, _p, _sz, _p],
    "cvae_bce_bwd": [_p, _p, _p, _p, _i64, _p],
    "cvae_sum_fwd": [_p, _p, _i64, _p, _sz, _p],
    "cvae_wmse_sparsity_fwd": [_p, _p, _p, _p, _i64, _i64, _p, _sz, _p],
    "cvae_wmse_sparsity_bwd": [_p] * 6 + [_i64, _i64, _p],
    "cvae_gauss_nll_fwd": [_p, _p, _p, _p, _i64, _p, _sz, _p],
    "cvae_gauss_nll_bwd": [_p] * 6 + [_i64, _p],
    "cvae_softmax_ce_fwd": [_p, _p, _p, _i64, _i64, _p, _sz, _p],
    "cvae_softmax_ce_bwd": [_p, _p, _p, _p, _i64, _i64, _p],
    "cvae_uniform_kl_fwd": [_p, _p, _i64, _i64, _p, _sz, _p],
    "cvae_uniform_kl_bwd": [_p, _p, _p, _i64, _i64, _p],
    "cvae_adam_step": [_p, _p, _p, _p, _i64, _f, _f, _f, _f, _f, _f, _p, _p],
    "cvae_adam_multi": [_p, _p, _p, _p, _p, _i, _f, _f, _f, _f, _f, _f, _p, _p, _p],
    "cvae_multi_copy": [_p, _p, _p, _i, _p],
    "cvae_counter_add": [_p, _i, _p],
    "cvae_sqnorm": [_p, _p, _i64, _p, _sz, _p],
    "cvae_sqnorm_multi": [_p, _p, _i, _p, _p, _sz, _p],
    "cvae_weighted_sum": [_p, _p, _i, _p, _p, _i, _p],
    "cvae_scale": [_p, _i64, _p, _p],
    "cvae_clip_coef": [_p, _p, _f, _p],
    "cvae_up2x_supported": [_i64] * 7,
    "cvae_up2x_fwd": [_p, _p] + [_i64] * 7 + [_i, _p],
    "cvae_elbo_up2x_partials": [_i64] * 4,
    "cvae_elbo_up2x_fwd": [_p] * 6 + [_f, _p, _p, _p, _p, _p] + [_i64] * 9 + [_i, _p],
    "cvae_elbo_up2x_bwd": [_p] * 5 + [_f] + [_p] * 5 + [_i64] * 9 + [_i, _p],
    "cvae_conv3_to_k4": [_p, _p, _i64, _i64, _p],
    "cvae_k4_to_conv3_grad": [_p, _p, _i64, _i64, _p],
    "cvae_clamp_fwd": [_p, _p, _f, _f, _i64, _p],
    "cvae_clamp_bwd": [_p, _p, _p, _f, _f, _i64, _p],
    "cvae_bn2d_workspace_bytes": [_i64, _i64],
    "cvae_bn2d_fwd": [_p] * 8 + [_i64, _i64, _f, _f, _i, _i, _i, _p, _sz, _p],
    "cvae_bn2d_bwd": [_p] * 9 + [_i64, _i64, _i, _i, _p, _sz, _p],
    "cvae_bn2d_batch_workspace_bytes": [_i64, _i64],
    "cvae_bn2d_batch_fwd": [_p] * 8 + [_i64, _i64, _f, _f, _i, _i, _p, _sz, _p],
    "cvae_bn2d_batch_fwd_res": [_p] * 8 + [_i64, _i64, _f, _f, _i, _i, _p, _sz, _p, _p],
    "cvae_bn2d_batch_bwd_workspace_bytes": [_i64, _i64],
    "cvae_bn2d_batch_bwd": [_p] * 9 + [_i64, _i64, _i, _i, _p, _sz, _p],
    "cvae_fold_bn_conv": [_i] + [_p] * 11 + [_p],
    "cvae_fold_bn_conv_bwd": [_i] + [_p] * 14 + [_p],
    "cvae_vit_tokens": [_p, _i, _p, _p, _p, _i64, _i64, _p],
    "cvae_layernorm256": [_p, _i64, _p, _p, _p, _i64, _f, _i, _p],
    "cvae_token_gemm": [_p, _i64, _p, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _i, _i, _p],
    "cvae_mhsa_fwd": [_p] * 4 + [_i64] * 9 + [_i, _p],
    "cvae_mhsa_fwd_train": [_p] * 5 + [_i64] * 9 + [_i, _p],
    "cvae_mhsa_bwd_workspace_bytes": [_i64, _i64],
    "cvae_mhsa_bwd": [_p] * 9 + [_i64] * 15 + [_i, _p, _sz, _p],
    "cvae_token_gemm_gelu_train": [_p, _i64, _p, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _i, _p],
    "cvae_token_gemm_bwd_data": [_p, _i64, _i, _p, _p, _i64, _p, _i64, _p, _i64, _i, _i64, _i64, _i64, _i, _p],
    "cvae_token_gemm_wgrad_workspace_bytes": [_i64] * 3,
    "cvae_token_gemm_wgrad": [_p, _i64, _i, _p, _i64, _p, _p, _i64, _i64, _i64, _i, _p, _sz, _p],
    "cvae_layernorm256_bwd_workspace_bytes": [_i64],
    "cvae_layernorm256_bwd": [_p, _i64, _i, _p, _i64, _p, _p, _i64, _i, _p, _p, _i64, _f, _p, _sz, _p],
    "cvae_vit_tokens_bwd": [_p, _p, _p, _p, _i, _p, _i, _i64, _i64, _p],
    "cvae_mhsa_fwd_train_dropout": [_p] * 5 + [_i64] * 9 + [_f, _u64, _p],
    "cvae_mhsa_bwd_dropout": [_p] * 9 + [_i64] * 15 + [_f, _u64, _p, _sz, _p],
    "cvae_token_gemm_dropout": [_p, _i64, _p, _p, _p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _i, _f, _u64, _i64, _i64, _p],
    "cvae_token_gemm_bwd_data_dropout": [_p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _f, _u64, _i64, _i64, _p],
    "cvae_dropout_rows": [_p, _i64, _p, _i64, _i64, _i64, _f, _u64, _i64, _i64, _p],
    "cvae_dropout_keys_step": [_u64, _p, _p, _i, _p],
    "cvae_mhsa_fwd_train_dropout_devkey": [_p] * 5 + [_i64] * 9 + [_f, _p, _p],
    "cvae_mhsa_bwd_dropout_devkey": [_p] * 9 + [_i64] * 15 + [_f, _p, _p, _sz, _p],
    "cvae_token_gemm_dropout_devkey": [_p, _i64, _p, _p, _p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _i, _f, _p, _i64, _i64, _p],
    "cvae_token_gemm_bwd_data_dropout_devkey": [_p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _f, _p, _i64, _i64, _p],
    "cvae_dropout_rows_devkey": [_p, _i64, _p, _i64, _i64, _i64, _f, _p, _i64, _i64, _p],
    "cvae_mhsa_weights": [_p] * 4 + [_i64] * 8 + [_i, _i, _p],
    "cvae_mhsa_rollout_step": [_p] * 5 + [_i64] * 7 + [_f, _i, _p],
    "cvae_gradcam256": [_p, _p, _p, _i64, _i64, _i, _i, _p],
    "cvae_mhsa_weight_grads": [_p] * 3 + [_i64] * 6 + [_i, _p],
    "cvae_mhsa_relevance_step_workspace_bytes": [_i64] * 3,
    "cvae_mhsa_relevance_step": [_p] * 7 + [_i64] * 9 + [_i, _p, _sz, _p],
    "cvae_conv_s1_weight_elems": [_i64, _i64, _i],
    "cvae_conv_s1_pack_weights": [_i, _p, _p, _p, _p],
    "cvae_conv_s1": [_p] * 5 + [_i64] * 5 + [_i, _i, _i, _p],
    "cvae_conv_s1_c1": [_p] * 4 + [_i64] * 4 + [_i, _i, _p],
    "cvae_latent_to_grid": [_p] * 4 + [_i64] * 4 + [_i, _p],
    "cvae_conv_s1_bwd_data": [_p] * 5 + [_i64] * 4 + [_i, _i, _i, _p],
    "cvae_conv_s1_c1_bwd_data": [_p] * 4 + [_i64] * 4 + [_i, _i, _p],
    "cvae_latent_to_grid_bwd_workspace_bytes": [_i64] * 4,
    "cvae_latent_to_grid_bwd": [_p] * 3 + [_i64] * 4 + [_i, _p, _sz, _p],
    "cvae_conv_s1_wgrad_workspace_bytes": [_i64] * 4 + [_i],
    "cvae_conv_s1_wgrad": [_p] * 4 + [_i64] * 4 + [_i, _i, _p, _sz, _p],
    "cvae_conv_s1_c1_wgrad_workspace_bytes": [_i64] * 3,
    "cvae_conv_s1_c1_wgrad": [_p] * 4 + [_i64] * 4 + [_i, _p, _sz, _p],
    "cvae_latent_to_grid_wgrad": [_p] * 4 + [_i64] * 4 + [_i, _p],
    "cvae_mlp_heads_fwd": [_p, _i, _p, _i, _i64, _p, _p, _p, _i64, _p, _i64, _p, _i64, _p, _i64, _i64, _p],
    "cvae_mlp_heads_train_workspace_bytes": [_p, _i, _p, _i, _i64],
    "cvae_mlp_heads_bwd_workspace_bytes": [_p, _i, _p, _i, _i64],
    "cvae_mlp_heads_train_fwd": [_p, _i, _p, _i, _p, _i64, _p, _p, _p, _i64, _p, _i64, _p, _i64, _p, _i64, _i64, _p, _sz, _p],
    "cvae_mlp_heads_bwd": [_p, _i, _p, _p, _p, _i, _p, _i64, _p, _p, _p, _i64, _p, _i64, _p, _i64, _p, _i64, _i64, _p, _sz, _p, _sz, _p],
    "cvae_row_diff_norms_workspace_bytes": [_i64, _i64, _i],
    "cvae_row_diff_norms": [_p] * 5 + [_i64, _i64, _i64, _i, _p, _sz, _p],
    "cvae_stack_mean_std": [_p, _i, _p, _p, _i64, _p],
    "cvae_bottleneck_sizes": [_p, _p, _p, _p, _p, _p],
    "cvae_bottleneck_fwd": [_p] * 10 + [_f, _f, _i, _p, _p, _p, _p, _p, _i, _p, _i, _p, _p],
    "cvae_bottleneck_bwd": [_p] * 12 + [_i, _p, _p, _p, _p, _i, _p, _p, _p],
    "cvae_bottleneck_bn_local_stats": [_p] * 5 + [_i64, _i64, _i64, _p],
    "cvae_bottleneck_bn_bwd_finish": [_p] * 7 + [_i, _p],
    "cvae_col_means_f64_workspace_bytes": [_i64, _i64],
    "cvae_col_means_f64": [_p, _i64, _i64, _i64, _p, _p, _sz, _p],
    "cvae_ridge_gram_f64_workspace_bytes": [_i64] * 3,
    "cvae_ridge_gram_f64": [_p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _d, _p, _p, _p, _sz, _p],
    "cvae_chol_f64": [_p, _i64, _p, _p],
    "cvae_trsm_f64": [_p, _i64, _p, _i64, _i64, _p, _p, _i64, _i64, _i64, _i, _p],
    "cvae_ridge_loo_f64": [_p, _i64, _p, _p, _i64, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p],
    "cvae_ridge_predict_f64": [_p, _i64, _p, _p, _i64, _i64, _i64, _p, _p],
    "cvae_ranking_stats_f64": [_p, _i64, _p, _i64, _i64, _i64, _p, _p, _p],
    "cvae_group_means_resampled_f64": [_p, _i64, _p, _p, _i64, _i64, _i64, _i64, _p, _p, _p],
    "cvae_eigh_max_sweeps": [],
    "cvae_eigh_f64_workspace_bytes": [_i64],
    "cvae_eigh_f64": [_p, _i64, _i64, _p, _p, _i64, _p, _p, _sz, _p],
    "cvae_centered_gram_f64_workspace_bytes": [_i64] * 3,
    "cvae_centered_gram_f64": [_p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _p, _p, _p, _sz, _p],
    "cvae_centered_matmul_f64": [_p, _i64, _i64, _p, _p, _i64, _i64, _i64, _i64, _i64, _p, _i64, _p],
    "cvae_ridge_path_f64": [_p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _p],
    "cvae_pca_components_f64": [_p, _p, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _p],
    "cvae_tsne_sqdist_f64": [_p, _i, _i64, _i64, _i64, _p, _p],
    "cvae_tsne_affinities_f64": [_p, _i64, _d, _d, _p, _p, _p, _p],
    "cvae_tsne_joint_f64_workspace_bytes": [_i64],
    "cvae_tsne_joint_f64": [_p, _p, _i64, _p, _p, _p, _sz, _p],
    "cvae_tsne_forces_f64": [_p, _p, _i64, _p, _p, _p, _p, _p],
    "cvae_tsne_grad_f64": [_p, _p, _p, _p, _i64, _d, _p, _p, _p],
    "cvae_tsne_update_f64": [_p] * 7 + [_i64, _d, _d, _d, _p, _p, _p, _p, _p],
    "cvae_tsne_fit_f64_workspace_bytes": [_i64],
    "cvae_tsne_fit_f64": [_p, _p, _i64, _d, _d, _i64, _i64, _d, _p, _p, _p, _sz, _p],
    "cvae_morph12_threads": [_i64, _i64],
    "cvae_morph12_f32": [_p, _i64, _i64, _i64, _f, _d, _d, _d, _d, _p, _p, _p],
    "cvae_mip_max": [_p, _p, _i64, _i64, _i64, _i64, _i, _p],
    "cvae_resize_bilinear_aa_f32": [_p, _p, _i64, _i64, _i64, _i64, _i64, _p],
    "cvae_minmax_binarise_workspace_bytes": [_i64, _i64, _i64],
    "cvae_minmax_binarise": [_p, _p, _p, _i64, _i64, _i64, _i, _i, _p, _sz, _p],
    "cvae_percentile_clip_scale_workspace_bytes": [_i64, _i64],
    "cvae_percentile_clip_scale": [_p, _p, _p, _i64, _i64, _p, _p, _p, _sz, _p],
}
_RESTYPE = {"cvae_strerror": C.c_char_p, "cvae_conv_wgrad_workspace_bytes": _sz,
            "cvae_conv_data_workspace_bytes": _sz, "cvae_elbo_up2x_partials": _i64, "cvae_channel_sum_workspace_bytes": _sz,
            "cvae_linear_workspace_bytes": _sz, "cvae_reduce_workspace_bytes": _sz, "cvae_bn2d_workspace_bytes": _sz, "cvae_bn2d_batch_workspace_bytes": _sz,
            "cvae_bn2d_batch_bwd_workspace_bytes": _sz,
            "cvae_small_dense_workspace_bytes": _sz, "cvae_row_diff_norms_workspace_bytes": _sz,
            "cvae_mlp_heads_train_workspace_bytes": _sz, "cvae_mlp_heads_bwd_workspace_bytes": _sz,
            "cvae_conv_s1_weight_elems": _i64, "cvae_latent_to_grid_bwd_workspace_bytes": _sz,
            "cvae_conv_s1_wgrad_workspace_bytes": _sz, "cvae_conv_s1_c1_wgrad_workspace_bytes": _sz, "cvae_mhsa_bwd_workspace_bytes": _sz,
            "cvae_token_gemm_wgrad_workspace_bytes": _sz, "cvae_layernorm256_bwd_workspace_bytes": _sz,
            "cvae_mhsa_relevance_step_workspace_bytes": _sz, "cvae_col_means_f64_workspace_bytes": _sz, "cvae_ridge_gram_f64_workspace_bytes": _sz,
            "cvae_eigh_f64_workspace_bytes": _sz, "cvae_centered_gram_f64_workspace_bytes": _sz, "cvae_tsne_joint_f64_workspace_bytes": _sz,
            "cvae_tsne_fit_f64_workspace_bytes": _sz, "cvae_minmax_binarise_workspace_bytes": _sz, "cvae_percentile_clip_scale_workspace_bytes": _sz}

for _name, _args in SIGNATURES.items():
    _fn = getattr(lib, _name)          # AttributeError here = header and library disagree: fail at import
    _fn.argtypes = _args
    _fn.restype = _RESTYPE.get(_name, _i)


class BottleneckDims(C.Structure):
    """cvae_bottleneck_dims"""
    _fields_ = [(n, _i64) for n in ("M", "D", "H", "W", "C", "OD", "OH", "OW", "m_dim", "t_dim", "N1", "N2", "Z", "HM")]


BOTTLENECK_PARAMS = ("W1", "b1", "W2", "b2", "Wmu", "bmu", "Wlv", "blv", "Wm0", "bm0", "gamma", "beta", "Wm3", "bm3", "Wm5", "bm5", "Wd", "bd")
BOTTLENECK_SAVED = ("h1", "h2", "mu", "logvar", "xhat", "invstd", "a1n", "a2", "m_hat", "zm")


class BottleneckPtrs18(C.Structure):
    """cvae_bottleneck_params / cvae_bottleneck_grads: 18 device pointers in BOTTLENECK_PARAMS order"""
    _fields_ = [(n, _p) for n in BOTTLENECK_PARAMS]


class BottleneckSaved(C.Structure):
    """cvae_bottleneck_saved"""
    _fields_ = [(n, _p) for n in BOTTLENECK_SAVED]


class BottleneckNoise(C.Structure):
    """cvae_bottleneck_noise"""
    _fields_ = [("seed", _u64), ("subsequence", _u64), ("call_counter", _p)]


HEADS_MAX_PANELS, HEADS_MAX_LAYERS, HEADS_MAX_WIDTH = 3, 3, 512      # CVAE_HEADS_MAX_*


class HeadsPanel(C.Structure):
    """cvae_heads_panel"""
    _fields_ = [("ptr", _p), ("width", _i64), ("stride", _i64)]


class HeadsLayer(C.Structure):
    """cvae_heads_layer"""
    _fields_ = [("W", _p), ("b", _p), ("W2", _p), ("b2", _p), ("out", _i64), ("out_first", _i64), ("bn_weight", _p), ("bn_bias", _p), ("bn_mean", _p),
                ("bn_var", _p), ("bn_eps", _f), ("leaky", _i), ("slope", _f)]


class HeadsBnTrain(C.Structure):
    """cvae_heads_bn_train"""
    _fields_ = [("running_mean", _p), ("running_var", _p), ("num_batches_tracked", _p), ("momentum", _f)]


class HeadsLayerGrad(C.Structure):
    """cvae_heads_layer_grad"""
    _fields_ = [(n, _p) for n in ("dW", "db", "dW2", "db2", "dgamma", "dbeta")]


class KernelTimer:
    """Optional HIP-event timing of individual C-ABI launches (bench.py's roofline leg).  Events are recorded on torch's
    current stream — the stream the kernels are enqueued on — and only read after a device sync, so timing adds no sync."""

    def __init__(self):
        self.events = {}

    def run(self, name, fn, *args):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        rc = fn(*args)
        e.record()
        self.events.setdefault(name, []).append((s, e))
        return rc

    def summary(self):
        """name -> (launches, mean milliseconds).  Call after torch.cuda.synchronize()."""
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) / len(v)) for k, v in self.events.items()}


TIMER = None          # set to a KernelTimer to time conv launches


def timed(name, fn, *args):
    if TIMER is None:
        return fn(*args)
    return TIMER.run(name, fn, *args)


def strerror(code):
    return lib.cvae_strerror(code).decode()


def check(rc, what):
    if rc != 0:
        raise CvaeError(f"{what} failed: {strerror(rc)} (code {rc})")


def dtype_code(dt):
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    raise CvaeError(f"unsupported compute dtype {dt}; the gfx950 kernels take float32 or bfloat16")


def act_code(act):
    return _ACT[act]


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise CvaeError("causal_vae_amd runs on MI355X only: got a CPU tensor (there is no CPU fallback; "
                            "move the model and its inputs to 'cuda')")

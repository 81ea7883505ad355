"""ViTVAEEncoder — the encoder half of the reference's ViTVAE (vessel_analysis/00_core/vit_backbone.py:50-179; the same class in
latent_translator/models.py) for eval-mode inference on MI355X: image -> CLS feature -> (mu, log_var).

Same constructor order as the reference up to fc_var (its decoder is built AFTER these, so `torch.manual_seed(s); ViTVAEEncoder(...)` draws the
reference's encoder weights), same attribute tree and state_dict keys: stem.{0,1,3,4,..}, pos_embedding, cls_token, transformer.{i}.{norm1,
attn.in_proj_weight, attn.in_proj_bias, attn.out_proj, norm2, mlp.0, mlp.3}, to_latent, fc_mu, fc_var.  The torch modules only hold the parameters;
the arithmetic runs in libcvae_hip.so:
  stem        5 x [Conv2d(k3, s2, p1) + BatchNorm2d + LeakyReLU(0.01)]: BatchNorm folded, k3 zero-embedded into k4/s2/p1 (ONE cvae_fold_bn_conv launch),
              then cvae_conv_down with the activation in its epilogue; its channels-last output [B, h, w, 256] IS `rearrange("b c h w -> b (h w) c")`
  tokens      cvae_vit_tokens: CLS + patches + position embedding -> fp32 residual stream
  block       cvae_layernorm256, cvae_token_gemm (packed QKV), cvae_mhsa_fwd, cvae_token_gemm (+ residual), cvae_layernorm256,
              cvae_token_gemm (GELU), cvae_token_gemm (+ residual): 7 launches
  last block  encode reads x[:, 0] only: K and V of all tokens (one GEMM), the CLS query (one more), everything else for the CLS row alone
              (n_query_rows = 1): 8 launches
ViTVAEEncoder stops there (encode only; it carries no decoder parameters).  _walk(x, save) is that sequence, once: save=False is inference (cls_features, encode);
save=True is the training forward (cls_features_with_grad, encode_with_grad): the same calls with attention and the GELU GEMM in their training forms, the residual
GEMMs writing fresh tensors, and what the backward reads kept in named records (_BlockStep per block, _Walk, _StemKept).

ViTVAE(ViTVAEEncoder) adds the decoder half (vit_backbone.py:115-156, 181-199): decoder_input and decoder are built AFTER the encoder's modules, in the
reference's order and with its attribute tree (decoder.{0,1,4,5,8,9,12,13,15,16,18}, decoder.{3,7,11}.conv.{0,1,3,4}), so `torch.manual_seed(s); ViTVAE(...)`
draws the reference's weights and the state_dict key sets are equal.  decode, per call:
  fold           every BatchNorm2d of the decoder folded into the conv in front of it, ONE cvae_fold_bn_conv launch (11 layers), on every call
  decoder_input  cvae_latent_to_grid: the fp32 nn.Linear weight read once, output already channels-last [B, gh, gw, 256] (no view, no transposition)
  256->128->64->32   ConvTranspose2d(k3, s2, p1, op1) zero-embedded into the transposed k4 weight: cvae_conv_up with LeakyReLU(0.01) in its epilogue
  ResBlock(C)    two cvae_conv_s1 launches (3 x 3 window): LeakyReLU(0.2) in the first, the block input as the residual of the second
  32->16, 16->16 cvae_conv_s1 in sub-pixel form (2 x 2 forward window to 64 channels, pixel-shuffle store), LeakyReLU(0.01)
  16->1          cvae_conv_s1_c1 -> fp32 [B, 1, H, W]
decode_with_grad / decode_vjp add the gradient of that image with respect to z through the FROZEN eval-mode decoder: the forward issues
decode's launches (the fold also writes the backward matrices) and keeps five gate activations and the three ResBlock inner activations; the backward is
cvae_conv_s1_c1_bwd_data, cvae_conv_s1_bwd_data (every LeakyReLU derivative in an epilogue), cvae_conv_down on the k4 weights and cvae_latent_to_grid_bwd.
Training, all in eval mode (BatchNorm2d on its running statistics; dropout only where train_transformer(dropout=True) asks for it): train_decoder, train_transformer (§16) and train_stem (§17: the
stem's backward is cvae_vit_tokens_bwd with the stem output as its gate, then per layer cvae_conv_wgrad and cvae_conv_down_bwd_data with the LeakyReLU
derivative of the producing layer in its epilogue, then one cvae_fold_bn_conv_bwd launch; train_stem(batch_stats=True), DESIGN §23: the stem on
batch statistics, the module still in eval mode — per layer the raw conv, cvae_bn2d_batch_fwd, and cvae_bn2d_bwd on the way back; train_decoder(batch_stats=
True), DESIGN §24: the same for the decoder's 11 BatchNorm2d layers, with cvae_bn2d_batch_fwd_res at the end of a ResBlock and cvae_bn2d_batch_bwd on the
way back; folded and batch-statistics training share one stage loop in _decode_walk and one reverse loop each in _decode_backward and _stem_backward);
ViTVAE.train_all / forward_train, vit_vae_loss and train_vit_vae
are the reference's ViTVAE training loop (latent_translator/engine.py:6-36).
The gradient with respect to the IMAGE: cls_features_vjp / encode_vjp (explicit, no graph), x.grad after cls_features_with_grad / encode_with_grad /
forward_train of an x that asks, saliency (plain and integrated gradients) and gradcam.  They share a data-only form of the backward (_walk_backward(params=False):
no weight-gradient launch) whose last hop, 32 channels to the one-channel image, is cvae_conv_down_image_bwd_data (fp32 result in both compute dtypes).
Looking inside with a target: that backward hands each block's attention cotangent to an optional hook; attention_gradients (d target / d attention
probabilities, cvae_mhsa_weight_grads) and attention_relevance (gradient-weighted attention relevance, one cvae_mhsa_relevance_step per block) are built on it.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import layers as hl
from .. import ops
from .._lib import CvaeError, require_gpu

STEM_CHANNELS = (32, 64, 128, 256, 256)
# What ViTVAEEncoder._walk(save=True) keeps for _walk_backward.
# _StemKept (only when the stem trains): x (the image as the first conv reads it: its weight-gradient operand), ys (the five layer outputs: each the next
# layer's input, its weight-gradient operand and its gate), k4 (the folded k4 weights, for the data gradients).  The batch-statistics walk (train_stem(batch_stats=
# True)) fills the rest: ys are then the BatchNorm + LeakyReLU outputs a_j, k4 the RAW k4 weights (the k3 -> k4 zero-embedding, no scale), pre the five raw
# conv outputs y_j, mean / rstd each layer's batch statistics as cvae_bn2d_bwd reads them; pre is None in the eval-mode (folded) walk, which is how _stem_backward's
# one loop tells whether ops.bn2d_bwd stands in front of a layer, and how _walk_backward tells whether the token launch carries the gate.
# _BlockStep, one per transformer block: X (the block's input rows [B N, 256], norm1's input), y (norm1's output: the in-projection's operand), qkv (the packed
# in-projection output; k and v alone [B, N, 512] in a CLS-only block), q (the CLS-only block's one query row per sample, else None), att / lse (attention's
# output and row statistic), X1 (the stream after attention: norm2's input), y2 (norm2's output), pre / hid (the MLP's pre-activation and its GELU), B, N,
# cls_only (everything from the attention's queries on ran for the CLS rows alone: att, X1, y2, pre, hid have B rows, not B N), drop (the block's three dropout
# sites as the forward ran them, DESIGN §18: ((p, key) or None) for the attention probabilities, the GELU output and the second Linear's output; hid is then
# the DROPPED GELU output, att the dropped attention's; the masks themselves are not kept, the backward recomputes them).
# _Walk: steps (the _BlockSteps in forward order), cls (to_latent's input [B, 256]), stem_dtype (the dtype dstem is returned in), B, N, stem (_StemKept or None),
# stem_out (the stem's channels-last output, what Grad-CAM weighs with dstem).
_StemKept = namedtuple("_StemKept", "x ys k4 pre mean rstd", defaults=(None, None, None))
_BlockStep = namedtuple("_BlockStep", "X y qkv q att lse X1 y2 pre hid B N cls_only drop")
_NO_DROP = (None, None, None)
_Walk = namedtuple("_Walk", "steps cls stem_dtype B N stem stem_out")


class _Block(nn.Module):
    """Parameter holder with the reference ViTBlock's children (vit_backbone.py:22-38), built in its order."""

    def __init__(self, dim, heads, mlp_dim, dropout=0.1):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = nn.MultiheadAttention(embed_dim=dim, num_heads=heads, dropout=dropout, batch_first=True)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = nn.Sequential(nn.Linear(dim, mlp_dim), nn.GELU(), nn.Dropout(dropout), nn.Linear(mlp_dim, dim), nn.Dropout(dropout))


class ViTVAEEncoder(nn.Module):
    compute_dtype = torch.float32
    _cls_only_last_block = True     # private (tests): False: the last block runs for every token like the others (same CLS row, bit for bit; tests compare the two)

    def __init__(self, in_channels=1, latent_dim=128, img_size=(768, 1280), patch_size=32, embed_dim=256, depth=6, heads=8, mlp_dim=512):
        super().__init__()
        H, W = (int(v) for v in img_size)
        if (embed_dim, heads, mlp_dim, patch_size, in_channels) != (256, 8, 512, 32, 1) or H < 32 or W < 32 or H % 32 or W % 32 or depth < 1 or latent_dim < 1:
            raise CvaeError("ViTVAEEncoder: the gfx950 kernels implement embed_dim 256, 8 heads, mlp_dim 512, patch_size 32, one input channel, image height "
                            f"and width multiples of 32 (got embed_dim={embed_dim}, heads={heads}, mlp_dim={mlp_dim}, patch_size={patch_size}, "
                            f"in_channels={in_channels}, img_size={tuple(img_size)}, depth={depth}, latent_dim={latent_dim})")
        self.latent_dim, self.embed_dim, self.patch_size, self.depth = latent_dim, embed_dim, patch_size, depth
        self.img_height, self.img_width = H, W
        stem, cin = [], in_channels
        for cout in STEM_CHANNELS:
            stem += [nn.Conv2d(cin, cout, kernel_size=3, stride=2, padding=1), nn.BatchNorm2d(cout), nn.LeakyReLU()]
            cin = cout
        self.stem = nn.Sequential(*stem)
        self.grid_h, self.grid_w = H // 32, W // 32
        self.num_patches = self.grid_h * self.grid_w
        self.pos_embedding = nn.Parameter(torch.randn(1, self.num_patches + 1, embed_dim))
        self.cls_token = nn.Parameter(torch.randn(1, 1, embed_dim))
        self.transformer = nn.Sequential(*[_Block(embed_dim, heads, mlp_dim) for _ in range(depth)])
        self.to_latent = nn.LayerNorm(embed_dim)
        self.fc_mu = nn.Linear(embed_dim, latent_dim)
        self.fc_var = nn.Linear(embed_dim, latent_dim)
        # the Philox keys of train_transformer(dropout=True)'s masks, one step per training forward: ops.DropoutKeys (host-side, the default) or, after
        # use_device_dropout_keys(), ops.DeviceDropoutKeys (the step counter on the device: what a captured step needs).  A plain attribute:
        # its device tensors are no buffers, the state_dict keys stay the reference's.
        self.dropout_keys = ops.DropoutKeys()

    def set_compute_dtype(self, dtype):
        if dtype not in (torch.float32, torch.bfloat16):
            raise CvaeError(f"compute dtype must be float32 or bfloat16, got {dtype}")
        self.compute_dtype = dtype
        return self

    # ---- the pipeline -------------------------------------------------------------------------------------------------------------
    def _check(self, x):
        if self.training:
            raise RuntimeError("ViTVAEEncoder: put the model in eval mode first (model.eval()): dropout and batch-statistics BatchNorm2d are not "
                               "implemented, the encoder runs inference only")
        if x.dim() != 4 or tuple(x.shape[1:]) != (1, self.img_height, self.img_width) or x.dtype != torch.float32:
            raise CvaeError(f"ViTVAEEncoder expects a float32 [B, 1, {self.img_height}, {self.img_width}] batch, got {tuple(x.shape)} {x.dtype}")
        require_gpu(x, self.cls_token)

    def _stem_fold_table(self):
        """ops.fold_bn_conv's entry for each of the stem's five (conv, BatchNorm2d) pairs."""
        mods = list(self.stem)
        return [(mods[i].weight, ops.FOLD_CONV_K3S2, mods[i].bias, mods[i + 1]) for i in range(0, len(mods), 3)]

    def _stem_cl(self, x, keep=None, batch_stats=False):
        """keep (a dict, the stem's backward): receives _StemKept's fields `x`, `ys` and `k4`.  The launches do not depend on it.
        batch_stats (the training walk after train_stem(batch_stats=True)): no fold — per layer the conv on the RAW weight and bias without an
        activation (the fold's launch with no BatchNorm: the k3 -> k4 zero-embedding at scale 1; the bias cancels in the normalised value but running_mean
        must contain it), then ops.bn2d_batch_fwd: this batch's statistics, LeakyReLU(0.01), the running statistics and counters updated in place.  keep then
        also receives `pre`, `mean` and `rstd`."""
        table = self._stem_fold_table()
        folded = ops.fold_bn_conv([(w, kind, b, None) for w, kind, b, _bn in table] if batch_stats else table)
        h, first_dtype = hl._image_cl(x, self.compute_dtype)
        if keep is not None:
            keep["x"], keep["ys"], keep["k4"] = h, [], [w for w, _b in folded]
            if batch_stats:
                keep["pre"], keep["mean"], keep["rstd"] = [], [], []
        for j, (w, b) in enumerate(folded):
            h = ops.ConvDown.apply(h, w, b, 2, None if batch_stats else "leaky001", False, False, None, first_dtype if j == 0 else None)
            if batch_stats:
                pre, (h, mean, rstd) = h, ops.bn2d_batch_fwd(h, table[j][3], "leaky001")
                if keep is not None:
                    keep["pre"].append(pre), keep["mean"].append(mean), keep["rstd"].append(rstd)
            if keep is not None:
                keep["ys"].append(h)
        return h                                                        # [B, 1, grid_h, grid_w, 256], compute dtype

    def _block(self, blk, tokens, cls_only, save, drop=_NO_DROP, attention=None):
        """One transformer block on the fp32 residual stream `tokens` [B, N, 256] -> (the stream after it [B, N, 256], or with cls_only the block's CLS rows
        [B, 256]: the same sums in the same order as the full block's row 0, `tokens` left as it was; _BlockStep or None).
        save=False (inference): the residual GEMMs of a full block write the stream in place and nothing is kept.  save=True: the same launches with attention
        and the GELU GEMM in their training forms (the same values plus lse / the pre-activation), and the residual GEMMs write fresh tensors: the block's input
        and its middle (after attention) are LayerNorm inputs the backward needs, so they are kept rather than copied.
        drop (with save): ((p, key) or None) per dropout site — attention probabilities, GELU output, second Linear's output.  A site with a pair
        runs the dropout form of its launch (as many launches as without); None: the plain launch.  The row sites' mask rows are the token rows b N + i of
        the [B N, .] stream, so a CLS-only block (rows b) passes (row0, row_step) = (0, N) and its one query row is query 0: the full block's CLS rows.
        attention (a callable): receives (q, k, lse) of the block's attention, views as ops.mhsa_weights takes them.  An inference block then runs
        its attention as ops.mhsa_train without dropout (the same `out`, bit for bit, plus lse); nothing else changes."""
        B, N, D = tokens.shape
        att_d, act_d, out_d = drop if save else _NO_DROP
        rows = (0, N) if cls_only else (0, 1)
        act_d, out_d = (None if d is None else d + rows for d in (act_d, out_d))       # the row sites as the ops take them
        dt = self.compute_dtype
        X = tokens.view(B * N, D)
        a = blk.attn
        y = ops.layernorm256(X, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps, dt)
        if not cls_only:
            qkv, q = ops.token_gemm(y, a.in_proj_weight, a.in_proj_bias).view(B, N, 3 * D), None
            heads, nq = (qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:]), None
            resid, X1 = X, (torch.empty_like(X) if save else None)      # None: in place on the stream
        else:
            qkv = ops.token_gemm(y, a.in_proj_weight[D:], a.in_proj_bias[D:]).view(B, N, 2 * D)
            q = ops.token_gemm(y.view(B, N, D)[:, 0], a.in_proj_weight[:D], a.in_proj_bias[:D]).view(B, 1, D)
            heads, nq = (q, qkv[:, :, :D], qkv[:, :, D:]), 1
            resid, X1 = tokens[:, 0], torch.empty(B, D, dtype=torch.float32, device=tokens.device)
        if save or attention is not None:
            att, lse = ops.mhsa_train(*heads, nq, dropout=att_d)
        else:
            att, lse = ops.mhsa(*heads, nq), None
        if attention is not None:
            attention(heads[0], heads[1], lse)
        X1 = ops.token_gemm(att.view(-1, D), a.out_proj.weight, a.out_proj.bias, "residual", resid=resid, out=X1)
        y2 = ops.layernorm256(X1, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps, dt)
        if save:
            hid, pre = ops.token_gemm_gelu_train(y2, blk.mlp[0].weight, blk.mlp[0].bias, dropout=act_d)
        else:
            hid, pre = ops.token_gemm(y2, blk.mlp[0].weight, blk.mlp[0].bias, "gelu"), None
        X2 = ops.token_gemm(hid, blk.mlp[3].weight, blk.mlp[3].bias, "residual", resid=X1, out=torch.empty_like(X1) if save else None, dropout=out_d)
        if not save:
            return (X2 if cls_only else tokens), None                   # a full block wrote the stream itself
        return (X2 if cls_only else X2.view(B, N, D)), _BlockStep(X, y, qkv, q, att, lse, X1, y2, pre, hid, B, N, cls_only, drop)

    @torch.no_grad()
    def _walk(self, x, save=False, keep_stem=False, collect=None, attention=None, dropout=True, cls_only_last=None, stem_batch_stats=False):
        """The encoder's launches up to to_latent -> (cls features [B, 256] fp32, saved).  save=False: inference, saved = None.  save=True: every block in its
        saving form and saved = _Walk for _walk_backward; keep_stem (with save): the stem's layer outputs and folded weights travel along (the same launches).
        collect (a dict, for tests): receives `stem` (channels-last stem output), `cls_rows` (the CLS row after every block) and `tokens` (the residual stream
        after every block that ran for all tokens).
        After train_transformer(dropout=True) a save=True walk runs every block in its dropout form: one step of self.dropout_keys per walk, the
        rates read from the block's modules.  save=False never drops.  With device keys (use_device_dropout_keys) the step is one more launch
        and the sites' keys are views of its table: the same masks, and nothing here reads the counter.
        attention (a callable; attention_weights / attention_rollout): called as attention(i, q, k, lse) after block i's attention, see _block.
        None (the default): exactly the launches above.
        dropout=False (the *_vjp entries and an image that asks for its gradient through frozen parameters): a save=True walk that never drops and
        draws no step, whatever train_transformer() asked for.
        cls_only_last: whether the last block runs for its CLS row alone (the same CLS row, bit for bit); None (the default): self._cls_only_last_block.
        stem_batch_stats (with save and keep_stem; the training forward after train_stem(batch_stats=True)): the stem normalises with this
        batch's statistics and updates its running buffers, see _stem_cl.  False (every inference and probe entry): the fold, no buffer changes."""
        if stem_batch_stats and not (save and keep_stem):
            raise CvaeError("ViTVAEEncoder._walk: the batch-statistics stem is the training walk's (save=True, keep_stem=True)")
        self._check(x)
        cls_only_last = self._cls_only_last_block if cls_only_last is None else cls_only_last
        drop_step = None
        if save and self._dropout and dropout:
            self._check_dropout_dtype()
            if isinstance(self.dropout_keys, ops.DeviceDropoutKeys):
                drop_step = self.dropout_keys.advance()                 # this walk's [depth, 4] key table: one launch, the counter moves on the device
            else:
                drop_step, self.dropout_keys.step = self.dropout_keys.step, self.dropout_keys.step + 1
        kept = {} if keep_stem else None
        stem = self._stem_cl(x, kept, stem_batch_stats)
        tokens = ops.vit_tokens(stem, self.cls_token, self.pos_embedding[0])
        if collect is not None:
            collect["stem"], collect["cls_rows"], collect["tokens"] = stem, [], []
        steps = []
        for i, blk in enumerate(self.transformer):
            cls_only = cls_only_last and i == self.depth - 1
            out, step = self._block(blk, tokens, cls_only, save, _NO_DROP if drop_step is None else self._block_dropout(blk, i, drop_step),
                                    None if attention is None else (lambda q, k, lse, i=i: attention(i, q, k, lse)))
            steps.append(step)
            if cls_only:
                cls = out
            else:
                tokens, cls = out, out[:, 0]
            if collect is not None:
                collect["cls_rows"].append(cls.clone())
                if not cls_only:
                    collect["tokens"].append(tokens.clone())
        out = ops.layernorm256(cls, self.to_latent.weight, self.to_latent.bias, self.to_latent.eps, torch.float32)
        return out, (_Walk(steps, cls, stem.dtype, tokens.shape[0], tokens.shape[1], _StemKept(**kept) if keep_stem else None, stem) if save else None)

    def cls_features(self, x):
        """to_latent(transformer(tokens)[:, 0]) -> [B, 256] fp32: steps A-D of CausalViTVAE.forward (vessel_analysis/00_core/models.py:262-278)."""
        return self._walk(x)[0]

    def _cls_features(self, x, collect=None):
        """cls_features with _walk's collect dict (for tests)."""
        return self._walk(x, collect=collect)[0]

    @torch.no_grad()
    def encode(self, x):
        """(mu, log_var) = (fc_mu, fc_var)(cls_features(x)), as ViTVAE.encode (vit_backbone.py:158-179) in eval mode; both [B, latent_dim] fp32."""
        c = self.cls_features(x)
        return ops.Linear.apply(c, self.fc_mu.weight, self.fc_mu.bias, None), ops.Linear.apply(c, self.fc_var.weight, self.fc_var.bias, None)

    # ---- looking inside: attention weights and attention rollout --------------------------------------------------------
    @torch.no_grad()
    def attention_weights(self, x, query="cls", average_heads=True, blocks=None):
        """The attention probabilities of the transformer blocks for the images x, what the reference's nn.MultiheadAttention returns next to its output
        (vit_backbone.py:43 drops it): fp32 [B, n_blocks, Nq, N], or [B, n_blocks, 8, Nq, N] with average_heads=False; N = num_patches + 1, token 0 is CLS.
        query="cls": Nq = 1, the CLS row of every block — the model's own form, the last block running for its CLS row alone.  query="all": Nq = N, every
        row; for this call only the last block runs for all tokens (its CLS row is the same, bit for bit).  blocks: the block indices to return (default: all,
        in order).  Size: B n_blocks (8) Nq N floats — per head with query="all" at 961 tokens (768 x 1280) that is 29.6 MB per image and block, 3.7 MB
        averaged; the CLS form is 3.8 KB (30.8 KB per head).
        Eval mode, no gradient, never drops, either compute dtype; the walk is cls_features' with each block's attention in its lse-saving form (the same
        values), and one ops.mhsa_weights launch per selected block.  No state of the model changes."""
        if query not in ("cls", "all"):
            raise CvaeError(f"ViTVAEEncoder.attention_weights: query must be \"cls\" or \"all\", got {query!r}")
        idx = list(range(self.depth)) if blocks is None else [int(i) for i in blocks]
        if not idx or any(not 0 <= i < self.depth for i in idx):
            raise CvaeError(f"ViTVAEEncoder.attention_weights: blocks must name at least one of the {self.depth} blocks (0 .. {self.depth - 1}), got {blocks!r}")
        found = {}

        def probe(i, q, k, lse):
            if i in idx:
                nq = k.shape[1] if query == "all" else 1
                found[i] = ops.mhsa_weights(q, k, lse if lse.shape[2] == nq else lse[:, :, :nq].contiguous(), nq, average_heads)

        self._walk(x, attention=probe, cls_only_last=False if query == "all" else None)
        return torch.stack([found[i] for i in idx], dim=1)

    @torch.no_grad()
    def attention_rollout(self, x, residual=0.5, as_grid=True):
        """Attention rollout (Abnar & Zuidema 2020) from the CLS token: the CLS row of prod_l (residual I + (1 - residual) Abar_l), the last block leftmost,
        Abar_l = block l's head-averaged attention matrix.  Computed as a row vector: r = e_cls, then one ops.mhsa_rollout_step per block from the last to the
        first; no N x N matrix is formed.  as_grid=True: the patch columns as fp32 [B, grid_h, grid_w] (the CLS column dropped, nothing renormalised: a map sums to
        1 minus its CLS entry); False: the whole row [B, N], which sums to 1.  residual in [0, 1]; 1 gives e_cls.
        Eval mode, no gradient, never drops, either compute dtype; the walk is cls_features' with each block's attention in its lse-saving form.  No state of
        the model changes."""
        residual = float(residual)
        if not 0.0 <= residual <= 1.0:
            raise CvaeError(f"ViTVAEEncoder.attention_rollout: 0 <= residual <= 1 expected, got {residual}")
        kept = []
        self._walk(x, attention=lambda i, q, k, lse: kept.append((q, k, lse)))
        B, N = x.shape[0], self.num_patches + 1
        r = torch.zeros(B, N, dtype=torch.float32, device=x.device)
        r[:, 0] = 1.0
        for q, k, lse in reversed(kept):
            r = ops.mhsa_rollout_step(q, k, lse, r, lse.shape[2], residual)
        return r[:, 1:].reshape(B, self.grid_h, self.grid_w) if as_grid else r

    # ---- training the conv stem (eval mode: BatchNorm2d on its running statistics) -------------------------------------
    _stem_grads = False             # train_stem(): cls_features_with_grad / encode_with_grad accumulate the stem's gradients
    _stem_batch_stats = False       # train_stem(batch_stats=True): their training forward normalises the stem with batch statistics

    def _stem_named(self):
        """(name, parameter) of the 20 stem tensors (conv weight and bias, BatchNorm2d weight and bias per layer) in named_parameters order."""
        return [(f"stem.{k}", p) for k, p in self.stem.named_parameters()]

    def freeze_stem(self):
        """requires_grad_(False) on everything train_stem() switched on: the stem is a frozen feature extractor again and its activations are not kept."""
        self.stem.requires_grad_(False)
        self._stem_grads = False
        self._stem_batch_stats = False
        return self

    def train_stem(self, batch_stats=False):
        """The counterpart of freeze_stem(): requires_grad_(True) on the stem's 20 tensors, and cls_features_with_grad / encode_with_grad from now on accumulate
        their `.grad`.  Returns those parameters in named_parameters order.  The model stays in EVAL mode.  batch_stats=False (default):
        BatchNorm2d normalises with its running statistics, which are not updated; its weight and bias learn, and so do the conv weights and biases, through
        the fold.  batch_stats=True: the training forward normalises every stem layer with the statistics of its batch and updates running_mean,
        running_var and num_batches_tracked, as the reference's vae.train() does — asked for by keyword, as dropout is, not with the module's mode (the module
        and its BatchNorm2d children stay in eval mode; cls_features, encode and every other inference or probe entry keep the fold on the running statistics
        and change no buffer).  freeze_stem() clears it.  Independent of train_transformer(): alone it gives stem gradients only — at
        the cost of the whole backward all the same: the gradient reaches the stem through the transformer, and the one backward chain computes the
        transformer's weight gradients on its way and drops them."""
        if self.training:
            raise RuntimeError("ViTVAEEncoder.train_stem: put the model in eval mode first (model.eval()): the stem trains on eval-mode BatchNorm2d "
                               "(running statistics), and batch statistics are asked for with batch_stats=True, not with the module's mode")
        self.stem.requires_grad_(True)
        self._stem_grads = True
        self._stem_batch_stats = bool(batch_stats)
        return [p for _k, p in self._stem_named()]

    @torch.no_grad()
    def _stem_backward(self, kept, g, collect=None, params=True, image=None):
        """{state_dict name: gradient} of the 20 stem tensors from g = the gradient of the LAST layer's pre-activation [B, n, 256] (vit_tokens_bwd with the stem
        output as its gate), compute dtype.  Per layer, last to first: the folded k4 weight's and bias's gradient from (g_j, the layer's input) at once, then
        g_{j-1} = conv_down_bwd_data(g_j) with leaky001' of the layer's input in the epilogue: no activation-backward launch.  Then ONE launch back through the
        fold.  collect: receives `stem_g` = [g_0 .. g_4].
        image (a dict): the result also holds `dx`, the gradient of the image, fp32 [B, 1, H, W]: the last hop is ops.conv_down_image_bwd_data on g_0
        and the first folded weight, with the dict as its keyword arguments (alpha, out, accumulate; {}: the plain form).  params=False is the data-only form: no _conv_wgrad launch and no fold_bn_conv_bwd, the data launches — hence every g_j and dx,
        bit for bit — are those of the full form.
        A walk that kept batch statistics (kept.pre): the same loop; g is the gradient of the last ACTIVATION a_4 (no gate on the token launch), and
        per layer ops.bn2d_bwd (cvae_bn2d_bwd on (y_j, g, a_j, gamma, mean, rstd)) turns it into g_j, the gradient of the raw conv output, plus dgamma and dbeta
        (with params=False its two sums are still part of g_j); conv_down_bwd_data runs on the raw weight with no gate.  _conv_wgrad then gives the raw k4
        weight's gradient, whose k3 part (the inverse of the zero-embedding) is the 3 x 3 weight's, and the conv bias's — zero in exact arithmetic (the mean is
        subtracted), computed and returned all the same, as autograd does.  No fold_bn_conv_bwd launch."""
        ys, k4, dt = kept.ys, kept.k4, self.compute_dtype
        batch, table = kept.pre is not None, self._stem_fold_table()
        g = g.view(ys[-1].shape)
        folded, norms, gs = [None] * len(ys), [None] * len(ys), [None] * len(ys)
        for j in reversed(range(len(ys))):
            if batch:
                g, *norms[j] = ops.bn2d_bwd(kept.pre[j], g.contiguous(), ys[j], table[j][3].weight, kept.mean[j], kept.rstd[j], "leaky001")
            gs[j] = g
            if params:
                folded[j] = ops._conv_wgrad(g, ys[j - 1] if j else kept.x, 2, k4[j].shape, want_sbias=True)
            if j:
                g = ops.conv_down_bwd_data(g, ops.pack_weight(k4[j], 2, True, dt), *((None, None) if batch else (ys[j - 1], "leaky001")))
        if collect is not None:
            collect["stem_g"] = gs
        grads = {"dx": ops.conv_down_image_bwd_data(g, k4[0], **image)} if image is not None else {}
        if params:
            if batch:
                quads = [(dk4[:, :, :3, :3].contiguous(), dbias, *norms[j]) for j, (dk4, dbias) in enumerate(folded)]
            else:
                quads = ops.fold_bn_conv_bwd([entry + tuple(folded[j]) for j, entry in enumerate(table)])
            grads.update(zip((k for k, _p in self._stem_named()), (d for quad in quads for d in quad)))      # four per layer, in named_parameters order
        return grads

    # ---- training the transformer (eval mode) -----------------------------------------------------------------------------
    _transformer_grads = False      # train_transformer(): cls_features_with_grad / encode_with_grad accumulate the transformer's gradients
    _TRANSFORMER_ROOTS = ("pos_embedding", "cls_token", "transformer", "to_latent", "fc_mu", "fc_var")

    def _transformer_named(self, heads=True):
        """(name, parameter) of everything train_transformer() trains, in named_parameters order; heads=False: without fc_mu / fc_var (what the one
        autograd.Function over the transformer takes: the two output layers are ops.Linear nodes of their own)."""
        roots = self._TRANSFORMER_ROOTS if heads else self._TRANSFORMER_ROOTS[:4]
        return [(k, p) for k, p in self.named_parameters() if k.split(".")[0] in roots]

    _dropout = False                # train_transformer(dropout=True): the training forward drops at the blocks' three sites

    def _check_dropout_dtype(self):
        if self.compute_dtype != torch.float32:
            raise CvaeError("ViTVAEEncoder: dropout is implemented for the float32 compute dtype only (the dropout kernels take no bfloat16 operands yet): "
                            "set_compute_dtype(torch.float32), or train_transformer(dropout=False)")

    def use_device_dropout_keys(self, on=True):
        """Swap self.dropout_keys between ops.DropoutKeys (host step counter; the default) and ops.DeviceDropoutKeys (the counter on the parameters' device,
        advanced by a launch: DESIGN §19), keeping the seed and the step, so the masks of the steps to come are the same either way.  Switching to host
        keys reads the counter back (a sync).  A model on the CPU has no device to keep the counter on: CvaeError, and the host keys stay."""
        keys, dev = self.dropout_keys, self.cls_token.device
        if on and not isinstance(keys, ops.DeviceDropoutKeys):
            if dev.type != "cuda":
                raise CvaeError(f"ViTVAEEncoder.use_device_dropout_keys: the model is on {dev}; device keys live on the GPU (there is no CPU fallback: move the "
                                "model to 'cuda' first)")
            self.dropout_keys = ops.DeviceDropoutKeys(self.depth, dev, seed=keys.seed, step=keys.step)
        elif not on and isinstance(keys, ops.DeviceDropoutKeys):
            self.dropout_keys = ops.DropoutKeys().load_state(keys.state())
        return self

    def _block_dropout(self, blk, i, step):
        """((p, key) or None) for block i's three sites at this step: the rates are the modules' (attn.dropout, mlp[2].p, mlp[4].p); a rate of 0 is None.
        step: the step number (host keys: key is an int) or the table of DeviceDropoutKeys.advance() (key is a one-element view of it)."""
        K = ops.DropoutKeys
        sites = ((blk.attn.dropout, K.ATTN), (blk.mlp[2].p, K.MLP_ACT), (blk.mlp[4].p, K.MLP_OUT))
        return tuple((float(p), self.dropout_keys.key(step, i, site)) if p > 0 else None for p, site in sites)

    def freeze_transformer(self):
        """requires_grad_(False) on everything train_transformer() switched on, and dropout off; cls_features_with_grad then equals cls_features and saves
        nothing."""
        for _k, p in self._transformer_named():
            p.requires_grad_(False)
        self._transformer_grads = False
        self._dropout = False
        return self

    def train_transformer(self, heads=True, dropout=False):
        """The counterpart of freeze_transformer(): requires_grad_(True) on transformer.*, pos_embedding, cls_token, to_latent.*, fc_mu.* and fc_var.*
        (heads=False: without fc_mu / fc_var, for a consumer of the cls features that never reaches them; they are frozen), and
        cls_features_with_grad / encode_with_grad from now on accumulate their `.grad`.  Returns those parameters in named_parameters order.  The model stays in
        EVAL mode and, unless train_stem() was called, the conv stem stays a frozen feature extractor: a stem parameter that asks for a gradient is then an error
        here, not a gradient that silently stays None.
        dropout=False (default): no dropout — next to BatchNorm2d's running statistics the difference from the reference's vae.train().  dropout=True (float32
        compute dtype only, else CvaeError): every training forward (cls_features_with_grad / encode_with_grad with a live graph) drops as the reference's
        ViTBlock does under train(): the attention probabilities, the GELU output and the second Linear's output, at the rates of blk.attn.dropout, blk.mlp[2].p
        and blk.mlp[4].p, with Philox masks keyed by self.dropout_keys (one step per forward) — not torch's RNG stream.  The module itself stays
        in eval mode; cls_features, encode and every other inference entry never drop."""
        if self.training:
            raise RuntimeError("ViTVAEEncoder.train_transformer: put the model in eval mode first (model.eval()): the transformer trains on an eval-mode "
                               "stem, and dropout is asked for with dropout=True, not with the module's mode")
        live = [k for k, p in self._stem_named() if p.requires_grad]
        if live and not self._stem_grads:
            raise RuntimeError(f"ViTVAEEncoder.train_transformer: the stem is a frozen feature extractor, but these parameters ask for a gradient: {live} "
                               "(model.stem.requires_grad_(False), or model.train_stem() for their gradients)")
        if dropout:
            self._check_dropout_dtype()
        self.freeze_transformer()
        for _k, p in self._transformer_named(heads):
            p.requires_grad_(True)
        self._transformer_grads = True
        self._dropout = bool(dropout)
        return [p for _k, p in self._transformer_named(heads)]

    def cls_features_with_grad(self, x, collect=None):
        """cls_features(x) (the same launches up to two extra outputs, the same bits) as a differentiable function of the transformer's and the stem's
        parameters: ONE autograd.Function over stem, tokens, blocks and to_latent whose backward accumulates `.grad` on pos_embedding, cls_token, transformer.* and
        to_latent.* (after train_transformer()) and on stem.* (after train_stem(): the five layer outputs are kept; otherwise nothing of the stem is).
        An image that asks (x.requires_grad) is on the graph too and backward fills x.grad, fp32 [B, 1, H, W]: with frozen parameters through the
        data-only backward (no weight-gradient launch; never drops), with live ones through the full backward plus the one image launch.  The forward values are
        cls_features(x.detach())'s, bit for bit — except after train_stem(batch_stats=True): with a live stem the forward then normalises the stem
        with this batch's statistics (and moves the running buffers), so it no longer equals cls_features, which keeps the running statistics.  When autograd
        is off or neither a parameter nor x asks, this is cls_features and nothing is saved; a parameter
        that asks without its train_*() call is an error, not a gradient that silently stays None.
        collect (a dict, for tests): the forward leaves `stem`, the stem's channels-last output as this walk computed it; the backward leaves `dstem`, the gradient of the stem's output [B, n, 256] in its dtype, and with a live stem `stem_g`, the
        gradients of the five pre-activations (`dstem` then costs one more token launch: the stem's backward starts from its gated form)."""
        named, stem = self._transformer_named(heads=False), self._stem_named()
        live_t, live_s = any(p.requires_grad for _k, p in named), any(p.requires_grad for _k, p in stem)
        if not (torch.is_grad_enabled() and (live_t or live_s or x.requires_grad)):
            return self.cls_features(x)
        if live_t and not self._transformer_grads:
            raise CvaeError("ViTVAEEncoder.cls_features_with_grad: transformer parameters ask for a gradient but train_transformer() was not called "
                            "(or call freeze_transformer())")
        if live_s and not self._stem_grads:
            raise CvaeError("ViTVAEEncoder.cls_features_with_grad: stem parameters ask for a gradient but train_stem() was not called (or call freeze_stem())")
        if live_s:
            named = named + stem
        if not (live_t or live_s):
            named = []                                                   # only the image asks: no parameter is an input of the node
        return _ClsFeaturesWithGrad.apply(x, self, collect, tuple(k for k, _p in named), *[p for _k, p in named])

    def encode_with_grad(self, x, collect=None):
        """encode(x) with gradients: (mu, log_var) from cls_features_with_grad through the differentiable ops.Linear (fc_mu, fc_var)."""
        c = self.cls_features_with_grad(x, collect)
        return ops.Linear.apply(c, self.fc_mu.weight, self.fc_mu.bias, None), ops.Linear.apply(c, self.fc_var.weight, self.fc_var.bias, None)

    # ---- the gradient with respect to the image: vjp entries, saliency, Grad-CAM ------------------------------------------
    def _cotangent(self, what, name, g, B, width, device):
        if g is None:
            return None
        if not torch.is_tensor(g) or tuple(g.shape) != (B, width) or g.dtype != torch.float32:
            raise CvaeError(f"ViTVAEEncoder.{what}: {name} must be a float32 [{B}, {width}] cotangent, got "
                            f"{(tuple(g.shape), g.dtype) if torch.is_tensor(g) else type(g).__name__}")
        require_gpu(g)
        return g.detach().contiguous()

    def _heads_vjp(self, c, g_mu, g_log_var):
        """The cotangent of the cls features c from those of mu and log_var: ops.Linear's own backward (its data launch alone: the weights are handed over
        detached) on a two-node graph that lives inside this call, the two results added — what autograd does after encode_with_grad, hence the same bits."""
        with torch.enable_grad():
            c = c.detach().requires_grad_(True)
            pairs = [(ops.Linear.apply(c, fc.weight.detach(), fc.bias.detach(), None), g) for fc, g in ((self.fc_mu, g_mu), (self.fc_var, g_log_var)) if g is not None]
            return torch.autograd.grad([y for y, _g in pairs], [c], [g for _y, g in pairs])[0]

    @torch.no_grad()
    def _data_backward(self, x, cotangent, image=None, stem=True, attention_grad=None, cls_only_last=None):
        """The eval-mode saving walk (never drops, draws no dropout step) and the data-only backward -> (the walk's _Walk, {`dstem`, and with stem `dx`}).
        cotangent: a callable, cls features [B, 256] -> their fp32 cotangent.  stem=False keeps nothing of the stem and stops at `dstem` (Grad-CAM).
        attention_grad: passed to _walk_backward; cls_only_last: passed to _walk (both DESIGN §22; the defaults issue exactly the launches above)."""
        out, saved = self._walk(x.detach(), save=True, keep_stem=stem, dropout=False, cls_only_last=cls_only_last)
        return saved, self._walk_backward(saved, cotangent(out).contiguous(), params=False, image=({} if image is None else image) if stem else None,
                                          attention_grad=attention_grad)

    @torch.no_grad()
    def cls_features_vjp(self, x, g, _image=None):
        """dx = (d cls_features(x) / d x)^T g, fp32 [B, 1, H, W], for a float32 [B, 256] cotangent g: the explicit form of what backward leaves in x.grad after
        cls_features_with_grad(x.requires_grad_()) — the same launches, the same bits — and the counterpart of ViTVAE.decode_vjp: no autograd graph, capturable.
        Eval mode, either compute dtype; never drops and draws no dropout step, also after train_transformer(dropout=True); works on a fully frozen model and
        issues no weight-gradient launch (the data-only backward); no parameter's .grad and no state of the model changes."""
        self._check(x)
        g = self._cotangent("cls_features_vjp", "g", g, x.shape[0], self.embed_dim, x.device)
        if g is None:
            raise CvaeError("ViTVAEEncoder.cls_features_vjp: a float32 [B, 256] cotangent is needed, got None")
        if x.shape[0] == 0:
            return torch.zeros_like(x)
        return self._data_backward(x, lambda _c: g, _image)[1]["dx"]

    @torch.no_grad()
    def encode_vjp(self, x, g_mu=None, g_log_var=None, _image=None):
        """dx = (d mu / d x)^T g_mu + (d log_var / d x)^T g_log_var, fp32 [B, 1, H, W]; either cotangent (float32 [B, latent_dim]) may be None, not both.
        cls_features_vjp behind the two output layers' data gradients: what backward leaves in x.grad after encode_with_grad(x.requires_grad_()), bit for bit."""
        self._check(x)
        g_mu = self._cotangent("encode_vjp", "g_mu", g_mu, x.shape[0], self.latent_dim, x.device)
        g_log_var = self._cotangent("encode_vjp", "g_log_var", g_log_var, x.shape[0], self.latent_dim, x.device)
        if g_mu is None and g_log_var is None:
            raise CvaeError("ViTVAEEncoder.encode_vjp: at least one of g_mu and g_log_var is needed")
        if x.shape[0] == 0:
            return torch.zeros_like(x)
        return self._data_backward(x, lambda c: self._heads_vjp(c, g_mu, g_log_var), _image)[1]["dx"]

    def _target_cotangent(self, what, B, target, index, device):
        """(target, the fp32 [B, width] cotangent that selects `index` of it): all ones for None, else ones in the named columns (their sum)."""
        if target not in ("mu", "log_var", "cls"):
            raise CvaeError(f"ViTVAEEncoder.{what}: target must be \"mu\", \"log_var\" or \"cls\", got {target!r}")
        width = self.embed_dim if target == "cls" else self.latent_dim
        if index is None:
            return torch.ones(B, width, dtype=torch.float32, device=device)
        idx = [index] if isinstance(index, (int, np.integer)) and not isinstance(index, bool) else list(index) if isinstance(index, (list, tuple)) else None
        if not idx or any(not isinstance(i, (int, np.integer)) or isinstance(i, bool) or not 0 <= i < width for i in idx) or len(set(idx)) != len(idx):
            raise CvaeError(f"ViTVAEEncoder.{what}: index must be None, an int or a list of distinct ints in 0 .. {width - 1} (target {target!r}), got {index!r}")
        g = torch.zeros(B, width, dtype=torch.float32, device=device)
        g[:, [int(i) for i in idx]] = 1.0
        return g

    def _target_vjp(self, x, target, g, image=None):
        if target == "cls":
            return self.cls_features_vjp(x, g, image)
        return self.encode_vjp(x, g, None, image) if target == "mu" else self.encode_vjp(x, None, g, image)

    @torch.no_grad()
    def saliency(self, x, target="mu", index=None, method="gradient", steps=16, baseline=None, absolute=True):
        """Which pixels move a latent coordinate: fp32 [B, H, W], the gradient with respect to the image of sum_{k in index} target[:, k]; target "mu",
        "log_var" or "cls" (the 256 cls features), index None (all coordinates), an int or a list of ints.
        method="gradient": one encode_vjp / cls_features_vjp with the matching one-hot / all-ones cotangent.
        method="integrated": integrated gradients by the midpoint rule, (x - baseline) * (1 / steps) sum_{k = 1..steps} grad(baseline + ((k - 1/2) / steps)
        (x - baseline)); baseline defaults to zeros.  One walk and one data-only backward per step, NOT batched: the steps meet in the image kernel's
        accumulate epilogue (alpha = 1 / steps; the first step writes, the others add), so no [steps, B, H, W] tensor and no zero fill exists, and memory is
        that of one vjp.  x == baseline gives exactly zero.
        absolute=True takes |.| at the end.  Eval mode, no gradient, never drops, either compute dtype; no state of the model changes."""
        self._check(x)
        if method not in ("gradient", "integrated"):
            raise CvaeError(f"ViTVAEEncoder.saliency: method must be \"gradient\" or \"integrated\", got {method!r}")
        g = self._target_cotangent("saliency", x.shape[0], target, index, x.device)
        x = x.detach()
        if method == "gradient":
            if baseline is not None:
                raise CvaeError("ViTVAEEncoder.saliency: a baseline belongs to method=\"integrated\"")
            out = self._target_vjp(x, target, g)
        else:
            if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
                raise CvaeError(f"ViTVAEEncoder.saliency: steps must be an int >= 1, got {steps!r}")
            if baseline is None:
                baseline = torch.zeros_like(x)
            elif not torch.is_tensor(baseline) or tuple(baseline.shape) != tuple(x.shape) or baseline.dtype != torch.float32 or baseline.device != x.device:
                raise CvaeError(f"ViTVAEEncoder.saliency: baseline must be a float32 {tuple(x.shape)} tensor on {x.device}, got "
                                f"{(tuple(baseline.shape), baseline.dtype, baseline.device) if torch.is_tensor(baseline) else type(baseline).__name__}")
            if x.shape[0] == 0:
                return torch.zeros_like(x[:, 0])
            diff = x - baseline.detach()
            out = torch.empty_like(x)
            for k in range(int(steps)):
                self._target_vjp(torch.add(baseline, diff, alpha=(k + 0.5) / int(steps)), target, g,
                                 {"alpha": 1.0 / int(steps), "out": out, "accumulate": k > 0})
            out = out * diff
        out = out[:, 0]
        return out.abs() if absolute else out

    @torch.no_grad()
    def gradcam(self, x, target="mu", index=None, normalize=True):
        """Grad-CAM on the stem's output, the last conv activation: fp32 [B, grid_h, grid_w], one value per patch.  The data-only backward of
        sum_{k in index} target[:, k] (target and index as in saliency) down to `dstem` — nothing of the stem is kept or walked back — then ops.gradcam on the
        stem output and `dstem`: the channel weights are dstem's means over the patches, the map is relu of the weighted channel sum, and with normalize it
        is scaled to [0, 1] per image as the reference's GradCAM does.  Eval mode, no gradient, never drops, either compute dtype; no state changes."""
        self._check(x)
        g = self._target_cotangent("gradcam", x.shape[0], target, index, x.device)
        B = x.shape[0]
        if B == 0:
            return torch.zeros(0, self.grid_h, self.grid_w, dtype=torch.float32, device=x.device)
        saved, grads = self._data_backward(x, self._head_cotangent(target, g), stem=False)
        return ops.gradcam(saved.stem_out.view(B, self.num_patches, self.embed_dim), grads["dstem"], normalize).view(B, self.grid_h, self.grid_w)

    # ---- looking inside, with a target: attention gradients and gradient-weighted relevance ------------------------------
    def _head_cotangent(self, target, g):
        """_data_backward's `cotangent` for the selector g of _target_cotangent."""
        if target == "cls":
            return lambda _c: g
        return lambda c: self._heads_vjp(c, g if target == "mu" else None, g if target == "log_var" else None)

    @torch.no_grad()
    def attention_gradients(self, x, target="mu", index=None, query="cls", blocks=None):
        """The gradient of sum_{k in index} target[:, k] (target and index as in saliency) with respect to the attention probabilities of the transformer
        blocks, taken as a free variable — what retain_grad() on a hook at the softmax output of the reference's blocks leaves: fp32 [B, n_blocks, 8, Nq, N],
        gA[b, l, h, i, j] = sum_d datt_l[b, i, 32 h + d] v_l[b, j, 32 h + d].  query and blocks as in attention_weights; with query="all" the last block's rows
        >= 1 are zeros, exactly: only its CLS output reaches any target.  One saving walk, the data-only backward down to `dstem` (nothing of the stem is
        walked back, no weight-gradient launch) and one ops.mhsa_weight_grads launch per selected block.
        Eval mode, no gradient, never drops, either compute dtype; no state of the model changes."""
        g = self._target_cotangent("attention_gradients", x.shape[0], target, index, x.device)
        if query not in ("cls", "all"):
            raise CvaeError(f"ViTVAEEncoder.attention_gradients: query must be \"cls\" or \"all\", got {query!r}")
        idx = list(range(self.depth)) if blocks is None else [int(i) for i in blocks]
        if not idx or any(not 0 <= i < self.depth for i in idx):
            raise CvaeError(f"ViTVAEEncoder.attention_gradients: blocks must name at least one of the {self.depth} blocks (0 .. {self.depth - 1}), got {blocks!r}")
        self._check(x)
        B, N = x.shape[0], self.num_patches + 1
        Nq = N if query == "all" else 1
        if B == 0:
            return torch.zeros(0, len(idx), 8, Nq, N, dtype=torch.float32, device=x.device)
        found = {}

        def probe(i, q, k, v, lse, datt, nq):
            if i not in idx:
                return
            if nq == Nq:
                found[i] = ops.mhsa_weight_grads(datt, v, nq)
            elif nq == 1:                                               # the last block under query="all": only its CLS row exists
                found[i] = torch.zeros(B, 8, Nq, N, dtype=torch.float32, device=x.device)
                found[i][:, :, :1] = ops.mhsa_weight_grads(datt, v, 1)
            else:                                                       # the CLS row of a block that ran for all tokens
                found[i] = ops.mhsa_weight_grads(datt[:, :1].contiguous(), v, 1)

        self._data_backward(x, self._head_cotangent(target, g), stem=False, attention_grad=probe, cls_only_last=False if query == "all" else None)
        return torch.stack([found[i] for i in idx], dim=1)

    @torch.no_grad()
    def attention_relevance(self, x, target="mu", index=None, as_grid=True):
        """Gradient-weighted attention relevance (Chefer, Gur & Wolf 2021, the self-attention rule) of sum_{k in index} target[:, k] from the CLS token:
        R = I, then R <- R + Abar_l R over the blocks, Abar_l = 1/8 sum_h max(0, gA_l P_l) with gA as in attention_gradients and P as in attention_weights;
        the map is R's CLS row.  Computed as a row vector, r = e_cls, then one ops.mhsa_relevance_step per block from the last to the first, inside the
        backward that forms each block's datt; no N x N matrix is formed.  Unlike attention_rollout the map depends on the target and on the sign of a head's
        contribution.  as_grid=True: the patch columns as fp32 [B, grid_h, grid_w] (the CLS column dropped, nothing renormalised); False: the whole row [B, N].
        One saving walk and the data-only backward down to `dstem`.  Eval mode, no gradient, never drops, either compute dtype; no state changes."""
        g = self._target_cotangent("attention_relevance", x.shape[0], target, index, x.device)
        self._check(x)
        B, N = x.shape[0], self.num_patches + 1
        r = torch.zeros(B, N, dtype=torch.float32, device=x.device)
        if B:
            r[:, 0] = 1.0
            row = [r]

            def step(_i, q, k, v, lse, datt, nq):
                row[0] = ops.mhsa_relevance_step(q, k, v, lse, datt, row[0], nq)

            self._data_backward(x, self._head_cotangent(target, g), stem=False, attention_grad=step)
            r = row[0]
        return r[:, 1:].reshape(B, self.grid_h, self.grid_w) if as_grid else r

    def _cls_rows_step(self, s):
        """The record a CLS-only block would have kept, cut from a full block's _BlockStep (the last block of a walk with _cls_only_last_block False): k / v
        as the column panels of the packed qkv, the CLS query row, and the CLS rows b N of att, lse, X1, y2, pre and hid — views with the stream's row stride,
        but for att and lse, which the attention backward reads as dense [B, 1, .] tensors (two B-row copies).  Row 0 of a full block equals the CLS-only
        block's row bit for bit, so _block_backward computes from it what it computes after a CLS-only forward."""
        B, N, D = s.B, s.N, self.embed_dim
        row0 = lambda t: t.view(B, N, -1)[:, 0]
        return s._replace(qkv=s.qkv[:, :, D:], q=s.qkv[:, :1, :D], att=s.att[:, :1].contiguous(), lse=s.lse[:, :, :1].contiguous(), X1=row0(s.X1), y2=row0(s.y2),
                          pre=row0(s.pre), hid=row0(s.hid), cls_only=True)

    def _block_backward(self, blk, name, s, G, grads, attention_grad=None):
        """One block's backward from its _BlockStep s: G = the fp32 gradient of the block's output ([B N, 256], or [B, 256] from a CLS-only block), updated in
        place where it can be; returns the gradient of the block's input [B N, 256] and leaves the parameter gradients in `grads` under their state_dict names.
        grads None is the data-only form: no token_gemm_wgrad launch; LayerNorm's parameter sums leave the launch that computes its dx and are
        dropped.  The data launches, and so the returned gradient's bits, are the same in both forms.
        attention_grad (a callable): receives (q, k, v, lse, datt, n_query_rows) once datt, the cotangent of the attention output, is formed — the
        views ops.mhsa_weight_grads / mhsa_relevance_step take.  None (the default): exactly the launches above."""
        B, N, D, dt, a = s.B, s.N, self.embed_dim, self.compute_dtype, blk.attn
        wgrad, grads = grads is not None, ({} if grads is None else grads)
        att_d, act_d, out_d = s.drop                                    # the forward's dropout sites: the masks are recomputed from (p, key), DESIGN §18
        rows = (0, N) if s.cls_only else (0, 1)
        Gm = G if out_d is None else ops.dropout_rows(G, out_d + rows)  # the MLP branch's cotangent; the skip carries G itself
        dpre = ops.token_gemm_bwd_data(Gm, blk.mlp[3].weight, dt, gate_pre=s.pre, dropout=None if act_d is None else act_d + rows)
        if wgrad:
            grads[name + "mlp.3.weight"], grads[name + "mlp.3.bias"] = ops.token_gemm_wgrad(Gm, s.hid)
        dy2 = ops.token_gemm_bwd_data(dpre, blk.mlp[0].weight, dt)
        if wgrad:
            grads[name + "mlp.0.weight"], grads[name + "mlp.0.bias"] = ops.token_gemm_wgrad(dpre, s.y2)
        _dx, grads[name + "norm2.weight"], grads[name + "norm2.bias"] = ops.layernorm256_bwd(dy2, s.X1, blk.norm2.weight, blk.norm2.eps, dx=G, accumulate=True)
        datt = ops.token_gemm_bwd_data(G, a.out_proj.weight, dt)
        if wgrad:
            grads[name + "attn.out_proj.weight"], grads[name + "attn.out_proj.bias"] = ops.token_gemm_wgrad(G, s.att.view(-1, D))
        qkv, y = s.qkv, s.y
        if attention_grad is not None:
            if s.cls_only:
                attention_grad(s.q, qkv[:, :, :D], qkv[:, :, D:], s.lse, datt.view(B, 1, D), 1)
            else:
                attention_grad(qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], s.lse, datt.view(B, N, D), N)
        dqkv = torch.empty(qkv.shape, dtype=qkv.dtype, device=qkv.device)       # dense, also where qkv is a column panel (_cls_rows_step)
        if not s.cls_only:
            ops.mhsa_bwd(qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], s.att, s.lse, datt.view(B, N, D), dqkv[:, :, :D], dqkv[:, :, D:2 * D], dqkv[:, :, 2 * D:],
                         dropout=att_d)
            dy = ops.token_gemm_bwd_data(dqkv.view(B * N, 3 * D), a.in_proj_weight, dt)
            if wgrad:
                grads[name + "attn.in_proj_weight"], grads[name + "attn.in_proj_bias"] = ops.token_gemm_wgrad(dqkv.view(B * N, 3 * D), y)
            _dx, grads[name + "norm1.weight"], grads[name + "norm1.bias"] = ops.layernorm256_bwd(dy, s.X, blk.norm1.weight, blk.norm1.eps, dx=G, accumulate=True)
            return G
        dq = torch.empty(s.q.shape, dtype=s.q.dtype, device=s.q.device)
        ops.mhsa_bwd(s.q, qkv[:, :, :D], qkv[:, :, D:], s.att, s.lse, datt.view(B, 1, D), dq, dqkv[:, :, :D], dqkv[:, :, D:], dropout=att_d)
        if wgrad:
            dW, db = torch.empty_like(a.in_proj_weight), torch.empty_like(a.in_proj_bias)
            ops.token_gemm_wgrad(dq.view(B, D), y.view(B, N, D)[:, 0], dW[:D], db[:D])
            ops.token_gemm_wgrad(dqkv.view(B * N, 2 * D), y, dW[D:], db[D:])
            grads[name + "attn.in_proj_weight"], grads[name + "attn.in_proj_bias"] = dW, db
        dy = ops.token_gemm_bwd_data(dqkv.view(B * N, 2 * D), a.in_proj_weight[D:], dt, out_dtype=torch.float32)
        ops.token_gemm_bwd_data(dq.view(B, D), a.in_proj_weight[:D], dt, resid=dy.view(B, N, D)[:, 0])       # the one q row joins the kv rows' gradient, in place
        Gin, grads[name + "norm1.weight"], grads[name + "norm1.bias"] = ops.layernorm256_bwd(dy, s.X, blk.norm1.weight, blk.norm1.eps)
        Gin.view(B, N, D)[:, 0].add_(G)                                 # the skip: only the CLS rows left this block
        return Gin

    @torch.no_grad()
    def _walk_backward(self, saved, g, collect=None, params=True, stem_params=None, image=None, attention_grad=None):
        """{state_dict name: gradient} of pos_embedding, cls_token, transformer.* and to_latent.*, plus `dstem`, from the cotangent g [B, 256] of the cls features;
        when the walk kept the stem's activations, of stem.* too (then `dstem` is there only with a collect dict, which also receives `stem_g`).
        DESIGN §21: params=False is the data-only form — every block in its data-only form, no parameter's gradient in the result, the same `dstem`.
        stem_params (default: whether the walk kept the stem) says the same for the stem's 20 tensors; image (a dict, needs a walk that kept the stem): the
        result also holds `dx`, see _stem_backward.
        attention_grad (a callable; attention_gradients / attention_relevance): called as attention_grad(i, q, k, v, lse, datt, n_query_rows) in
        block i's backward, from the last block to the first, see _block_backward.  None (the default): exactly the launches above."""
        steps, cls, stem_dtype, B, N, kept = saved[:6]
        D, grads = self.embed_dim, {}
        stem_params = bool(params) and ((kept is not None) if stem_params is None else bool(stem_params))
        # to_latent reads the CLS rows alone, so the last block's cotangent is its [B, 256] CLS rows whichever form its forward ran: the backward of a full
        # last block is the CLS-only block's, on the CLS rows of what it kept (_cls_rows_step) — the same launches, hence the same bits, in both forms
        G, grads["to_latent.weight"], grads["to_latent.bias"] = ops.layernorm256_bwd(g, cls, self.to_latent.weight, self.to_latent.eps)
        for i in reversed(range(self.depth)):
            s = steps[i] if (steps[i].cls_only or i < self.depth - 1) else self._cls_rows_step(steps[i])
            G = self._block_backward(self.transformer[i], f"transformer.{i}.", s, G, grads if params else None,
                                     None if attention_grad is None else (lambda *a, i=i: attention_grad(i, *a)))
        if kept is None or not (stem_params or image is not None):
            dpos, dcls, grads["dstem"] = ops.vit_tokens_bwd(G.view(B, N, D), stem_dtype)
        elif kept.pre is not None:                                      # batch statistics: the LeakyReLU derivative is cvae_bn2d_bwd's, so no gate
            dpos, dcls, grads["dstem"] = ops.vit_tokens_bwd(G.view(B, N, D), stem_dtype)
            grads.update(self._stem_backward(kept, grads["dstem"], collect, stem_params, image))
        else:                                                           # the stem's last activation is a LeakyReLU output: its derivative rides on the token launch
            if collect is not None:
                grads["dstem"] = ops.vit_tokens_bwd(G.view(B, N, D), stem_dtype)[2]
            dpos, dcls, g_last = ops.vit_tokens_bwd(G.view(B, N, D), stem_dtype, gate=kept.ys[-1].view(B, N - 1, D), gate_act="leaky001")
            grads.update(self._stem_backward(kept, g_last, collect, stem_params, image))
        grads["pos_embedding"], grads["cls_token"] = dpos.view(1, N, D), dcls.view(1, 1, D)
        return grads if params else {k: grads[k] for k in ("dstem", "dx") if k in grads}


class _ClsFeaturesWithGrad(torch.autograd.Function):
    """ViTVAEEncoder.cls_features_with_grad: the transformer's parameters (and, after train_stem(), the stem's behind them) are inputs, so autograd accumulates
    their gradients, zero_grad works and a parameter rewritten between forward and backward is an error.  An x that asks for its gradient gets it:
    the stem's gates travel along, the walk reads the detached image (the same launches as for an x that does not ask), and with no parameter among the
    inputs the backward is the data-only one."""

    @staticmethod
    def forward(ctx, x, model, collect, names, *params):
        stem_live, wants_x = any(k.startswith("stem.") for k in names), ctx.needs_input_grad[0]
        out, saved = model._walk(x.detach() if wants_x else x, save=True, keep_stem=stem_live or wants_x, dropout=bool(params),
                                 stem_batch_stats=stem_live and model._stem_batch_stats)
        if collect is not None:
            collect["stem"] = saved.stem_out
        ctx.model, ctx.saved, ctx.collect, ctx.names, ctx.stem_live = model, saved, collect, names, stem_live      # activations of this call: private to the node, freed with it
        ctx.save_for_backward(*params)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        params = ctx.saved_tensors                                     # raises if a parameter was modified in place since the forward
        if g is None:
            return (None,) * (4 + len(params))
        grads = ctx.model._walk_backward(ctx.saved, g.contiguous(), ctx.collect, params=bool(params), stem_params=ctx.stem_live,
                                         image={} if ctx.needs_input_grad[0] else None)
        if ctx.collect is not None:
            ctx.collect["dstem"] = grads["dstem"]
        return (grads.get("dx"), None, None, None) + tuple(grads[k].view(p.shape) if need else None for k, p, need in zip(ctx.names, params, ctx.needs_input_grad[4:]))


class _ResBlock(nn.Module):
    """Parameter holder with the reference ResBlock's child (vit_backbone.py:7-19): x + conv(x)."""

    def __init__(self, channels):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(channels, channels, 3, 1, 1), nn.BatchNorm2d(channels), nn.LeakyReLU(0.2, inplace=True),
                                  nn.Conv2d(channels, channels, 3, 1, 1), nn.BatchNorm2d(channels))


DECODER_CHANNELS = (128, 64, 32, 16, 16)     # outputs of the five transposed convs; a ResBlock follows each of the first three
# One decoder stage: kind "up" (wide transposed conv, cvae_conv_up), "sub" (narrow one, sub-pixel conv_s1) or "res" (ResBlock); layers = its (conv, bn)
# pairs; fold = their positions in the fold table; gates = its output is a LeakyReLU(0.01) output: the gate in the backward of whatever reads it.
_Stage = namedtuple("_Stage", "kind layers fold gates")
# What _decode_walk keeps of a stage for _decode_backward: gate_in (the stage's input when the stage before it gates, else None), inner (a ResBlock's inner
# activation), mats (the backward matrix of every GEMM layer, in layer order), k4 (an "up" stage's folded k4 weight), x (the stage's input, kept only when
# weight gradients are wanted: a ResBlock sum and the grid are no gates, so gate_in does not cover them).  The batch-statistics walk (train_decoder(batch_stats=
# True)) fills the rest: pre = the raw conv output of every layer of the stage, mean / rstd = each layer's batch statistics as cvae_bn2d_batch_bwd
# reads them, out = the stage's output activation; there k4 and mats come from the RAW weights and gate_in stays None (no data launch carries a gate).  pre is
# None in the eval-mode (folded) walk, which is how _decode_backward's one loop tells where ops.bn2d_batch_bwd stands and which ending to take.
_Step = namedtuple("_Step", "stage gate_in inner mats k4 x pre mean rstd out", defaults=(None, None, None, None))


class ViTVAE(ViTVAEEncoder):
    """The reference's ViTVAE for eval-mode inference: encode (ViTVAEEncoder), decode, reparameterize, forward, reconstruct."""

    def __init__(self, in_channels=1, latent_dim=128, img_size=(768, 1280), patch_size=32, embed_dim=256, depth=6, heads=8, mlp_dim=512):
        super().__init__(in_channels, latent_dim, img_size, patch_size, embed_dim, depth, heads, mlp_dim)
        self.decoder_input = nn.Linear(latent_dim, embed_dim * self.grid_h * self.grid_w)
        dec, cin = [], embed_dim
        for i, cout in enumerate(DECODER_CHANNELS):
            dec += [nn.ConvTranspose2d(cin, cout, kernel_size=3, stride=2, padding=1, output_padding=1), nn.BatchNorm2d(cout), nn.LeakyReLU()]
            if i < 3:
                dec.append(_ResBlock(cout))
            cin = cout
        dec.append(nn.Conv2d(cin, in_channels, kernel_size=3, padding=1))
        self.decoder = nn.Sequential(*dec)

    def _decoder_plan(self):
        """([_Stage] in execution order, the output conv).  A stage's `fold` holds the positions of its layers in the fold table: the one place they are counted."""
        mods, plan, i, n = list(self.decoder), [], 0, 0
        while i < len(mods) - 1:
            if isinstance(mods[i], _ResBlock):
                c = mods[i].conv
                kind, layers, step = "res", ((c[0], c[1]), (c[3], c[4])), 1
            else:
                kind, layers, step = "up" if mods[i].out_channels % 32 == 0 else "sub", ((mods[i], mods[i + 1]),), 3
            plan.append(_Stage(kind, layers, tuple(range(n, n + len(layers))), kind != "res"))
            i, n = i + step, n + len(layers)
        return plan, mods[-1]

    @staticmethod
    def _fold_table(plan, grad):
        """ops.fold_bn_conv's entries for the plan; grad: the _GRAD kinds (the same forward matrices, bit for bit, plus the backward ones from the same launch)."""
        kinds = {"up": ops.FOLD_CONVT_K3S2, "sub": ops.FOLD_CONVT_K3S2_SUBPIXEL_GRAD if grad else ops.FOLD_CONVT_K3S2_SUBPIXEL,
                 "res": ops.FOLD_CONV_K3S1_GRAD if grad else ops.FOLD_CONV_K3S1}
        return [(conv.weight, kinds[st.kind], conv.bias, bn) for st in plan for conv, bn in st.layers]

    def _check_latent(self, z, what="the decoder runs inference only"):
        if self.training:
            raise RuntimeError(f"ViTVAE: put the model in eval mode first (model.eval()): batch-statistics BatchNorm2d is not implemented, {what}")
        if z.dim() != 2 or z.shape[1] != self.latent_dim or z.dtype != torch.float32:
            raise CvaeError(f"ViTVAE.decode expects a float32 [B, {self.latent_dim}] batch, got {tuple(z.shape)} {z.dtype}")

    @torch.no_grad()
    def decode(self, z, collect=None):
        """ViTVAE.decode (vit_backbone.py:186-193) in eval mode: [B, latent_dim] fp32 -> [B, 1, H, W] fp32.  collect: as _decode_walk."""
        self._check_latent(z)
        require_gpu(z, self.decoder_input.weight)
        return self._decode_walk(z, False, collect)[0]

    @torch.no_grad()
    def _decode_walk(self, z, save, collect=None, keep_inputs=False, batch_stats=False):
        """The decoder's launches -> (image, saved).  save=False: the forward fold kinds, in bf16 one pack of the 8 GEMM matrices, saved = None.  save=True: the
        same launches with the fold's _GRAD kinds (one pack of 16: forward and backward matrices) and saved = ([_Step per stage], the output conv, its gate)
        for _decode_backward: DESIGN §13's set (the gates are the outputs of stages 0, 2, 4, 6 and 7; a ResBlock sum and the grid are no gates).
        keep_inputs (with save): every step also keeps its stage's input, what the weight gradients are multiplied with; the launches are the same.
        collect (a dict, for tests): receives `grid` (decoder_input's output, channels-last [B, gh, gw, 256]), `stages` (the channels-last activation after
        each of the 8 stages: 5 transposed convs, 3 ResBlocks, in execution order) and `res_inner` (the three ResBlock inner activations).
        batch_stats (with save and keep_inputs: _DecodeWithGrad's training walk after train_decoder(batch_stats=True)): no fold of statistics — the
        fold's launch with no BatchNorm gives the raw k4 weights and the raw forward / backward matrices; every conv runs with its own bias (it cancels in the
        normalised value, but running_mean must contain it) and no activation, and ops.bn2d_batch_fwd behind it normalises with THIS batch's statistics, applies
        the activation (a ResBlock's second layer: adds the block's input instead) and updates the layer's running statistics and counter in place."""
        dt = self.compute_dtype
        plan, out_conv = self._decoder_plan()
        if batch_stats and not (save and keep_inputs):
            raise CvaeError("ViTVAE._decode_walk: batch statistics belong to the training walk (save=True, keep_inputs=True): inference keeps the running statistics")
        table = self._fold_table(plan, save)
        if batch_stats:
            table = [(w, kind, b, None) for w, kind, b, _bn in table]
        folded = ops.fold_bn_conv(table)                               # one launch, on every call: parameters may have been rewritten
        gemm = [k for st in plan if st.kind != "up" for k in st.fold]
        fwd, bwd = [folded[k][0] for k in gemm], [folded[k][2] for k in gemm] if save else []
        if dt == torch.bfloat16:                                       # one launch for all of them
            packed = ops.conv_s1_pack_weights(fwd + bwd)
            fwd, bwd = packed[:len(gemm)], packed[len(gemm):]
        mats, bmats = dict(zip(gemm, fwd)), dict(zip(gemm, bwd))
        B = z.shape[0]
        h = ops.latent_to_grid(z, self.decoder_input.weight, self.decoder_input.bias, self.embed_dim, dt).view(B, self.grid_h, self.grid_w, self.embed_dim)
        if collect is not None:
            collect["grid"], collect["stages"], collect["res_inner"] = h, [], []

        def layer(conv, bn, act, resid=None):
            """One conv layer and what stands behind it -> (h, pre, mean, rstd); conv(act, resid) is the layer's launch.  Folded: the launch carries the
            activation and the residual.  Batch statistics: the raw conv, then ops.bn2d_batch_fwd with both."""
            if not batch_stats:
                return conv(act, resid), None, None, None
            pre = conv(None, None)
            a, mean, rstd = ops.bn2d_batch_fwd(pre, bn, act, resid=resid)
            return a, pre, mean, rstd

        steps, gate = [], None                                         # gate: the stage's input when that is a LeakyReLU(0.01) output
        for st in plan:
            inner = k4 = None
            x_in = h if keep_inputs else None
            bns = [bn for _conv, bn in st.layers]
            if st.kind == "up":
                k4, b = folded[st.fold[0]]
                _B, hh, ww, c = h.shape
                x5, shape = h.view(B, 1, hh, ww, c), (B, 2 * hh, 2 * ww, k4.shape[1])
                outs = [layer(lambda act, _r: ops.ConvUp.apply(x5, k4, b, 2, act, False, False, None).view(shape), bns[0], "leaky001")]
            elif st.kind == "sub":
                k, = st.fold
                outs = [layer(lambda act, _r: ops.conv_s1(h, mats[k], folded[k][1], ops.CONV_S1_SUBPIXEL, act), bns[0], "leaky001")]
            else:
                k0, k1 = st.fold
                first = layer(lambda act, _r: ops.conv_s1(h, mats[k0], folded[k0][1], ops.CONV_S1_K3, act), bns[0], "leaky02")
                inner = first[0]
                outs = [first, layer(lambda act, r: ops.conv_s1(inner, mats[k1], folded[k1][1], ops.CONV_S1_K3, act, resid=r), bns[1], None, resid=h)]
                if collect is not None:
                    collect["res_inner"].append(inner)
            h = outs[-1][0]
            if save:                                                   # the batch-statistics walk alone fills pre, mean, rstd and out, and keeps no gate
                stats = dict(pre=[o[1] for o in outs], mean=[o[2] for o in outs], rstd=[o[3] for o in outs], out=h) if batch_stats else {}
                steps.append(_Step(st, None if batch_stats else gate, inner, [bmats[k] for k in st.fold if k in bmats], k4, x_in, **stats))
            gate = h if st.gates else None
            if collect is not None:
                collect["stages"].append(h)
        return ops.conv_s1_c1(h, out_conv.weight, out_conv.bias), ((steps, out_conv, gate) if save else None)

    # ---- the gradient with respect to the latent (frozen decoder, eval mode) -----------------------------------------------------
    _decoder_grads = False          # train_decoder(): decode_with_grad also accumulates the decoder parameters' gradients
    _decoder_batch_stats = False    # train_decoder(batch_stats=True): its training walk normalises the decoder with batch statistics

    def freeze_decoder(self):
        """requires_grad_(False) on decoder_input and decoder: what decode_with_grad asks for when it is to return no weight gradients."""
        self.decoder_input.requires_grad_(False)
        self.decoder.requires_grad_(False)
        self._decoder_grads = False
        self._decoder_batch_stats = False
        return self

    def train_decoder(self, batch_stats=False):
        """The counterpart of freeze_decoder(): requires_grad_(True) on decoder_input and decoder, and decode_with_grad from now on accumulates `.grad` on every
        decoder parameter next to dz.  The decoder stays in EVAL mode.  batch_stats=False (default): BatchNorm2d normalises with its running
        statistics, which are not updated; its weight and bias learn, and so do the conv weights and biases, through the fold.  batch_stats=True:
        decode_with_grad's walk normalises each of the decoder's 11 BatchNorm2d layers with the statistics of its batch and updates running_mean, running_var
        and num_batches_tracked, as the reference's vae.train() does — asked for by keyword, as dropout and the stem's batch statistics are, not with the
        module's mode.  decode, decode_vjp, reconstruct, forward and fit_latent keep the fold on the running statistics and change no buffer.
        freeze_decoder() clears it."""
        self.decoder_input.requires_grad_(True)
        self.decoder.requires_grad_(True)
        self._decoder_grads = True
        self._decoder_batch_stats = bool(batch_stats)
        return self

    def _decoder_params(self):
        """The decoder's parameters in the order _DecodeWithGrad takes them and returns their gradients: decoder_input's weight and bias, then (conv weight, conv
        bias, BatchNorm weight, BatchNorm bias) per fold-table entry, then the output conv's weight and bias."""
        plan, out_conv = self._decoder_plan()
        ps = [self.decoder_input.weight, self.decoder_input.bias]
        for st in plan:
            for conv, bn in st.layers:
                ps += [conv.weight, conv.bias, bn.weight, bn.bias]
        return ps + [out_conv.weight, out_conv.bias]

    def _check_grad_path(self, z):
        self._check_latent(z, "the decoder's gradient path runs through eval-mode BatchNorm only")
        live = sorted(f"{root}.{k}" for root in ("decoder_input", "decoder") for k, p in getattr(self, root).named_parameters() if p.requires_grad)
        if live and not self._decoder_grads:
            raise CvaeError("ViTVAE.decode_with_grad returns the gradient with respect to z only, through a frozen decoder: these parameters ask for a gradient "
                            f"that would silently stay None: {live} (call model.freeze_decoder(), or model.train_decoder() for their gradients)")
        require_gpu(z, self.decoder_input.weight)

    def _decode_backward(self, saved, g_img, z=None):
        """dz [B, latent_dim] fp32 from the image cotangent [B, 1, H, W] fp32: the chain of DESIGN §13, _decode_walk's steps in reverse.  `g` is the gradient
        with respect to a transposed conv's PRE-activation (the producing epilogue applied leaky001' from the saved output) or to a ResBlock's output; no
        activation-backward launch.
        z (the walk's latent; the walk ran with keep_inputs): returns (dz, gradients of _decoder_params() in that order) — the same launches for dz, and next to
        them each layer's weight gradient from its input and the `g` of its pre-activation, then ONE launch back through the fold.
        After the batch-statistics walk (steps[..].pre; always with z): the same loop, and `g` is the gradient of a stage's output ACTIVATION — no
        data-gradient launch carries a gate (gate_in is None there, a ResBlock's inner gate is left out); the activation's derivative is ops.bn2d_batch_bwd's,
        which turns g into the gradient of the raw conv output plus dgamma and dbeta.  The weight gradients are then the raw weights' ("up": the 3 x 3 part of
        the k4 weight's, as cvae_fold_bn_conv_bwd picks it); the conv biases' are zero in exact arithmetic (the mean is subtracted), computed and returned all
        the same, as autograd does.  No fold_bn_conv_bwd launch."""
        steps, out_conv, out_gate = saved
        batch = steps[0].pre is not None
        dt = self.compute_dtype
        B = g_img.shape[0]
        folded, norms = {}, {}                                         # fold-table position -> (gradient of the layer's weight, of its bias); -> (dgamma, dbeta)

        def through_norm(s, i, g, a, act):
            """The gradient of layer i's conv output from g, the gradient of the activation `a` behind its BatchNorm2d; the folded walk has no such hop."""
            if batch:
                g, *norms[s.stage.fold[i]] = ops.bn2d_batch_bwd(s.pre[i], g, a, s.stage.layers[i][1].weight, s.mean[i], s.rstd[i], act)
            return g

        d_out = ops.conv_s1_c1_wgrad(out_gate, g_img) if z is not None else None
        g = ops.conv_s1_c1_bwd_data(g_img, out_conv.weight, *((None, None) if batch else (out_gate, "leaky001")), dt)
        for s in reversed(steps):
            act = "leaky001" if s.gate_in is not None else None
            if s.stage.kind == "res":
                g2 = through_norm(s, 1, g, None, None)
                t = ops.conv_s1_bwd_data(g2, s.mats[1], ops.CONV_S1_K3, **({} if batch else {"gate": s.inner, "gate_act": "leaky02"}))
                if z is not None:
                    folded[s.stage.fold[1]] = ops.conv_s1_wgrad(s.inner, g2, ops.CONV_S1_K3)
                t = through_norm(s, 0, t, s.inner, "leaky02")
                if z is not None:
                    folded[s.stage.fold[0]] = ops.conv_s1_wgrad(s.x, t, ops.CONV_S1_K3)
                g = ops.conv_s1_bwd_data(t, s.mats[0], ops.CONV_S1_K3, resid=g, gate=s.gate_in, gate_act=act)
                continue
            g = through_norm(s, 0, g, s.out, "leaky001")
            if s.stage.kind == "sub":
                if z is not None:
                    folded[s.stage.fold[0]] = ops.conv_s1_wgrad(s.x, g, ops.CONV_S1_SUBPIXEL)
                g = ops.conv_s1_bwd_data(g, s.mats[0], ops.CONV_S1_SUBPIXEL_T, cin=s.stage.layers[0][0].in_channels, gate=s.gate_in, gate_act=act)
            else:
                w = s.k4
                _B, hh, ww, c = g.shape
                if z is not None:
                    folded[s.stage.fold[0]] = ops._conv_wgrad(s.x.view(B, 1, hh // 2, ww // 2, w.shape[0]), g.view(B, 1, hh, ww, c), 2, w.shape, want_lbias=True)
                g = ops._conv_down(g.view(B, 1, hh, ww, c), ops.pack_weight(w, 2, False, dt), None, None, w.shape[0], 2, None).view(B, hh // 2, ww // 2, w.shape[0])
        g = g.view(B, self.grid_h * self.grid_w, self.embed_dim)
        dz = ops.latent_to_grid_bwd(g, self.decoder_input.weight)
        if z is None:
            return dz
        grads = list(ops.latent_to_grid_wgrad(g, z))
        layers = [(s.stage.kind, conv, bn, k) for s in steps for (conv, bn), k in zip(s.stage.layers, s.stage.fold)]
        if batch:
            for kind, _conv, _bn, k in layers:
                dw, dbias = folded[k]
                grads += [dw[:, :, :3, :3].contiguous() if kind == "up" else dw, dbias, *norms[k]]
        else:
            kinds = {"up": ops.FOLD_CONVT_K3S2, "sub": ops.FOLD_CONVT_K3S2_SUBPIXEL, "res": ops.FOLD_CONV_K3S1}
            for quad in ops.fold_bn_conv_bwd([(conv.weight, kinds[kind], conv.bias, bn) + tuple(folded[k]) for kind, conv, bn, k in layers]):
                grads += quad
        return dz, grads + list(d_out)

    def decode_with_grad(self, z, collect=None):
        """decode(z) (the same launches, the same bits) as a differentiable function of z: backward returns d image / d z through the frozen eval-mode
        decoder, and nothing else — a decoder parameter with requires_grad=True is an error (freeze_decoder()).  Not twice differentiable.
        After train_decoder(): the same image and the same dz, bit for bit (the same walk, the same launches), and backward also accumulates `.grad` on every
        decoder parameter: the decoder in eval mode (running statistics, not updated), conv and BatchNorm parameters learning through the fold.
        After train_decoder(batch_stats=True): the walk normalises with the batch's statistics and moves the running statistics, so the image is
        no longer decode's bit for bit; the gradients are those of the reference's decoder under .train()."""
        self._check_grad_path(z)
        if self._decoder_grads:
            return _DecodeWithGrad.apply(z, self, collect, *self._decoder_params())
        return _DecodeWithGrad.apply(z, self, collect)

    @torch.no_grad()
    def decode_vjp(self, z, grad_image):
        """dz = (d decode(z) / d z)^T grad_image, fp32 [B, latent_dim]: the explicit form of decode_with_grad's backward (capturable in a graph).  dz only, also
        after train_decoder()."""
        self._check_grad_path(z)
        if tuple(grad_image.shape) != (z.shape[0], 1, self.img_height, self.img_width) or grad_image.dtype != torch.float32:
            raise CvaeError(f"ViTVAE.decode_vjp expects a float32 [{z.shape[0]}, 1, {self.img_height}, {self.img_width}] cotangent, got "
                            f"{tuple(grad_image.shape)} {grad_image.dtype}")
        require_gpu(grad_image)
        if z.shape[0] == 0:
            return torch.zeros_like(z)
        _image, saved = self._decode_walk(z.detach(), True)
        return self._decode_backward(saved, grad_image.contiguous())

    # ---- training the whole model (eval mode) --------------------------------------------------------------------------
    def train_all(self, dropout=False, stem_batch_stats=False, decoder_batch_stats=False):
        """train_stem(batch_stats=stem_batch_stats) + train_transformer(dropout=dropout) + train_decoder(batch_stats=decoder_batch_stats): every parameter asks for
        a gradient and forward_train's graph reaches every one of them.  Returns all parameters (named_parameters order), for the optimizer.  The model stays
        in EVAL mode (see train_vit_vae); stem_batch_stats=True: the stem's BatchNorm2d layers train on batch statistics all the same;
        decoder_batch_stats=True: so do the decoder's.  With both, every BatchNorm2d of the model trains as under the reference's .train()."""
        self.train_stem(batch_stats=stem_batch_stats)
        self.train_transformer(dropout=dropout)
        self.train_decoder(batch_stats=decoder_batch_stats)
        return list(self.parameters())

    def forward_train(self, x, eps=None):
        """(recons, x, mu, log_var) as forward(), on the autograd graph: encode_with_grad -> ops.Reparameterize -> decode_with_grad.  eps [B, latent_dim] fp32, or
        None: drawn with torch.randn on x's device.  For the same eps the values are those of the eval path, bit for bit (the same launches)."""
        mu, log_var = self.encode_with_grad(x)
        if eps is None:
            eps = torch.randn(mu.shape, dtype=torch.float32, device=mu.device)
        elif tuple(eps.shape) != tuple(mu.shape) or eps.dtype != torch.float32:
            raise CvaeError(f"ViTVAE.forward_train: eps must be a float32 {tuple(mu.shape)} matrix, got {tuple(eps.shape)} {eps.dtype}")
        return self.decode_with_grad(ops.Reparameterize.apply(mu, log_var, eps)), x, mu, log_var

    def reparameterize(self, mu, log_var):
        """vit_backbone.py:181-184: mu + randn_like(std) * std on torch's generator."""
        std = torch.exp(0.5 * log_var)
        return mu + torch.randn_like(std) * std

    @torch.no_grad()
    def forward(self, x):
        """(recons, x, mu, log_var) as ViTVAE.forward (vit_backbone.py:195-199), eval mode."""
        mu, log_var = self.encode(x)
        return self.decode(self.reparameterize(mu, log_var)), x, mu, log_var

    @torch.no_grad()
    def reconstruct(self, x):
        """decode(mu(x)): the deterministic reconstruction."""
        return self.decode(self.encode(x)[0])


class _DecodeWithGrad(torch.autograd.Function):
    """ViTVAE.decode_with_grad: z -> image, with dz as the only gradient; after train_decoder() the decoder's parameters (ViTVAE._decoder_params()) are inputs
    too, so autograd accumulates their gradients, zero_grad works and a parameter rewritten between forward and backward is an error."""

    @staticmethod
    def forward(ctx, z, model, collect, *params):
        zd = z.detach()
        image, saved = model._decode_walk(zd, True, collect, keep_inputs=bool(params), batch_stats=bool(params) and model._decoder_batch_stats)
        ctx.model, ctx.saved = model, saved                            # activations and folded matrices of this call: private to the node, freed with it
        ctx.z = zd.contiguous() if params else None
        ctx.save_for_backward(*params)
        return image

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        params = ctx.saved_tensors                                     # raises if a parameter was modified in place since the forward
        if g.shape[0] == 0:
            return (g.new_zeros(0, ctx.model.latent_dim), None, None) + tuple(torch.zeros_like(p) for p in params)
        if not params:
            return ctx.model._decode_backward(ctx.saved, g.contiguous()), None, None
        dz, grads = ctx.model._decode_backward(ctx.saved, g.contiguous(), ctx.z)
        return (dz, None, None) + tuple(d.view(p.shape) for d, p in zip(grads, params))


def fit_latent(model, x, z0, steps, lr, loss="sse"):
    """Fit a latent to images: Adam on z through decode_with_grad and the project's losses.  x [B, 1, H, W] fp32, z0 [B, latent_dim] fp32 (not modified);
    loss "sse" (ops.sse) or "vessel" (ops.VesselRecon: recon + sparsity, vessel_analysis/01_train/train.py:27-46).  Returns (z, losses): the fitted
    latent and the loss BEFORE each of the `steps` updates as a list of floats (read from the device once, at the end)."""
    if loss not in ("sse", "vessel"):
        raise CvaeError(f"fit_latent: loss must be 'sse' or 'vessel', got {loss!r}")
    require_gpu(x, z0)
    z = z0.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([z], lr=lr)
    losses = []
    batch_stats, model._decoder_batch_stats = model._decoder_batch_stats, False      # a latent is fitted to the decoder as inference runs it: the fold, no buffer moved
    try:
        for _ in range(int(steps)):
            opt.zero_grad(set_to_none=True)
            recon = model.decode_with_grad(z)
            value = ops.sse(recon, x) if loss == "sse" else sum(ops.VesselRecon.apply(recon, x))
            value.backward()
            opt.step()
            losses.append(value.detach())
    finally:
        model._decoder_batch_stats = batch_stats
    return z.detach(), [float(v) for v in torch.stack(losses).cpu()] if losses else []


def vit_vae_loss(recons, x, mu, log_var, beta=1.0):
    """The loss of the reference's ViTVAE loop (latent_translator/engine.py:25-27): mse_loss(recons, x, mean) + beta * (-0.5 * mean(1 + log_var - mu^2 -
    exp(log_var))).  The image term is ops.sse / numel on the GPU (one reduction, the gradient from one launch); the [B, latent] arithmetic stays in torch.
    Host tensors (a loss of stored arrays, the CPU tests) take torch's mse_loss: the expression itself, no kernel involved."""
    recon = ops.sse(recons, x) / x.numel() if recons.is_cuda else F.mse_loss(recons, x, reduction="mean")
    kld = -0.5 * torch.mean(1 + log_var - mu.pow(2) - log_var.exp())
    return recon + beta * kld


def vit_vae_train_step(model, optimizer, x, eps=None, beta=1.0):
    """One iteration of train_vit_vae's loop: zero_grad, model.forward_train(x, eps), vit_vae_loss, backward, optimizer.step() -> the loss, a 0-dim device
    tensor.  Needs model.train_all() (or the train_*() calls of the parts that learn) first.  Nothing here syncs with the host, so the step can be
    captured (GraphedViTTrainStep)."""
    optimizer.zero_grad()
    loss = vit_vae_loss(*model.forward_train(x, eps), beta=beta)
    loss.backward()
    optimizer.step()
    return loss.detach()


def _check_graph_optimizer(what, optimizer):
    from ..optim import FusedAdam
    if not isinstance(optimizer, FusedAdam) or not optimizer.device_step:
        raise CvaeError(f"{what} needs FusedAdam(..., device_step=True): a captured step replays with the step count on the device "
                        f"(got {type(optimizer).__name__}" + (" with device_step=False" if isinstance(optimizer, FusedAdam) else "") + ")")


def train_vit_vae(model, loader, optimizer, device, epochs, beta=1.0, dropout=False, graph=False, stem_batch_stats=False, decoder_batch_stats=False):
    """The reference's ViTVAE training loop (latent_translator/engine.py:6-36), same signature plus `dropout` and `graph`: per batch["x"], zero_grad, model.forward_train,
    vit_vae_loss, backward, optimizer.step() (vit_vae_train_step).  It runs in THIS project's training regime, which is not the reference's model.train(): the model is put in eval
    mode, so every BatchNorm2d normalises with its running statistics, which are not updated (as train_decoder() and train_stem() state), and there is no
    dropout unless dropout=True: then the transformer blocks drop as the reference's do under train(), at the modules' rates, with Philox masks
    (train_transformer(dropout=True); float32 compute dtype).  stem_batch_stats=True: the conv stem's five BatchNorm2d layers normalise with
    batch statistics and update their running statistics, as the reference's do (train_stem(batch_stats=True)); decoder_batch_stats=True: so do the
    decoder's eleven (train_decoder(batch_stats=True)).  With both, BatchNorm2d runs as under the reference's model.train().  All parameters learn (model.train_all() is called, so an optimizer built over
    model.parameters() fits).  Returns the per-epoch mean losses as a list of floats (sample-weighted, read from the device once per epoch).
    graph=True (needs FusedAdam(device_step=True), else CvaeError): the step is captured once, from the first batch, as one HIP graph (GraphedViTTrainStep,
    DESIGN §19) and replayed for every batch of that shape; a batch of another shape (a ragged last one) takes the eager step.  With dropout the keys then
    live on the device (model.use_device_dropout_keys()), for the eager steps too."""
    if graph:
        _check_graph_optimizer("train_vit_vae(graph=True)", optimizer)
    model.eval()
    model.train_all(dropout=dropout, stem_batch_stats=stem_batch_stats, decoder_batch_stats=decoder_batch_stats)
    history, graphed = [], None
    for _ep in range(int(epochs)):
        total, n = [], 0
        for batch in loader:
            x = batch["x"].to(device)
            if graph and graphed is None:
                from .train import GraphedViTTrainStep
                graphed = GraphedViTTrainStep(model, optimizer, (x,), beta=beta)
            if graphed is not None and x.shape == graphed.batch[0].shape:
                loss = graphed(x)
            else:
                loss = vit_vae_train_step(model, optimizer, x, beta=beta)
            total.append(loss.detach() * x.shape[0])
            n += x.shape[0]
        history.append(float(torch.stack(total).sum().cpu()) / max(n, 1) if total else 0.0)
    return history


def resize_pos_embedding(pos, src_grid, dst_grid):
    """A position embedding [1, 1 + hs * ws, D] for another patch grid: the CLS row is kept, the grid rows are laid out as a [D, hs, ws] image and
    resized bicubically (align_corners=False) to dst_grid — what the reference's latent_translator does when it loads a 768 x 1280 checkpoint into
    a 384 x 640 model.  Host-side torch, run once at load."""
    (hs, ws), (hd, wd) = src_grid, dst_grid
    if pos.dim() != 3 or pos.shape[0] != 1 or pos.shape[1] != 1 + hs * ws:
        raise CvaeError(f"resize_pos_embedding: {tuple(pos.shape)} is not [1, 1 + {hs} * {ws}, D]")
    if (hs, ws) == (hd, wd):
        return pos
    D = pos.shape[2]
    grid = pos[:, 1:].transpose(1, 2).reshape(1, D, hs, ws)
    grid = F.interpolate(grid.float(), size=(hd, wd), mode="bicubic", align_corners=False)
    return torch.cat([pos[:, :1], grid.flatten(2).transpose(1, 2).to(pos.dtype)], dim=1)


def _source_grid(n, dst_grid):
    """The patch grid of a checkpoint's n position rows: the one with the target's aspect ratio."""
    hd, wd = dst_grid
    for hs in range(1, n + 1):
        if n % hs == 0 and hs * wd == (n // hs) * hd:
            return hs, n // hs
    raise CvaeError(f"load_vitvae_state_dict: cannot tell the patch grid of a pos_embedding with {n} grid rows from the model's {hd} x {wd} grid "
                    "(different aspect ratio): pass src_grid=(h, w)")


def load_vitvae_state_dict(model, state_dict, src_grid=None):
    """Load a full reference ViTVAE checkpoint.  Into a ViTVAE every key is loaded and the returned list is empty; into a ViTVAEEncoder the decoder keys
    (decoder_input.*, decoder.*) are dropped and returned as a sorted list.  A pos_embedding of another patch grid is resized (resize_pos_embedding;
    src_grid = the checkpoint's (h, w) grid when it does not share the model's aspect ratio; decoder_input then has another shape, so this serves the
    encoder only); every other missing, unexpected or mis-shaped key is an error."""
    own = model.state_dict()
    owns_decoder = any(k.startswith(("decoder_input.", "decoder.")) for k in own)
    dropped = [] if owns_decoder else sorted(k for k in state_dict if k.startswith(("decoder_input.", "decoder.")))
    sd = {k: v for k, v in state_dict.items() if k not in set(dropped)}
    unexpected, missing = sorted(set(sd) - set(own)), sorted(set(own) - set(sd))
    if unexpected or missing:
        raise CvaeError(f"load_vitvae_state_dict: unexpected keys {unexpected}, missing keys {missing}")
    pos = sd["pos_embedding"]
    if tuple(pos.shape) != tuple(own["pos_embedding"].shape):
        if pos.dim() != 3 or pos.shape[0] != 1 or pos.shape[2] != model.embed_dim:
            raise CvaeError(f"load_vitvae_state_dict: pos_embedding {tuple(pos.shape)} cannot be resized to {tuple(own['pos_embedding'].shape)}")
        dst = (model.grid_h, model.grid_w)
        sd["pos_embedding"] = resize_pos_embedding(pos.detach().cpu(), src_grid or _source_grid(pos.shape[1] - 1, dst), dst)
    bad = [k for k, v in sd.items() if tuple(v.shape) != tuple(own[k].shape)]
    if bad:
        raise CvaeError(f"load_vitvae_state_dict: shape mismatch for {bad}")
    model.load_state_dict(sd, strict=True)
    return dropped


@torch.no_grad()
def extract_vit_latents(model, loader, device):
    """The reference's latent_translator/engine.py:38-52: eval mode, mu of every batch["x"], stacked as one numpy array.  The per-batch results stay on the
    device; one host copy is made at the end."""
    model.eval()
    zs = [model.encode(batch["x"].to(device))[0] for batch in loader]
    return torch.cat(zs, dim=0).cpu().numpy() if zs else np.zeros((0, model.latent_dim), dtype=np.float32)


@torch.no_grad()
def extract_vit_attention(model, loader, device, residual=0.5):
    """attention_rollout(batch["x"], residual) of every batch of the loader (extract_vit_latents' protocol), stacked as one numpy array [n, grid_h, grid_w];
    model: a ViTVAE / ViTVAEEncoder, or a CausalViTVAE (its backbone's map).  The per-batch maps stay on the device; one host copy is made at the end."""
    model.eval()
    enc = getattr(model, "backbone", model)
    maps = [model.attention_rollout(batch["x"].to(device), residual=residual) for batch in loader]
    return torch.cat(maps, dim=0).cpu().numpy() if maps else np.zeros((0, enc.grid_h, enc.grid_w), dtype=np.float32)


@torch.no_grad()
def extract_vit_saliency(model, loader, device, **kw):
    """saliency(batch["x"], **kw) of every batch of the loader (extract_vit_latents' protocol), stacked as one numpy array [n, H, W]; model: a ViTVAE /
    ViTVAEEncoder, or a CausalViTVAE (its backbone's map).  The per-batch maps stay on the device; one host copy is made at the end."""
    model.eval()
    enc = getattr(model, "backbone", model)
    maps = [model.saliency(batch["x"].to(device), **kw) for batch in loader]
    return torch.cat(maps, dim=0).cpu().numpy() if maps else np.zeros((0, enc.img_height, enc.img_width), dtype=np.float32)


@torch.no_grad()
def extract_vit_relevance(model, loader, device, **kw):
    """attention_relevance(batch["x"], **kw) of every batch of the loader (extract_vit_attention's protocol), stacked as one numpy array [n, grid_h, grid_w]
    ([n, N] with as_grid=False); model: a ViTVAE / ViTVAEEncoder, or a CausalViTVAE (its backbone's map).  One host copy is made at the end."""
    model.eval()
    enc = getattr(model, "backbone", model)
    maps = [model.attention_relevance(batch["x"].to(device), **kw) for batch in loader]
    empty = (0, enc.grid_h, enc.grid_w) if kw.get("as_grid", True) else (0, enc.num_patches + 1)
    return torch.cat(maps, dim=0).cpu().numpy() if maps else np.zeros(empty, dtype=np.float32)

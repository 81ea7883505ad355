"""CausalViTVAE — the reference's ViT-backbone vessel model (vessel_analysis/00_core/models.py:181-307) for eval-mode inference on MI355X:
(x, m, t) -> z -> (z, m) -> x through the ViTVAE backbone and three small dense heads.

Built in the reference's order (backbone, enc_adapter, dec_adapter, morph_predictor_shared, morph_predictor_mu, morph_predictor_logvar) with its
attribute tree, so `torch.manual_seed(s); CausalViTVAE()` draws the reference's weights and the state_dict key sets are equal.  The torch modules only
hold the parameters; per call:
  encode         backbone.cls_features (steps A-D of the reference forward), then ONE cvae_mlp_heads_fwd launch: [cls_out | m | t] -> enc_adapter ->
                 mu (clamp +-100) | logvar (clamp +-10), and z = mu + eps exp(logvar / 2) in the same launch when eps is given
  predict_morph  ONE launch: t -> morph_predictor_shared -> morph_predictor_mu | morph_predictor_logvar (clamp +-10), the two last-layer weights read in place
  decode         ONE launch: [m | z] -> dec_adapter -> z_vit, then backbone.decode
The heads are fp32 in both compute dtypes (they set mu and z_vit and take no time); set_compute_dtype switches the backbone only.
No cat, BatchNorm1d, clamp, chunk or element-wise launch sits between the backbone's launches and the three heads launches.

Training the adapters (train_adapters, forward_train): the three heads run in training mode (batch-statistics BatchNorm1d, running statistics updated) and
are differentiable (ops.mlp_heads_train); the gradient reaches them through backbone.decode_with_grad.  The ONE difference from the reference: its
`vae.train()` also puts the backbone's dropout and BatchNorm2d in training mode and its optimizer updates backbone weights; here the backbone is frozen and
stays in eval mode."""
import torch
import torch.nn as nn

from .. import ops
from .._lib import CvaeError
from ..vessel.config import CONFIG
from .models import ViTVAE, load_vitvae_state_dict


class AdapterMLP(nn.Sequential):
    """Linear -> BatchNorm1d -> LeakyReLU(slope) -> Linear with the reference's nn.Sequential indices (state_dict keys `0.weight`, `1.running_mean`, `3.bias`, ..).
    A parameter holder: forward(x) runs the whole stack as one fused launch (ops.mlp_heads) in eval mode, so the reference consumers'
    `model.dec_adapter(torch.cat([m, z], 1))` works unchanged."""

    def __init__(self, in_features, hidden, out_features, slope=0.2):
        super().__init__(nn.Linear(in_features, hidden), nn.BatchNorm1d(hidden), nn.LeakyReLU(slope), nn.Linear(hidden, out_features))

    def head_layers(self):
        return [(self[0], self[1], self[2].negative_slope), (self[3], None, None)]

    def _require_eval(self):
        if self.training:
            raise RuntimeError("AdapterMLP: put the model in eval mode first (model.eval()): batch-statistics BatchNorm1d is not implemented, the adapter "
                               "runs inference only")

    @torch.no_grad()
    def fused(self, panels, **kw):
        """ops.mlp_heads on the logical concatenation of `panels` (no cat buffer)."""
        self._require_eval()
        return ops.mlp_heads(panels, self.head_layers(), **kw)

    def forward(self, x):
        return self.fused([x])[0]


class _SharedTrunk(nn.Sequential):
    """morph_predictor_shared's parameter holder (Linear, LeakyReLU, Linear, LeakyReLU: keys `0.*`, `2.*`).  It never runs alone: the trunk and the two output
    layers are one launch (CausalViTVAE.predict_morph)."""

    def forward(self, t):
        raise RuntimeError("morph_predictor_shared holds parameters only: call CausalViTVAE.predict_morph(t), which runs the trunk and both output layers "
                           "in one launch")


class CausalViTVAE(nn.Module):
    """Eval-mode inference, and training of the adapter heads on the frozen eval-mode backbone (train_adapters / forward_train).  Differences from the
    reference class, all stated here:
      * training: the reference's `vae.train()` also puts the backbone's dropout and BatchNorm2d in training mode and updates backbone weights; here the
        backbone is frozen and in eval mode, and only the three heads learn.
      * pretrained_path: the reference loads the backbone checkpoint with strict=False and so ignores any mismatch; here a missing, unexpected or mis-shaped
        key is an error that names the keys (load_vitvae_state_dict).  The one exception is load_vitvae_state_dict's own: a pos_embedding of another
        patch grid is resized to this model's grid (it matters only with img_size=; decoder_input.weight of another grid is still a shape error).  The file
        is read on the CPU.
      * keyword-only img_size / depth build a smaller backbone (tests); the defaults are the reference's.
      * forward / reparameterize take an optional eps [B, Z]; without it they draw torch.randn_like, as the reference does.
      * m, t, z and eps may be any float32 [B, w] views: m0.expand(B, -1) or one eps draw expanded over the rows is copied before the launch.
      * every entry but forward_train runs under no_grad and raises in training mode."""
    decode_signature = "z_m"       # decode(z, m): counterfactual.batched_counterfactual and vessel.analysis dispatch on this name

    def __init__(self, pretrained_path=None, *, img_size=None, depth=6):
        super().__init__()
        if img_size is None:
            img_size = (CONFIG["IMG_HEIGHT"], CONFIG["IMG_WIDTH"])
        self.backbone = ViTVAE(img_size=tuple(img_size), patch_size=32, embed_dim=256, depth=depth, heads=8, mlp_dim=512, latent_dim=512)
        if pretrained_path:
            state_dict = torch.load(pretrained_path, map_location="cpu")
            load_vitvae_state_dict(self.backbone, state_dict)
        self.vit_embed_dim, self.vit_latent_dim = 256, 512
        self.my_z_dim, self.m_dim, self.t_dim = CONFIG["Z_DIM"], CONFIG["M_DIM"], CONFIG["T_DIM"]
        self.enc_adapter = AdapterMLP(self.vit_embed_dim + self.m_dim + self.t_dim, 512, self.my_z_dim * 2)
        self.dec_adapter = AdapterMLP(self.my_z_dim + self.m_dim, 256, self.vit_latent_dim)
        self.morph_predictor_shared = _SharedTrunk(nn.Linear(self.t_dim, 64), nn.LeakyReLU(0.2), nn.Linear(64, 64), nn.LeakyReLU(0.2))
        self.morph_predictor_mu = nn.Linear(64, self.m_dim)
        self.morph_predictor_logvar = nn.Linear(64, self.m_dim)

    # ---- training the adapters on the frozen backbone -----------------------------------------------------------------------------
    _adapters_only = False
    _train_decoder = False
    _train_transformer = False
    _train_stem = False

    def head_parameters(self):
        return [p for mod in (self.enc_adapter, self.dec_adapter, self.morph_predictor_shared, self.morph_predictor_mu, self.morph_predictor_logvar)
                for p in mod.parameters()]

    def train_adapters(self, decoder=False, transformer=False, stem=False, dropout=False, stem_batch_stats=False, decoder_batch_stats=False):
        """Freeze the backbone (requires_grad_(False) on every backbone parameter, eval mode) and keep it in eval mode through later model.train() calls; the
        heads go to training mode.  Returns the list of head parameters, for the optimizer.  Every call starts from the frozen state (backbone.freeze_decoder(), so
        a default call after a decoder=True one switches the decoder's gradients off again).
        decoder=True: the backbone's decoder learns too (backbone.train_decoder(): decoder_input and decoder ask for gradients, still in eval mode: BatchNorm2d on
        its running statistics, which are not updated); the encoder stays frozen.  Returns head plus decoder parameters.  decoder_batch_stats=True (needs
        decoder=True): the decoder's 11 BatchNorm2d layers normalise with batch statistics in the training forward and update their running statistics
        (backbone.train_decoder(batch_stats=True); the backbone module itself stays in eval mode).
        transformer=True: the backbone's transformer learns too (backbone.train_transformer(): pos_embedding, cls_token, transformer, to_latent; eval mode; the
        conv stem stays frozen).  dropout=True (needs transformer=True; float32 compute dtype): its blocks then drop in the training forward as the
        reference's do under train() (backbone.train_transformer(dropout=True)); default: no dropout.  fc_mu and fc_var stay frozen and are not returned: this model reads the cls features, not the
        backbone's (mu, log_var), so no gradient ever reaches them.  Returns head plus transformer parameters (plus the decoder's with decoder=True).
        stem=True (needs transformer=True): the backbone's conv stem learns too (backbone.train_stem(): eval-mode BatchNorm2d on its running statistics;
        DESIGN §17), the whole backbone is then fine-tuned as vessel_analysis/01_train/train.py does; its parameters are returned too.  stem_batch_stats=True
        (needs stem=True): the stem's BatchNorm2d layers normalise with batch statistics in the training forward and update their running statistics, as that
        script's .train() does (backbone.train_stem(batch_stats=True); the backbone module itself stays in eval mode)."""
        if stem and not transformer:
            raise CvaeError("CausalViTVAE.train_adapters: stem=True needs transformer=True (the stem's gradient arrives through the transformer)")
        if stem_batch_stats and not stem:
            raise CvaeError("CausalViTVAE.train_adapters: stem_batch_stats=True needs stem=True (a frozen stem runs the fold on its running statistics)")
        if decoder_batch_stats and not decoder:
            raise CvaeError("CausalViTVAE.train_adapters: decoder_batch_stats=True needs decoder=True (a frozen decoder runs the fold on its running statistics)")
        if dropout and not transformer:
            raise CvaeError("CausalViTVAE.train_adapters: dropout=True needs transformer=True (the dropout sites are the transformer blocks'; a frozen "
                            "transformer runs its inference form)")
        self.backbone.requires_grad_(False)
        self.backbone.freeze_decoder()
        self.backbone.freeze_transformer()
        self.backbone.freeze_stem()
        self._adapters_only, self._train_decoder, self._train_transformer, self._train_stem = True, bool(decoder), bool(transformer), bool(stem)
        self.train()
        params = self.head_parameters()
        if stem:
            params += self.backbone.train_stem(batch_stats=stem_batch_stats)
        if transformer:
            params += self.backbone.train_transformer(heads=False, dropout=dropout)
        if decoder:
            self.backbone.train_decoder(batch_stats=decoder_batch_stats)
            params += list(self.backbone.decoder_input.parameters()) + list(self.backbone.decoder.parameters())
        return params

    def train(self, mode=True):
        """nn.Module.train; after train_adapters() the backbone stays in eval mode whatever `mode` is."""
        super().train(mode)
        if self._adapters_only:
            self.backbone.eval()
        return self

    def forward_train(self, x, m, t, eps=None):
        """The reference 6-tuple (recon_x, m_mu, mu, logvar, m_mu, m_logvar) attached to the autograd graph of the head parameters: backbone.cls_features
        under no_grad, enc_adapter, the morph predictor and dec_adapter in training mode (ops.mlp_heads_train: batch statistics, running statistics updated),
        then backbone.decode_with_grad.  The backbone is fp32 or bf16; the heads are fp32.  Needs train_adapters() first; after train_adapters(decoder=True)
        the backbone's decoder parameters may ask for gradients, and backward accumulates them (eval-mode decoder); after
        train_adapters(transformer=True) cls_features_with_grad takes cls_features' place and the transformer's parameters learn through enc_adapter's cls_out
        panel."""
        roots = ((("decoder_input", "decoder") if self._train_decoder else ()) + (self.backbone._TRANSFORMER_ROOTS if self._train_transformer else ())
                 + (("stem",) if self._train_stem else ()))
        live = [k for k, p in self.backbone.named_parameters() if p.requires_grad and k.split(".")[0] not in roots]
        if self.backbone.training or live:
            raise RuntimeError("CausalViTVAE.forward_train trains the adapter heads on a frozen eval-mode backbone: call model.train_adapters() first "
                               f"(backbone.training={self.backbone.training}, {len(live)} backbone parameters require grad)")
        B = x.shape[0]
        m, t = self._rows("m", m, self.m_dim, B), self._rows("t", t, self.t_dim, B)
        eps = torch.randn(B, self.my_z_dim, dtype=torch.float32, device=x.device) if eps is None else self._rows("eps", eps, self.my_z_dim, B)
        cls_out = self.backbone.cls_features_with_grad(x) if self._train_transformer else self.backbone.cls_features(x)
        mu, logvar, z = ops.mlp_heads_train([cls_out, m, t], self.enc_adapter.head_layers(), split=self.my_z_dim, clamp0=(-100.0, 100.0),
                                            clamp1=(-10.0, 10.0), eps=eps)
        m_mu, m_logvar, _z = ops.mlp_heads_train([t], self.morph_layers(), clamp1=(-10.0, 10.0))
        z_vit, _s, _z = ops.mlp_heads_train([m, z], self.dec_adapter.head_layers())
        return self.backbone.decode_with_grad(z_vit), m_mu, mu, logvar, m_mu, m_logvar

    def morph_layers(self):
        s = self.morph_predictor_shared
        return [(s[0], None, s[1].negative_slope), (s[2], None, s[3].negative_slope), ((self.morph_predictor_mu, self.morph_predictor_logvar), None, None)]

    def set_compute_dtype(self, dtype):
        """float32 or bfloat16 for the backbone; the heads stay fp32."""
        self.backbone.set_compute_dtype(dtype)
        return self

    @property
    def compute_dtype(self):
        return self.backbone.compute_dtype

    # ---- checks -------------------------------------------------------------------------------------------------------------------
    def _require_eval(self):
        if self.training:
            raise RuntimeError("CausalViTVAE: put the model in eval mode first (model.eval()): dropout and batch-statistics BatchNorm are not implemented, "
                               "the model runs inference only")

    def _rows(self, name, v, width, B=None):
        if v.dim() != 2 or v.shape[1] != width or v.dtype != torch.float32 or (B is not None and v.shape[0] != B):
            raise CvaeError(f"CausalViTVAE: {name} must be a float32 [{'B' if B is None else B}, {width}] matrix, got {tuple(v.shape)} {v.dtype}")
        return v            # any strides: ops.mlp_heads reads a row-major view in place and copies an expanded or transposed one

    # ---- the model ----------------------------------------------------------------------------------------------------------------
    def _encode(self, x, m, t, eps):
        self._require_eval()
        B = x.shape[0]
        m, t = self._rows("m", m, self.m_dim, B), self._rows("t", t, self.t_dim, B)
        if eps is not None:
            eps = self._rows("eps", eps, self.my_z_dim, B)
        cls_out = self.backbone.cls_features(x)
        return self.enc_adapter.fused([cls_out, m, t], split=self.my_z_dim, clamp0=(-100.0, 100.0), clamp1=(-10.0, 10.0), eps=eps)

    @torch.no_grad()
    def encode(self, x, m, t):
        """(mu, logvar) of q(z | x, m, t), clamped as forward clamps them (models.py:285-286): backbone.cls_features, then one heads launch."""
        mu, logvar, _z = self._encode(x, m, t, None)
        return mu, logvar

    @torch.no_grad()
    def predict_morph(self, t):
        """(m_mu, m_logvar) of p(m | t), m_logvar clamped to +-10 (models.py:291-294): one launch."""
        self._require_eval()
        t = self._rows("t", t, self.t_dim)
        m_mu, m_logvar, _z = ops.mlp_heads([t], self.morph_layers(), clamp1=(-10.0, 10.0))
        return m_mu, m_logvar

    def attention_rollout(self, x, **kw):
        """backbone.attention_rollout(x, **kw): where the encoder's CLS token looks.  The adapters read the CLS features only, so this is the
        whole image path of encode."""
        self._require_eval()
        return self.backbone.attention_rollout(x, **kw)

    def saliency(self, x, **kw):
        """backbone.saliency(x, **kw): which pixels move the backbone's mu / log_var / cls features, fp32 [B, H, W]."""
        self._require_eval()
        return self.backbone.saliency(x, **kw)

    def gradcam(self, x, **kw):
        """backbone.gradcam(x, **kw): Grad-CAM on the backbone's stem output, fp32 [B, grid_h, grid_w]."""
        self._require_eval()
        return self.backbone.gradcam(x, **kw)

    def attention_gradients(self, x, **kw):
        """backbone.attention_gradients(x, **kw): the gradient of a backbone target with respect to the attention probabilities."""
        self._require_eval()
        return self.backbone.attention_gradients(x, **kw)

    def attention_relevance(self, x, **kw):
        """backbone.attention_relevance(x, **kw): gradient-weighted attention relevance of a backbone target, fp32 [B, grid_h, grid_w]."""
        self._require_eval()
        return self.backbone.attention_relevance(x, **kw)

    @torch.no_grad()
    def decode(self, z, m):
        """backbone.decode(dec_adapter(cat[m, z])) -> [B, 1, H, W] (models.py:299-305).  Note the argument order: z first, m second; the concatenation is
        [m, z].  One heads launch (no cat buffer), then the backbone's decoder."""
        self._require_eval()
        z = self._rows("z", z, self.my_z_dim)
        m = self._rows("m", m, self.m_dim, z.shape[0])
        return self.backbone.decode(self.dec_adapter.fused([m, z])[0])

    @torch.no_grad()
    def reparameterize(self, mu, logvar, eps=None):
        """mu + eps * exp(0.5 * logvar); eps=None draws torch.randn_like, as the reference does (models.py:252-255)."""
        self._require_eval()
        if mu.dim() != 2:
            raise CvaeError(f"CausalViTVAE.reparameterize: mu must be a float32 [B, Z] matrix, got {tuple(mu.shape)}")
        B, Z = mu.shape
        mu, logvar = self._rows("mu", mu, Z), self._rows("logvar", logvar, Z, B)
        eps = torch.randn_like(mu) if eps is None else self._rows("eps", eps, Z, B)
        return ops.Reparameterize.apply(mu.contiguous(), logvar.contiguous(), eps.contiguous())

    @torch.no_grad()
    def forward(self, x, m, t, eps=None):
        """(recon_x, m_hat, mu, logvar, m_mu, m_logvar) as the reference forward in eval mode (models.py:257-307), m_hat is m_mu.  eps [B, Z] or None (drawn
        with torch.randn on x's device); the encoder heads launch writes z itself."""
        self._require_eval()
        if eps is None:
            eps = torch.randn(x.shape[0], self.my_z_dim, dtype=torch.float32, device=x.device)
        mu, logvar, z = self._encode(x, m, t, eps)
        m_mu, m_logvar = self.predict_morph(t)
        recon_x = self.decode(z, m)
        return recon_x, m_mu, mu, logvar, m_mu, m_logvar

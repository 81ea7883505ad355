"""ViT-VAE inference (the reference's ViTVAE, vessel_analysis/00_core/vit_backbone.py:50-199 and latent_translator/models.py), eval mode only:
ViTVAEEncoder: image -> (mu, log_var) / CLS features; ViTVAE: the same plus decode / forward / reconstruct; CausalViTVAE (vessel_analysis/00_core/models.py:181-307): that backbone
between the fused adapter heads of the (x, m, t) -> z -> (z, m) -> x model; CausalViTVAE.train_adapters / forward_train train those heads on the frozen
eval-mode backbone (the reference's vae.train() also trains the backbone and runs its dropout and BatchNorm2d in training mode: here it stays frozen, or
learns in eval mode: train_decoder / train_transformer / train_stem; the BatchNorm2d layers train on batch statistics when asked by keyword: the stem's with
train_stem(batch_stats=True) / stem_batch_stats=True, DESIGN §23, the decoder's with train_decoder(batch_stats=True) / decoder_batch_stats=True).  ViTVAE.train_all / forward_train, vit_vae_loss and train_vit_vae: the reference's ViTVAE
training loop (latent_translator/engine.py:6-36) end to end, in that eval-mode regime.  vit_vae_train_step / causal_vit_train_step: one step of either
recipe; GraphedViTTrainStep: that step captured as one HIP graph, which train_vit_vae(graph=True) replays.
Looking inside: ViTVAEEncoder.attention_weights / attention_rollout (so ViTVAE's, and CausalViTVAE.attention_rollout through its backbone) and
extract_vit_attention, the rollout maps of a loader.  The gradient with respect to the image: ViTVAEEncoder.cls_features_vjp / encode_vjp, x.grad
after cls_features_with_grad / encode_with_grad / ViTVAE.forward_train of an image that asks, saliency (plain and integrated gradients) and gradcam (both also
on CausalViTVAE, through its backbone), and extract_vit_saliency for a loader.  Looking inside with a target: ViTVAEEncoder.attention_gradients
(the gradient with respect to the attention probabilities) and attention_relevance (gradient-weighted attention relevance), both also on CausalViTVAE, and
extract_vit_relevance for a loader.  The latent translator (translator.py): fit_translator_ridge / translate_vit_latents (a float64 Ridge from the
latents to the morphology table, ranked by exact leave-one-out R²) and bootstrap_feature_stability with its helpers, the reference's
latent_translator/analysis.py.  Choosing alpha and looking at the latents: fit_translator_ridge_cv (alpha from a grid by exact leave-one-out on one
eigendecomposition; translate_vit_latents takes the grid too) and latent_pca / pca_vit_latents (the reference's PCA of its latents, pca.py).  The non-linear
view (tsne.py): latent_tsne / tsne_vit_latents, the reference's TSNE calls as the exact method in float64."""
from .models import (ViTVAE, ViTVAEEncoder, load_vitvae_state_dict, extract_vit_latents, extract_vit_attention, extract_vit_saliency, extract_vit_relevance,   # noqa: F401
                     resize_pos_embedding, fit_latent, vit_vae_loss, train_vit_vae, vit_vae_train_step)
from .causal import AdapterMLP, CausalViTVAE   # noqa: F401
from .train import GraphedViTTrainStep, causal_vit_train_step   # noqa: F401
from .translator import (RidgeTranslator, fit_translator_ridge, fit_translator_ridge_cv, translate_vit_latents, compute_group_means, pairwise_contrasts, contrast_delta,   # noqa: F401
                         topk_features, bootstrap_feature_stability)
from .pca import LatentPCA, latent_pca, pca_vit_latents   # noqa: F401
from .tsne import LatentTSNE, latent_tsne, tsne_vit_latents   # noqa: F401

__all__ = ["ViTVAE", "ViTVAEEncoder", "load_vitvae_state_dict", "extract_vit_latents", "extract_vit_attention", "extract_vit_saliency", "extract_vit_relevance", "resize_pos_embedding", "fit_latent",
           "vit_vae_loss", "train_vit_vae", "vit_vae_train_step", "AdapterMLP", "CausalViTVAE", "GraphedViTTrainStep", "causal_vit_train_step",
           "RidgeTranslator", "fit_translator_ridge", "translate_vit_latents", "compute_group_means", "pairwise_contrasts", "contrast_delta", "topk_features",
           "bootstrap_feature_stability", "fit_translator_ridge_cv", "LatentPCA", "latent_pca", "pca_vit_latents",
           "LatentTSNE", "latent_tsne", "tsne_vit_latents"]

"""ViT-VAE encoder inference (the encoder half of the reference's ViTVAE, vessel_analysis/00_core/vit_backbone.py:50-179 and
latent_translator/models.py): image -> (mu, log_var) / CLS features, eval mode only."""
from .models import ViTVAEEncoder, load_vitvae_state_dict, extract_vit_latents, resize_pos_embedding   # noqa: F401

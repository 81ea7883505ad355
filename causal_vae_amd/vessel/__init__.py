from .train import loss_function, total_loss, train_step, train_one_epoch, validate   # noqa: F401
from .models import CausalVesselVAE               # noqa: F401
from .config import CONFIG                         # noqa: F401
from .analysis import feature_importance, ensemble_reconstruction, z_permutation_grid   # noqa: F401
from .images import prepare_vessel_images, prepare_translator_images   # noqa: F401

"""Projection of real images into the generator (reference: projection/projection.py)."""
from .noise_ops import noise_normalize_, noise_regularize          # noqa: F401
from .pca import GroupPCA, get_pca_groups          # noqa: F401
from .project import (get_avg_latent, get_lr, latent_noise, load_source_images, make_image, merge_group_latents,          # noqa: F401
                      project)

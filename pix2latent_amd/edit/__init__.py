"""pix2latent.edit: re-render a saved inversion with an edited class or z (reference pix2latent/edit)."""
from .editor import BigGANLatentEditor
from .ganspace import biggan_components

__all__ = ['BigGANLatentEditor', 'biggan_components']

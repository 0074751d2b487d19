"""pix2latent.edit: re-render a saved inversion with an edited class or z (reference pix2latent/edit), or,
for StyleGAN2, with its latent moved along a GANSpace direction of W."""
from .editor import BigGANLatentEditor, StyleGAN2LatentEditor
from .ganspace import biggan_components, stylegan2_components

__all__ = ['BigGANLatentEditor', 'StyleGAN2LatentEditor', 'biggan_components', 'stylegan2_components']

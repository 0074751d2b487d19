"""The reference's second name of color_transform.py (pix2latent/transform/transform_functions.py,
byte-identical there): the same classes."""
from .color_transform import (ColorTransform, HueTransform, GammaTransform, SaturationTransform,  # noqa: F401
                              BrightnessTransform, ContrastTransform, _negate, _invert)

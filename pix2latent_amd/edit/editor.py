"""BigGANLatentEditor (reference pix2latent/edit/editor.py): loads the `vars.npy` an inversion saved and
re-renders its best candidate with the class swapped or z moved along a GANSpace direction."""
import numpy as np
import torch

from ..model import BigGAN
from ..utils.checkpoint import load_result
from .ganspace import biggan_components

SWEEP_CHUNK = 18            # render_z_sweep: images per forward


class BigGANLatentEditor():
    def __init__(self, model=None):
        # (the reference sets self.model only when it builds the model itself)
        self.model = BigGAN().eval().cuda() if model is None else model

    def _device(self):
        return getattr(self.model, '_dev', torch.device('cuda'))

    def load_result(self, var_path):
        """ load optimized result """
        self._var = load_result(var_path)
        self._idx = np.argmin(self._var.loss[-1][1]['loss'])
        self._z = self._var.input.z.data[self._idx].unsqueeze(0).float().to(self._device())
        self._c = self._var.input.c.data[self._idx].unsqueeze(0).float().to(self._device())
        return

    def edit_class(self, cls_idx, alpha=1.0):
        """ edit class variable """
        c_orig = self._c
        c_edit = self.model.get_class_embedding(cls_idx)
        _c = (alpha * c_edit) + ((1.0 - alpha) * c_orig)

        with torch.no_grad():
            out = self.model(self._z, _c)[0]
        return out

    def _components(self):
        if not hasattr(self, 'components'):
            self.components = biggan_components(self.model, self._c)
        return self.components

    def edit_z(self, component, sigma):
        """ edit z-space using prinicipal component """
        u = self._components()[component:component + 1]

        with torch.no_grad():
            out = self.model(self._z + sigma * u, self._c)[0]
        return out

    def render_z_sweep(self, components, sigmas):
        """edit_z for every (component, sigma) pair, component-major: image i * len(sigmas) + j is
        edit_z(components[i], sigmas[j]), bit for bit (the generator is batch-invariant).  Rendered in
        batches of at most 18.  Returns [len(components) * len(sigmas), 3, 256, 256]."""
        U = self._components()
        zs = [self._z + s * U[k:k + 1] for k in components for s in sigmas]
        if not zs:
            return torch.empty(0, 3, 256, 256, device=self._device())
        z = torch.cat(zs)
        c = self._c.repeat(z.shape[0], 1)
        outs = []
        with torch.no_grad():
            for i in range(0, z.shape[0], SWEEP_CHUNK):
                outs.append(self.model(z[i:i + SWEEP_CHUNK], c[i:i + SWEEP_CHUNK]))
        return torch.cat(outs)

    def default(self):
        """ optimized result """
        with torch.no_grad():
            out = self.model(self._z, self._c)[0]
        return out

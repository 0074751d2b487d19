"""BigGANLatentEditor (reference pix2latent/edit/editor.py): loads the `vars.npy` an inversion saved and
re-renders its best candidate with the class swapped or z moved along a GANSpace direction.
StyleGAN2LatentEditor does the same for the StyleGAN2 results (z or w+ search): the latent moves along a
principal direction of W, in all layers or in some, or a single StyleSpace channel moves by a multiple of its spread
(`edit_s`; results of z, w+ and s search alike)."""
import numpy as np
import torch

from ..model import BigGAN
from ..utils.checkpoint import load_result
from .ganspace import biggan_components, stylegan2_components

SWEEP_CHUNK = 18            # render_z_sweep / render_w_sweep: images per forward
NOISE_SEED = 0              # StyleGAN2LatentEditor, z search: the seed of its fixed per-layer noise


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


class StyleGAN2LatentEditor():
    def __init__(self, model, style_samples=100000):
        """style_samples: how many mapped z the channel stds of edit_s are taken over (model.style_stats)"""
        self.model = model
        self.style_samples = style_samples

    def _device(self):
        return self.model._dev

    def load_result(self, var_path):
        """ load optimized result: the best candidate's latent as w+ [1, n_latent, 512] and its per-layer
        noises (list of [1, 1, h, w]).  z search: w = mapping(z) in every layer, and a noise list drawn once
        from a seeded CPU generator (the model draws fresh noise on every forward, which would change the
        image between two renders of one edit).  w+ search: the stored latent and its stored noises.  s search: the
        stored styles [1, S_total] and noises; there is no latent, so edit_w / render_w_sweep / default render from
        the styles.  Every result also leaves its styles (`model.styles` of the latent for z and w+) for edit_s. """
        model, dev = self.model, self._device()
        self._var = load_result(var_path)
        self._idx = np.argmin(self._var.loss[-1][1]['loss'])
        z = self._var.input.z.data[self._idx].detach().float().to(dev)
        n_latent = model._desc.n_latent
        with torch.no_grad():
            if model.search == 's':
                self._latent = None
                self._styles = z.reshape(1, model.n_styles).contiguous()
                flat = self._var.input.noises.data[self._idx].detach().float().to(dev)
                self._noises = [n.contiguous() for n in model.reshape_noise(flat.reshape(1, -1))]
                return
            if model.search == 'z':
                w = model.mapping(z.reshape(1, 512))
                self._latent = w.unsqueeze(1).expand(-1, n_latent, -1).contiguous()
                g = torch.Generator().manual_seed(NOISE_SEED)
                self._noises = [torch.randn(1, 1, s[-2], s[-1], generator=g).to(dev) for s in model.noise_shape]
            else:
                self._latent = z.reshape(1, n_latent, 512).contiguous()
                flat = self._var.input.noises.data[self._idx].detach().float().to(dev)
                self._noises = [n.contiguous() for n in model.reshape_noise(flat.reshape(1, -1))]
            self._styles = model.styles(self._latent)
        return

    def _components(self):
        if not hasattr(self, 'components'):
            self.components, self.stdev, self.mean = stylegan2_components(self.model)
        return self.components

    def _layers(self, layers):
        n_latent = self.model._desc.n_latent
        idx = list(range(n_latent)) if layers is None else [int(l) for l in layers]
        bad = [l for l in idx if not 0 <= l < n_latent]
        if bad:
            raise ValueError('layers must be in [0, %d), got %s' % (n_latent, bad))
        return idx

    def _edited(self, component, sigma, idx):
        """the latent with sigma * stdev[k] * components[k] added to the rows `idx`"""
        if self._latent is None:
            raise ValueError('an s-search result has no W latent to move: use edit_s')
        U = self._components()
        latent = self._latent.clone()
        latent[:, idx] = latent[:, idx] + sigma * self.stdev[component] * U[component]
        return latent

    def _render(self, latent):
        B = latent.shape[0]
        noises = [n.expand(B, -1, -1, -1) for n in self._noises]
        with torch.no_grad():
            return self.model.synthesis(latent, noises)

    def edit_w(self, component, sigma, layers=None):
        """ edit the latent along a principal direction of W in `layers` (indices in [0, n_latent); None:
        all of them) """
        return self._render(self._edited(component, sigma, self._layers(layers)))[0]

    def render_w_sweep(self, components, sigmas, layers=None):
        """edit_w for every (component, sigma) pair, component-major: image i * len(sigmas) + j is
        edit_w(components[i], sigmas[j], layers), bit for bit (the generator is batch-invariant).  Rendered
        in batches of at most 18.  Returns [len(components) * len(sigmas), 3, S, S]."""
        idx = self._layers(layers)
        S = self.model.im_res
        ws = [self._edited(k, s, idx) for k in components for s in sigmas]
        if not ws:
            return torch.empty(0, 3, S, S, device=self._device())
        w = torch.cat(ws)
        return torch.cat([self._render(w[i:i + SWEEP_CHUNK]) for i in range(0, w.shape[0], SWEEP_CHUNK)])

    # ---- StyleSpace: one channel of one layer
    def _style_std(self):
        if not hasattr(self, 'style_std'):
            self.style_mean, self.style_std = (t.float() for t in self.model.style_stats(num_samples=self.style_samples))
        return self.style_std

    def _style_index(self, layer, channel):
        """position of (layer, channel) in the flat style vector; `layer` counts `model.style_layout` (network
        order: the numbering of the StyleSpace paper)"""
        layout = self.model.style_layout
        if int(layer) != layer or not 0 <= layer < len(layout):
            raise ValueError('layer must be in [0, %d), got %s' % (len(layout), layer))
        e = layout[int(layer)]
        if int(channel) != channel or not 0 <= channel < e.channels:
            raise ValueError('channel of layer %d (%s) must be in [0, %d), got %s' % (layer, e.name, e.channels, channel))
        return e.offset + int(channel)

    def _edited_s(self, layer, channel, sigma):
        i = self._style_index(layer, channel)
        styles = self._styles.clone()
        styles[:, i] = styles[:, i] + sigma * self._style_std()[i]
        return styles

    def _render_s(self, styles):
        B = styles.shape[0]
        flat = torch.cat([n.reshape(1, -1) for n in self._noises], dim=1).expand(B, -1).contiguous()
        with torch.no_grad():
            return self.model.forward_s(styles, flat)

    def edit_s(self, layer, channel, sigma):
        """ move style channel `channel` of layer `layer` (index into model.style_layout) by sigma times the
        channel's std under the generator's prior (model.style_stats) """
        return self._render_s(self._edited_s(layer, channel, sigma))[0]

    def render_s_sweep(self, edits, sigmas):
        """edit_s for every ((layer, channel), sigma) pair, edit-major: image i * len(sigmas) + j is
        edit_s(*edits[i], sigmas[j]), bit for bit (the generator is batch-invariant).  Rendered in batches of at
        most SWEEP_CHUNK.  Returns [len(edits) * len(sigmas), 3, S, S]."""
        S = self.model.im_res
        ss = [self._edited_s(l, c, s) for (l, c) in edits for s in sigmas]
        if not ss:
            return torch.empty(0, 3, S, S, device=self._device())
        st = torch.cat(ss)
        return torch.cat([self._render_s(st[i:i + SWEEP_CHUNK]) for i in range(0, st.shape[0], SWEEP_CHUNK)])

    def default(self):
        """ optimized result """
        if self._latent is None:
            return self._render_s(self._styles)[0]
        return self._render(self._latent)[0]

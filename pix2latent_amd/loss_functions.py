"""Loss functions of the pix2latent hot path on the native MI355X path.

Host-side mirror of the reference file pix2latent/loss_functions.py: same names,
constructor arguments and `__call__(output, target, weight=None, loss_mask=None)`
signatures.  The weighted L1 + LPIPS-VGG16 combination used by every inversion
example (`ProjectionLoss`, reference loss_functions.py:86-100) runs as
`p2l_projloss_fwd/bwd` in libp2l_hip:

  * target features / resized weight maps are cached per (target, weight,
    loss_mask) identity instead of being recomputed each step (reference
    loss_functions.py:142 runs the perceptual net on the target every call);
  * bilinear upsampling of the five LPIPS maps followed by the weighted spatial
    sum is evaluated as a sum at tap resolution against the adjoint-resized
    weight map (exact identity; only summation order differs).

The weighted L2 pixel term (the StyleGAN2 projector's MSE; `ReconstructionLoss('l2')`,
`ProjectionLoss(pixel_loss='l2', pixel_weight=...)`) runs as `p2l_l2_loss_fwd/_bwd`
(csrc/p2l_pixel.hip).  The un-weighted variants, and CPU tensors, use
plain torch ops on the tensor's own device.
"""
import collections
import ctypes as C
import os
import warnings

import torch
from torch import nn

from . import _native as N
from . import lanes
from .utils import synthetic

LPIPS_SHIFT = (-.030, -.088, -.188)
LPIPS_SCALE = (.458, .448, .450)


def l1_loss(out, target):
    """ computes loss = | x - y |"""
    return torch.abs(target - out)


def l2_loss(out, target):
    """ computes loss = (x - y)^2 """
    return ((target - out) ** 2)


def invertibility_loss(ims, target_transform, transform_params, mask=None):
    """ MSE(ims - T^{-1}(T(ims))) (reference loss_functions.py:30-38) """
    if ims.size(0) == 1:
        ims = ims.repeat(len(transform_params), 1, 1, 1)
    transformed = target_transform(ims, transform_params)
    inverted = target_transform(transformed, transform_params, invert=True)
    if mask is None:
        return torch.mean((ims - inverted) ** 2, [1, 2, 3])
    return masked_l2_loss(ims, inverted, mask)


def _masked(fn, out, target, mask):
    if mask.size(0) == 1:
        mask = mask.repeat(out.size(0), 1, 1, 1)
    if target.size(0) == 1:
        target = target.repeat(out.size(0), 1, 1, 1)
    loss = fn(out, target)
    return torch.sum(loss * mask, [1, 2, 3]) / torch.sum(mask, [1, 2, 3])


def masked_l1_loss(out, target, mask):
    return _masked(l1_loss, out, target, mask)


def masked_l2_loss(out, target, mask):
    return _masked(l2_loss, out, target, mask)


def weight_regularization(orig_model, curr_model, reg='l1', weight_dict=None):
    """ reference loss_functions.py:64-83 (not on the hot path) """
    w = 1.0
    reg_loss = 0.0
    orig_state_dict = orig_model.state_dict()
    for param_name, curr_param in curr_model.named_parameters():
        if 'bn' in param_name:
            continue
        orig_param = orig_state_dict[param_name]
        if reg == 'l1':
            l = torch.abs(curr_param - orig_param).mean()
        elif reg == 'l2':
            l = ((curr_param - orig_param) ** 2).mean()
        elif reg == 'inf':
            l = torch.max(torch.abs(curr_param - orig_param))
        if weight_dict is not None:
            w = weight_dict[param_name]
        reg_loss += w * l
    return reg_loss


# ---------------------------------------------------------------------------
# StyleGAN2 noise regulariser (the projector's noise_regularize)
# ---------------------------------------------------------------------------
def _flat_noises(noises):
    """the reference's [B, T] variable, or the list of [B,1,h,w] maps `reshape_noise` makes of it"""
    if torch.is_tensor(noises):
        return noises
    return torch.cat([n.reshape(n.size(0), -1) for n in noises], 1)


def noise_regularize_torch(noises, noise_shape):
    """The definition in torch ops, on any device: per layer a pyramid of 2x2 means in fp32,
    ((a + b) + (c + d)) * 0.25, down to side 8; per level ax = mean n[y,x] n[y,x-1] and
    ay = mean n[y,x] n[y-1,x] with wrap-around, in fp64; R = sum of ax^2 + ay^2.  The CPU path of
    `noise_regularize` and the comparison point of tools/bench_noise_reg.py."""
    from . import ops
    noises = _flat_noises(noises)
    B = noises.size(0)
    total = torch.zeros(B, dtype=torch.float64, device=noises.device)
    off = 0
    for s in ops.noise_sizes(noise_shape):
        n = noises[:, off:off + s * s].reshape(B, s, s)
        off += s * s
        while True:
            d = n.double()
            ax = (d * torch.roll(d, 1, 2)).mean((1, 2))
            ay = (d * torch.roll(d, 1, 1)).mean((1, 2))
            total = total + ax * ax + ay * ay
            if s <= 8:
                break
            n = ((n[:, 0::2, 0::2] + n[:, 0::2, 1::2]) + (n[:, 1::2, 0::2] + n[:, 1::2, 1::2])) * 0.25
            s //= 2
    assert off == noises.size(1), 'noises is [B, sum res^2]'
    return total.float()


class _NoiseRegFn(torch.autograd.Function):
    """R [B] of noises [B, T] through p2l_sg2_noise_reg_fwd / _bwd.  The workspace is a tensor of this call,
    saved for the backward: nothing is shared between lanes or with a captured graph, nothing waits for the host."""

    @staticmethod
    def forward(ctx, noises, sizes):
        from . import ops
        x = noises.detach()
        loss, _, ws = ops.noise_reg_fwd(x, sizes)
        ctx.save_for_backward(x, ws)
        ctx.sizes = sizes
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gloss):
        from . import ops
        x, ws = ctx.saved_tensors
        return ops.noise_reg_bwd(x, ctx.sizes, ws, gloss.float().contiguous()), None


def noise_regularize(noises, noise_shape):
    """R [B] fp32: the sum over layers and pyramid levels of the squared mean products of horizontally and
    vertically adjacent noise pixels (wrap-around), differentiable in `noises` ([B, T], or the list of
    [B,1,h,w] maps).  Device tensors run the HIP kernels, CPU tensors `noise_regularize_torch`."""
    from . import ops
    noises = _flat_noises(noises)
    if not noises.is_cuda:
        return noise_regularize_torch(noises, noise_shape)
    if noises.dtype != torch.float32 or not noises.is_contiguous():
        noises = noises.float().contiguous()
    return _NoiseRegFn.apply(noises, ops.noise_sizes(noise_shape))


class NoiseRegularizer(object):
    """`weight * noise_regularize(noises)` per candidate: the `regularizer=` of the noise variable
    (`var_manager.register('noises', ..., regularizer=LF.NoiseRegularizer(model.noise_shape))`).
    `weight` defaults to the StyleGAN2 projector's 1e5."""

    def __init__(self, noise_shape, weight=1e5):
        from . import ops
        self.noise_shape = ops.noise_sizes(noise_shape)
        self.weight = float(weight)

    def graph_key(self):
        """what a captured step bakes in of this term (optimizer/base_optimizer.py `_graph_key`)"""
        return ('NoiseRegularizer', self.noise_shape, self.weight)

    def __call__(self, noises):
        return self.weight * noise_regularize(noises, self.noise_shape)


# ---------------------------------------------------------------------------
# Whitened-PCA prior on a latent: W+ / z / the class vector
# ---------------------------------------------------------------------------
EIG_FLOOR = 2.0 ** -40      # of the largest eigenvalue: below it an fp64 eigh cannot tell an eigenvalue from zero


def to_p_space(w):
    """x = 5 w where w < 0, else w: the inverse of the StyleGAN2 mapping network's last leaky ReLU (slope 0.2), in
    the dtype of w (5 w rounds in fp32; the prior's kernels form it in fp64, where it is exact).  -0.0 and 0 take
    slope 1"""
    return torch.where(w < 0, w * 5.0, w)


def _rows3(w):
    """[B, D] -> [B, 1, D]"""
    if w.dim() == 2:
        return w.unsqueeze(1)
    if w.dim() != 3:
        raise ValueError('the latent is [B, D] or [B, L, D], got %s' % (tuple(w.shape),))
    return w


def latent_prior_torch(w, basis, mean, layer_weights=None, p_space=True):
    """The definition in torch ops, on any device.  w [B, L, D] (or [B, D]: L = 1), basis A [K, D], mean [D],
    layer_weights [L] (None: 1 / L each):
        x = 5 w where p_space and w < 0, else w;  d = x - mean;  v = d A^T;  P[b] = sum_l a_l (1 / K) sum_k v[b,l,k]^2
    in fp64, rounded once to fp32.  The CPU path of `latent_prior` and the comparison point of
    tools/bench_latent_prior.py."""
    w = _rows3(w)
    B, L, D = w.shape
    A = torch.as_tensor(basis, dtype=torch.float64).to(w.device)
    m = torch.as_tensor(mean, dtype=torch.float64).to(w.device)
    if layer_weights is None:
        a = torch.full((L,), 1.0 / L, dtype=torch.float64, device=w.device)
    else:
        a = torch.as_tensor(layer_weights, dtype=torch.float64).to(w.device)
    if A.dim() != 2 or A.size(1) != D or m.shape != (D,) or a.shape != (L,):
        raise ValueError('latent_prior_torch: w %s, basis %s, mean %s, layer weights %s'
                         % (tuple(w.shape), tuple(A.shape), tuple(m.shape), tuple(a.shape)))
    x = w.double()
    if p_space:
        x = torch.where(w < 0, x * 5.0, x)
    v = (x - m) @ A.t()
    return (((v * v).sum(2) / A.size(0)) * a).sum(1).float()


class _LatentPriorFn(torch.autograd.Function):
    """P [B] of w [B, L, D] through p2l_latent_prior_fwd / _bwd.  The workspace (v, fp64) is a tensor of this call,
    saved for the backward: nothing is shared between lanes or with a captured graph, nothing waits for the host."""

    @staticmethod
    def forward(ctx, w, prior):
        from . import ops
        x = w.detach()
        basis, basis_t, mean, layer_w = prior._device_tensors(x.device, x.size(1))
        loss, ws = ops.latent_prior_fwd(x, basis_t, mean, layer_w, prior.p_space)
        ctx.save_for_backward(x, ws, basis, layer_w)
        ctx.p_space = prior.p_space
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gloss):
        from . import ops
        x, ws, basis, layer_w = ctx.saved_tensors
        return ops.latent_prior_bwd(x, basis, layer_w, ctx.p_space, ws, gloss.float().contiguous()), None


def latent_prior(w, prior):
    """P [B] fp32 of the latent w ([B, L, D] or [B, D]) under `prior` (a `LatentPrior`; its `weight` is NOT applied),
    differentiable in w.  Device tensors run the HIP kernels, CPU tensors `latent_prior_torch`."""
    if not w.is_cuda:
        return latent_prior_torch(w, prior.basis, prior.mean, prior.layer_weights, prior.p_space)
    shape = w.shape
    w = _rows3(w)
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    if w.size(2) != prior.dim or (prior.layer_weights is not None and w.size(1) != prior.layer_weights.numel()):
        raise ValueError('latent_prior: a latent %s under a prior of dimension %d%s'
                         % (tuple(shape), prior.dim, '' if prior.layer_weights is None
                            else ' with %d layer weights' % prior.layer_weights.numel()))
    return _LatentPriorFn.apply(w, prior)


class LatentPrior(object):
    """`weight * P(x)` per candidate, P the mean squared whitened coordinate of the latent:
        P[b] = sum_l a_l (1 / K) sum_k (A (x[b,l] - mean))_k^2,   A = Lambda_K^-1/2 V_K^T
    from the top K eigenpairs of a covariance, so that E[P] = 1 for latents of that distribution.  The
    `regularizer=` of a latent variable (`var_manager.register('z', ..., regularizer=LF.LatentPrior.stylegan2(model))`);
    with `p_space` the latent first goes back through the mapping network's last leaky ReLU (`to_p_space`): the
    P_N / P_N+ prior of Zhu et al., "Improved StyleGAN Embedding" (2020).  Built by one of the constructors below.

    basis [K, D], mean [D], layer_weights [L] or None (1 / L each, for whatever L the latent has) are fp64 on the
    CPU; the device copies (the basis in both orientations) are made once per device."""

    def __init__(self, basis, mean, weight=1.0, layer_weights=None, p_space=False, device='cuda'):
        import hashlib
        self.basis = torch.as_tensor(basis, dtype=torch.float64).cpu().contiguous()
        self.mean = torch.as_tensor(mean, dtype=torch.float64).cpu().contiguous()
        if self.basis.dim() != 2 or self.mean.shape != (self.basis.size(1),):
            raise ValueError('basis is [K, D] and mean [D], got %s and %s'
                             % (tuple(self.basis.shape), tuple(self.mean.shape)))
        self.num_components, self.dim = self.basis.shape
        if layer_weights is not None:
            layer_weights = torch.as_tensor(layer_weights, dtype=torch.float64).cpu().reshape(-1).contiguous()
        self.layer_weights = layer_weights
        self.weight = float(weight)
        self.p_space = bool(p_space)
        self.device = torch.device(device)
        h = hashlib.sha1(self.basis.numpy().tobytes())
        h.update(self.mean.numpy().tobytes())
        self._digest = h.hexdigest()
        self._on_device = {}
        if self.device.type == 'cuda' and torch.cuda.is_available():
            self._device_tensors(self.device, None)

    # ---- constructors
    @classmethod
    def from_covariance(cls, C, mean, num_components=None, weight=1.0, layer_weights=None, p_space=False,
                        device='cuda'):
        """C [D, D] and mean [D] of x (of `to_p_space(w)` when p_space).  The top `num_components` (None: all)
        eigenpairs of an fp64 `torch.linalg.eigh`; components with lambda_k < 2^-40 lambda_1 are dropped with a
        warning, and `num_components` above the kept rank is reduced to it."""
        C = torch.as_tensor(C, dtype=torch.float64).cpu()
        D = C.shape[0]
        if C.dim() != 2 or C.shape[1] != D:
            raise ValueError('C must be square, got %s' % (tuple(C.shape),))
        if num_components is not None and num_components < 1:
            raise ValueError('num_components must be at least 1, got %d' % num_components)
        lam, V = torch.linalg.eigh(C)
        lam, V = lam.flip(0), V.flip(1)
        if not lam[0] > 0:
            raise ValueError('the covariance has no positive eigenvalue')
        kept = int((lam >= EIG_FLOOR * lam[0]).sum())
        if kept < D:
            warnings.warn('LatentPrior: %d of %d components have an eigenvalue below 2^-40 of the largest and are '
                          'dropped' % (D - kept, D))
        K = kept if num_components is None else min(int(num_components), kept)
        basis = (V[:, :K] / lam[:K].sqrt()).t().contiguous()
        return cls(basis, mean, weight, layer_weights, p_space, device)

    @classmethod
    def from_samples(cls, x, num_components=None, weight=1.0, layer_weights=None, p_space=False, device='cuda'):
        """from samples x [N, D] (already in P space when p_space): mean and unbiased covariance in fp64"""
        x = torch.as_tensor(x).detach().double().cpu()
        if x.dim() != 2 or x.size(0) < 2:
            raise ValueError('samples are [N >= 2, D], got %s' % (tuple(x.shape),))
        N_, D = x.shape
        if N_ <= D:
            warnings.warn('LatentPrior.from_samples: %d samples of dimension %d: the covariance has rank %d at most'
                          % (N_, D, N_ - 1))
        mean = x.mean(0)
        xc = x - mean
        C = xc.t() @ xc / (N_ - 1)
        return cls.from_covariance(C, mean, num_components, weight, layer_weights, p_space, device)

    @classmethod
    def standard_normal(cls, dim, weight=1.0, device='cuda'):
        """identity basis, zero mean: P = |z|^2 / dim (BigGAN z, StyleGAN2 z)"""
        return cls(torch.eye(dim, dtype=torch.float64), torch.zeros(dim, dtype=torch.float64), weight, None, False,
                   device)

    @classmethod
    def stylegan2(cls, model, num_components=512, num_samples=100000, weight=1.0, layer_weights=None):
        """the P_N+ prior of a StyleGAN2: statistics of to_p_space(mapping(z)) from `num_samples` draws
        (`edit.ganspace.p_covariance`, z on the CPU generator), cached on the model per
        (num_components, num_samples)"""
        from .edit import ganspace
        cache = getattr(model, '_latent_prior_stats', None)
        if cache is None:
            cache = model._latent_prior_stats = {}
        key = (num_components, num_samples)
        if key not in cache:
            C, mean = ganspace.p_covariance(model, num_samples)
            base = cls.from_covariance(C, mean, num_components, 1.0, None, True, model._dev)
            cache[key] = (base.basis, base.mean)
        basis, mean = cache[key]
        return cls(basis, mean, weight, layer_weights, True, model._dev)

    # ----
    def _device_tensors(self, device, L):
        """(basis [K, D], basis_t [D, K], mean [D], layer weights [L] or None for L = None) fp64 on `device`"""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        for key in ((device, None), (device, L)):
            if key in self._on_device:
                continue
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('LatentPrior: first use on %s inside a graph capture; call it once eagerly' % device)
            if key[1] is None:
                b = self.basis.to(device)
                self._on_device[key] = (b, b.t().contiguous(), self.mean.to(device))
            elif self.layer_weights is None:
                self._on_device[key] = torch.full((L,), 1.0 / L, dtype=torch.float64).to(device)
            else:
                self._on_device[key] = self.layer_weights.to(device)
        return self._on_device[(device, None)] + (self._on_device.get((device, L)) if L is not None else None,)

    def graph_key(self):
        """what a captured step bakes in of this term (optimizer/base_optimizer.py `_graph_key`)"""
        lw = None if self.layer_weights is None else tuple(self.layer_weights.tolist())
        return ('LatentPrior', self.dim, self.num_components, lw, self.weight, self.p_space, self._digest)

    def __call__(self, x):
        return self.weight * latent_prior(x, self)


# ---------------------------------------------------------------------------
# Anchor of an optimised activation: the F of F/W+ inversion
# ---------------------------------------------------------------------------
def _anchor_shape_ok(f, anchor):
    return tuple(anchor.shape) in (tuple(f.shape[1:]), tuple(f.shape))


def feature_anchor_torch(f, anchor, weight=1.0):
    """The definition in torch ops, on any device.  f [B, ...], anchor of the shape of f[0] (shared by the candidates)
    or of f:   loss[b] = weight * (1 / n) * sum_i (f[b, i] - anchor[i])^2,  n = the elements of one candidate,
    in fp64, rounded once to fp32; differentiable in f.  The CPU path of `feature_anchor`."""
    anchor = torch.as_tensor(anchor).to(f.device)
    if not _anchor_shape_ok(f, anchor):
        raise ValueError('feature_anchor: f %s under an anchor %s' % (tuple(f.shape), tuple(anchor.shape)))
    d = (f.double() - anchor.double()).reshape(f.size(0), -1)
    return (float(weight) * ((d * d).sum(1) / d.size(1))).float()


class _FeatureAnchorFn(torch.autograd.Function):
    """loss [B] of f through p2l_feature_anchor_fwd / _bwd: the backward reads f and the anchor again, nothing is
    shared between lanes or with a captured graph, nothing waits for the host."""

    @staticmethod
    def forward(ctx, f, anchor, weight):
        from . import ops
        x = f.detach()
        ctx.save_for_backward(x, anchor)
        ctx.weight = weight
        return ops.feature_anchor_fwd(x, anchor, weight)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gloss):
        from . import ops
        x, anchor = ctx.saved_tensors
        return ops.feature_anchor_bwd(x, anchor, ctx.weight, gloss.float().contiguous()), None, None


def feature_anchor(f, anchor, weight=1.0):
    """loss [B] fp32 = weight * mean_i (f[b, i] - anchor[i])^2, differentiable in f ([B, ...]; anchor of the shape
    of f[0] or of f, fp32, on the device of f).  Device tensors run the HIP kernels, CPU tensors
    `feature_anchor_torch`."""
    if not f.is_cuda:
        return feature_anchor_torch(f, anchor, weight)
    if not _anchor_shape_ok(f, anchor):
        raise ValueError('feature_anchor: f %s under an anchor %s' % (tuple(f.shape), tuple(anchor.shape)))
    if anchor.device != f.device or anchor.dtype != torch.float32 or not anchor.is_contiguous():
        raise ValueError('feature_anchor: the anchor is a contiguous fp32 tensor on %s' % f.device)
    if f.dtype != torch.float32 or not f.is_contiguous():
        f = f.float().contiguous()
    return _FeatureAnchorFn.apply(f, anchor, float(weight))


class FeatureAnchor(object):
    """`weight * mean((F - anchor)^2)` per candidate: the `regularizer=` of an optimised activation
    (`var_manager.register('feat', ..., regularizer=LF.FeatureAnchor(feat0))`) -- the term ||F - F_init||^2 of the
    F/W+ space of BDInvert (Kang et al. 2021) and the FS space of Barbershop (Zhu et al. 2021), which keeps F near
    the activations of the W+ solution it started from.  `anchor` has the shape of one candidate ([C, r, r], shared)
    or of all of them ([B, C, r, r]).  A contiguous fp32 device tensor is read in place (no copy is made: writing to
    it changes the term, and its version is part of the graph key); anything else is copied to the device of F at
    its first use there, which therefore must not happen inside a graph capture."""

    def __init__(self, anchor, weight=1.0):
        self.anchor = torch.as_tensor(anchor).detach()
        self.weight = float(weight)
        self._on_device = {}

    def _device_anchor(self, device):
        a = self.anchor
        if a.device == device and a.dtype == torch.float32 and a.is_contiguous():
            return a
        key = (str(device), a.data_ptr(), a._version)
        if key not in self._on_device:
            if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('FeatureAnchor: first use on %s inside a graph capture; call it once eagerly'
                                   % device)
            self._on_device = {key: a.to(device, torch.float32).contiguous()}
        return self._on_device[key]

    def graph_key(self):
        """what a captured step bakes in of this term (optimizer/base_optimizer.py `_graph_key`): the anchor's
        address and version, the weight and the shape"""
        a = self.anchor
        return ('FeatureAnchor', a.data_ptr(), a._version, self.weight, tuple(a.shape))

    def __call__(self, f):
        return feature_anchor(f, self._device_anchor(f.device), self.weight)


# ---------------------------------------------------------------------------
# Diagonal prior on the StyleSpace variable
# ---------------------------------------------------------------------------
def style_prior_torch(x, center, scale, weight=1.0):
    """The definition in torch ops, on any device.  x [B, n], center [n], scale [n] (> 0):
        loss[b] = weight * (1 / n) * sum_i ((x[b, i] - center[i]) * (1 / scale[i]))^2
    in fp64, rounded once to fp32; differentiable in x.  The CPU path of `diag_prior`."""
    center = torch.as_tensor(center).to(x.device).double().reshape(-1)
    inv = 1.0 / torch.as_tensor(scale).to(x.device).double().reshape(-1)
    if x.dim() != 2 or center.numel() != x.size(1) or inv.numel() != x.size(1):
        raise ValueError('style_prior: x %s under a center of %d and a scale of %d channels'
                         % (tuple(x.shape), center.numel(), inv.numel()))
    d = (x.double() - center) * inv
    return (float(weight) * ((d * d).sum(1) / d.size(1))).float()


class _DiagPriorFn(torch.autograd.Function):
    """loss [B] of x through p2l_diag_prior_fwd / _bwd: the backward reads x, center and 1 / scale again, nothing is
    shared between lanes or with a captured graph, nothing waits for the host."""

    @staticmethod
    def forward(ctx, x, center, inv_scale, weight):
        from . import ops
        x = x.detach()
        ctx.save_for_backward(x, center, inv_scale)
        ctx.weight = weight
        return ops.diag_prior_fwd(x, center, inv_scale, weight)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gloss):
        from . import ops
        x, center, inv_scale = ctx.saved_tensors
        return ops.diag_prior_bwd(x, center, inv_scale, ctx.weight, gloss.float().contiguous()), None, None, None


def diag_prior(x, center, inv_scale, weight=1.0):
    """loss [B] fp32 = weight * mean_i ((x[b, i] - center[i]) * inv_scale[i])^2, differentiable in x [B, n]; center and
    inv_scale are contiguous fp64 [n] on the device of x.  Device tensors run the HIP kernels, CPU tensors
    `style_prior_torch` (with scale = 1 / inv_scale)."""
    if not x.is_cuda:
        return style_prior_torch(x, center, 1.0 / torch.as_tensor(inv_scale).double(), weight)
    n = x.size(1) if x.dim() == 2 else -1
    for t, what in ((center, 'center'), (inv_scale, 'inv_scale')):
        if t.device != x.device or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != n:
            raise ValueError('diag_prior: %s is a contiguous fp64 tensor of %d values on %s (x is %s)'
                             % (what, n, x.device, tuple(x.shape)))
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    return _DiagPriorFn.apply(x, center, inv_scale, float(weight))


class StylePrior(object):
    """`weight * mean_i (((S - center) / scale)_i^2)` per candidate: the `regularizer=` of the StyleSpace variable of
    `StyleGAN2(search='s')` (`var_manager.register('z', (model.n_styles,), ..., regularizer=LF.StylePrior.around(s0,
    model))`).  The 9 088 style channels are free once they no longer come from W+; the term keeps each within its
    own spread under the generator's prior (StyleSpace, Wu et al. 2021: channel statistics over mapped z).
    center [n] and scale [n] (> 0) are kept in fp64 on the CPU; the device copies (center and 1 / scale) are made at
    the first use on a device, which therefore must not happen inside a graph capture."""

    def __init__(self, center, scale, weight=1.0):
        import hashlib
        self.center = torch.as_tensor(center).detach().double().cpu().reshape(-1).contiguous()
        self.scale = torch.as_tensor(scale).detach().double().cpu().reshape(-1).contiguous()
        if self.center.numel() != self.scale.numel() or self.center.numel() < 1:
            raise ValueError('StylePrior: center and scale are [n], got %d and %d values'
                             % (self.center.numel(), self.scale.numel()))
        if not bool((self.scale > 0).all()) or not bool(torch.isfinite(self.scale).all()):
            raise ValueError('StylePrior: every scale is positive and finite (see min_std of the constructors)')
        self.weight = float(weight)
        h = hashlib.sha1(self.center.numpy().tobytes())
        h.update(self.scale.numpy().tobytes())
        self._digest = h.hexdigest()
        self._on_device = {}

    @staticmethod
    def _scale_of(model, num_samples, min_std):
        mean, std = model.style_stats(num_samples=num_samples)
        return mean, std.clamp(min=float(min_std))

    @classmethod
    def stylegan2(cls, model, num_samples=100000, weight=1.0, min_std=1e-3):
        """centred on the channel means of `model.style_stats(num_samples)` with the channel stds as scale: styles of
        mapped normal z score about `weight`.  A std below `min_std` takes that floor (a channel the affine leaves
        constant would divide by zero)."""
        mean, scale = cls._scale_of(model, num_samples, min_std)
        return cls(mean, scale, weight)

    @classmethod
    def around(cls, styles0, model, num_samples=100000, weight=1.0, min_std=1e-3):
        """centred on styles0 [S_total] (`model.styles` of a W+ solution) with the same scale: the distance from
        the start in units of each channel's spread"""
        _, scale = cls._scale_of(model, num_samples, min_std)
        return cls(torch.as_tensor(styles0).reshape(-1), scale, weight)

    def _device_tensors(self, device):
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._on_device:
            if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('StylePrior: first use on %s inside a graph capture; call it once eagerly' % device)
            self._on_device[device] = (self.center.to(device), (1.0 / self.scale).to(device))
        return self._on_device[device]

    def graph_key(self):
        """what a captured step bakes in of this term (optimizer/base_optimizer.py `_graph_key`)"""
        return ('StylePrior', self.center.numel(), self.weight, self._digest)

    def __call__(self, x):
        if not x.is_cuda:
            return style_prior_torch(x, self.center, self.scale, self.weight)
        if x.dim() != 2 or x.size(1) != self.center.numel():
            raise ValueError('StylePrior: x %s under a prior of %d channels' % (tuple(x.shape), self.center.numel()))
        center, inv = self._device_tensors(x.device)
        return diag_prior(x, center, inv, self.weight)


# ---------------------------------------------------------------------------
# `lpips_size`: the LPIPS term on an area-pooled image (the StyleGAN2 projector's 256^2)
# ---------------------------------------------------------------------------
POOL_FACTORS = (1, 2, 4, 8, 16)


def area_pool_torch(x, f):
    """pool_f(x) of x [..., H, W]: log2 f nested 2x2 means in fp32, each level ((a + b) + (c + d)) * 0.25 -- the
    cell order of `noise_regularize_torch`.  The definition in torch ops, on any device and for any channel count:
    the CPU path, and what the HIP kernels (csrc/p2l_pool.hip) are held to bit for bit."""
    f = int(f)
    H, W = x.shape[-2:]
    if f not in POOL_FACTORS or H % f or W % f:
        raise ValueError('area_pool_torch: factor %d on %s (a factor of %s that divides H and W)'
                         % (f, tuple(x.shape), POOL_FACTORS))
    x = x.float()
    while f > 1:
        x = ((x[..., 0::2, 0::2] + x[..., 0::2, 1::2]) + (x[..., 1::2, 0::2] + x[..., 1::2, 1::2])) * 0.25
        f //= 2
    return x


def lpips_pool_factor(shape, lpips_size):
    """f = H // lpips_size for an output of `shape` [B,3,H,W] (1 for lpips_size=None), or a ValueError that names
    the shapes: from shape arithmetic alone, before anything is launched"""
    if lpips_size is None:
        return 1
    s = int(lpips_size)
    H, W = int(shape[-2]), int(shape[-1])
    if s < 1 or H % s:
        raise ValueError('lpips_size=%d does not divide the height of the output %s' % (s, tuple(shape)))
    f = H // s
    if f not in POOL_FACTORS:
        raise ValueError('lpips_size=%d on an output %s is a pooling factor of %d: supported are %s'
                         % (s, tuple(shape), f, POOL_FACTORS))
    if W % f:
        raise ValueError('lpips_size=%d on an output %s: the pooling factor %d does not divide the width %d'
                         % (s, tuple(shape), f, W))
    return f


class _Pooled(object):
    """what a pooled loss keeps per (target, weight, loss_mask) chunk: pool_f(target), pool_f(weight * loss_mask),
    the full-resolution weight sum of the L1 term"""

    def __init__(self, target, weight, wsum, held):
        self.target, self.weight, self.wsum, self.held = target, weight, wsum, held
        self.guard = _StreamGuard().filled()


# ---------------------------------------------------------------------------
# native engine shared by Reconstruction / Perceptual / Projection losses
# ---------------------------------------------------------------------------
class _LpipsParams(object):
    """packed backbone + LPIPS-lin parameters of one network on the device.  A subclass names its descriptor
    struct and packs its backbone's weights into it (`_pack_backbone`); the scaling layer and the linear layers
    are the same for every network."""
    prefix, desc_cls, taps = None, None, 5

    def __init__(self, weights, device):
        self.lib = N.lib()
        self.dev = torch.device(device)
        self.keep = []
        d = self.desc = self.desc_cls()
        # d scaled / d img = 1/scale per input channel: folded into the first conv's input-gradient copy
        self._pack_backbone(d, weights, torch.tensor([1.0 / s for s in LPIPS_SCALE]).view(1, 3, 1, 1))
        for k in range(self.taps):
            d.lin[k] = self._t(weights['lpips.lin%d.weight' % k].reshape(-1))
        s16, t16 = torch.zeros(16), torch.zeros(16)
        for c in range(3):
            s16[c] = 1.0 / LPIPS_SCALE[c]
            t16[c] = -LPIPS_SHIFT[c] / LPIPS_SCALE[c]
        d.in_s = self._t(s16)
        d.in_t = self._t(t16)

    def _t(self, t):
        t = t.detach().to(self.dev, torch.float32).contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def _pack(self, w, taps, n_pad, k_pad, flip, fmt=None):
        if fmt is None:
            fmt = getattr(self, 'wfmt', N.WFMT_F32) if taps == 9 else N.WFMT_F32
        return self._packed(N.pack_conv_weight(w.detach().to(self.dev, torch.float32), taps, n_pad, k_pad, flip, fmt))

    def _gpack(self, w, taps, n_pad, k_pad, flip):
        return self._packed(N.pack_gconv_weight(w.detach().to(self.dev, torch.float32), taps, n_pad, k_pad, flip))

    def _packed(self, dst):
        torch.cuda.current_stream().synchronize()
        self.keep.append(dst)
        return dst.data_ptr()


class _VggLpipsParams(_LpipsParams):
    """VGG16 (P2LVggLpips)."""
    prefix, desc_cls = 'vgg', N.P2LVggLpips

    def _pack_backbone(self, d, weights, inv_scale):
        self.wfmt = N.default_wfmt()       # all 13 convs are 3x3
        thin = N.default_thin() and self.wfmt != N.WFMT_F32    # first conv: 3 real input channels
        d.wfmt = (self.wfmt | (N.WFMT_FLAG_THIN if thin else 0) |
                  (N.WFMT_FLAG_NO_AMAX if N.default_no_amax() else 0))
        for i, (cin, cout) in enumerate(synthetic.VGG_CONVS):
            w = weights['vgg.conv%d.weight' % i].float()
            if i == 0:
                f0 = N.WFMT_BF16X3T if thin else None
                d.w[i] = self._pack(w, 9, cout, 16, False, f0)
                d.wt[i] = self._pack(w * inv_scale, 9, 32, cout, True, f0)
            else:
                d.w[i] = self._pack(w, 9, cout, cin, False)
                d.wt[i] = self._pack(w, 9, cin, cout, True)
            d.b[i] = self._t(weights['vgg.conv%d.bias' % i])


class _AlexLpipsParams(_LpipsParams):
    """torchvision-AlexNet features (P2LAlexLpips)."""
    prefix, desc_cls = 'alex', N.P2LAlexLpips

    def _pack_backbone(self, d, weights, inv_scale):
        for i, (cin, cout, k) in enumerate(synthetic.ALEX_CONVS):
            w = weights['alex.conv%d.weight' % i].float()
            if i == 0:
                d.w[i] = self._pack(w, k * k, cout, 16, False)
                # direct input-gradient kernel: [k*k][3][cout]
                d.wt[i] = self._t((w * inv_scale).permute(2, 3, 1, 0).reshape(k * k, 3, cout))
            else:
                d.w[i] = self._pack(w, k * k, cout, cin, False)
                d.wt[i] = self._pack(w, k * k, cin, cout, True)
            d.b[i] = self._t(weights['alex.conv%d.bias' % i])


class _SqueezeLpipsParams(_LpipsParams):
    """torchvision-SqueezeNet1.1 features (P2LSqueezeLpips, csrc/p2l_plan_squeeze.hip)."""
    prefix, desc_cls, taps = 'squeeze', N.P2LSqueezeLpips, 7

    def _pack_backbone(self, d, weights, inv_scale):
        w = weights['squeeze.conv0.weight'].float()
        d.w0 = self._gpack(w, 9, 64, 16, False)
        d.b0 = self._t(weights['squeeze.conv0.bias'])
        d.wt0 = self._t((w * inv_scale).permute(2, 3, 1, 0).reshape(9, 3, 64))
        for i, (cin, sq, ex) in enumerate(synthetic.SQZ_FIRES):
            g = lambda part, what: weights['squeeze.fire%d.%s.%s' % (i, part, what)].float()
            # squeeze 1x1: output channels padded to one 64-wide tile (the launch stores `sq` of them)
            d.sq_w[i] = self._gpack(g('squeeze', 'weight'), 1, 64, cin, False)
            d.sq_b[i] = self._t(torch.cat([g('squeeze', 'bias').cpu(), torch.zeros(64 - sq)]))
            d.sq_wt[i] = self._gpack(g('squeeze', 'weight'), 1, cin, sq, True)
            d.e1_w[i] = self._gpack(g('expand1x1', 'weight'), 1, ex, sq, False)
            d.e1_b[i] = self._t(g('expand1x1', 'bias'))
            d.e1_wt[i] = self._gpack(g('expand1x1', 'weight'), 1, 64, ex, True)
            d.e3_w[i] = self._gpack(g('expand3x3', 'weight'), 9, ex, sq, False)
            d.e3_b[i] = self._t(g('expand3x3', 'bias'))
            d.e3_wt[i] = self._gpack(g('expand3x3', 'weight'), 9, 64, ex, True)


class _CacheSlot(object):
    """target-dependent state of one (target, weight, loss_mask) chunk."""

    def __init__(self, cache_floats, cache_cls, B, H, W, dev):
        taps = len(cache_cls().nft)
        nft_off = (C.c_size_t * taps)()
        wt_off = (C.c_size_t * taps)()
        wsum_off = C.c_size_t(0)
        n = cache_floats(B, H, W, nft_off, wt_off, C.byref(wsum_off))
        self.buf = torch.empty(n, device=dev, dtype=torch.float32)
        self.desc = cache_cls()
        base = self.buf.data_ptr()
        for k in range(taps):
            self.desc.nft[k] = base + 4 * nft_off[k]
            self.desc.wt[k] = base + 4 * wt_off[k]
        self.desc.wsum = base + 4 * wsum_off.value
        self.held = None
        self.B = B
        self.guard = _StreamGuard()
        self.last_use = {}           # stream -> event behind its latest forward / backward over this slot

    def used(self):
        """called behind every launch sequence that READS the slot (loss forward, loss backward)"""
        if torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
            st = torch.cuda.current_stream()
            self.last_use[st.cuda_stream] = st.record_event()

    def wait_for_readers(self):
        if torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
            st = torch.cuda.current_stream()
            for sid, ev in self.last_use.items():
                if sid != st.cuda_stream:
                    st.wait_event(ev)
        self.last_use = {}


class _StreamGuard(object):
    """Orders streams on a tensor that ONE stream filled and others read (lanes: the side streams of a step
    synchronise with the caller's stream, not with each other).  `filled()` records an event on the filling
    stream; `reader()` makes any OTHER stream wait for it once.  Inside a graph capture nothing is recorded:
    the memo entries and slots a captured step touches were made by the eager steps before it."""

    def __init__(self):
        self.event, self.seen = None, set()

    @staticmethod
    def _capturing():
        return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()

    def filled(self):
        if not torch.cuda.is_available():
            return self
        st = torch.cuda.current_stream()
        self.event = None if self._capturing() else st.record_event()
        self.seen = {st.cuda_stream}
        return self

    def reader(self):
        if self.event is None or not torch.cuda.is_available():
            return
        st = torch.cuda.current_stream()
        if st.cuda_stream not in self.seen and not self._capturing():
            st.wait_event(self.event)
            self.seen.add(st.cuda_stream)


# _LpipsParams.prefix -> (stem of *_ws_bytes / _prepare / _fwd / _bwd, its cache_floats, its cache struct)
_LOSS_ABI = {'vgg': ('p2l_projloss', 'p2l_loss_cache_floats', N.P2LLossCache),
             'alex': ('p2l_alexloss', 'p2l_alex_cache_floats', N.P2LLossCache),
             'squeeze': ('p2l_sqzloss', 'p2l_sqz_cache_floats', N.P2LLossCache7)}


class _LossEngine(object):
    """workspace + target caches for p2l_projloss_*; one per loss object.

    The cache is keyed on the identity (data_ptr, version, shape) of the target /
    weight / loss_mask tensors.  A population is evaluated in several chunks per
    step, each with its own slice of the per-sample targets, so several slots
    are kept (LRU): the VGG pass over the targets runs once per chunk and
    generation, not once per step as in the reference (loss_functions.py:142).
    """
    MAX_SLOTS = 8

    def __init__(self, vgg_params):
        self.lib = N.lib()
        self.vgg = vgg_params          # an _LpipsParams
        lib = self.lib
        self.prefix = getattr(vgg_params, 'prefix', 'vgg')     # None = L1-only engine
        stem, cache_floats, self.cache_cls = _LOSS_ABI[self.prefix]
        self.f_cache = getattr(lib, cache_floats)
        self.f_ws, self.f_prepare, self.f_fwd, self.f_bwd = (
            getattr(lib, stem + what) for what in ('_ws_bytes', '_prepare', '_fwd', '_bwd'))
        self.res = None          # (H, W) the caches were made at
        self._scratch = lanes.Scratch()      # arena + image staging per lane (one per stream)
        self.slots = {}          # key -> _CacheSlot (insertion order = LRU order; equal content shares a slot)
        self.keep = {}           # key -> the tensors it identifies (kept alive)
        self.cache = None        # P2LLossCache of the slot bound by the last prepare()
        self._memo = {}
        self._pooled = {}        # (idents of target / weight / loss_mask, f, want_l1) -> _Pooled, LRU order

    # per-lane scratch (the cached target features are shared: read-only while steps run)
    lanes_ok = True
    _lanes = property(lambda self: self._scratch.lanes)
    # what the current lane holds, for readers outside (oracle/replay.py, tools/): the engine fetches the record once
    ws = property(lambda self: self._scratch.here().ws)
    ws_bytes = property(lambda self: self._scratch.here().ws_bytes)
    img16 = property(lambda self: self._scratch.here().img16)
    dimg16 = property(lambda self: self._scratch.here().dimg16)
    shape = property(lambda self: None if self.img16 is None else tuple(self.img16.shape[:3]))

    def _ws_bytes(self, B, H, W):
        nbytes = self.f_ws(B, H, W)
        if nbytes == 0:
            raise N.NativeError('loss workspace sizing rejected shape %s' % ((B, H, W),))
        return nbytes

    def _alloc(self, B, H, W, dev):
        """the lane's workspace + image staging, sized for the LARGEST chunk seen at this resolution (a ragged
        last chunk, 32 samples = 9,9,9,5, alternates B every step)"""
        if self.res != (H, W):
            # resolution changed: caches are void, and so is every lane's scratch
            self.slots, self.keep, self.res = {}, {}, (H, W)
            self._scratch.clear()
        return self._scratch.grow(B, H, W, self._ws_bytes, dev)

    @staticmethod
    def _ident(t):
        return None if t is None else (t.data_ptr(), t._version, tuple(t.shape))

    @staticmethod
    def _conform(name, t, B, like):
        """the reference multiplies / subtracts these against output [B,3,H,W] with torch
        broadcasting (loss_functions.py:117-124,143-147): accept [H,W]-matching tensors with
        1 or 3 channels and 1 or B samples, and say so when they do not fit (the native
        kernels read 3*H*W floats per sample unconditionally)."""
        e = t
        if e.dim() == 3:
            e = e.unsqueeze(0)
        H, W = like.shape[2:]
        if e.dim() != 4 or tuple(e.shape[2:]) != (H, W) or e.size(1) not in (1, 3) or \
                e.size(0) not in (1, B):
            raise ValueError('%s of shape %s does not broadcast against the output %s'
                             % (name, tuple(t.shape), tuple(like.shape)))
        if e.size(0) != B or e.size(1) != 3:
            e = e.expand(B, 3, H, W)
        return e.contiguous().float()

    def bind(self, name, t, B, like=None):
        """-> contiguous fp32 [B,3,H,W] (None stays None, except `weight`), memoised on the
        source tensor's identity so that the target cache key stays stable."""
        if t is None:
            if name != 'weight':
                return None
            # reference returns an un-reduced map when weight is None; its only
            # consumer (closure.py:55) takes .view(b,-1).mean(1), which equals the
            # weighted form with unit weights.
            key = ('ones', B, tuple(like.shape[2:]), str(like.device))
            if self._memo.get(name, (None, None))[0] != key:
                self._memo[name] = (key, torch.ones(B, 3, like.size(2), like.size(3),
                                                    device=like.device), _StreamGuard().filled())
            # (filled on the stream of the lane that came first; the other lane's stream waits for it once)
            self._memo[name][2].reader()
            return self._memo[name][1]
        if t.dim() == 4 and tuple(t.shape) == (B, 3) + tuple(like.shape[2:]) and \
                t.is_contiguous() and t.dtype == torch.float32 and t.device == like.device:
            return t
        key = (self._ident(t), B)
        if self._memo.get(name, (None, None))[0] != key:
            self._memo[name] = (key, self._conform(name, t.to(like.device), B, like),
                                _StreamGuard().filled(), t)
        self._memo[name][2].reader()
        return self._memo[name][1]

    def _memoised(self, what, target, weight, loss_mask, make):
        """-> the _Pooled `make()` gave for these conformed tensors, memoised on their identity and version as
        `bind` does (key: the three identities + `what`; LRU, 2 * MAX_SLOTS entries).  The sources are kept alive in
        the entry: their data_ptr identifies them."""
        key = (self._ident(target), self._ident(weight), self._ident(loss_mask)) + what
        ent = self._pooled.pop(key, None)
        if ent is None:
            if len(self._pooled) >= 2 * self.MAX_SLOTS:
                self._pooled.pop(next(iter(self._pooled)))
            ent = make()
        else:
            ent.guard.reader()                 # (made on another lane's stream, perhaps in this very step)
        self._pooled[key] = ent
        return ent

    def _wsum(self, target, weight, loss_mask):
        B, HW3 = target.size(0), target[0].numel()
        wsum = torch.empty(B, device=target.device, dtype=torch.float32)
        N.check(self.lib.p2l_weight_sum(N.ptr(weight), N.ptr(loss_mask), N.ptr(wsum), B, HW3, N.stream()),
                'p2l_weight_sum')
        return wsum

    def pooled(self, target, weight, loss_mask, f, want_l1):
        """-> _Pooled of conformed full-resolution tensors: pooling runs once per chunk and generation, a step makes
        no new device tensors, and the cache slot of the pooled-size LPIPS term (keyed on the identity of the POOLED
        tensors) stays the same."""
        from . import ops
        held = (target, weight, loss_mask)

        def make():
            wsum = self._wsum(*held) if want_l1 else None
            return _Pooled(ops.area_pool_nchw(target, f), ops.area_pool_nchw(weight, f, mul=loss_mask), wsum, held)
        return self._memoised((f, want_l1), *held, make=make)

    def weight_sum(self, target, weight, loss_mask):
        """-> wsum [B] of conformed tensors (p2l_weight_sum), once per chunk and generation.  For a pixel term that
        runs without a cache slot."""
        held = (target, weight, loss_mask)
        return self._memoised(('wsum',), *held, make=lambda: _Pooled(None, None, self._wsum(*held), held)).wsum

    def read(self, slot):
        """behind the last launch of a loss forward / backward that READS `slot`: with a second lane its stream may
        be the one that evicts the slot (one stream: program order already protects an evicted slot)"""
        if len(self._lanes) > 1:
            slot.used()

    def _same_content(self, target, weight, loss_mask, use_lpips, B):
        """A generation of a CMA run starts from FRESH variables (reference base_cma_optimizer.py:79):
        new target / weight tensors with the old CONTENT; and the chunks of one population carry copies
        of the same default target.  Instead of running the LPIPS network over the targets again
        (round 5, tools/gen_overhead.py: the first step of a generation took 32 ms instead of 17), a slot
        whose tensors are unmodified since it was prepared and EQUAL to the new ones -- compared
        exactly, on the device, one host sync -- serves the new tensors too (a second key for the slot)."""
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            return None                                   # (no host sync inside a graph capture)
        seen = set()
        for old_key in reversed(list(self.slots)):
            slot = self.slots[old_key]
            if id(slot) in seen:
                continue
            seen.add(id(slot))
            if getattr(slot, 'use_lpips', None) != use_lpips or slot.B != B or slot.held is None:
                continue
            # `held` may be conformed copies another lane's stream made in this very step: ordered by the
            # event recorded behind that lane's prepare
            slot.guard.reader()
            differ = None
            for new, old, ver in zip((target, weight, loss_mask), slot.held, slot.versions):
                if (new is None) != (old is None):
                    differ = True
                    break
                if new is None:
                    continue
                if old._version != ver or new.shape != old.shape or new.device != old.device:
                    differ = True                      # (modified in place since: its old content is gone)
                    break
                if new.data_ptr() == old.data_ptr():
                    continue
                d = (new != old).any()
                differ = d if differ is None else (differ | d)
            if differ is True:
                continue
            if differ is None or not bool(differ):
                return slot
        return None

    def prepare(self, out, target, weight, loss_mask, use_lpips):
        B, _, H, W = out.shape
        s = self._alloc(B, H, W, out.device)
        key = (self._ident(target), self._ident(weight), self._ident(loss_mask), use_lpips)
        slot = self.slots.pop(key, None)
        if slot is None:
            slot = self._same_content(target, weight, loss_mask, use_lpips, B)
        if slot is None:
            if len(self.slots) >= self.MAX_SLOTS:
                lru = next(iter(self.slots))
                old = self.slots.pop(lru)                         # evict the LRU key ...
                self.keep.pop(lru, None)
                shared = any(v is old for v in self.slots.values())
                slot = old if (old.B == B and not shared) else None   # ... and reuse its memory
                if slot is not None:
                    # ... once every stream that read its features is done with them (another lane may
                    # still be inside the forward / backward that uses the evicted chunk's slot)
                    slot.wait_for_readers()
            if slot is None:
                slot = _CacheSlot(self.f_cache, self.cache_cls, B, H, W, out.device)
            vref = C.byref(self.vgg.desc) if use_lpips else None
            N.check(self.f_prepare(vref, N.ptr(target), N.ptr(weight), N.ptr(loss_mask), B, H, W,
                                   C.byref(slot.desc), N.ptr(s.ws), C.c_size_t(s.ws_bytes),
                                   N.stream()), 'p2l_%sloss_prepare' % self.prefix)
            # what the slot was prepared FROM (content comparisons), with the versions of that moment
            slot.held = (target, weight, loss_mask)
            slot.versions = tuple(None if t is None else t._version for t in slot.held)
            slot.use_lpips = use_lpips
            # another lane (stream) may be the next reader of these features
            slot.guard.filled()
        else:
            slot.guard.reader()                                    # (once per stream)
        if len(self.slots) >= 2 * self.MAX_SLOTS:                 # (keys, several may share a slot)
            lru = next(iter(self.slots))
            self.slots.pop(lru)
            self.keep.pop(lru, None)
        self.slots[key] = slot      # most recently used last
        # keep the key's tensors alive so that data_ptr identity stays meaningful
        self.keep[key] = (target, weight, loss_mask)
        self.cache = slot.desc
        return slot


def _channels(t):
    return None if t is None else (t.size(0) if t.dim() == 3 else t.size(1))


def _pixel_factor(weight, loss_mask):
    """Reference broadcasting quirk (loss_functions.py:119-123): with a ONE-channel `_weight = loss_mask * weight`
    the numerator sum(|t - o| * _weight) runs over the 3 image channels but the denominator sum(_weight) over one,
    i.e. the pixel term is 3x the 3-channel-weight value.  (The LPIPS map has one channel itself, so its term is
    not.)  -> 3 for a one-channel `weight * loss_mask`, else 1"""
    wc, mc = _channels(weight), _channels(loss_mask)
    return 3.0 if (wc == 1 and mc in (None, 1)) else 1.0


def _stale_error():
    return N.NativeError('loss workspace was reused by a later forward before '
                         'backward(); use one loss object per in-flight graph')


# What one call of `_ImageLossFn` runs (made once per call in `_apply`):
#   f         0 = no plan; else the plan runs at [H/f, W/f] (1: on the packed image, > 1: on the pooled one)
#   use_fwd, beta_fwd   `use_lpips` and `beta` of the plan's forward;  use_bwd, beta: of its backward
#   pixel     None | 'plan' (the L1 term the plan computes itself) | 'l1' | 'l2' (p2l_l1_/l2_loss_* beside it)
#   scale     weight of an 'l1' / 'l2' pixel term inside the Function: loss = scale * pixel + beta * lpips
# An 'l1' / 'l2' term beside a full-size plan (f = 1) reads the image the plan staged (img16), puts its block partials
# in `pix_part`, takes `wsum` from the slot's cache and ADDS its gradient into dimg16; otherwise (f = 0, f > 1) it
# stages the image itself (full16 / l1_part / dfull16 of `grow_full`) with the memoised full-size `wsum`.
_Form = collections.namedtuple('_Form', 'f use_fwd beta_fwd use_bwd beta pixel scale')


def _apply(eng, output, target, weight, loss_mask, beta, pixel, f=1, pixel_weight=1.0):
    """pixel_weight * (weighted `pixel` term, 'l1' | 'l2') + beta * (LPIPS term at [H/f, W/f]) [B] through the one
    native Function; pixel = None / beta = None: the other term alone.  The factor 3 of a one-channel weight
    (`_pixel_factor`) belongs to the pixel term: where the plan computes that term itself it takes beta / 3 and the
    result is multiplied by 3 out here, as a torch op that autograd sees."""
    B = output.size(0)
    k = _pixel_factor(weight, loss_mask)
    outside = 1.0
    if pixel is None:                      # LPIPS alone: the plan's L1 is switched off in the backward (use_lpips = 2)
        form = _Form(f, 1, float(beta), 2, float(beta), None, 1.0)
    elif beta is None and pixel == 'l2':   # no plan, no arena, no cache slot
        form, outside = _Form(0, 0, 0.0, 0, 0.0, 'l2', 1.0), k
    elif beta is None:                     # the plan without its network
        form, outside = _Form(1, 0, 0.0, 0, 0.0, 'plan', 1.0), k
    elif pixel == 'l1' and f == 1:
        form, outside = _Form(1, 1, float(beta) / k, 1, float(beta) / k, 'plan', 1.0), k
    else:                                  # the plan as the LPIPS term alone, the pixel term beside it
        form = _Form(f, 1, 1.0, 2, float(beta), pixel, float(pixel_weight) * k)
    loss = _ImageLossFn.apply(output, eng.bind('target', target, B, like=output),
                              eng.bind('weight', weight, B, like=output),
                              eng.bind('loss_mask', loss_mask, B, like=output), eng, form)
    return loss if outside == 1.0 else outside * loss


class _ImageLossFn(torch.autograd.Function):
    """Every native image loss: one sequence of optional steps over a `_Form`.  Forward: stage the image for the
    plan (pack, or pool + pack in one launch); the plan; stage the image at full size if the pixel term is not on
    the plan's buffer; the pixel term; combine.  Backward, the mirror: the plan; the pixel term; ONE unpack launch.

      form (chosen in the losses' __call__)        plan forward         pixel term                  plan backward  returns
      L1 + beta LPIPS, f = 1  (ProjectionLoss)     use_lpips 1, beta/k  the plan's own              1, beta/k      loss
      L1 alone (ReconstructionLoss 'l1')           use_lpips 0, NULL net  the plan's own            0              loss
      LPIPS alone, any f  (PerceptualLoss, a = 0)  use_lpips 1, beta    --                          2              lp
      L2 alone (ReconstructionLoss 'l2')           --                   l2 on full16, accumulate 0  --             l2
      a L2 + beta LPIPS, f = 1                     use_lpips 1, 1.0     l2 on img16, accumulate 1   2, beta        a k l2 + beta lp
      a L1|L2 + beta LPIPS, f > 1                  use_lpips 1, 1.0     l1|l2 on full16, acc. 0     2, beta        a k pix + beta lp

    (k = `_pixel_factor`, a = pixel_weight; a L1 with 0 < a != 1 is a * (L1 + (beta / a) LPIPS) in ProjectionLoss.)
    * The plan's forward has no LPIPS-only form: with a pixel term beside it, or pooled, it runs with use_lpips = 1
      and beta = 1, and its own L1 pass -- at full size in the fifth row -- is computed and discarded (DESIGN.md
      section 14); the backward's use_lpips = 2 writes d (beta * LPIPS) alone into dimg16.
    * L2 alone: stage the image (one launch), the weight sum once per (target, weight, loss_mask) identity, the
      kernels, unpack; the staging and the block partials are the lane's full-resolution scratch
      (`lanes.Scratch.grow_full`), no LPIPS arena is allocated.
    * L2 beside a full-size plan: on the image the plan staged, block partials in `pix_part`, the weight sum the one
      in the slot's cache; p2l_l2_loss_bwd adds the pixel term with gscale = a k g into dimg16.
    * f > 1: the engine's plan is allocated and prepared at the pooled size; the pixel term runs at full resolution,
      and the backward ends in ONE launch that writes d out = d pixel + expand_f(d LPIPS) / f^2.
    `eng.last_l1` is the pixel term of the last forward (the L2 value where that is the pixel term; the plan's
    by-product where there is none), `eng.last_lpips` the LPIPS term."""

    @staticmethod
    def forward(ctx, output, target, weight, loss_mask, eng, form):
        lib, f, pixel = eng.lib, form.f, form.pixel
        B, _, H, W = output.shape
        out_c = output.contiguous().float()
        new = lambda: torch.empty(B, device=output.device, dtype=torch.float32)
        slot = ent = wsum = loss = l1 = lp = None
        if f:
            # the plan, on the packed image (f = 1) or on the pooled one
            if f > 1:
                ent = eng.pooled(target, weight, loss_mask, f, pixel is not None)
                wsum, planned = ent.wsum, (ent.target, ent.weight, None)
                slot = eng.prepare(ent.target, *planned, 1)            # (first argument: shape and device)
            else:
                planned = (target, weight, loss_mask)
                slot = eng.prepare(out_c, *planned, form.use_fwd)
            s = eng._scratch.here()
            if f > 1:
                N.check(lib.p2l_area_pool3_to_nhwc16(N.ptr(out_c), N.ptr(s.img16), B, H, W, f, N.stream()),
                        'p2l_area_pool3_to_nhwc16')
            else:
                N.check(lib.p2l_nchw3_to_nhwc16(N.ptr(out_c), N.ptr(s.img16), B, H, W, N.stream()),
                        'p2l_nchw3_to_nhwc16')
            loss, l1, lp = new(), new(), new()
            # (the plan's own L1 term lands in `l1`: a by-product unless pixel == 'plan')
            N.check(eng.f_fwd(C.byref(eng.vgg.desc) if form.use_fwd else None, N.ptr(s.img16),
                              *map(N.ptr, planned), C.byref(slot.desc), N.f32(form.beta_fwd), form.use_fwd,
                              B, H // f, W // f, N.ptr(s.ws), C.c_size_t(s.ws_bytes), N.ptr(loss), N.ptr(l1),
                              N.ptr(lp), N.stream()), 'p2l_%sloss_fwd' % eng.prefix)
        if pixel in ('l1', 'l2'):
            nblk = getattr(lib, 'p2l_%s_loss_nblk' % pixel)(H, W)
            if f == 1:
                s = eng._scratch.grow_part(s.cap * nblk, output.device)
                img, part, wsum_p = s.img16, s.pix_part, C.c_void_p(slot.desc.wsum)
            else:
                if wsum is None:
                    wsum = eng.weight_sum(target, weight, loss_mask)
                s = eng._scratch.grow_full(B, H, W, nblk, output.device)
                N.check(lib.p2l_nchw3_to_nhwc16(N.ptr(out_c), N.ptr(s.full16), B, H, W, N.stream()),
                        'p2l_nchw3_to_nhwc16')
                img, part, wsum_p = s.full16, s.l1_part, N.ptr(wsum)
            l1 = new()
            N.check(getattr(lib, 'p2l_%s_loss_fwd' % pixel)(
                N.ptr(img), N.ptr(target), N.ptr(weight), N.ptr(loss_mask), wsum_p, N.ptr(l1), N.ptr(part),
                B, H, W, N.stream()), 'p2l_%s_loss_fwd' % pixel)
            if f:
                # loss = scale * l1 + beta * lp
                N.check(lib.p2l_vec_scale_div(N.ptr(l1), None, N.ptr(loss), B, N.f32(form.scale), N.stream()),
                        'p2l_vec_scale_div')
                N.check(lib.p2l_reduce_rows(N.ptr(lp), N.ptr(loss), B, 1, N.f32(form.beta), None, 1, N.stream()),
                        'p2l_reduce_rows')
        if f:
            eng.read(slot)
        ctx.eng, ctx.form, ctx.slot, ctx.ent, ctx.wsum = eng, form, slot, ent, wsum
        ctx.save_for_backward(out_c, target, weight, loss_mask if loss_mask is not None else torch.empty(0))
        ctx.has_mask = loss_mask is not None
        ctx.stamp = eng._scratch.stamp()
        eng.last_l1, eng.last_lpips = l1, lp
        return lp if pixel is None else loss if f else l1

    @staticmethod
    def backward(ctx, gloss):
        with lanes.use(ctx.stamp[0]):    # (autograd's thread: the scratch of the forward's lane)
            eng, form, slot, ent = ctx.eng, ctx.form, ctx.slot, ctx.ent
            lib, f, pixel = eng.lib, form.f, form.pixel
            out_c, target, weight, loss_mask = ctx.saved_tensors
            if not ctx.has_mask:
                loss_mask = None
            B, _, H, W = out_c.shape
            if eng._scratch.stale(ctx.stamp):
                raise _stale_error()
            s = eng._scratch.here()
            g = gloss.contiguous().float()
            beside = pixel in ('l1', 'l2')
            if f:
                planned = (ent.target, ent.weight, None) if f > 1 else (target, weight, loss_mask)
                N.check(eng.f_bwd(C.byref(eng.vgg.desc) if form.use_bwd else None, N.ptr(s.img16),
                                  *map(N.ptr, planned), C.byref(slot.desc), N.f32(form.beta), form.use_bwd,
                                  N.ptr(g), B, H // f, W // f, N.ptr(s.ws), C.c_size_t(s.ws_bytes), N.ptr(s.dimg16),
                                  N.stream()), 'p2l_%sloss_bwd' % eng.prefix)
            on_plan = beside and f == 1           # the pixel term reads the slot too (its wsum)
            if f and not on_plan:
                eng.read(slot)
            dpix = None
            if beside:
                gl = g if form.scale == 1.0 else g * form.scale
                img, dpix, wsum_p = (s.img16, s.dimg16, C.c_void_p(slot.desc.wsum)) if on_plan else \
                    (s.full16, s.dfull16, N.ptr(ctx.wsum))
                N.check(getattr(lib, 'p2l_%s_loss_bwd' % pixel)(
                    N.ptr(img), N.ptr(target), N.ptr(weight), N.ptr(loss_mask), wsum_p, N.ptr(gl), N.ptr(dpix),
                    B, H, W, 1 if on_plan else 0, N.stream()), 'p2l_%s_loss_bwd' % pixel)
                if on_plan:
                    eng.read(slot)
            dout = torch.empty(B, 3, H, W, device=out_c.device, dtype=torch.float32)
            if f > 1:
                N.check(lib.p2l_area_unpool16_add_nchw3(N.ptr(s.dimg16), N.ptr(dpix), N.ptr(dout), B, H, W, f,
                                                        N.stream()), 'p2l_area_unpool16_add_nchw3')
            else:
                N.check(lib.p2l_nhwc16_to_nchw3(N.ptr(s.dimg16 if f else dpix), N.ptr(dout), B, H, W, N.stream()),
                        'p2l_nhwc16_to_nchw3')
            return dout, None, None, None, None, None


_VGG_PARAMS = {}
# net -> (packed-parameter class, synthetic weights, loader of the upstream checkpoint pair)
_LPIPS_NETS = {'vgg': (_VggLpipsParams, 'lpips_vgg_weights', 'load_lpips_vgg'),
               'alex': (_AlexLpipsParams, 'lpips_alex_weights', 'load_lpips_alex'),
               'squeeze': (_SqueezeLpipsParams, 'lpips_squeeze_weights', 'load_lpips_squeeze')}


def _vgg_params(net, weights, device):
    """packed LPIPS network parameters: 'alex' (the reference default,
    loss_functions.py:87), 'vgg' (BASELINE north_star) or 'squeeze'.  A weight dict keyed 'alex.conv*' /
    'vgg.conv*' / 'squeeze.conv0*' selects the network by itself."""
    if weights is not None:
        net = ('alex' if 'alex.conv0.weight' in weights else
               'squeeze' if 'squeeze.conv0.weight' in weights else 'vgg')
    if net in ('vgg16',):
        net = 'vgg'
    if net not in _LPIPS_NETS:
        raise NotImplementedError("lpips_net='%s': LPIPS networks with a native path are "
                                  "'alex', 'vgg' and 'squeeze' (all three lpips v0.1 ships)" % net)
    params_cls, synth, loader = _LPIPS_NETS[net]
    key = (net, id(weights), str(device), N.default_wfmt(), N.default_no_amax())
    if key not in _VGG_PARAMS:
        if weights is None:
            path = os.environ.get('P2L_LPIPS_%s_WEIGHTS' % net.upper())
            if path and ',' in path:
                # the two upstream files: torchvision backbone state_dict, lpips v0.1 linear layers
                # (reference loss_functions.py:131 -> lpips.LPIPS(net=...))
                from .utils import checkpoint
                backbone, lin = (torch.load(f.strip(), map_location='cpu') for f in path.split(',')[:2])
                w = getattr(checkpoint, loader)(backbone, lin)
            elif path:
                w = torch.load(path, map_location='cpu')
            else:
                warnings.warn('LPIPS-%s: no pretrained weights available (no network); using '
                              'seeded random-init weights of the same architecture' % net)
                w = getattr(synthetic, synth)()
        else:
            w = weights
        _VGG_PARAMS[key] = params_cls(w, device)
    return _VGG_PARAMS[key]


def _native_ok(output, target, weight):
    return (output.is_cuda and output.dim() == 4 and output.size(1) == 3 and
            target is not None)


class ProjectionLoss(nn.Module):
    """ The default loss that is used in the paper (reference loss_functions.py:86-100).

    lpips_net: 'alex' (reference default), 'vgg' or 'squeeze'; all three are native HIP plans.
    lpips_size: None (the reference: LPIPS over the output as it is) or the height the output, the target and
        `weight * loss_mask` are area-pooled to in front of the LPIPS term, as the StyleGAN2 projector does with
        256 (`area_pool_torch`; the factor H // lpips_size is 1, 2, 4, 8 or 16).  The L1 term stays at full
        resolution.
    pixel_loss, pixel_weight: the loss is `pixel_weight * pixel term + beta * LPIPS term` with the weighted 'l1'
        (the reference) or 'l2' (the StyleGAN2 projector's MSE term) pixel term; both fixed at construction.
        `ProjectionLoss(lpips_net='vgg', beta=1, pixel_loss='l2', pixel_weight=mse, lpips_size=256)` is the
        projector's image loss.
    """

    def __init__(self, lpips_net='alex', beta=10, weights=None, device='cuda', lpips_size=None,
                 pixel_loss='l1', pixel_weight=1.0):
        super().__init__()
        if pixel_loss not in ('l1', 'l2'):
            raise ValueError("pixel_loss is 'l1' or 'l2', got %r" % (pixel_loss,))
        pixel_weight = float(pixel_weight)
        if not (0.0 <= pixel_weight < float('inf')):
            raise ValueError('pixel_weight must be finite and not negative, got %r' % (pixel_weight,))
        self.pixel_loss, self.pixel_weight = pixel_loss, pixel_weight
        self.beta = beta
        self.lpips_size = None if lpips_size is None else int(lpips_size)
        self._engine = _LossEngine(_vgg_params(lpips_net, weights, device))
        self.rloss_fn = ReconstructionLoss()
        self.ploss_fn = PerceptualLoss(net=lpips_net, weights=weights, device=device, lpips_size=lpips_size)
        return

    def __call__(self, output, target, weight=None, loss_mask=None):
        f = lpips_pool_factor(output.shape, self.lpips_size)
        eng, a = self._engine, self.pixel_weight
        if self.pixel_loss == 'l2':
            return _apply(eng, output, target, weight, loss_mask, self.beta, 'l2', f, a)
        if a == 1.0:
            return _apply(eng, output, target, weight, loss_mask, self.beta, 'l1', f)
        if a == 0.0:                            # the LPIPS term alone
            return self.beta * _apply(eng, output, target, weight, loss_mask, 1.0, None, f)
        # a * L1 + beta * LPIPS = a * (L1 + (beta / a) * LPIPS): the rescaling route of the factor 3
        return a * _apply(eng, output, target, weight, loss_mask, self.beta / a, 'l1', f)


class ReconstructionLoss(nn.Module):
    """ Reconstruction loss with spatial weighting (reference loss_functions.py:104-124) """

    def __init__(self, loss_type='l1'):
        super(ReconstructionLoss, self).__init__()
        if loss_type in ['l1', 1]:
            self.loss_fn = l1_loss
            self._native = True
        elif loss_type in ['l2', 2]:
            self.loss_fn = l2_loss
            self._native = True
        else:
            raise ValueError('Unknown loss_type {}'.format(loss_type))
        self._engine = None
        return

    def __call__(self, output, target, weight=None, loss_mask=None):
        if self._native and weight is not None and _native_ok(output, target, weight):
            if self._engine is None:
                self._engine = _LossEngine(None)
            pixel = 'l2' if self.loss_fn is l2_loss else 'l1'
            return _apply(self._engine, output, target, weight, loss_mask, None, pixel)
        loss = self.loss_fn(output, target)
        if weight is not None:
            _weight = weight if loss_mask is None else (loss_mask * weight)
            n = torch.sum(loss * _weight, [1, 2, 3])
            d = torch.sum(_weight, [1, 2, 3])
            loss = n / d
        return loss


class PerceptualLoss(nn.Module):
    """ LPIPS loss with spatial weighting (reference loss_functions.py:127-148); `lpips_size` as in
    ProjectionLoss: the LPIPS term of the area-pooled tensors """

    def __init__(self, net='vgg', use_gpu=True, weights=None, device='cuda', lpips_size=None):
        super(PerceptualLoss, self).__init__()
        self.lpips_size = None if lpips_size is None else int(lpips_size)
        self._engine = _LossEngine(_vgg_params(net, weights, device))
        return

    def __call__(self, output, target, weight=None, loss_mask=None):
        f = lpips_pool_factor(output.shape, self.lpips_size)
        return _apply(self._engine, output, target, weight, loss_mask, 1.0, None, f)

"""Colour transformations of the target: hue, gamma, saturation, brightness, contrast
(reference pix2latent/transform/color_transform.py, also importable under its second name
`transform_functions`).

The reference runs every candidate through PIL on the host: `(x + 1) / 2`, `mul(255).byte()`,
one torchvision PIL operation with `factor = float(t_i)`, `to_tensor` (`/ 255` in fp32) and
`2 * (y - 0.5)`.  Here the same result, float for float, comes from

  * device tensors: one fused HIP launch per chain of colour ops (`p2l_color_adjust`, plus one
    pre-pass per contrast op for the mean of the L image), each candidate with its own parameter
    read from device memory;
  * CPU tensors: the numpy restatement below of the integer rules of Pillow (derived by probing
    Pillow exhaustively, tools/make_color_golden.py) and of the torchvision wrappers.

Unlike the reference, which always returns `.cuda()`, the result stays on the input's device:
a CPU input gives a CPU result.  The result is detached (the reference's is; colour
transformations are not differentiable).  DESIGN.md section 8 states the exact semantics.
"""
import ctypes as C

import numpy as np
import torch

# op codes of p2l_color_adjust (include/p2l.h P2L_COLOR_*)
OP_BRIGHTNESS, OP_SATURATION, OP_CONTRAST, OP_GAMMA, OP_HUE = 0, 1, 2, 3, 4
_MAX_OPS = 8


# ---------------------------------------------------------------------------------------------
# host restatement of the integer rules (numpy on uint8 images [B, 3, H, W])
# ---------------------------------------------------------------------------------------------
def to_bytes(ims):
    """the reference's TVF.to_pil_image on (x + 1) / 2: fp32 `mul(255).byte()` (truncation; torch
    wraps out-of-range values modulo 256)"""
    return ((ims.detach().cpu().float() + 1.0) / 2.0).mul(255).byte().numpy()


def from_bytes(k):
    """TVF.to_tensor (fp32 / 255) then 2 * (y - 0.5)"""
    return 2.0 * (torch.from_numpy(np.ascontiguousarray(k)).float().div(255) - 0.5)


def luma(k):
    """PIL convert('L') of RGB bytes [..., 3, H, W] -> int32 [..., H, W]"""
    k = k.astype(np.int32)
    return (k[..., 0, :, :] * 19595 + k[..., 1, :, :] * 38470 + k[..., 2, :, :] * 7471 + 0x8000) >> 16


def blend(deg, img, alpha):
    """PIL Image.blend(deg, img, alpha) with alpha a float32: deg + alpha * (img - deg) in fp32,
    truncated; outside [0, 1] the fp32 value is clipped to [0, 255] first"""
    alpha = np.float32(alpha)
    deg = np.asarray(deg, dtype=np.int32)
    v = deg.astype(np.float32) + alpha * (np.asarray(img, dtype=np.int32) - deg).astype(np.float32)
    if not (0.0 <= alpha <= 1.0):
        v = np.clip(v, np.float32(0), np.float32(255))
    return v.astype(np.uint8)


def rgb_to_hsv(k):
    """PIL convert('HSV') of RGB bytes [..., 3, H, W] (Convert.c rgb2hsv: float, with the
    h / 6 + 1, fmod and * 255 steps in double) -> uint8 [..., 3, H, W]"""
    r, g, b = (k[..., i, :, :].astype(np.int32) for i in range(3))
    maxc = np.maximum(r, np.maximum(g, b))
    minc = np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = (maxc - minc).astype(np.float32)
    cr[grey] = 1
    s = cr / np.where(grey, 1, maxc).astype(np.float32)
    rc = (maxc - r).astype(np.float32) / cr
    gc = (maxc - g).astype(np.float32) / cr
    bc = (maxc - b).astype(np.float32) / cr
    h = np.where(r == maxc, (bc - gc).astype(np.float64),
                 np.where(g == maxc, 2.0 + rc.astype(np.float64) - bc,
                          4.0 + gc.astype(np.float64) - rc)).astype(np.float32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    uh[grey] = 0
    us[grey] = 0
    return np.stack([uh, us, maxc], axis=-3).astype(np.uint8)


def _round_half_away(v):
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5))


def hsv_to_rgb(k):
    """PIL convert('RGB') of HSV bytes [..., 3, H, W] (Convert.c hsv2rgb: double with float
    intermediates f, fs and fs * f, C round()) -> uint8 [..., 3, H, W]"""
    h, s, v = (k[..., i, :, :].astype(np.int32) for i in range(3))
    h6 = h.astype(np.float32).astype(np.float64) * 6.0 / 255.0
    i = np.floor(h6).astype(np.int32)
    f = (h6 - i).astype(np.float32)
    fs = (s.astype(np.float64) / 255.0).astype(np.float32)
    vd = v.astype(np.float64)
    p = _round_half_away(vd * (1.0 - fs.astype(np.float64)))
    q = _round_half_away(vd * (1.0 - (fs * f).astype(np.float64)))
    t = _round_half_away(vd * (1.0 - fs.astype(np.float64) * (1.0 - f.astype(np.float64))))
    p, q, t = (np.clip(a, 0, 255).astype(np.int32) for a in (p, q, t))
    sel = i % 6
    choices_r = [v, q, p, p, t, v]
    choices_g = [t, v, v, q, p, p]
    choices_b = [p, p, t, v, v, q]
    out = np.stack([np.choose(sel, choices_r), np.choose(sel, choices_g), np.choose(sel, choices_b)], axis=-3)
    grey = (s == 0)[..., None, :, :]
    out = np.where(grey, v[..., None, :, :], out)
    return out.astype(np.uint8)


def gamma_lut(gamma):
    """torchvision F_pil.adjust_gamma (gain 1): int((255 + 1 - 1e-3) * gain * pow(k / 255.0, gamma))
    with Python doubles, as bytes"""
    g = float(gamma)
    return np.array([int((255 + 1 - 1e-3) * 1 * pow(e / 255.0, g)) for e in range(256)], dtype=np.uint8)


def hue_shift(factor):
    """torchvision F_pil.adjust_hue: np.array(factor * 255).astype(np.uint8) -- truncation towards
    zero, negative values wrap modulo 256"""
    return int(float(factor) * 255) & 255


def host_op(op, k, f):
    """one torchvision PIL operation with factor f (a float32 value) on one uint8 image [3, H, W]"""
    f = np.float32(f)
    if op == OP_BRIGHTNESS:
        return blend(0, k, f)
    if op == OP_SATURATION:
        return blend(np.broadcast_to(luma(k)[None], k.shape), k, f)
    if op == OP_CONTRAST:
        L = luma(k)
        mean = int(float(L.sum(dtype=np.int64)) / L.size + 0.5)
        return blend(mean, k, f)
    if op == OP_GAMMA:
        return gamma_lut(f)[k]
    if op == OP_HUE:
        hsv = rgb_to_hsv(k)
        hsv[0] = (hsv[0].astype(np.int32) + hue_shift(f)) & 255
        return hsv_to_rgb(hsv)
    raise ValueError('unknown colour op %r' % (op,))


def host_chain(ims, ops, params):
    """the reference's chain of ColorTransform.apply calls on the host: ims [B,3,H,W] fp32,
    ops a list of op codes, params a list of [B] float32 arrays (already clamped)"""
    for op, p in zip(ops, params):
        k = to_bytes(ims)
        p = np.asarray(p, dtype=np.float32).reshape(-1)
        out = np.stack([host_op(op, k[b], p[b]) for b in range(k.shape[0])])
        ims = from_bytes(out)
    return ims


# ---------------------------------------------------------------------------------------------
# device path
# ---------------------------------------------------------------------------------------------
class P2LColorOp(C.Structure):
    """include/p2l.h P2LColorOp"""
    _fields_ = [('op', C.c_int32), ('reserved', C.c_int32), ('param', C.c_void_p), ('lut', C.c_void_p)]


class P2LColorChain(C.Structure):
    """include/p2l.h P2LColorChain"""
    _fields_ = [('size', C.c_size_t), ('n_ops', C.c_int32), ('reserved', C.c_int32),
                ('ops', P2LColorOp * _MAX_OPS)]


def native_chain(ops, params, B, device):
    """(P2LColorChain, tensors it points to) for `ops` with per-image params ([B] fp32 device tensors,
    already clamped).  Gamma needs its per-image LUT built on the host in double: one small
    device-to-host copy of its parameter."""
    assert 0 < len(ops) <= _MAX_OPS
    chain = P2LColorChain()
    chain.size = C.sizeof(P2LColorChain)
    chain.n_ops = len(ops)
    keep = []
    for j, (op, p) in enumerate(zip(ops, params)):
        p = p.detach().to(device=device, dtype=torch.float32).contiguous().view(-1)
        assert p.numel() == B, 'one parameter per image expected'
        keep.append(p)
        chain.ops[j].op = op
        chain.ops[j].param = p.data_ptr()
        if op == OP_GAMMA:
            lut = torch.from_numpy(np.stack([gamma_lut(g) for g in p.cpu().numpy()])).to(device)
            keep.append(lut)
            chain.ops[j].lut = lut.data_ptr()
    return chain, keep


def device_chain(ims, ops, params, out=None):
    """the chain in one native call: ims [B,3,H,W] on the device, params a list of [B] fp32 device
    tensors (already clamped); the result goes to `out` (may be `ims` itself) or a new tensor"""
    from .. import _native as N
    src = ims.detach().float().contiguous()
    B, Cn, H, W = src.shape
    if out is None:
        dst = torch.empty_like(src)
    else:
        assert out.shape == src.shape and out.dtype == torch.float32 and out.is_contiguous()
        dst = out.detach()
    chain, keep = native_chain(ops, params, B, src.device)
    L = N.lib()
    nbytes = L.p2l_color_adjust_ws_bytes(C.byref(chain), B)
    ws = torch.empty(max((nbytes + 7) // 8, 1), device=src.device, dtype=torch.int64)
    N.check(L.p2l_color_adjust(C.byref(chain), N.ptr(src), N.ptr(dst), B, Cn, H, W, C.c_void_p(ws.data_ptr()),
                               C.c_size_t(nbytes), N.stream()), 'p2l_color_adjust')
    del keep
    return dst


def apply_chain(ims, ops, params):
    """device tensors -> the HIP kernel; CPU tensors -> the host restatement"""
    if ims.is_cuda:
        return device_chain(ims, ops, params)
    return host_chain(ims, ops, [p.detach().cpu().float().numpy() for p in params])


# ---------------------------------------------------------------------------------------------
# the reference's public classes
# ---------------------------------------------------------------------------------------------
class ColorTransform(object):
    """
    Base class for color transformations. Any function that inherits this class
    is not differentiable. A differentiable version could be implemented but
    since we use BasinCMA we use the default PyTorch/PIL color transfomration.
    """

    def __init__(self, fn, t=[1], t_range=(0.667, 1.5), t_inv_fn=None,
                 optimize=True):
        """
        Args:
            fn: colour op code (OP_*) of this transformation
            t: Default starting parameter. This is used for initializing search
            t_range: A tuple that limits the transformation range (min, max)
            optimize: If trainable you returns the parameter
        """
        assert t_range[1] > t_range[0], 't_range should be increasing'
        self.fn = fn
        self.t = np.array(t, dtype=np.float32)
        self.t_inv_fn = t_inv_fn
        self.t_min, self.t_max = t_range
        self.is_spatial = False
        self.optimize = optimize
        return

    def get_opt_param(self):
        if self.optimize:
            return self.t
        return []

    def clamped(self, t, invert=False):
        """the per-image parameter [B] the op uses: t_inv_fn (on invert), then the clamp"""
        assert t.size(1) == 1
        if invert:
            t = self.t_inv_fn(t)
        return torch.clamp(t, self.t_min, self.t_max).reshape(-1).float()

    def apply(self, ims, t, invert=False):
        """ Applies transformation fn(im, t) -- NOT DIFFERENTIABLE """
        assert ims.size(0) == t.size(0)
        assert t.size(1) == 1
        return apply_chain(ims, [self.fn], [self.clamped(t, invert)])

    def __call__(self, ims, t, invert=False):
        return self.apply(ims, t, invert)

    def __str__(self):
        return 'ColorTransform: {}'.format(_OP_NAMES.get(self.fn, self.fn))


_OP_NAMES = {OP_HUE: 'adjust_hue', OP_BRIGHTNESS: 'adjust_brightness', OP_GAMMA: 'adjust_gamma',
             OP_SATURATION: 'adjust_saturation', OP_CONTRAST: 'adjust_contrast'}


class HueTransform(ColorTransform):
    def __init__(self, t=[0], t_min=-0.5, t_max=0.5):
        super().__init__(fn=OP_HUE,
                         t=t,
                         t_range=(t_min + 1e-6, t_max - 1e-6),
                         t_inv_fn=_negate)
        return


class BrightnessTransform(ColorTransform):
    def __init__(self, t=[1], t_min=0.667, t_max=1.5):
        super().__init__(fn=OP_BRIGHTNESS,
                         t=t,
                         t_range=(t_min, t_max),
                         t_inv_fn=_invert)
        return


class GammaTransform(ColorTransform):
    def __init__(self, t=[1], t_min=0.667, t_max=1.5):
        super().__init__(fn=OP_GAMMA,
                         t=t,
                         t_range=(t_min, t_max),
                         t_inv_fn=_invert)
        return


class SaturationTransform(ColorTransform):
    def __init__(self, t=[1], t_min=0.667, t_max=1.5):
        super().__init__(fn=OP_SATURATION,
                         t=t,
                         t_range=(t_min, t_max),
                         t_inv_fn=_invert)
        return


class ContrastTransform(ColorTransform):
    def __init__(self, t=[1], t_min=0.667, t_max=1.5):
        super().__init__(fn=OP_CONTRAST,
                         t=t,
                         t_range=(t_min, t_max),
                         t_inv_fn=_invert)
        return


#NOTE: Since lambda functions cant be pickled easily.
def _negate(x):
    return -x


def _invert(x):
    return 1.0 / x

"""Image helpers needed by the optimizers and the drop-in examples (subset of
reference pix2latent/utils/image.py: read :15-64, save :67-71, to_grid :74-76,
to_image :79-109, binarize :135-145, poisson_blend :183-209).  PIL / torch only: cv2
and torchvision are not available in this environment and are not needed for the hot
path; poisson_blend runs on the native Poisson solver instead of cv2.seamlessClone."""
import math
import warnings

import numpy as np
import torch
import torch.nn.functional as F


def make_grid(x, nrow=8, padding=2, pad_value=0.0):
    """[B,C,H,W] -> [C, rows*(H+pad)+pad, cols*(W+pad)+pad] collage with the
    layout of torchvision.utils.make_grid (which to_grid used in the reference)."""
    if x.dim() == 3:
        x = x.unsqueeze(0)
    B, C, H, W = x.shape
    if B == 1:
        return x[0]
    xmaps = min(nrow, B)
    ymaps = int(math.ceil(float(B) / xmaps))
    hh, ww = H + padding, W + padding
    grid = x.new_full((C, hh * ymaps + padding, ww * xmaps + padding), pad_value)
    k = 0
    for yy in range(ymaps):
        for xx in range(xmaps):
            if k >= B:
                break
            grid[:, yy * hh + padding: yy * hh + padding + H,
                 xx * ww + padding: xx * ww + padding + W] = x[k]
            k += 1
    return grid


def to_grid(x):
    grid_sz = int(np.ceil(np.sqrt(x.size(0))))
    return make_grid(x, grid_sz, pad_value=-1)


def to_image(output, to_cpu=True, denormalize=True, jpg_format=True,
             to_numpy=True, cv2_format=True):
    """ Formats torch tensor in the form BCHW -> BHWC """
    is_batched = True
    if len(list(output.size())) == 3:
        output = output.unsqueeze(0)
        is_batched = False
    tmp = output.detach().float()
    if to_cpu:
        tmp = tmp.cpu()
    tmp = tmp.permute(0, 2, 3, 1)
    if denormalize:
        tmp = (tmp + 1.0) / 2.0
    if jpg_format:
        tmp = (tmp * 255).int()
    if cv2_format and output.size(1) > 1:
        tmp = tmp[:, :, :, [2, 1, 0]]
    if to_numpy:
        tmp = tmp.numpy()
    if not is_batched:
        return tmp.squeeze(0)
    return tmp


def binarize(mask, min=0.0, max=1.0, eps=1e-3):
    """ used to convert continuous valued mask to binary mask """
    if type(mask) is torch.Tensor:
        assert mask.max() <= 1 + 1e-6, mask.max()
        assert mask.min() >= -1 - 1e-6, mask.min()
        mask = (mask > 1.0 - eps).float()
        return mask.clamp_(min, max)
    elif type(mask) is np.ndarray:
        mask = (mask > 1.0 - eps).astype(float)
        return np.clip(mask, min, max, out=mask)
    return False


def read(im_path, as_transformed_tensor=False, im_size=512, transform_style=None):
    """PIL-only version of the reference reader: Resize(short side, bilinear) ->
    CenterCrop -> [-1,1] ('biggan' / None), or pad-to-square -> Resize
    ('stylegan'/'stylegan2')."""
    from PIL import Image
    im = Image.open(im_path).convert('RGB')
    w, h = im.size
    if not as_transformed_tensor:
        return im
    if transform_style in ('stylegan', 'stylegan2'):
        side = max(h, w)
        canvas = Image.new('RGB', (side, side))
        canvas.paste(im, ((side - w) // 2, (side - h) // 2))
        im = canvas.resize((im_size, im_size), Image.BILINEAR)
    elif transform_style in (None, 'biggan'):
        if w <= h:
            nw, nh = im_size, int(im_size * h / w)
        else:
            nw, nh = int(im_size * w / h), im_size
        im = im.resize((nw, nh), Image.BILINEAR)
        left, top = int(round((nw - im_size) / 2.)), int(round((nh - im_size) / 2.))
        im = im.crop((left, top, left + im_size, top + im_size))
    else:
        raise ValueError(f'unknown transformation style {transform_style}')
    t = torch.from_numpy(np.asarray(im, dtype=np.uint8).copy()).permute(2, 0, 1).float() / 255.
    return (t - 0.5) / 0.5


def save(save_path, im):
    from PIL import Image
    if type(im) is torch.Tensor:
        im = to_image(im, cv2_format=False)
    Image.fromarray(np.asarray(im, dtype=np.uint8)).save(save_path)
    return True


def resize_area(img_uint8, factor):
    """HWC uint8 collage resize (replaces cv2.resize INTER_AREA in log_result)."""
    t = torch.from_numpy(np.asarray(img_uint8)).permute(2, 0, 1).unsqueeze(0).float()
    t = F.interpolate(t, scale_factor=factor, mode='area')
    return t[0].permute(1, 2, 0).round().byte().numpy()


def _poisson_mask(mask, B, H, W):
    """mask [H,W] | [1|B,H,W] | [1|B,1,H,W], any dtype -> uint8 [1|B,H,W] (> 0.5 = inside)"""
    if mask.dim() == 4:
        if mask.shape[1] != 1:
            raise ValueError('poisson_blend_tensors: a 4-d mask is [1|B, 1, H, W], got %s' % (tuple(mask.shape),))
        mask = mask[:, 0]
    elif mask.dim() == 2:
        mask = mask.unsqueeze(0)
    elif mask.dim() != 3:
        raise ValueError('poisson_blend_tensors: mask must be [H, W], [1|B, H, W] or [1|B, 1, H, W], got %s'
                         % (tuple(mask.shape),))
    if tuple(mask.shape[1:]) != (H, W) or mask.shape[0] not in (1, B):
        raise ValueError('poisson_blend_tensors: mask %s does not fit %d images of %d x %d'
                         % (tuple(mask.shape), B, H, W))
    if mask.dtype == torch.bool:
        return mask.to(torch.uint8).contiguous()
    return (mask > 0.5).to(torch.uint8).contiguous()


def poisson_blend_tensors(target, mask, generated, tol=1e-8, max_iter=None, return_info=False):
    """Seamless (Poisson) compositing of `generated` into `target` over `mask`, on the device.

    target [1|B,C,H,W] and generated [B,C,H,W] are device tensors in [-1, 1]; mask is [H,W],
    [1|B,1,H,W] or [1|B,H,W] of any dtype, > 0.5 meaning inside.  Per image and channel, with Omega =
    the masked pixels off the image's outermost one-pixel frame: the result is `target` outside Omega
    and clamp(generated + u, -1, 1) inside, where u solves the 5-point Laplace equation on Omega with
    Dirichlet data target - generated around it (this is the contract, not
    cv2.seamlessClone's bytes).  Conjugate gradients in fp64 (p2l_poisson_blend) until
    |r| <= tol |b| or `max_iter` iterations (default 10 * (H + W)).

    Returns [B,C,H,W] fp32, and warns when a system ended above `tol` (one small device-to-host copy).
    return_info=True returns (out, iters, relres) -- [B,C] int32 / fp64 device tensors -- and copies
    nothing to the host.  No CPU fallback: off-device inputs raise NativeError."""
    from .. import _native as N
    for name, v in (('target', target), ('mask', mask), ('generated', generated)):
        if not torch.is_tensor(v):
            raise TypeError('poisson_blend_tensors: %s must be a tensor' % name)
    if generated.dim() != 4 or target.dim() != 4:
        raise ValueError('poisson_blend_tensors: target and generated must be [B, C, H, W], got %s and %s'
                         % (tuple(target.shape), tuple(generated.shape)))
    B, Cn, H, W = generated.shape
    if tuple(target.shape[1:]) != (Cn, H, W) or target.shape[0] not in (1, B):
        raise ValueError('poisson_blend_tensors: target %s does not fit generated %s'
                         % (tuple(target.shape), tuple(generated.shape)))
    if B < 1 or Cn < 1 or H < 1 or W < 1:
        raise ValueError('poisson_blend_tensors: empty input %s' % (tuple(generated.shape),))
    m8 = _poisson_mask(mask, B, H, W)
    if max_iter is None:
        max_iter = 10 * (H + W)
    if not (tol >= 0) or max_iter < 0:
        raise ValueError('poisson_blend_tensors: tol %r, max_iter %r' % (tol, max_iter))
    dev = generated.device
    if dev.type != 'cuda' or target.device != dev or m8.device != dev:
        raise N.NativeError('poisson_blend_tensors runs on the HIP device only (no CPU fallback): target on %s, '
                            'mask on %s, generated on %s' % (target.device, mask.device, generated.device))
    L = N.lib()
    tgt = target.detach().float().contiguous()
    gen = generated.detach().float().contiguous()
    out = torch.empty_like(gen)
    iters = torch.empty(B, Cn, device=dev, dtype=torch.int32)
    relres = torch.empty(B, Cn, device=dev, dtype=torch.float64)
    nbytes = L.p2l_poisson_blend_ws_bytes(B, Cn, H, W)
    if nbytes == 0:
        raise ValueError('poisson_blend_tensors: %s is beyond what the solver indexes' % (tuple(generated.shape),))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        N.check(L.p2l_poisson_blend(tgt.data_ptr(), 0 if tgt.shape[0] == 1 else Cn * H * W,
                                    m8.data_ptr(), 0 if m8.shape[0] == 1 else H * W,
                                    gen.data_ptr(), out.data_ptr(), B, Cn, H, W, float(tol), int(max_iter),
                                    iters.data_ptr(), relres.data_ptr(), ws.data_ptr(), nbytes, N.stream()),
                'p2l_poisson_blend')
    if return_info:
        return out, iters, relres
    worst = float(relres.max())
    if worst > tol:
        warnings.warn('poisson_blend_tensors: conjugate gradients stopped after max_iter = %d iterations at a relative '
                      'residual of %.3g (tol %.3g)' % (max_iter, worst, tol), RuntimeWarning, stacklevel=2)
    return out


def _poisson_bytes(target, mask, generated):
    """the reference's range conventions: images H x W x 3 in 0..1 (a maximum <= 1) or 0..255 -> uint8
    (truncated, as its astype(np.uint8)); mask H x W x {1,3} in 0..1 or 0..255 -> bool [H, W] of its
    first channel, thresholded at half its range"""
    target, generated, mask = np.asarray(target), np.asarray(generated), np.asarray(mask)
    if target.ndim != 3 or target.shape[2] != 3 or generated.shape != target.shape:
        raise ValueError('poisson_blend: target and generated must both be H x W x 3, got %s and %s'
                         % (target.shape, generated.shape))
    if mask.ndim != 3 or mask.shape[:2] != target.shape[:2] or mask.shape[2] not in (1, 3):
        raise ValueError('poisson_blend: mask must be H x W x 1 or H x W x 3 over the same %d x %d pixels, got %s'
                         % (target.shape[0], target.shape[1], mask.shape))
    target, generated, mask = target.astype(np.float64), generated.astype(np.float64), mask.astype(np.float64)
    if np.max(target) <= 1.0:
        target = target * 255.
    if np.max(generated) <= 1.0:
        generated = generated * 255.
    if np.max(mask) > 1.0:
        mask = mask / 255.
    to_u8 = lambda x: np.clip(x, 0, 255).astype(np.uint8)
    return to_u8(target), mask[:, :, 0] > 0.5, to_u8(generated)


def _blend_device():
    from .. import _native as N
    if not torch.cuda.is_available():
        raise N.NativeError('poisson_blend runs on the HIP device only (no CPU fallback)')
    return torch.device('cuda', torch.cuda.current_device())


def poisson_blend(target, mask, generated):
    """Reference signature (pix2latent/utils/image.py:183): H x W x 3 arrays in 0..1 or 0..255, mask
    H x W x 1|3 in 0..1 or 0..255 -> the H x W x 3 uint8 composite.  The blend is
    poisson_blend_tensors' (the Poisson equation of DESIGN.md section 10 on the native solver, NOT
    cv2.seamlessClone byte for byte); channels are independent, so any channel order is fine."""
    t8, m, g8 = _poisson_bytes(target, mask, generated)
    dev = _blend_device()
    to_t = lambda a: (torch.from_numpy(a.astype(np.float32)).permute(2, 0, 1).unsqueeze(0) / 127.5 - 1.0).to(dev)
    out = poisson_blend_tensors(to_t(t8), torch.from_numpy(m).to(dev), to_t(g8))
    out = (out[0].permute(1, 2, 0).double().cpu().numpy() + 1.0) * 127.5
    return np.rint(np.clip(out, 0, 255)).astype(np.uint8)

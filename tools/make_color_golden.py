"""Writes tests/golden/color_transform.npz: the reference's colour transformations
(pix2latent/transform/color_transform.py) computed through Pillow and the torchvision PIL
wrappers restated below, on random and edge images, every op at its range ends, at its
identity and on both sides of Image.blend's branch at 1, negative hue, and two chains in
the order the reference's setup_transform_fn builds them.

Before writing, it checks the integer rules of pix2latent_amd.transform.color_transform
(the host restatement the HIP kernel follows) against Pillow EXHAUSTIVELY: convert('L')
and the HSV round trip over all 2^24 byte triples, Image.blend over all 256 x 256 byte
pairs at factors inside and outside [0, 1].

    python tools/make_color_golden.py [--probe-only]
"""
import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image, ImageEnhance, ImageStat  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pix2latent_amd.transform import color_transform as CT  # noqa: E402


# ---- the torchvision PIL wrappers the reference calls (torchvision/transforms/_functional_pil.py) ----
def tv_adjust_brightness(img, f):
    return ImageEnhance.Brightness(img).enhance(f)


def tv_adjust_saturation(img, f):
    return ImageEnhance.Color(img).enhance(f)


def tv_adjust_contrast(img, f):
    return ImageEnhance.Contrast(img).enhance(f)


def tv_adjust_gamma(img, gamma, gain=1):
    input_mode = img.mode
    img = img.convert('RGB')
    gamma_map = [int((255 + 1 - 1e-3) * gain * pow(ele / 255.0, gamma)) for ele in range(256)] * 3
    return img.point(gamma_map).convert(input_mode)


def tv_adjust_hue(img, hue_factor):
    assert -0.5 <= hue_factor <= 0.5
    input_mode = img.mode
    h, s, v = img.convert('HSV').split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over='ignore', invalid='ignore'):
        np_h += np.array(hue_factor * 255).astype(np.uint8)
    h = Image.fromarray(np_h, 'L')
    return Image.merge('HSV', (h, s, v)).convert(input_mode)


TV = {CT.OP_BRIGHTNESS: tv_adjust_brightness, CT.OP_SATURATION: tv_adjust_saturation,
      CT.OP_CONTRAST: tv_adjust_contrast, CT.OP_GAMMA: tv_adjust_gamma, CT.OP_HUE: tv_adjust_hue}


def pil_apply(ims, op, params):
    """the reference's ColorTransform.apply with already-clamped float32 params [B]: returns uint8 [B,3,H,W]"""
    x = (ims.detach().cpu() + 1.0) / 2.0
    out = []
    for im, p in zip(x, params):
        arr = np.transpose(im.mul(255).byte().numpy(), (1, 2, 0))          # TVF.to_pil_image
        y = TV[op](Image.fromarray(np.ascontiguousarray(arr), mode='RGB'), float(np.float32(p)))
        out.append(np.transpose(np.array(y, dtype=np.uint8), (2, 0, 1)))
    return np.stack(out)


def pil_chain(ims, ops, params):
    """the chain of ColorTransform.apply calls: the bytes of the last op (its output is from_bytes of them)"""
    for op, p in zip(ops, params):
        k = pil_apply(ims, op, p)
        ims = CT.from_bytes(k)
    return k


# ---- exhaustive probes ---------------------------------------------------------------------------
def all_triples():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255]).astype(np.uint8).reshape(3, 4096, 4096)


def probe():
    k = all_triples()
    img = Image.fromarray(np.ascontiguousarray(np.transpose(k, (1, 2, 0))), mode='RGB')
    L = np.array(img.convert('L'), dtype=np.int32)
    assert (CT.luma(k) == L).all(), 'convert(L)'
    print('convert(L): all 2^24 triples match')
    hsv = np.transpose(np.array(img.convert('HSV'), dtype=np.uint8), (2, 0, 1))
    mine = CT.rgb_to_hsv(k)
    bad = (mine != hsv).any(0)
    assert not bad.any(), ('rgb->hsv', int(bad.sum()), k[:, bad][:, :5].T, hsv[:, bad][:, :5].T, mine[:, bad][:, :5].T)
    print('RGB->HSV: all 2^24 triples match')
    back = Image.frombytes('HSV', img.size, np.ascontiguousarray(np.transpose(k, (1, 2, 0))).tobytes()).convert('RGB')
    back = np.transpose(np.array(back, dtype=np.uint8), (2, 0, 1))
    mine = CT.hsv_to_rgb(k)
    bad = (mine != back).any(0)
    assert not bad.any(), ('hsv->rgb', int(bad.sum()), k[:, bad][:, :5].T, back[:, bad][:, :5].T, mine[:, bad][:, :5].T)
    print('HSV->RGB: all 2^24 triples match')
    a = np.repeat(np.arange(256, dtype=np.uint8), 256).reshape(256, 256)
    b = np.tile(np.arange(256, dtype=np.uint8), 256).reshape(256, 256)
    ia, ib = Image.fromarray(a, 'L'), Image.fromarray(b, 'L')
    rng = np.random.RandomState(0)
    alphas = [0.0, 0.5, 0.667, 0.9, 1.0, 1.1, 1.5, 2.0, -0.25, 1e-6,
              np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))]
    alphas += list(rng.uniform(0.6, 1.0, 150)) + list(rng.uniform(1.0, 1.6, 150))
    for al in alphas:
        al = float(np.float32(al))
        ref = np.array(Image.blend(ia, ib, al), dtype=np.uint8)
        assert (CT.blend(a, b, al) == ref).all(), ('blend', al)
    print('Image.blend: all 256 x 256 byte pairs match at %d factors in and outside [0, 1]' % len(alphas))
    # the wrappers end to end on random images and parameters
    g = torch.Generator().manual_seed(11)
    ims = torch.rand(6, 3, 19, 29, generator=g) * 2 - 1
    for op, (lo, hi) in ((CT.OP_BRIGHTNESS, (0.667, 1.5)), (CT.OP_SATURATION, (0.667, 1.5)),
                         (CT.OP_CONTRAST, (0.667, 1.5)), (CT.OP_GAMMA, (0.667, 1.5)), (CT.OP_HUE, (-0.5, 0.5))):
        for _ in range(4):
            p = (torch.rand(6, generator=g) * (hi - lo) + lo).numpy()
            ref = CT.from_bytes(pil_apply(ims, op, p))
            assert torch.equal(ref, CT.host_chain(ims, [op], [p])), ('wrapper', op, p)
    print('wrappers: host restatement == Pillow on random images / parameters')


# ---- the golden ----------------------------------------------------------------------------------
RANGES = {CT.OP_HUE: (-0.5 + 1e-6, 0.5 - 1e-6), CT.OP_GAMMA: (0.667, 1.5), CT.OP_SATURATION: (0.667, 1.5),
          CT.OP_BRIGHTNESS: (0.667, 1.5), CT.OP_CONTRAST: (0.667, 1.5)}
NAMES = {CT.OP_HUE: 'hue', CT.OP_GAMMA: 'gamma', CT.OP_SATURATION: 'saturation',
         CT.OP_BRIGHTNESS: 'brightness', CT.OP_CONTRAST: 'contrast'}
CHAINS = {'chain5': [CT.OP_HUE, CT.OP_GAMMA, CT.OP_SATURATION, CT.OP_BRIGHTNESS, CT.OP_CONTRAST],
          'chain3': [CT.OP_HUE, CT.OP_SATURATION, CT.OP_CONTRAST]}


def param_values(op):
    lo, hi = (float(np.float32(v)) for v in RANGES[op])
    f = np.float32
    if op == CT.OP_HUE:
        return [lo, hi, 0.0, -0.1, 0.1, -0.25, 0.37, -1e-3, -0.4321, 0.2]
    return [lo, hi, 1.0, float(np.nextafter(f(1), f(0))), float(np.nextafter(f(1), f(2))), 0.9, 1.1, 0.75,
            1.3, 0.999]


def edge_images(H, W, g):
    """random, exact +-1, flat grey, saturated primaries, just below byte boundaries, to_tensor values"""
    out = [torch.rand(3, H, W, generator=g) * 2 - 1,
           torch.rand(3, H, W, generator=g) * 2 - 1,
           torch.where(torch.rand(3, H, W, generator=g) < 0.5, -torch.ones(3, H, W), torch.ones(3, H, W)),
           torch.zeros(3, H, W)]
    prim = torch.tensor([[1, -1, -1], [-1, 1, -1], [-1, -1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1],
                         [1, 1, 1], [-1, -1, -1]], dtype=torch.float32)
    idx = torch.randint(0, 8, (H, W), generator=g)
    out.append(prim[idx].permute(2, 0, 1).contiguous())
    # x whose (x + 1) / 2 * 255 lands just below the integer k, and the exact to_tensor outputs 2 (k/255 - 0.5)
    k = torch.randint(1, 256, (3, H, W), generator=g).float()
    x = 2.0 * (k / 255 - 0.5)
    out.append(torch.nextafter(x, torch.full_like(x, -2.0)))
    out.append(x)
    out.append(2.0 * (torch.randint(0, 256, (3, H, W), generator=g).float() / 255 - 0.5))
    # a smooth, strongly coloured image (hue wheel)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing='ij')
    out.append(torch.stack([torch.sin(3 * xx), torch.cos(2 * yy + xx), torch.sin(xx * yy * 4 + 1)]).float())
    return out


def make_set(name, n, H, W, g, res):
    base = edge_images(H, W, g)
    ims = torch.stack([base[i % len(base)] for i in range(n)])
    if n > len(base):      # extra random images beyond the edge set
        ims[len(base):] = torch.rand(n - len(base), 3, H, W, generator=g) * 2 - 1
    res['%s_ims' % name] = ims.numpy()
    for op in NAMES:
        vals = param_values(op)
        for r in range(3):
            p = np.array([vals[(b * 3 + r) % len(vals)] for b in range(n)], dtype=np.float32)
            res['%s_%s_%d_p' % (name, NAMES[op], r)] = p
            res['%s_%s_%d_out' % (name, NAMES[op], r)] = pil_apply(ims, op, p)
    for cname, ops in CHAINS.items():
        ps = []
        for j, op in enumerate(ops):
            lo, hi = RANGES[op]
            ps.append((torch.rand(n, generator=g) * (hi - lo) + lo).numpy().astype(np.float32))
        ps = np.stack(ps)
        ps[:, 0] = [param_values(op)[0] for op in ops]             # image 0: every op at its lower end
        res['%s_%s_p' % (name, cname)] = ps
        res['%s_%s_out' % (name, cname)] = pil_chain(ims, ops, list(ps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--probe-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'color_transform.npz'))
    a = ap.parse_args()
    probe()
    if a.probe_only:
        return
    import PIL
    g = torch.Generator().manual_seed(7)
    res = {'pillow_version': np.array(PIL.__version__),
           'chain5_ops': np.array(CHAINS['chain5'], dtype=np.int32),
           'chain3_ops': np.array(CHAINS['chain3'], dtype=np.int32)}
    make_set('a', 12, 16, 16, g, res)       # tiles exactly onto 256^2 and 1024^2
    make_set('b', 4, 37, 53, g, res)
    make_set('c', 22, 1, 1, g, res)
    np.savez_compressed(a.out, **res)
    print('wrote %s (%d KB)' % (a.out, os.path.getsize(a.out) // 1024))


if __name__ == '__main__':
    main()

"""Reference of the feature-space (F/W+) run of StyleGAN2 for tests/test_sg2_feature_gpu.py: the partial synthesis
composed from the oracle's public pieces (oracle/stylegan2_ref.py `styled_conv`, `to_rgb`, `_clamp`), walking
`convs.{2j}` / `convs.{2j+1}` / `to_rgbs.{j}` from the cut, and the decision tape of a native partial run for
`R.replay`.  Test infrastructure only."""
import math

import torch

from oracle import stylegan2_ref as R


def cut_of(res):
    """(l0, j0) of the cut at resolution res"""
    j0 = int(math.log2(res)) - 2
    return 2 * j0 + 1, j0


def features(W, latent, noises_flat, size, res):
    """(feat [B,C,r,r], skip [B,3,r,r]) of the oracle's full run: the output of the plain styled conv at `res` and the
    partial RGB there (the prefix of R.synthesis)"""
    noises = R.reshape_noise(noises_flat, size)
    _, j0 = cut_of(res)
    b = latent.shape[0]
    out = W['input.input'].repeat(b, 1, 1, 1)
    out = R.styled_conv(W, 'conv1', out, latent[:, 0], noises[0])
    skip = R.to_rgb(W, 'to_rgb1', out, latent[:, 1])
    i = 1
    for j in range(j0):
        out = R.styled_conv(W, 'convs.%d' % (2 * j), out, latent[:, i], noises[2 * j + 1], upsample=True)
        out = R.styled_conv(W, 'convs.%d' % (2 * j + 1), out, latent[:, i + 1], noises[2 * j + 2])
        skip = R.to_rgb(W, 'to_rgbs.%d' % j, out, latent[:, i + 2], skip)
        i += 2
    return out, skip


def forward_f(W, latent, noises_flat, feat, skip, size, res):
    """the suffix of R.forward_w from the cut on: reads latent[:, l0:], the noise maps of the convs >= l0, feat, skip"""
    noises = R.reshape_noise(noises_flat, size)
    l0, j0 = cut_of(res)
    out = feat
    i = l0
    for j in range(j0, int(math.log2(size)) - 2):
        out = R.styled_conv(W, 'convs.%d' % (2 * j), out, latent[:, i], noises[2 * j + 1], upsample=True)
        out = R.styled_conv(W, 'convs.%d' % (2 * j + 1), out, latent[:, i + 1], noises[2 * j + 2])
        skip = R.to_rgb(W, 'to_rgbs.%d' % j, out, latent[:, i + 2], skip)
        i += 2
    return R._clamp(skip)


def decisions(model, B, out, res):
    """the tape of the LAST native partial forward of `model` on B candidates, in the order forward_f takes the
    decisions: the leaky-ReLU signs of the styled convs l0 .. n_conv-1 (signs of the saved post-activation outputs)
    and which pixels the clamp let through (`out`: the image the native run returned)"""
    l0, _ = cut_of(res)
    items = [(model.saved_activation(l, B) > 0).permute(0, 3, 1, 2).contiguous().cpu()
             for l in range(l0, model._desc.n_conv)]
    items.append((out.detach().abs() < 1.0).cpu())
    return items

"""Reference of the StyleSpace (S) run of StyleGAN2 for tests/test_sg2_style_gpu.py: the synthesis composed from the
oracle's public pieces (oracle/stylegan2_ref.py `styled_conv`, `to_rgb`, `_clamp`) in network order -- conv1, to_rgb1,
then per resolution convs.{2j}, convs.{2j+1}, to_rgbs.{j} -- with one style row per layer.  The row reaches
`modulated_conv` in place of its affine's output: while the reference runs, `R.equal_linear` is a function that returns
the first cin columns of the row it is given (cin = the rows of the modulation weight); it is restored afterwards.
Test infrastructure only."""
import contextlib
import math

import torch

from oracle import stylegan2_ref as R


def layers(size):
    """[(prefix, kind, W+ row)] in network order"""
    out = [('conv1', 'conv', 0), ('to_rgb1', 'rgb', 1)]
    i = 1
    for j in range(int(math.log2(size)) - 2):
        out += [('convs.%d' % (2 * j), 'conv', i), ('convs.%d' % (2 * j + 1), 'conv', i + 1),
                ('to_rgbs.%d' % j, 'rgb', i + 2)]
        i += 2
    return out


def slices(W, size):
    """[(prefix, kind, row, offset, cin)]: a layer's place in the flat vector, from the weights alone"""
    out, off = [], 0
    for p, kind, row in layers(size):
        cin = W[p + '.conv.modulation.weight'].shape[0]
        out.append((p, kind, row, off, cin))
        off += cin
    return out


def styles(W, latent, size):
    """[B, S_total]: the oracle's own affines of the W+ rows, in network order"""
    return torch.cat([R.equal_linear(latent[:, row], W[p + '.conv.modulation.weight'], W[p + '.conv.modulation.bias'])
                      for p, _, row, _, _ in slices(W, size)], dim=1)


@contextlib.contextmanager
def _rows_for_affines():
    keep = R.equal_linear

    def take(x, weight, bias, lr_mul=1.0, activation=False):
        assert not activation                     # (the mapping network does not run here)
        return x[:, :weight.shape[0]]

    R.equal_linear = take
    try:
        yield
    finally:
        R.equal_linear = keep


def forward_s(W, styles_flat, noises_flat, size):
    """R.forward_w with every affine's output replaced by its slice of styles_flat [B, S_total]"""
    noises = R.reshape_noise(noises_flat, size)
    sl = {p: styles_flat[:, off:off + cin] for p, _, _, off, cin in slices(W, size)}
    b = styles_flat.shape[0]
    with _rows_for_affines():
        out = W['input.input'].repeat(b, 1, 1, 1)
        out = R.styled_conv(W, 'conv1', out, sl['conv1'], noises[0])
        skip = R.to_rgb(W, 'to_rgb1', out, sl['to_rgb1'])
        for j in range(int(math.log2(size)) - 2):
            p0, p1, pr = 'convs.%d' % (2 * j), 'convs.%d' % (2 * j + 1), 'to_rgbs.%d' % j
            out = R.styled_conv(W, p0, out, sl[p0], noises[2 * j + 1], upsample=True)
            out = R.styled_conv(W, p1, out, sl[p1], noises[2 * j + 2])
            skip = R.to_rgb(W, pr, out, sl[pr], skip)
        return R._clamp(skip)


def decisions(model, B, out):
    """the tape of the LAST native forward of `model` on B candidates, in the order forward_s takes the decisions: the
    leaky-ReLU signs of every styled conv (signs of the saved post-activation outputs) and which pixels the clamp let
    through (`out`: the image the native run returned) -- tests/_sg2_feature_ref.py `decisions` with l0 = 0"""
    items = [(model.saved_activation(l, B) > 0).permute(0, 3, 1, 2).contiguous().cpu()
             for l in range(model._desc.n_conv)]
    items.append((out.detach().abs() < 1.0).cpu())
    return items


def affine_transpose(W, dstyles, size, n_latent):
    """dstyles [B, S_total] pushed through the transposes of the affines, fp64 on the host: dW+ [B, n_latent, 512]"""
    d = dstyles.detach().double().cpu()
    out = torch.zeros(d.shape[0], n_latent, 512, dtype=torch.float64)
    for p, _, row, off, cin in slices(W, size):
        A = W[p + '.conv.modulation.weight'].double() * (1 / math.sqrt(512))      # s = w A^T + b
        out[:, row] += d[:, off:off + cin] @ A
    return out

"""Feature-space (F/W+) inversion of StyleGAN2, the part that needs no GPU: the arithmetic of the cut against the
oracle's layer tables, the host-side refusals of the new C entry points, and `LF.feature_anchor_torch` against a
numpy fp64 restatement."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWS = -1, -3
NEW_SYMBOLS = ['p2l_sg2_synthesis_from_fwd', 'p2l_sg2_synthesis_from_bwd', 'p2l_sg2_capture', 'p2l_nhwc_to_nchw',
               'p2l_nchw_to_nhwc', 'p2l_feature_anchor_ws_bytes', 'p2l_feature_anchor_fwd', 'p2l_feature_anchor_bwd']


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(ROOT, 'pix2latent_amd', 'libp2l_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from pix2latent_amd import _native as N
    return N.lib()


def legal_res(size):
    return [2 ** k for k in range(2, int(math.log2(size)))]


def desc(size, widths=None):
    """extents of the rosinality generator as model/stylegan2.py fills them (no device pointers)"""
    from pix2latent_amd import _native as N
    from pix2latent_amd.utils import synthetic as S
    ch = dict(S.sg2_channels(2))
    ch.update(widths or {})
    d = N.P2LStyleGAN2()
    log_size = int(math.log2(size))
    d.size, d.style_dim, d.n_latent = size, 512, 2 * log_size - 2
    d.n_conv, d.n_rgb = 2 * (log_size - 2) + 1, log_size - 1
    off = 0
    for l in range(d.n_conv):
        c = d.conv[l]
        c.res = 4 if l == 0 else 2 ** ((l + 1) // 2 + 2)
        c.up = int(l % 2 == 1)
        c.cin = ch[c.res // 2] if c.up else ch[c.res]
        c.cout = ch[c.res]
        c.latent_idx, c.noise_off = l, off
        off += c.res * c.res
    d.noise_total = off
    for j in range(d.n_rgb):
        r = d.rgb[j]
        r.res = 4 * 2 ** j
        r.cin, r.after_conv, r.latent_idx = ch[r.res], 2 * j, 2 * j + 1
    d.wfmt = 2
    return d


@pytest.mark.parametrize('size', [64, 512, 1024])
def test_feature_cut_against_the_oracle_tables(size):
    from pix2latent_amd.model.stylegan2 import StyleGAN2, feature_cut
    from pix2latent_amd.utils import synthetic as S
    from oracle import stylegan2_ref as R
    assert StyleGAN2.feature_cut is feature_cut             # (the class attribute works without a model or a device)
    shapes = R.noise_shapes(size)
    n_conv, n_latent = R.num_layers(size), R.n_latent(size)
    assert legal_res(size)[0] == 4 and legal_res(size)[-1] == size // 2
    d = desc(size)
    for r in legal_res(size):
        cut = StyleGAN2.feature_cut(size, r)
        k = int(math.log2(r))
        assert (cut.l0, cut.j0) == (2 * (k - 2) + 1, k - 2)
        assert 1 <= cut.l0 < n_conv
        # conv l0 - 1 is the plain conv at r, conv l0 the up conv to 2 r: their noise maps say so
        assert shapes[cut.l0 - 1][2:] == [r, r] and shapes[cut.l0][2:] == [2 * r, 2 * r]
        assert cut.C == R.channels()[r] == S.sg2_channels()[r]
        # the oracle's synthesis: conv l reads latent[:, l]; to_rgbs.{j} reads latent[:, 2 j + 3] and is ToRGB j + 1
        rows = set(range(cut.l0, n_conv)) | {2 * j + 3 for j in range(cut.j0, int(math.log2(size)) - 2)}
        assert cut.rows == sorted(rows) == list(range(cut.l0, n_latent))
        assert cut.noise_off == sum(s[2] * s[3] for s in shapes[:cut.l0])
        # ... and the descriptor the model fills agrees
        assert d.conv[cut.l0].up == 1 and d.conv[cut.l0 - 1].res == r and d.conv[cut.l0].cin == cut.C
        assert d.rgb[cut.j0].res == r and d.rgb[cut.j0].after_conv == cut.l0 - 1
        assert d.conv[cut.l0].noise_off == cut.noise_off
    assert StyleGAN2.feature_cut(64, 16, {16: 64}).C == 64


@pytest.mark.parametrize('size', [64, 512, 1024])
def test_illegal_resolutions_raise(size):
    from pix2latent_amd.model.stylegan2 import StyleGAN2
    for r in (3, 6, size, 2 * size, 0, -4, 2, 4.5):
        with pytest.raises(ValueError):
            StyleGAN2.feature_cut(size, r)


def test_symbols_and_version(lib):
    from pix2latent_amd import _native as N
    assert lib.p2l_version() == N.ABI_VERSION == 101
    hdr = open(os.path.join(ROOT, 'include', 'p2l.h')).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in N.EXPORTS and s + '(' in hdr, s


def test_entry_points_refuse_on_the_host(lib):
    """fake non-null pointers: everything below returns before a launch, so nothing is dereferenced and no device
    is needed"""
    d = desc(64)
    m, fake, B = C.byref(d), C.c_void_p(4096), 3
    ws_bytes = lib.p2l_sg2_ws_bytes(m, B)
    assert ws_bytes > 0
    big = C.c_size_t(ws_bytes)

    def fwd(res=16, feat=fake, skip=fake, lat=fake, nz=fake, Bn=B, ws=fake, nb=big, img=fake, mm=m):
        return lib.p2l_sg2_synthesis_from_fwd(mm, res, feat, skip, lat, nz, Bn, ws, nb, img, None)

    def bwd(res=16, lat=fake, nz=fake, Bn=B, ws=fake, nb=big, dimg=fake, dlat=fake, mm=m):
        return lib.p2l_sg2_synthesis_from_bwd(mm, res, lat, nz, Bn, ws, nb, dimg, dlat, None, None, None, None)

    def cap(res=16, Bn=B, ws=fake, nb=big, feat=fake, skip=fake, mm=m):
        return lib.p2l_sg2_capture(mm, res, Bn, ws, nb, feat, skip, None)

    for fn in (fwd, bwd, cap):
        for res in (3, 6, 64, 128, 0, -16, 2):
            assert fn(res=res) == EINVAL, (fn.__name__, res)
        assert fn(Bn=0) == EINVAL and fn(Bn=-2) == EINVAL
        assert fn(mm=None) == EINVAL
        assert fn(nb=C.c_size_t(ws_bytes - 4)) == EWS
        assert fn(nb=C.c_size_t(0)) == EWS
        assert fn(ws=None) == EWS
    for k in ('feat', 'skip', 'lat', 'nz', 'img'):
        assert fwd(**{k: None}) == EINVAL, k
    for k in ('lat', 'nz', 'dimg', 'dlat'):
        assert bwd(**{k: None}) == EINVAL, k
    for k in ('feat', 'skip'):
        assert cap(**{k: None}) == EINVAL, k
    # a descriptor whose layers do not sit where the cut expects them
    bad = desc(64)
    bad.conv[5].up = 0
    assert lib.p2l_sg2_synthesis_from_fwd(C.byref(bad), 16, fake, fake, fake, fake, B, fake, big, fake, None) == EINVAL
    # transposes
    for fn in (lib.p2l_nhwc_to_nchw, lib.p2l_nchw_to_nhwc):
        assert fn(None, fake, 1, 4, 4, 4, None) == EINVAL
        assert fn(fake, None, 1, 4, 4, 4, None) == EINVAL
        for bad_sizes in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0), (-1, 4, 4, 4), (65536, 4, 4, 4)):
            assert fn(fake, fake, *bad_sizes, None) == EINVAL, bad_sizes
    # the anchor term
    assert lib.p2l_feature_anchor_ws_bytes(3, 1) == 3 * 8
    assert lib.p2l_feature_anchor_ws_bytes(3, 4096) == 3 * 8 and lib.p2l_feature_anchor_ws_bytes(3, 4097) == 6 * 8
    assert lib.p2l_feature_anchor_ws_bytes(0, 16) == 0 and lib.p2l_feature_anchor_ws_bytes(2, 0) == 0
    assert lib.p2l_feature_anchor_ws_bytes(2, 2 ** 31) == 0
    n = 513
    nb = C.c_size_t(lib.p2l_feature_anchor_ws_bytes(3, n))

    def afwd(f=fake, a=fake, stride=0, Bn=3, n_=n, loss=fake, ws=fake, nb_=nb):
        return lib.p2l_feature_anchor_fwd(f, a, stride, Bn, n_, 1.0, loss, ws, nb_, None)

    def abwd(f=fake, a=fake, stride=0, Bn=3, n_=n, df=fake):
        return lib.p2l_feature_anchor_bwd(f, a, stride, None, Bn, n_, 1.0, df, None)

    for k in ('f', 'a', 'loss'):
        assert afwd(**{k: None}) == EINVAL, k
    for k in ('f', 'a', 'df'):
        assert abwd(**{k: None}) == EINVAL, k
    for fn in (afwd, abwd):
        assert fn(Bn=0) == EINVAL and fn(n_=0) == EINVAL and fn(stride=n - 1) == EINVAL and fn(stride=-1) == EINVAL
    assert afwd(ws=None) == EWS and afwd(nb_=C.c_size_t(nb.value - 8)) == EWS
    assert afwd(ws=C.c_void_p(4100)) == EWS                     # not 8-byte aligned


def anchor_numpy(f, a, weight, gloss=None):
    """loss[b] = weight (1 / n) sum_i (f[b,i] - a[i])^2 and dloss = gloss[b] (2 weight / n) (f - a), fp64"""
    B = f.shape[0]
    rows = B if a.shape == f.shape else 1                     # (n = 1, B = 1 never meet here)
    d = f.astype(np.float64).reshape(B, -1) - a.astype(np.float64).reshape(rows, -1)
    n = d.shape[1]
    loss = weight * (d * d).sum(1) / n
    g = np.ones(B) if gloss is None else np.asarray(gloss, dtype=np.float64)
    return loss, (g[:, None] * (2.0 * weight / n) * d).reshape(f.shape)


@pytest.mark.parametrize('shared', [True, False], ids=['shared', 'per-candidate'])
@pytest.mark.parametrize('n', [1, 63, 513, 8192])
def test_feature_anchor_torch_is_the_definition(n, shared):
    import pix2latent_amd.loss_functions as LF
    g = torch.Generator().manual_seed(n)
    B, weight = 3, 0.37
    shape = {1: (1, 1, 1), 63: (7, 3, 3), 513: (57, 3, 3), 8192: (32, 16, 16)}[n]
    f = torch.randn(B, *shape, generator=g)
    a = torch.randn(*shape, generator=g) if shared else torch.randn(B, *shape, generator=g)
    gloss = torch.tensor([1.0, 2.0, -1.0])
    fr = f.clone().requires_grad_(True)
    loss = LF.feature_anchor_torch(fr, a, weight)
    assert loss.dtype == torch.float32 and loss.shape == (B,)
    (loss * gloss).sum().backward()
    ref_loss, ref_grad = anchor_numpy(f.numpy(), a.numpy(), weight, gloss.numpy())
    # the two are the same fp64 expression up to the order of the sum: a few fp64 ulps in front of the rounding
    assert np.allclose(loss.detach().numpy().astype(np.float64), ref_loss, rtol=2e-7, atol=0)
    assert np.allclose(fr.grad.numpy().astype(np.float64), ref_grad, rtol=2e-7, atol=1e-30)
    # gloss scales the gradient: rows 1 and 2 against the unit row computed alone
    fr1 = f.clone().requires_grad_(True)
    LF.feature_anchor_torch(fr1, a, weight).sum().backward()
    assert torch.equal(fr.grad[0], fr1.grad[0])
    assert torch.equal(fr.grad[1], 2 * fr1.grad[1]) and torch.equal(fr.grad[2], -fr1.grad[2])
    # the class on CPU tensors is weight * that mean, and the CPU path of feature_anchor is this function
    reg = LF.FeatureAnchor(a, weight=weight)
    assert torch.equal(reg(f), LF.feature_anchor_torch(f, a, weight))
    assert torch.equal(LF.feature_anchor(f, a, weight), LF.feature_anchor_torch(f, a, weight))
    with pytest.raises(ValueError):
        LF.feature_anchor_torch(f, torch.zeros(2, 2), weight)


def test_feature_anchor_graph_key_follows_anchor_and_weight():
    import pix2latent_amd.loss_functions as LF
    a = torch.zeros(4, 2, 2)
    reg = LF.FeatureAnchor(a, weight=1.0)
    k0 = reg.graph_key()
    assert k0 == LF.FeatureAnchor(a, weight=1.0).graph_key()
    assert LF.FeatureAnchor(a, weight=2.0).graph_key() != k0
    assert LF.FeatureAnchor(a.clone(), weight=1.0).graph_key() != k0          # another address
    a.add_(1.0)                                                                  # same address, new version
    assert reg.graph_key() != k0
    reg.weight = 3.0
    assert reg.graph_key()[3] == 3.0

"""StyleSpace (S) search of StyleGAN2, the part that needs no GPU: the layout against the oracle's synthesis loop and
the descriptor, the host-side refusals of the new C entry points, and `LF.style_prior_torch` against a numpy fp64
restatement."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_sg2_feature import desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWS = -1, -3
NEW_SYMBOLS = ['p2l_sg2_style_layout', 'p2l_sg2_styles', 'p2l_sg2_synthesis_s_fwd', 'p2l_sg2_synthesis_s_bwd',
               'p2l_col_moments_f64', 'p2l_diag_prior_ws_bytes', 'p2l_diag_prior_fwd', 'p2l_diag_prior_bwd']
# the two width tables of tests/test_stylegan2_gpu.py (restated: that module is marked gpu as a whole)
WIDTHS = {'wide': None, 'narrow': {4: 128, 8: 128, 16: 64, 32: 32, 64: 32}}
CASES = [(64, 'wide'), (64, 'narrow'), (512, 'wide'), (1024, 'wide')]


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(ROOT, 'pix2latent_amd', 'libp2l_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from pix2latent_amd import _native as N
    return N.lib()


def oracle_order(size):
    """(layer name, W+ row) in the order R.synthesis runs the layers: its styled_conv / to_rgb replaced by recorders
    while it runs (no arithmetic, so this works at 1024^2), restored afterwards"""
    from oracle import stylegan2_ref as R
    calls = []
    keep = R.styled_conv, R.to_rgb

    class _Row(object):                       # latent[:, i] -> i
        def __getitem__(self, idx):
            return idx[1]

    def conv(W, p, x, style, noise, upsample=False):
        calls.append((p, 'conv', style))
        return x

    def rgb(W, p, x, style, skip=None):
        calls.append((p, 'rgb', style))
        return x

    class _Lat(_Row):
        shape = (1,)

    R.styled_conv, R.to_rgb = conv, rgb
    try:
        R.synthesis({'input.input': torch.zeros(1, 1, 4, 4)}, _Lat(), [None] * R.num_layers(size), size)
    finally:
        R.styled_conv, R.to_rgb = keep
    return calls


def test_symbols_and_version(lib):
    from pix2latent_amd import _native as N
    assert lib.p2l_version() == N.ABI_VERSION == 101
    hdr = open(os.path.join(ROOT, 'include', 'p2l.h')).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in N.EXPORTS and s + '(' in hdr, s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.p2l_diag_prior_ws_bytes.restype is C.c_size_t


@pytest.mark.parametrize('size,width', CASES, ids=['%d-%s' % c for c in CASES])
def test_style_layout_against_the_oracle_loop_and_the_descriptor(lib, size, width):
    from pix2latent_amd.model.stylegan2 import StyleGAN2, style_layout
    assert StyleGAN2.style_layout(size, WIDTHS[width]) == style_layout(size, WIDTHS[width])   # (no model, no device)
    layout = style_layout(size, WIDTHS[width])
    d = desc(size, WIDTHS[width])
    order = oracle_order(size)
    assert len(layout) == len(order) == d.n_conv + d.n_rgb
    off = 0
    seen = {'conv': 0, 'rgb': 0}
    for e, (name, kind, row) in zip(layout, order):
        assert (e.name, e.kind) == (name, kind)
        assert e.index == seen[kind]                                # each kind counts up in network order
        seen[kind] += 1
        assert e.offset == off                                      # contiguous
        layer = d.conv[e.index] if kind == 'conv' else d.rgb[e.index]
        assert e.channels == layer.cin and e.res == layer.res and layer.latent_idx == row
        off += e.channels
    total = off
    if width == 'wide':
        assert total == {64: 7168, 512: 8960, 1024: 9088}[size]
        n_rgb = sum(e.channels for e in layout if e.kind == 'rgb')
        assert (total - n_rgb, n_rgb) == {64: (4608, 2560), 512: (5952, 3008), 1024: (6048, 3040)}[size]
    # rgb[j] follows conv[rgb[j].after_conv]
    names = [(e.kind, e.index) for e in layout]
    for j in range(d.n_rgb):
        assert names.index(('rgb', j)) == names.index(('conv', d.rgb[j].after_conv)) + 1
    # the library's layout of the same descriptor
    co, ro, tot = (C.c_int32 * d.n_conv)(), (C.c_int32 * d.n_rgb)(), C.c_int32(-1)
    assert lib.p2l_sg2_style_layout(C.byref(d), co, ro, C.byref(tot)) == 0
    assert tot.value == total
    for e in layout:
        assert (co if e.kind == 'conv' else ro)[e.index] == e.offset
    assert lib.p2l_sg2_style_layout(C.byref(d), None, None, None) == 0


def test_style_layout_refuses_bad_sizes():
    from pix2latent_amd.model.stylegan2 import style_layout
    for size in (0, 4, 48, -64):
        with pytest.raises(ValueError):
            style_layout(size)


def test_entry_points_refuse_on_the_host(lib):
    """fake non-null pointers: everything below returns before a launch, so nothing is dereferenced and no device
    is needed"""
    d = desc(64)
    m, fake, B = C.byref(d), C.c_void_p(4096), 3
    ws_bytes = lib.p2l_sg2_ws_bytes(m, B)
    assert ws_bytes > 0
    big = C.c_size_t(ws_bytes)
    tot = C.c_int32(0)
    # layout
    assert lib.p2l_sg2_style_layout(None, None, None, C.byref(tot)) == EINVAL
    bad = desc(64)
    bad.rgb[2].after_conv = 99                               # a ToRGB that follows no conv
    assert lib.p2l_sg2_style_layout(C.byref(bad), None, None, C.byref(tot)) == EINVAL
    bad = desc(64)
    bad.conv[3].cin = 0
    assert lib.p2l_sg2_style_layout(C.byref(bad), None, None, C.byref(tot)) == EINVAL
    bad = desc(64)
    bad.n_conv = 0
    assert lib.p2l_sg2_style_layout(C.byref(bad), None, None, C.byref(tot)) == EINVAL

    def sty(mm=m, lat=fake, Bn=B, out=fake):
        return lib.p2l_sg2_styles(mm, lat, Bn, out, None)

    def fwd(mm=m, st=fake, nz=fake, Bn=B, ws=fake, nb=big, img=fake):
        return lib.p2l_sg2_synthesis_s_fwd(mm, st, nz, Bn, ws, nb, img, None)

    def bwd(mm=m, st=fake, nz=fake, Bn=B, ws=fake, nb=big, dimg=fake, dst=fake, dnz=None):
        return lib.p2l_sg2_synthesis_s_bwd(mm, st, nz, Bn, ws, nb, dimg, dst, dnz, None)

    for fn in (sty, fwd, bwd):
        assert fn(mm=None) == EINVAL
        assert fn(Bn=0) == EINVAL and fn(Bn=-2) == EINVAL
        assert fn(mm=C.byref(bad)) == EINVAL
    for k in ('lat', 'out'):
        assert sty(**{k: None}) == EINVAL, k
    for k in ('st', 'nz', 'img'):
        assert fwd(**{k: None}) == EINVAL, k
    for k in ('st', 'nz', 'dimg', 'dst'):
        assert bwd(**{k: None}) == EINVAL, k
    for fn in (fwd, bwd):
        assert fn(nb=C.c_size_t(ws_bytes - 4)) == EWS
        assert fn(nb=C.c_size_t(0)) == EWS
        assert fn(ws=None) == EWS
    # column moments
    def mom(x=fake, rows=7, cols=5, ld=5, s=fake, q=fake, acc=0):
        return lib.p2l_col_moments_f64(x, rows, cols, ld, s, q, acc, None)

    for k in ('x', 's', 'q'):
        assert mom(**{k: None}) == EINVAL, k
    assert mom(rows=0) == EINVAL and mom(rows=-1) == EINVAL and mom(cols=0) == EINVAL and mom(ld=4) == EINVAL
    assert mom(rows=2 ** 62, ld=8, cols=8) == EINVAL
    # the prior
    assert lib.p2l_diag_prior_ws_bytes(3, 1) == 3 * 8
    assert lib.p2l_diag_prior_ws_bytes(3, 4096) == 3 * 8 and lib.p2l_diag_prior_ws_bytes(3, 4097) == 6 * 8
    assert lib.p2l_diag_prior_ws_bytes(2, 9088) == 2 * 3 * 8
    assert lib.p2l_diag_prior_ws_bytes(0, 16) == 0 and lib.p2l_diag_prior_ws_bytes(2, 0) == 0
    assert lib.p2l_diag_prior_ws_bytes(2, 2 ** 31) == 0 and lib.p2l_diag_prior_ws_bytes(65536, 4) == 0
    n = 513
    nb = C.c_size_t(lib.p2l_diag_prior_ws_bytes(3, n))

    def pfwd(x=fake, c=fake, r=fake, Bn=3, n_=n, loss=fake, ws=fake, nb_=nb):
        return lib.p2l_diag_prior_fwd(x, c, r, Bn, n_, 1.0, loss, ws, nb_, None)

    def pbwd(x=fake, c=fake, r=fake, Bn=3, n_=n, dx=fake):
        return lib.p2l_diag_prior_bwd(x, c, r, None, Bn, n_, 1.0, dx, None)

    for k in ('x', 'c', 'r', 'loss'):
        assert pfwd(**{k: None}) == EINVAL, k
    for k in ('x', 'c', 'r', 'dx'):
        assert pbwd(**{k: None}) == EINVAL, k
    for fn in (pfwd, pbwd):
        assert fn(Bn=0) == EINVAL and fn(Bn=65536) == EINVAL and fn(n_=0) == EINVAL and fn(n_=2 ** 31) == EINVAL
    assert pfwd(ws=None) == EWS and pfwd(nb_=C.c_size_t(nb.value - 8)) == EWS
    assert pfwd(ws=C.c_void_p(4100)) == EWS                     # not 8-byte aligned


def prior_numpy(x, center, scale, weight, gloss=None):
    """loss[b] = weight (1 / n) sum_i ((x[b,i] - c[i]) / s[i])^2 and its gradient times gloss[b], fp64"""
    d = (x.astype(np.float64) - center[None]) / scale[None]
    n = d.shape[1]
    g = np.ones(x.shape[0]) if gloss is None else np.asarray(gloss, dtype=np.float64)
    return weight * (d * d).sum(1) / n, g[:, None] * (2.0 * weight / n) * d / scale[None]


@pytest.mark.parametrize('n', [1, 63, 513, 4097, 9088])
def test_style_prior_torch_is_the_definition(n):
    import pix2latent_amd.loss_functions as LF
    g = torch.Generator().manual_seed(n)
    B, weight = 3, 0.37
    x = torch.randn(B, n, generator=g)
    center = torch.randn(n, generator=g).double()                  # (fp32 values: x can sit on the centre)
    scale = torch.rand(n, generator=g, dtype=torch.float64) + 0.05
    gloss = torch.tensor([1.0, 2.0, -1.0])
    xr = x.clone().requires_grad_(True)
    loss = LF.style_prior_torch(xr, center, scale, weight)
    assert loss.dtype == torch.float32 and loss.shape == (B,)
    (loss * gloss).sum().backward()
    ref_loss, ref_grad = prior_numpy(x.numpy(), center.numpy(), scale.numpy(), weight, gloss.numpy())
    # the same fp64 expression up to the order of the sum and 1 / s: a few fp64 ulps in front of the rounding
    assert np.allclose(loss.detach().numpy().astype(np.float64), ref_loss, rtol=2e-7, atol=0)
    assert np.allclose(xr.grad.numpy().astype(np.float64), ref_grad, rtol=2e-7, atol=1e-30)
    x1 = x.clone().requires_grad_(True)
    LF.style_prior_torch(x1, center, scale, weight).sum().backward()
    assert torch.equal(xr.grad[0], x1.grad[0])
    assert torch.equal(xr.grad[1], 2 * x1.grad[1]) and torch.equal(xr.grad[2], -x1.grad[2])
    # the class on CPU tensors is this function; at the centre the term is zero, one scale away it is the weight
    reg = LF.StylePrior(center, scale, weight=weight)
    assert torch.equal(reg(x), LF.style_prior_torch(x, center, scale, weight))
    assert reg(center.float().view(1, -1)).item() == 0.0
    one = LF.style_prior_torch((center + scale).view(1, -1), center, scale, weight).item()
    assert abs(one - weight) < 1e-6
    with pytest.raises(ValueError):
        LF.style_prior_torch(x, center[:-1] if n > 1 else torch.zeros(2), scale, weight)


def test_style_prior_refuses_bad_scales_and_keys_follow_content():
    import pix2latent_amd.loss_functions as LF
    c = torch.zeros(8)
    for bad in (torch.zeros(8), -torch.ones(8), torch.full((8,), float('inf')), torch.ones(7)):
        with pytest.raises(ValueError):
            LF.StylePrior(c, bad)
    k0 = LF.StylePrior(c, torch.ones(8)).graph_key()
    assert k0 == LF.StylePrior(c.clone(), torch.ones(8)).graph_key()
    keys = {k0, LF.StylePrior(c, torch.ones(8), weight=2.0).graph_key(), LF.StylePrior(c + 1, torch.ones(8)).graph_key(),
            LF.StylePrior(c, 2 * torch.ones(8)).graph_key()}
    assert len(keys) == 4

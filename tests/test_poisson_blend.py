"""Poisson blend, the part that needs no GPU: the two C symbols and their host-only planning call, the refusals of
both Python wrappers, and the numpy form's range conventions and byte mapping (the device call stubbed by the
fp64 reference of tests/_poisson_ref.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _poisson_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from pix2latent_amd import _native as N
    return N.lib()


def test_symbols_declared_exported_and_bound(lib):
    from pix2latent_amd import _native as N
    hdr = open(os.path.join(ROOT, 'include', 'p2l.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('p2l_poisson_blend_ws_bytes', 'p2l_poisson_blend'):
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert hasattr(lib, name), name
        assert name in N.EXPORTS
        assert getattr(lib, name).argtypes is not None
    assert lib.p2l_poisson_blend_ws_bytes.restype is C.c_size_t
    assert lib.p2l_version() == 101


def test_ws_bytes_is_host_only_and_monotone(lib):
    ws = lib.p2l_poisson_blend_ws_bytes
    base = ws(2, 3, 64, 48)
    assert base >= 2 * 3 * 3 * 62 * 46 * 8           # x, r and p of every system, fp64, over the largest Omega
    assert ws(3, 3, 64, 48) > base and ws(2, 4, 64, 48) > base
    assert ws(2, 3, 65, 48) > base and ws(2, 3, 64, 49) > base
    prev = 0
    for s in (1, 3, 16, 256, 1024):
        cur = ws(1, 3, s, s)
        assert cur > prev
        prev = cur
    for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0), (-1, 3, 8, 8), (1, 3, -8, 8)):
        assert ws(*bad) == 0, bad


def test_entry_point_refuses_bad_arguments_on_the_host(lib):
    """(fake non-null device pointers: nothing is launched or dereferenced)"""
    fake = C.c_void_p(4096)
    need = lib.p2l_poisson_blend_ws_bytes(1, 3, 8, 8)
    args = lambda **kw: [kw.get('target', fake), 0, kw.get('mask', fake), 0, kw.get('gen', fake), kw.get('out', fake),
                         kw.get('B', 1), 3, 8, 8, kw.get('tol', 1e-8), kw.get('max_iter', 10),
                         kw.get('iters', fake), kw.get('relres', fake), kw.get('ws', fake),
                         C.c_size_t(kw.get('ws_bytes', need)), None]
    for k in ('target', 'mask', 'gen', 'out', 'iters', 'relres'):
        assert lib.p2l_poisson_blend(*args(**{k: None})) == -1, k
    assert lib.p2l_poisson_blend(*args(B=0)) == -1
    assert lib.p2l_poisson_blend(*args(tol=-1.0)) == -1
    assert lib.p2l_poisson_blend(*args(tol=float('nan'))) == -1
    assert lib.p2l_poisson_blend(*args(max_iter=-1)) == -1
    assert lib.p2l_poisson_blend(*args(ws_bytes=need - 1)) == -3
    assert lib.p2l_poisson_blend(*args(ws=None)) == -3


def test_tensor_form_refuses_cpu_tensors():
    from pix2latent_amd import _native as N
    from pix2latent_amd.utils import image as I
    t = torch.zeros(1, 3, 8, 8)
    with pytest.raises(N.NativeError, match='no CPU fallback'):
        I.poisson_blend_tensors(t, torch.ones(8, 8), t.clone())


def test_alias_package_resolves():
    import pix2latent.utils.image as alias
    from pix2latent_amd.utils import image as I
    assert alias.poisson_blend is I.poisson_blend and alias.poisson_blend_tensors is I.poisson_blend_tensors


def test_tensor_form_validates_shapes():
    from pix2latent_amd.utils import image as I
    g = torch.zeros(2, 3, 8, 10)
    ok_m = torch.ones(8, 10)
    for target in (torch.zeros(2, 3, 8, 9), torch.zeros(3, 3, 8, 10), torch.zeros(2, 1, 8, 10), torch.zeros(3, 8, 10)):
        with pytest.raises(ValueError):
            I.poisson_blend_tensors(target, ok_m, g)
    for mask in (torch.ones(10, 8), torch.ones(8, 9), torch.ones(3, 8, 10), torch.ones(2, 3, 8, 10),
                 torch.ones(2, 1, 8, 9), torch.ones(80)):
        with pytest.raises(ValueError):
            I.poisson_blend_tensors(torch.zeros(1, 3, 8, 10), mask, g)
    with pytest.raises(ValueError):
        I.poisson_blend_tensors(g, ok_m, g, tol=-1.0)
    with pytest.raises(ValueError):
        I.poisson_blend_tensors(g, ok_m, g, max_iter=-2)


def test_numpy_form_validates_shapes():
    from pix2latent_amd.utils import image as I
    img = np.zeros((8, 10, 3))
    m = np.ones((8, 10, 1))
    for t, mm, g in ((np.zeros((8, 10, 4)), m, np.zeros((8, 10, 4))),          # C other than 3
                     (np.zeros((8, 10, 1)), m, np.zeros((8, 10, 1))),
                     (img, m, np.zeros((8, 9, 3))),                            # shape mismatch
                     (img, np.ones((8, 9, 1)), img),                           # mask with the wrong extent
                     (img, np.ones((8, 10, 2)), img),
                     (img, np.ones((8, 10)), img)):
        with pytest.raises(ValueError):
            I.poisson_blend(t, mm, g)


@pytest.fixture()
def stubbed(monkeypatch):
    """the numpy form with the device call replaced by the fp64 reference on CPU tensors; records its arguments"""
    from pix2latent_amd.utils import image as I
    calls = []

    def fake_tensors(target, mask, generated, **kw):
        calls.append((target.clone(), mask.clone(), generated.clone()))
        m = mask.numpy().astype(bool)
        out, _ = R.blend(target.numpy(), m[None] if m.ndim == 2 else m, generated.numpy())
        return torch.from_numpy(out.astype(np.float32))

    monkeypatch.setattr(I, '_blend_device', lambda: torch.device('cpu'))
    monkeypatch.setattr(I, 'poisson_blend_tensors', fake_tensors)
    return I, calls


def _byte_case(seed=0, H=24, W=30):
    rng = np.random.default_rng(seed)
    t8 = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    g8 = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    t8[0, 0, 0] = g8[0, 0, 0] = 255                  # (the maximum decides the range: keep it a 0..255 image)
    m = R.disk(H, W, 11, 14, 7.5)
    return t8, m, g8


def test_numpy_form_range_conventions(stubbed):
    I, calls = stubbed
    t8, m, g8 = _byte_case()
    m3 = np.repeat(m[:, :, None], 3, axis=2)
    outs = [I.poisson_blend(t8, 255 * m3.astype(np.uint8), g8),                      # bytes, H x W x 3 mask 0..255
            I.poisson_blend(t8 / 255., m[:, :, None].astype(np.float64), g8 / 255.),  # 0..1, H x W x 1 mask 0..1
            I.poisson_blend(t8.astype(np.float32), m3.astype(np.float32), (g8 / 255.).astype(np.float32))]
    assert len(calls) == 3
    for c in calls[1:]:
        for a, b in zip(calls[0], c):
            assert a.dtype == b.dtype and torch.equal(a, b)
    tt, mm, gg = calls[0]
    assert tt.shape == gg.shape == (1, 3) + m.shape and tt.dtype == torch.float32
    assert np.array_equal(mm.numpy().astype(bool).reshape(m.shape), m)
    # byte k travels as k / 127.5 - 1
    assert torch.equal(tt[0].permute(1, 2, 0), torch.from_numpy(t8.astype(np.float32)) / 127.5 - 1.0)
    assert float(tt.min()) >= -1.0 and float(tt.max()) <= 1.0
    for o in outs:
        assert o.dtype == np.uint8 and o.shape == t8.shape and np.array_equal(o, outs[0])
    # a mask is thresholded at half of its range, and its first channel counts
    odd = np.zeros(m.shape + (3,), dtype=np.float64)
    odd[:, :, 0] = np.where(m, 0.6, 0.4)
    odd[:, :, 1] = 1.0 - odd[:, :, 0]
    I.poisson_blend(t8, odd, g8)
    assert np.array_equal(calls[-1][1].numpy().astype(bool).reshape(m.shape), m)
    I.poisson_blend(t8, np.where(m, 200, 100)[:, :, None], g8)
    assert np.array_equal(calls[-1][1].numpy().astype(bool).reshape(m.shape), m)


def test_numpy_form_byte_mapping(stubbed):
    """out = rint(clip((blend + 1) * 127.5, 0, 255)), half to even, target bytes untouched outside Omega"""
    I, _ = stubbed
    t8, m, g8 = _byte_case()
    got = I.poisson_blend(t8, m[:, :, None].astype(np.uint8), g8)
    tf = (t8.astype(np.float32) / np.float32(127.5) - np.float32(1)).transpose(2, 0, 1)[None]
    gf = (g8.astype(np.float32) / np.float32(127.5) - np.float32(1)).transpose(2, 0, 1)[None]
    ref, _ = R.blend(tf, m[None], gf)
    ref_bytes = (ref[0].transpose(1, 2, 0) + 1.0) * 127.5
    frac = np.abs(ref_bytes - np.floor(ref_bytes) - 0.5)
    assert frac.min() > 1e-4                          # no value at a tie: fp32 rounding of the stub cannot flip one
    want = np.rint(np.clip(ref_bytes, 0, 255)).astype(np.uint8)
    assert np.array_equal(got, want)
    om = R.omega_of(m)
    assert np.array_equal(got[~om], t8[~om])
    assert (got[om] != g8[om]).any()                 # (the membrane did something)


def test_reference_solves_its_own_system():
    """the reference against the definition: the residual of the 5-point equation, written out with loops"""
    t = R.images(5, 1, 1, 12, 14)[0, 0]
    g = R.images(6, 1, 1, 12, 14)[0, 0]
    m = R.disk(12, 14, 4, 5, 5.5)                     # touches the top and left borders
    out, om, A, b = R.blend_channel(t, m, g)
    assert not om[0].any() and not om[:, 0].any() and om.sum() > 20
    u = np.zeros(om.shape)
    u[om] = out[om] - g.astype(np.float64)[om]       # (|out| < 1 here: the clamp is idle)
    assert np.abs(out).max() < 1.0
    d = t.astype(np.float64) - g.astype(np.float64)
    worst = 0.0
    for y, x in zip(*np.nonzero(om)):
        lhs, rhs = 4.0 * u[y, x], 0.0
        for qy, qx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if om[qy, qx]:
                lhs -= u[qy, qx]
            else:
                rhs += d[qy, qx]
        worst = max(worst, abs(lhs - rhs))
    assert worst < 1e-12
    assert np.array_equal(out[~om], t.astype(np.float64)[~om])
    assert abs(A - A.T).max() == 0 and A.shape == (om.sum(), om.sum()) and b.shape == (om.sum(),)

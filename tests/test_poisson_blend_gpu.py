"""Poisson blend on the device (p2l_poisson_blend through pix2latent_amd.utils.image) against the fp64 direct solve
of the same system (tests/_poisson_ref.py).

Accuracy bound inside Omega, per system, for a call with tol = 1e-10:
    max|out - ref| <= 1e-10 * |b|_2 / lambda_min(A) + 2^-23
-- the a-priori CG bound |e| <= |r| / lambda_min with the REQUESTED tol (never the residual the kernel reports),
plus one fp32 rounding of the output.  lambda_min comes from numpy.linalg.eigvalsh on the dense fp64 A, computed once per
mask and shared (the mask that covers the whole image has 2 052, 6 020 and 7 332 unknowns at the three sizes; for that
rectangle the result is also held to the closed form 4 - 2 cos(pi / (h + 1)) - 2 cos(pi / (w + 1))).  The whole-image mask
at 96 x 80 is the case whose state does not fit in LDS: it holds the workspace form of the kernel to the same bound."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

import _poisson_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(40, 56), (72, 88), (96, 80)]
MASKS = ['blob_hole', 'two_parts', 'full', 'off_borders', 'single', 'empty']
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def lam_min(H, W, name):
    """smallest eigenvalue of the system of a mask (A depends on the mask alone); None for an empty Omega"""
    m = R.mask_cases(H, W)[name]
    _, A, _ = R.poisson_system(np.zeros((H, W)), m, np.zeros((H, W)))
    if A.shape[0] == 0:
        return None
    lam = float(np.linalg.eigvalsh(A.toarray())[0])
    if name == 'full':
        assert abs(lam - (4 - 2 * np.cos(np.pi / (H - 1)) - 2 * np.cos(np.pi / (W - 1)))) < 1e-12
    return lam


@functools.lru_cache(maxsize=None)
def inputs(seed, B, H, W):
    return R.images(seed, B, 3, H, W), R.images(seed + 100, B, 3, H, W)


def I():
    from pix2latent_amd.utils import image
    return image


def check_against_reference(out, iters, relres, target, masks, names, generated, H, W, tol, max_iter):
    """every system of a call: the bound inside Omega, torch.equal outside, relres <= tol, iters < max_iter"""
    ref, systems = R.blend(target, masks, generated)
    got = out.double().cpu().numpy()
    tgt = torch.from_numpy(np.broadcast_to(target, generated.shape).copy())
    iters, relres = iters.cpu().numpy(), relres.cpu().numpy()
    assert np.isfinite(got).all()
    for b in range(generated.shape[0]):
        name = names[b % len(names)]
        lam = lam_min(H, W, name)
        for c in range(generated.shape[1]):
            om, A, rhs = systems[b][c]
            outside = torch.from_numpy(~om)
            assert torch.equal(out[b, c].cpu()[outside], tgt[b, c][outside]), (name, b, c)
            assert relres[b, c] <= tol and 0 <= iters[b, c] < max_iter, (name, b, c, iters[b, c], relres[b, c])
            if lam is None:
                assert iters[b, c] == 0 and relres[b, c] == 0.0
                continue
            bound = tol * np.linalg.norm(rhs) / lam + 2.0 ** -23
            err = np.abs(got[b, c][om] - ref[b, c][om]).max()
            print('%dx%d %-11s b%d c%d n=%5d iters=%4d relres=%.2e err=%.3e bound=%.3e'
                  % (H, W, name, b, c, A.shape[0], iters[b, c], relres[b, c], err, bound))
            assert err <= bound, (name, b, c, err, bound)


SINGLE_CASES = [(H, W, n) for (H, W) in SIZES for n in MASKS]


@pytest.mark.parametrize('H,W,name', SINGLE_CASES)
def test_single_image_against_fp64_direct_solve(dev, H, W, name):
    t, g = inputs(0, 1, H, W)
    m = R.mask_cases(H, W)[name]
    max_iter = 10 * (H + W)
    out, iters, relres = I().poisson_blend_tensors(torch.from_numpy(t).to(dev), torch.from_numpy(m).to(dev),
                                                   torch.from_numpy(g).to(dev), tol=TOL, return_info=True)
    assert out.shape == (1, 3, H, W) and out.dtype == torch.float32
    assert iters.shape == relres.shape == (1, 3) and iters.dtype == torch.int32 and relres.dtype == torch.float64
    check_against_reference(out, iters, relres, t, m[None], [name], g, H, W, TOL, max_iter)
    if name == 'empty':
        assert torch.equal(out.cpu(), torch.from_numpy(t))


BATCH_NAMES = ['blob_hole', 'two_parts', 'off_borders', 'single', 'empty']


def batch_names(H):
    """the five masks of a per-image batch: the six of MASKS less one, another one at each image size"""
    k = {40: 0, 72: 1, 96: 2}[H]
    return [n for n in MASKS if n != ('empty', 'single', 'two_parts')[k]]


@pytest.mark.parametrize('mask_shared', [True, False])
@pytest.mark.parametrize('target_shared', [True, False])
@pytest.mark.parametrize('H,W', SIZES)
def test_batch_of_five_shared_or_per_image(dev, H, W, target_shared, mask_shared):
    t, g = inputs(1, 5, H, W)
    if target_shared:
        t = t[:1]
    cases = R.mask_cases(H, W)
    names = ['full' if H == 96 else 'blob_hole'] if mask_shared else batch_names(H)
    masks = np.stack([cases[n] for n in names])
    # the three accepted layouts of a mask, any dtype
    mt = torch.from_numpy(masks)
    mt = {40: mt.float()[:, None], 72: mt.to(torch.uint8), 96: mt.double()[:, None]}[H]
    if mask_shared and H == 72:
        mt = mt[0]
    out, iters, relres = I().poisson_blend_tensors(torch.from_numpy(t).to(dev), mt.to(dev),
                                                   torch.from_numpy(g).to(dev), tol=TOL, return_info=True)
    check_against_reference(out, iters, relres, t, masks, names, g, H, W, TOL, 10 * (H + W))


def test_degenerate_inputs(dev):
    H, W = 40, 56
    t, _ = inputs(2, 5, H, W)
    tt = torch.from_numpy(t).to(dev)
    for name in ('blob_hole', 'full', 'empty'):
        m = torch.from_numpy(R.mask_cases(H, W)[name]).to(dev)
        out, iters, relres = I().poisson_blend_tensors(tt, m, tt.clone(), return_info=True)
        assert torch.equal(out, tt), name            # generated == target: b = 0, u = 0
        assert int(iters.abs().max()) == 0 and float(relres.abs().max()) == 0.0
        assert torch.isfinite(out).all() and torch.isfinite(relres).all()
    g = torch.from_numpy(inputs(3, 5, H, W)[1]).to(dev)
    out, iters, relres = I().poisson_blend_tensors(tt, torch.zeros(H, W, device=dev), g, return_info=True)
    assert torch.equal(out, tt) and int(iters.max()) == 0 and torch.isfinite(relres).all()
    # images too small to have an interior
    s = torch.from_numpy(R.images(4, 2, 3, 2, 7)).to(dev)
    out = I().poisson_blend_tensors(s, torch.ones(2, 7, device=dev), -s)
    assert torch.equal(out, s)


def test_256_disk_within_an_eighth_of_a_level(dev):
    """the product requirement at the default tol = 1e-8: invisible after quantisation to 8 bits"""
    S = 256
    t, g = inputs(5, 2, S, S)
    m = R.disk(S, S, S / 2, S / 2, 0.4 * S)
    ref, systems = R.blend(t, m[None], g)
    out, iters, relres = I().poisson_blend_tensors(torch.from_numpy(t).to(dev), torch.from_numpy(m).to(dev),
                                                   torch.from_numpy(g).to(dev), return_info=True)
    om = systems[0][0][0]
    err = np.abs(out.double().cpu().numpy() - ref)
    print('256^2 disk: n=%d iters=%s relres=%s err=%.3e' % (om.sum(), iters.flatten().tolist(),
                                                            ['%.2e' % v for v in relres.flatten().tolist()], err.max()))
    assert err.max() <= 9.8e-4, 'max|out - ref| = %.3e (iters %s)' % (err.max(), iters.flatten().tolist())
    assert (err[:, :, ~om] == 0).all()
    assert float(relres.max()) <= 1e-8 and int(iters.max()) < 10 * (S + S)


def test_bit_identical_between_calls_and_batch_invariant(dev):
    H, W = 72, 88
    t, g = inputs(6, 5, H, W)
    cases = R.mask_cases(H, W)
    masks = torch.from_numpy(np.stack([cases[n] for n in BATCH_NAMES])).to(dev)
    tt, gg = torch.from_numpy(t).to(dev), torch.from_numpy(g).to(dev)
    run = lambda: I().poisson_blend_tensors(tt, masks, gg, tol=TOL, return_info=True)
    out1, it1, rr1 = run()
    x = torch.randn(512, 512, device=dev)
    (x @ x).sum().item()                              # other work in between
    out2, it2, rr2 = run()
    assert torch.equal(out1, out2) and torch.equal(it1, it2) and torch.equal(rr1, rr2)
    for k in range(5):
        o, it, rr = I().poisson_blend_tensors(tt[k:k + 1], masks[k:k + 1], gg[k:k + 1], tol=TOL, return_info=True)
        assert torch.equal(o[0], out1[k]) and torch.equal(it[0], it1[k]) and torch.equal(rr[0], rr1[k]), k
    # ... and a shared target / mask gives what the repeated one gives
    o, it, rr = I().poisson_blend_tensors(tt[:1], masks[0], gg, tol=TOL, return_info=True)
    o2, _, _ = I().poisson_blend_tensors(tt[:1].repeat(5, 1, 1, 1), masks[:1].repeat(5, 1, 1), gg, tol=TOL,
                                         return_info=True)
    assert torch.equal(o, o2)


def test_max_iter_warns_and_stays_finite(dev):
    H, W = 72, 88
    t, g = inputs(7, 1, H, W)
    m = torch.from_numpy(R.mask_cases(H, W)['blob_hole']).to(dev)
    tt, gg = torch.from_numpy(t).to(dev), torch.from_numpy(g).to(dev)
    with pytest.warns(RuntimeWarning, match='max_iter'):
        out = I().poisson_blend_tensors(tt, m, gg, max_iter=3)
    assert torch.isfinite(out).all()
    out, iters, relres = I().poisson_blend_tensors(tt, m, gg, max_iter=3, return_info=True)
    assert int(iters.min()) == int(iters.max()) == 3 and float(relres.min()) > 1e-8 and torch.isfinite(relres).all()
    with warnings.catch_warnings():
        warnings.simplefilter('error')               # a converged call is silent
        I().poisson_blend_tensors(tt, m, gg)


def test_entry_point_refusals(dev):
    from pix2latent_amd import _native as N
    L = N.lib()
    B, Cn, H, W = 1, 3, 40, 56
    t = torch.zeros(B, Cn, H, W, device=dev)
    g, out = t.clone(), t.clone()
    m = torch.ones(H, W, device=dev, dtype=torch.uint8)
    iters = torch.full((B, Cn), -7, device=dev, dtype=torch.int32)
    relres = torch.zeros(B, Cn, device=dev, dtype=torch.float64)
    need = L.p2l_poisson_blend_ws_bytes(B, Cn, H, W)
    ws = torch.empty(need, device=dev, dtype=torch.uint8)
    call = lambda tp, mp, gp, op, ip, rp, wp, nb: L.p2l_poisson_blend(tp, 0, mp, 0, gp, op, B, Cn, H, W, 1e-8, 100, ip,
                                                                      rp, wp, nb, N.stream())
    ptrs = [t.data_ptr(), m.data_ptr(), g.data_ptr(), out.data_ptr(), iters.data_ptr(), relres.data_ptr()]
    assert call(*ptrs, ws.data_ptr(), need - 1) == -3          # a workspace one byte short
    assert call(*ptrs, None, need) == -3
    for k in range(6):
        bad = list(ptrs)
        bad[k] = None
        assert call(*bad, ws.data_ptr(), need) == -1, k
    torch.cuda.synchronize()
    assert int(iters.min()) == -7                               # nothing was launched
    assert call(*ptrs, ws.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert int(iters.max()) == 0 and torch.equal(out, t)


def test_numpy_form_matches_rounded_reference(dev):
    H, W, seed = 72, 88, 0
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 128 + 60 * np.sin(yy / 9.0)[:, :, None] + 50 * np.cos(xx / 7.0)[:, :, None]
    t8 = np.clip(base + rng.uniform(-40, 40, size=(H, W, 3)), 0, 255).astype(np.uint8)
    g8 = np.clip(base[::-1] + 30 + rng.uniform(-40, 40, size=(H, W, 3)), 0, 255).astype(np.uint8)
    t8[0, 0, 0] = g8[0, 0, 0] = 255
    m = R.mask_cases(H, W)['blob_hole']
    tf = (t8.astype(np.float32) / np.float32(127.5) - np.float32(1)).transpose(2, 0, 1)[None]
    gf = (g8.astype(np.float32) / np.float32(127.5) - np.float32(1)).transpose(2, 0, 1)[None]
    ref, _ = R.blend(tf, m[None], gf)
    ref_bytes = (ref[0].transpose(1, 2, 0) + 1.0) * 127.5
    # on the reference alone: no value within 1e-5 of a .5 tie
    assert np.abs(ref_bytes - np.floor(ref_bytes) - 0.5).min() > 1e-5
    want = np.rint(np.clip(ref_bytes, 0, 255)).astype(np.uint8)
    got = I().poisson_blend(t8, (255 * m[:, :, None]).astype(np.uint8), g8)
    assert got.dtype == np.uint8 and got.shape == (H, W, 3)
    assert np.array_equal(got, want), int((got != want).sum())
    got01 = I().poisson_blend(t8 / 255., np.repeat(m[:, :, None], 3, axis=2).astype(np.float32), g8 / 255.)
    assert np.array_equal(got01, want)

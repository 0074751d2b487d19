"""pix2latent.edit on the host: the float64 path from S = Zc^T Zc and G = W_z^T W_z against the reference's
literal algorithm (edit/ganspace.py) on a small affine gen_z, the closed form against numpy's lstsq, the
sign rule, the alias imports, argument checks, and the Gram ABI's host-side refusals."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pix2latent_amd.edit import ganspace as GS

D, FEAT, N = 128, 1024, 600
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(seed, k):
    """affine gen_z 2D -> FEAT, one class embedding, and the reference's CPU draws z then u0"""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(FEAT, 2 * D, generator=g, dtype=torch.float64) / 16
    b = torch.randn(FEAT, generator=g, dtype=torch.float64)
    c = torch.randn(1, D, generator=g, dtype=torch.float64)
    torch.manual_seed(seed)
    z = torch.randn(N, D)
    u0 = torch.randn(D, k)
    return W, b, c, z.double(), u0


def _sign_rule(m):
    """numpy restatement: flip each column so that its first entry of largest magnitude is positive"""
    m = np.asarray(m)
    idx = np.argmax(np.abs(m), axis=0)             # (numpy: the first occurrence)
    s = np.sign(m[idx, np.arange(m.shape[1])])
    s[s == 0] = 1
    return s


def _literal(W, b, c, z, u0, k, method):
    """the reference's biggan_components step by step in float64, exact SVD for the randomized sketch"""
    feat = torch.cat([z, c.repeat(N, 1)], 1) @ W.t() + b
    feat_mean = feat.mean(0).unsqueeze(0)
    _, _, Vh = torch.linalg.svd(feat - feat_mean, full_matrices=False)
    v = Vh[:k].t()
    x = torch.mm(feat - feat_mean, v)
    x = x * torch.from_numpy(_sign_rule((z.t() @ x).numpy()))
    if method == 'lstsq':
        u = torch.from_numpy(np.linalg.lstsq(x.numpy(), z.numpy(), rcond=None)[0]).t()
    else:
        u = torch.nn.parameter.Parameter(u0.double().clone())
        opt = torch.optim.Adam([u], lr=1)
        for i in range(100):
            opt.zero_grad()
            loss = ((z - torch.mm(x, u.t())) ** 2).mean()
            loss.backward()
            opt.step()
            for param_group in opt.param_groups:
                param_group['lr'] = param_group['lr'] * 0.98
        u = u.detach()
    return F.normalize(u, p=2, dim=1).permute(1, 0), v, x


def _grams(W, z):
    zc = z - z.mean(0)
    Wz = W[:, :D]
    return zc.t() @ zc, Wz.t() @ Wz


@pytest.mark.parametrize('seed,k', [(0, 32), (1, 7), (2, 128)])
def test_sgd_matches_the_literal_reference(seed, k):
    W, b, c, z, u0 = _problem(seed, k)
    S, G = _grams(W, z)
    got = GS.components_from_grams(S, G, N, u0, k, 'sgd')
    ref, _, _ = _literal(W, b, c, z, u0, k, 'sgd')
    assert got.shape == (k, D) and got.dtype == torch.float64
    assert (got - ref).abs().max().item() < 1e-9


def test_lstsq_matches_numpy_lstsq():
    k = 32
    W, b, c, z, u0 = _problem(3, k)
    S, G = _grams(W, z)
    got = GS.components_from_grams(S, G, N, None, k, 'lstsq')
    ref, _, _ = _literal(W, b, c, z, u0, k, 'lstsq')
    assert (got - ref).abs().max().item() < 1e-9


def test_principal_directions_are_the_exact_pca():
    """v_k = W_z L^-T y_k are the top right singular vectors of the centred features (up to sign), the
    coordinates x = Zc L Y, x^T x = diag(lam) and z^T x = S L Y"""
    k = 16
    W, b, c, z, _ = _problem(4, k)
    S, G = _grams(W, z)
    lam, Y, zx = GS.principal_directions(S, G, k)
    _, v, x = _literal(W, b, c, z, None, k, 'lstsq')
    L = torch.linalg.cholesky(G)
    vk = W[:, :D] @ torch.linalg.solve_triangular(L.t(), Y, upper=True)
    assert (vk.norm(dim=0) - 1).abs().max().item() < 1e-12
    assert ((vk * v).sum(0).abs() - 1).abs().max().item() < 1e-10
    assert (x.t() @ x - torch.diag(lam)).abs().max().item() < 1e-9 * lam[0].item()
    assert (z.t() @ x - zx).abs().max().item() < 1e-9 * zx.abs().max().item()


def test_sign_rule():
    k = 24
    W, _, _, z, _ = _problem(5, k)
    S, G = _grams(W, z)
    _, _, zx = GS.principal_directions(S, G, k)
    a = zx.abs()
    idx = a.numpy().argmax(0)
    assert (zx[idx, torch.arange(k)] > 0).all()
    # ties: the lowest row index decides; an all-zero column keeps its sign
    m = torch.tensor([[1.0, -2.0, 0.0, 0.5], [-1.0, 2.0, 0.0, -3.0], [0.5, 1.0, 0.0, 3.0]], dtype=torch.float64)
    assert GS.orient(m).tolist() == [1.0, -1.0, 1.0, -1.0]
    assert GS.orient(m).tolist() == _sign_rule(m.numpy()).tolist()


def test_components_do_not_depend_on_the_bias_or_class():
    """the premise of the Gram route, on the literal algorithm itself"""
    k = 8
    W, b, c, z, u0 = _problem(6, k)
    r1, _, _ = _literal(W, b, c, z, u0, k, 'sgd')
    r2, _, _ = _literal(W, 3 * b + 1, -2 * c + 0.5, z, u0, k, 'sgd')
    assert (r1 - r2).abs().max().item() < 1e-9


def test_alias_imports():
    import pix2latent.edit
    from pix2latent.edit import BigGANLatentEditor
    from pix2latent.edit.ganspace import biggan_components
    from pix2latent.edit.editor import BigGANLatentEditor as E2
    import pix2latent_amd.edit as impl
    assert pix2latent.edit is impl
    assert BigGANLatentEditor is E2 is impl.BigGANLatentEditor
    assert biggan_components is GS.biggan_components
    for m in ('edit', 'edit.editor', 'edit.ganspace'):
        import sys
        assert sys.modules['pix2latent.' + m] is sys.modules['pix2latent_amd.' + m]


def test_biggan_components_checks_its_arguments():
    fake = types.SimpleNamespace(z_dim=128)          # (every check runs before any device work)
    with pytest.raises(ValueError, match='feat_size'):
        GS.biggan_components(fake, 0, feat_size=120)
    with pytest.raises(ValueError, match='num_components'):
        GS.biggan_components(fake, 0, num_components=129)
    with pytest.raises(ValueError, match='num_components'):
        GS.biggan_components(fake, 0, num_components=0)
    with pytest.raises(TypeError):
        GS.biggan_components(fake, 'dog')
    with pytest.raises(AssertionError):
        GS.biggan_components(fake, 0, method='svd')
    with pytest.raises(ValueError):
        GS.components_from_grams(torch.eye(4), torch.eye(4), 10, None, 2, 'svd')


def test_editor_keeps_the_model_it_is_given():
    from pix2latent_amd.edit import BigGANLatentEditor
    m = object()
    assert BigGANLatentEditor(m).model is m


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(ROOT, 'pix2latent_amd', 'libp2l_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from pix2latent_amd import _native as N
    return N.lib()


def test_gram_abi_refuses_bad_arguments_on_the_host(lib):
    """sizes and workspace are checked before any launch (fake non-null device pointers)"""
    ws = lib.p2l_gram_f64_ws_bytes(12800, 128, 0)
    assert ws > 0 and ws % 8 == 0
    assert lib.p2l_gram_f64_ws_bytes(12800, 128, 1) == ws          # the plan follows the rows only
    assert lib.p2l_gram_f64_ws_bytes(12800, 3, 0) == ws
    assert lib.p2l_gram_f64_ws_bytes(1 << 40, 128, 0) == lib.p2l_gram_f64_ws_bytes(1 << 20, 128, 0)  # capped
    for args in ((0, 1, 0), (5, 0, 0), (5, 129, 0), (5, 4, 2), (-1, 4, 1)):
        assert lib.p2l_gram_f64_ws_bytes(*args) == 0, args
    f = 4096
    call = lambda X, rows, cols, ld, trans, g, s, w, nb: lib.p2l_gram_f64(X, rows, cols, ld, trans, g, s, w, nb,  # noqa: E731
                                                                          None)
    for rows, cols, ld, trans in ((0, 4, 4, 0), (8, 0, 4, 0), (8, 129, 200, 0), (8, 4, 3, 0), (8, 4, 7, 1),
                                  (8, 4, 8, 2)):
        assert call(f, rows, cols, ld, trans, f, f, f, 1 << 30) == -1, (rows, cols, ld, trans)
    assert call(None, 8, 4, 4, 0, f, f, f, 1 << 30) == -1
    assert call(f, 8, 4, 4, 0, None, f, f, 1 << 30) == -1
    assert call(f, 8, 4, 4, 0, f, None, f, 1 << 30) == -1
    need = lib.p2l_gram_f64_ws_bytes(8, 4, 0)
    assert call(f, 8, 4, 4, 0, f, f, f, need - 1) == -3
    assert call(f, 8, 4, 4, 0, f, f, None, need) == -3

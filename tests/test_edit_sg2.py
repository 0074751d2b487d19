"""pix2latent.edit for StyleGAN2 on the host: components_from_covariance against numpy's SVD of centred float64
samples with a planted spectrum, the properties of its result, the sign rule, argument checks, the alias
imports, and the host-side refusals of the wide Gram ABI (p2l_gram_f64_wide)."""
import os
import types

import numpy as np
import pytest
import torch

from pix2latent_amd.edit import ganspace as GS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, K = 4000, 512, 32


@pytest.fixture(scope='module')
def planted():
    """N x D float64 samples whose centred singular values are known: the top K fall by 15 % each
    (100 ... 1.31), a flat tail of 0.5 sits below them; a non-zero mean on top"""
    rng = np.random.default_rng(0)
    Z = rng.standard_normal((N, D))
    Q, _ = np.linalg.qr(Z - Z.mean(0))                   # orthonormal columns, each of zero mean
    R, _ = np.linalg.qr(rng.standard_normal((D, D)))
    s = np.full(D, 0.5)
    s[:K] = 100.0 * 1.15 ** -np.arange(K)
    X = (Q * s) @ R.T + rng.standard_normal(D)
    Xc = X - X.mean(0)
    C = Xc.T @ Xc / (N - 1)
    _, sv, Vh = np.linalg.svd(Xc, full_matrices=False)
    assert np.abs(sv[:K] / s[:K] - 1).max() < 1e-10      # (the construction holds)
    return C, sv, Vh


def _sign_rule(V):
    """numpy restatement, per row: the first entry of largest magnitude is positive"""
    idx = np.argmax(np.abs(V), axis=1)                   # (numpy: the first occurrence)
    sgn = np.sign(V[np.arange(V.shape[0]), idx])
    sgn[sgn == 0] = 1
    return V * sgn[:, None]


def test_components_match_the_svd(planted):
    """eigenvector perturbation <= |E| / gap with |E| ~ 1e-13 and relative gaps >= 0.1: 1e-9, the figure of
    tests/test_edit.py"""
    C, sv, Vh = planted
    V, stdev = GS.components_from_covariance(torch.from_numpy(C), K)
    assert V.shape == (K, D) and stdev.shape == (K,) and V.dtype == stdev.dtype == torch.float64
    assert V.device.type == 'cpu'
    ref = _sign_rule(Vh[:K])
    assert np.abs(V.numpy() - ref).max() < 1e-9
    lam = sv[:K] ** 2 / (N - 1)
    assert np.abs(stdev.numpy() ** 2 / lam - 1).max() < 1e-10


@pytest.mark.parametrize('k', (1, 7, 32, 512))
def test_properties_of_the_result(planted, k):
    C, _, _ = planted
    V, stdev = GS.components_from_covariance(C, k)       # (a numpy array is taken as well)
    assert V.shape == (k, D)
    assert (V @ V.t() - torch.eye(k, dtype=torch.float64)).abs().max().item() < 1e-12
    assert (stdev[1:] <= stdev[:-1]).all() and (stdev >= 0).all()
    a = V.abs()
    assert (V[torch.arange(k), a.argmax(1)] > 0).all()


def test_sign_rule_with_a_tie():
    """the lowest index decides a tie: the eigenvectors of [[2, 1], [1, 2]] are (1, 1) and (1, -1) / sqrt 2;
    and a negative eigenvalue (a covariance that rounding made indefinite) gives stdev 0"""
    m = torch.tensor([[1.0, -0.5], [1.0, 0.5], [0.5, -0.5]], dtype=torch.float64)
    assert GS.orient(m).tolist() == [1.0, -1.0]
    m = torch.tensor([[-1.0, 0.5], [1.0, 0.5], [0.5, -0.5]], dtype=torch.float64)
    assert GS.orient(m).tolist() == [-1.0, 1.0]
    C = torch.zeros(4, 4, dtype=torch.float64)
    C[:2, :2] = torch.tensor([[2.0, 1.0], [1.0, 2.0]])
    C[2, 2], C[3, 3] = 0.5, -1e-18
    V, stdev = GS.components_from_covariance(C, 4)
    r = 0.5 ** 0.5
    want = torch.tensor([[r, r, 0, 0], [r, -r, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float64)
    assert (V - want).abs().max().item() < 1e-15
    assert (stdev - torch.tensor([3.0 ** 0.5, 1.0, r, 0.0], dtype=torch.float64)).abs().max().item() < 1e-15
    assert stdev[3].item() == 0.0


def test_num_components_out_of_range(planted):
    C, _, _ = planted
    for k in (0, -1, 513):
        with pytest.raises(ValueError, match='num_components'):
            GS.components_from_covariance(C, k)
    with pytest.raises(ValueError):
        GS.components_from_covariance(torch.zeros(4, 5), 2)
    fake = types.SimpleNamespace(_dev=torch.device('cpu'))       # (every check runs before any device work)
    for k in (0, 513):
        with pytest.raises(ValueError, match='num_components'):
            GS.stylegan2_components(fake, num_components=k)
    with pytest.raises(ValueError, match='num_samples'):
        GS.stylegan2_components(fake, num_samples=1)
    with pytest.raises(ValueError, match='num_samples'):
        GS.w_covariance(fake, 1)
    with pytest.raises(ValueError, match='chunk_rows'):
        GS.w_covariance(fake, 10, chunk_rows=0)
    with pytest.raises(ValueError):
        GS.gram_f64_wide(torch.zeros(4, 4), 4, 4, 4)             # not a device tensor


def test_alias_imports():
    import pix2latent.edit
    from pix2latent.edit import StyleGAN2LatentEditor, stylegan2_components
    from pix2latent.edit.editor import StyleGAN2LatentEditor as E2
    import pix2latent_amd.edit as impl
    assert StyleGAN2LatentEditor is E2 is impl.StyleGAN2LatentEditor
    assert stylegan2_components is GS.stylegan2_components is pix2latent.edit.ganspace.stylegan2_components
    assert {'StyleGAN2LatentEditor', 'stylegan2_components', 'BigGANLatentEditor', 'biggan_components'} \
        <= set(impl.__all__)
    m = object()
    assert StyleGAN2LatentEditor(m).model is m


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(ROOT, 'pix2latent_amd', 'libp2l_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from pix2latent_amd import _native as N_
    return N_.lib()


def test_wide_gram_abi_refuses_bad_arguments_on_the_host(lib):
    """sizes and workspace are checked before any launch (fake non-null device pointers)"""
    slot = (64 * 256 + 128) * 8                  # one block's partial: 64 tiles and 128 column sums, fp64
    assert lib.p2l_gram_f64_wide_ws_bytes(1, 1) == slot
    # one row range per 256 rows until pairs x ranges reaches 512 blocks; pairs = 1, 3, 6, 10
    assert lib.p2l_gram_f64_wide_ws_bytes(4099, 128) == 17 * slot
    assert lib.p2l_gram_f64_wide_ws_bytes(4099, 129) == 17 * 3 * slot
    assert lib.p2l_gram_f64_wide_ws_bytes(4099, 512) == 17 * 10 * slot
    assert lib.p2l_gram_f64_wide_ws_bytes(4099, 385) == lib.p2l_gram_f64_wide_ws_bytes(4099, 512)
    big = lib.p2l_gram_f64_wide_ws_bytes(10 ** 6, 512)
    assert big == 51 * 10 * slot and big < 70e6
    assert lib.p2l_gram_f64_wide_ws_bytes(1 << 40, 512) == big           # capped
    assert lib.p2l_gram_f64_wide_ws_bytes(10 ** 6, 256) == 170 * 3 * slot
    for args in ((0, 1), (5, 0), (5, 513), (-1, 4)):
        assert lib.p2l_gram_f64_wide_ws_bytes(*args) == 0, args
    f = 4096
    call = lambda X, rows, cols, ld, g, s, w, nb: lib.p2l_gram_f64_wide(X, rows, cols, ld, g, s, w, nb, None)  # noqa: E731
    for rows, cols, ld in ((0, 4, 4), (8, 0, 4), (8, 513, 600), (8, 4, 3), (8, 512, 511)):
        assert call(f, rows, cols, ld, f, f, f, 1 << 30) == -1, (rows, cols, ld)
    assert call(None, 8, 4, 4, f, f, f, 1 << 30) == -1
    assert call(f, 8, 4, 4, None, f, f, 1 << 30) == -1
    assert call(f, 8, 4, 4, f, None, f, 1 << 30) == -1
    need = lib.p2l_gram_f64_wide_ws_bytes(8, 4)
    assert call(f, 8, 4, 4, f, f, f, need - 1) == -3
    assert call(f, 8, 4, 4, f, f, None, need) == -3

"""The whitened latent prior without a GPU: the closed-form gradient against autograd through
`LF.latent_prior_torch`, the whitening identity of `LatentPrior.from_samples`, the eigenvalue floor, `graph_key`,
`standard_normal`, and the host-side argument checks of the two launch entry points (fake pointers: every refusal
comes before a launch, nothing is dereferenced)."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _latent_prior_ref as PR  # noqa: E402

import pix2latent_amd.loss_functions as LF  # noqa: E402


@pytest.mark.parametrize('p_space', [True, False])
@pytest.mark.parametrize('L', [1, 6])
def test_closed_form_gradient_against_autograd(p_space, L):
    B, D, K = 3, 64, 40
    w, A, m, a = PR.make_case(B, L, D, K, seed=10 * L + p_space)
    assert (w == 0).any() and np.signbit(w[w == 0]).any() and (w < 0).any()
    gloss = np.array([1.5, -0.5, 2.0])
    ref = PR.reference(w, A, m, a, p_space, gloss)
    t = torch.from_numpy(w).clone().requires_grad_(True)
    P = LF.latent_prior_torch(t, torch.from_numpy(A), torch.from_numpy(m), torch.from_numpy(a), p_space)
    assert P.dtype == torch.float32 and P.shape == (B,)
    (P.double() * torch.from_numpy(gloss)).sum().backward()
    err_p = np.abs(P.detach().double().numpy() - ref['P']) / ref['P']
    err_g = np.abs(t.grad.double().numpy() - ref['dw']).max() / np.abs(ref['dw']).max()
    print('p_space %d L %d: P rel err %s  grad err / max %.3g' % (p_space, L, err_p, err_g))
    assert (err_p <= 2.0 ** -23).all()
    assert err_g <= 1e-6
    if p_space:
        # zeros of either sign take slope 1, and the flag matters
        assert (PR.slope(w, True)[w == 0] == 1.0).all() and (PR.slope(w, True)[w < 0] == 5.0).all()
        assert not np.allclose(PR.reference(w, A, m, a, False, gloss)['P'], ref['P'])
    # the public entry point on CPU tensors is the same expression, and LatentPrior applies its weight
    prior = LF.LatentPrior(A, m, weight=3.0, layer_weights=a, p_space=p_space)
    t2 = torch.from_numpy(w).clone().requires_grad_(True)
    P2 = LF.latent_prior(t2, prior)
    assert torch.equal(P2.detach(), P.detach())
    assert torch.equal(prior(torch.from_numpy(w)), 3.0 * P.detach())
    if L == 1:
        assert torch.equal(LF.latent_prior(torch.from_numpy(w[:, 0]), prior), P.detach())      # [B, D] is L = 1


def test_to_p_space_keeps_zero_signs():
    w = torch.tensor([-1.5, -0.0, 0.0, 2.0, -0.25])
    x = LF.to_p_space(w)
    assert torch.equal(x, torch.tensor([-7.5, -0.0, 0.0, 2.0, -1.25]))
    assert torch.signbit(x)[1] and not torch.signbit(x)[2]
    import pix2latent.loss_functions as LFA
    assert LFA.LatentPrior is LF.LatentPrior and LFA.latent_prior is LF.latent_prior


@pytest.fixture(scope='module')
def samples():
    """X [8192, 512] fp64: eigenvalues log-spaced over four decades in a random orthogonal frame, non-zero mean"""
    N, D = 8192, 512
    g = torch.Generator().manual_seed(0)
    Q, _ = torch.linalg.qr(torch.randn(D, D, generator=g, dtype=torch.float64))
    lam = torch.logspace(0, -4, D, dtype=torch.float64)
    X = (torch.randn(N, D, generator=g, dtype=torch.float64) * lam.sqrt()) @ Q.t()
    return X + 0.5 * torch.randn(D, generator=g, dtype=torch.float64)


@pytest.mark.parametrize('K', [512, 64])
def test_whitening_identity(samples, K):
    """statistics from the fp64 samples, P of their fp32 roundings: the in-sample mean of P is (N - 1) / N but for
    the rounding of X, which `rounding_bound` propagates through |A| |x|"""
    N = samples.size(0)
    prior = LF.LatentPrior.from_samples(samples, num_components=K)
    assert prior.num_components == K and prior.dim == 512 and prior.p_space is False
    P = prior(samples.float()).double().numpy()
    bound = PR.rounding_bound(samples.numpy(), prior.basis.numpy(), prior.mean.numpy()).mean()
    diff = abs(P.mean() - (N - 1.0) / N)
    print('K %d: mean P - (N - 1) / N = %.3g, bound %.3g' % (K, diff, bound))
    assert bound < 1e-2
    assert diff <= bound
    # ... and the components are whitened: unit in-sample variance along each
    v = (samples - prior.mean) @ prior.basis.t()
    assert ((v * v).sum(0) / (N - 1) - 1.0).abs().max().item() < 1e-9


def test_from_samples_warns_when_the_covariance_cannot_have_full_rank():
    x = torch.randn(20, 32, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    with pytest.warns(UserWarning) as rec:
        prior = LF.LatentPrior.from_samples(x)
    assert any('20 samples of dimension 32' in str(r.message) for r in rec)
    assert prior.num_components == 19


def test_eigenvalue_floor():
    D, rank = 64, 40
    g = torch.Generator().manual_seed(2)
    Bm = torch.randn(D, rank, generator=g, dtype=torch.float64)
    Cm = Bm @ Bm.t()
    mean = torch.randn(D, generator=g, dtype=torch.float64)
    with pytest.warns(UserWarning, match='24 of 64 components'):
        full = LF.LatentPrior.from_covariance(Cm, mean)
    assert full.num_components == rank
    with pytest.warns(UserWarning):
        over = LF.LatentPrior.from_covariance(Cm, mean, num_components=50)     # reduced, not an error
    assert over.num_components == rank and torch.equal(over.basis, full.basis)
    with pytest.warns(UserWarning):
        few = LF.LatentPrior.from_covariance(Cm, mean, num_components=10)
    assert few.num_components == 10 and torch.equal(few.basis, full.basis[:10])
    # the kept directions whiten C: A C A^T = I
    err = (full.basis @ Cm @ full.basis.t() - torch.eye(rank, dtype=torch.float64)).abs().max().item()
    assert err < 1e-9, err
    # a full-rank covariance: no warning
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        ok = LF.LatentPrior.from_covariance(Cm + torch.eye(D, dtype=torch.float64), mean)
    assert ok.num_components == D


def test_graph_key():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(400, 64, generator=g, dtype=torch.float64)
    y = torch.randn(400, 64, generator=g, dtype=torch.float64)
    a = LF.LatentPrior.from_samples(x)
    k = a.graph_key()
    assert k == LF.LatentPrior.from_samples(x.clone()).graph_key()
    assert k[:3] == ('LatentPrior', 64, 64) and hash(k) is not None
    others = [LF.LatentPrior.from_samples(x, weight=2.0), LF.LatentPrior.from_samples(x, num_components=32),
              LF.LatentPrior.from_samples(x, layer_weights=[0.5, 0.5]),
              LF.LatentPrior.from_samples(x, layer_weights=[0.25, 0.75]),
              LF.LatentPrior.from_samples(x, p_space=True), LF.LatentPrior.from_samples(y),
              LF.LatentPrior.from_covariance(torch.cov(x.t()), x.mean(0) + 1.0)]
    keys = [k] + [o.graph_key() for o in others]
    assert len(set(keys)) == len(keys)
    # what the optimizer asks (optimizer/base_optimizer.py)
    from pix2latent_amd.optimizer.base_optimizer import _regularizer_key
    assert _regularizer_key(a) == k


def test_standard_normal():
    z = torch.randn(5, 128, generator=torch.Generator().manual_seed(4))
    prior = LF.LatentPrior.standard_normal(128)
    assert prior.num_components == prior.dim == 128 and prior.p_space is False
    want = (z.double() ** 2).sum(1) / 128
    got = prior(z)
    assert got.dtype == torch.float32
    assert ((got.double() - want).abs() <= 2.0 ** -23 * want).all()
    t = z.clone().requires_grad_(True)
    LF.LatentPrior.standard_normal(128, weight=0.5)(t).sum().backward()
    assert torch.allclose(t.grad, z / 128, rtol=1e-6, atol=0)


def test_argument_checks_come_before_any_launch():
    from pix2latent_amd import _native as N
    lib = N.lib()
    fake, sz = C.c_void_p(4096), C.c_size_t
    ws_bytes = lib.p2l_latent_prior_ws_bytes
    assert ws_bytes(3, 18, 512) == 3 * 18 * 512 * 8 and ws_bytes(1, 1, 1) == 8
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (65536, 1, 1), (1, 1, 513)):
        assert ws_bytes(*bad) == 0, bad

    def fwd(B=2, L=3, D=128, K=100, w=fake, basis=fake, mean=fake, lw=fake, loss=fake, ws=fake, nbytes=None):
        nbytes = B * L * K * 8 if nbytes is None else nbytes
        return lib.p2l_latent_prior_fwd(w, basis, mean, lw, B, L, D, K, 1, loss, ws, sz(max(nbytes, 0)), None)

    def bwd(B=2, L=3, D=128, K=100, w=fake, basis=fake, lw=fake, dw=fake, ws=fake, nbytes=None):
        nbytes = B * L * K * 8 if nbytes is None else nbytes
        return lib.p2l_latent_prior_bwd(w, basis, lw, None, B, L, D, K, 1, ws, sz(max(nbytes, 0)), dw, None)

    EINVAL, EWS = -1, -3
    for f in (fwd, bwd):
        assert f(D=96) == EINVAL and f(D=576, K=100) == EINVAL and f(D=0, K=0) == EINVAL      # D: multiple of 64, <= 512
        assert f(K=129) == EINVAL and f(K=0) == EINVAL                                        # 1 <= K <= D
        assert f(L=0) == EINVAL and f(B=0) == EINVAL and f(B=65536) == EINVAL
        assert f(w=None) == EINVAL and f(basis=None) == EINVAL and f(lw=None) == EINVAL
        assert f(ws=None) == EWS and f(nbytes=2 * 3 * 100 * 8 - 1) == EWS and f(ws=C.c_void_p(4100)) == EWS
    assert fwd(mean=None) == EINVAL and fwd(loss=None) == EINVAL and bwd(dw=None) == EINVAL

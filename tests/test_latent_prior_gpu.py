"""The whitened latent prior on the device (csrc/p2l_latent_prior.hip) against the fp64 reference
of tests/_latent_prior_ref.py, its statistics from the device Gram, and the term inside the closure and a replayed HIP
graph.

Bounds.  Both sides are fp64 and differ in the ORDER of their sums and in the one final rounding to fp32:
|P - P_ref| <= 2^-23 |P_ref| + 1e-12 P_abs and, elementwise, |dw - dw_ref| <= 2^-23 |dw_ref| + 1e-12 G_abs, with P_abs
and G_abs the same expressions over absolute values.  A wrong slope, a missing layer weight or a dropped component is
1e-2 or more."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _latent_prior_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE = 64
N_STAT = 16384


def _dev64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _run(w, A, m, a, p_space, dev, gloss=None):
    """(P, dw) of the raw entry points for numpy operands"""
    from pix2latent_amd import ops
    wd = w if torch.is_tensor(w) else torch.from_numpy(w).to(dev)
    Ad = _dev64(A, dev)
    lw = _dev64(a, dev)
    P, ws = ops.latent_prior_fwd(wd, Ad.t().contiguous(), _dev64(m, dev), lw, p_space)
    dw = ops.latent_prior_bwd(wd, Ad, lw, p_space, ws, gloss)
    return P, dw


CASES = [(3, 18, 512, 512, 1),      # the StyleGAN2 W+ shape
         (5, 1, 128, 128, 0),       # BigGAN z / c
         (2, 14, 512, 40, 1),       # K not a multiple of the 64-component tile, L not a multiple of the 8-row chunk
         (1, 1, 64, 1, 1)]          # smallest of everything


@pytest.mark.parametrize('B,L,D,K,p_space', CASES)
def test_against_reference(dev, B, L, D, K, p_space):
    w, A, m, a = PR.make_case(B, L, D, K, seed=B + L + K)
    gloss = np.linspace(0.5, 1.5, B).astype(np.float32)
    ref = PR.reference(w, A, m, a, p_space, gloss)
    P, dw = _run(w, A, m, a, p_space, dev, torch.from_numpy(gloss).to(dev))
    P, dw = P.double().cpu().numpy(), dw.double().cpu().numpy()
    tol_p = 2.0 ** -23 * np.abs(ref['P']) + 1e-12 * ref['P_abs']
    tol_g = 2.0 ** -23 * np.abs(ref['dw']) + 1e-12 * ref['G_abs']
    print('(%d, %d, %d, %d, %d): P %s  |P - ref| / tol %.3g  |dw - ref| / tol %.3g'
          % (B, L, D, K, p_space, ref['P'], (np.abs(P - ref['P']) / tol_p).max(),
             (np.abs(dw - ref['dw']) / np.maximum(tol_g, 1e-300)).max()))
    assert (ref['P'] > 0).all() and np.abs(ref['dw']).max() > 0
    assert (np.abs(P - ref['P']) <= tol_p).all()
    assert (np.abs(dw - ref['dw']) <= tol_g).all()


@pytest.fixture(scope='module')
def small(dev):
    """the (2, 14, 512, 40, 1) case on the device: operands, P, dw with gloss = NULL"""
    w, A, m, a = PR.make_case(2, 14, 512, 40, seed=56)
    wd = torch.from_numpy(w).to(dev)
    return (wd, A, m, a), _run(wd, A, m, a, 1, dev)


def test_exact_zero_at_the_mean(dev):
    """m_j an fp32 value where m_j >= 0 and 5 x an fp32 value where m_j < 0, w with x == m: d = 0 in every entry"""
    rs = np.random.RandomState(1)
    B, L, D, K = 2, 3, 128, 100
    _, A, _, a = PR.make_case(B, L, D, K, seed=2)
    w1 = rs.randn(D).astype(np.float32)
    w1[:4] = [0.0, -0.0, 1.0, -1.0]
    m = w1.astype(np.float64) * PR.slope(w1, True)
    w = np.ascontiguousarray(np.broadcast_to(w1, (B, L, D)))
    assert (m < 0).any() and (m > 0).any()
    P, dw = _run(w, A, m, a, 1, dev)
    assert (P == 0).all() and (dw == 0).all()
    # ... and not with the flag off (the negative entries are then 4 |w| away)
    P, dw = _run(w, A, m, a, 0, dev)
    assert (P > 0).all() and (dw != 0).any()


def test_gloss(small, dev):
    (wd, A, m, a), (P, dw) = small
    ones = _run(wd, A, m, a, 1, dev, torch.ones(2, device=dev))[1]
    assert torch.equal(ones, dw)                              # NULL = ones
    scaled = _run(wd, A, m, a, 1, dev, torch.tensor([2.0, -1.0], device=dev))[1]
    assert torch.equal(scaled[0], 2.0 * dw[0]) and torch.equal(scaled[1], -dw[1])
    zero = _run(wd, A, m, a, 1, dev, torch.tensor([0.0, 1.0], device=dev))[1]
    assert (zero[0] == 0).all() and torch.equal(zero[1], dw[1])
    # ... and through LF.latent_prior and autograd
    import pix2latent_amd.loss_functions as LF
    prior = LF.LatentPrior(A, m, weight=1.0, layer_weights=a, p_space=True, device=dev)
    t = wd.clone().requires_grad_(True)
    R = LF.latent_prior(t, prior)
    (R * torch.tensor([2.0, -1.0], device=dev)).sum().backward()
    assert torch.equal(t.grad, scaled) and torch.equal(R.detach(), P)
    t0 = wd.clone().requires_grad_(True)
    (LF.latent_prior(t0, prior) * torch.tensor([0.0, 1.0], device=dev)).sum().backward()
    assert torch.equal(t0.grad, zero)
    # the CPU path states the same numbers
    cpu = LF.latent_prior(wd.cpu(), prior).double()
    assert ((cpu - P.cpu().double()).abs() <= 2.0 ** -22 * cpu).all()


def test_bits(small, dev):
    (wd, A, m, a), (P, dw) = small
    again = _run(wd, A, m, a, 1, dev)
    assert torch.equal(again[0], P) and torch.equal(again[1], dw)
    for b in range(2):
        one = _run(wd[b:b + 1].contiguous(), A, m, a, 1, dev)
        assert torch.equal(one[0][0], P[b]) and torch.equal(one[1][0], dw[b]), b
    # ... and as another row of a larger batch
    big = _run(torch.cat([wd[1:], wd, wd[:1]]).contiguous(), A, m, a, 1, dev)
    assert torch.equal(big[0], P[[1, 0, 1, 0]]) and torch.equal(big[1], dw[[1, 0, 1, 0]])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _run(wd, A, m, a, 1, dev)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(other[0], P) and torch.equal(other[1], dw)


def test_argument_checks(small, dev):
    """refused before any launch: nothing runs on the device"""
    from pix2latent_amd import _native as N, ops
    (wd, A, m, a), _ = small
    lib = N.lib()
    B, L, D, K = 2, 14, 512, 40
    Ad = _dev64(A, dev)
    At, md, lw = Ad.t().contiguous(), _dev64(m, dev), _dev64(a, dev)
    loss, dw = torch.empty(B, device=dev), torch.empty_like(wd)
    ws = torch.empty(B * L * K, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731

    def fwd(L=L, D=D, K=K, basis=p(At), nbytes=ws.numel() * 8):
        return lib.p2l_latent_prior_fwd(p(wd), basis, p(md), p(lw), B, L, D, K, 1, p(loss), p(ws), nbytes, N.stream())

    def bwd(L=L, D=D, K=K, basis=p(Ad), nbytes=ws.numel() * 8):
        return lib.p2l_latent_prior_bwd(p(wd), basis, p(lw), None, B, L, D, K, 1, p(ws), nbytes, p(dw), N.stream())

    for f in (fwd, bwd):
        assert f(D=96) == -1 and f(K=D + 1) == -1 and f(L=0) == -1 and f(basis=None) == -1
        assert f(nbytes=ws.numel() * 8 - 8) == -3
        assert f() == 0
    with pytest.raises(N.NativeError, match='p2l_latent_prior_fwd'):
        ops.latent_prior_fwd(torch.zeros(1, 1, 96, device=dev), torch.zeros(96, 4, dtype=torch.float64, device=dev),
                             torch.zeros(96, dtype=torch.float64, device=dev),
                             torch.ones(1, dtype=torch.float64, device=dev), 0)
    torch.cuda.synchronize()


# ---- statistics and the closure: the 64^2 synthetic StyleGAN2 ------------------------------------------------------
@pytest.fixture(scope='module')
def problem(dev):
    warnings.simplefilter('ignore')
    from pix2latent_amd.utils import synthetic as S
    from pix2latent_amd.model.stylegan2 import StyleGAN2
    import pix2latent_amd.loss_functions as LF
    W = S.stylegan2_weights(SIZE, 0, channels={4: 128, 8: 128, 16: 64, 32: 32, 64: 32})
    model = StyleGAN2(model='cars', search='w+', weights=W, size=SIZE, device=dev)
    loss_fn = LF.ProjectionLoss(lpips_net='vgg', weights=S.lpips_vgg_weights(1), device=dev)
    return model, loss_fn, S.synthetic_target(SIZE, 1), S.synthetic_weight_mask(SIZE)


def _sg2_prior(model, **kw):
    """LatentPrior.stylegan2 at N_STAT samples; the draws behind the cached statistics are those of seed 11"""
    import pix2latent_amd.loss_functions as LF
    torch.manual_seed(11)
    return LF.LatentPrior.stylegan2(model, num_samples=N_STAT, **kw)


def test_p_covariance(problem, dev):
    from pix2latent_amd.edit import ganspace
    import pix2latent_amd.loss_functions as LF
    model = problem[0]
    torch.manual_seed(5)
    Cm, mean = ganspace.p_covariance(model, N_STAT, chunk_rows=4096)
    torch.manual_seed(5)
    with torch.no_grad():
        x = torch.cat([LF.to_p_space(model.mapping(torch.randn(4096, 512))).double().cpu() for _ in range(4)])
    assert (x < -1.0).any()                                   # the slope-5 side is populated
    mu = x.mean(0)
    xc = x - mu
    want = xc.t() @ xc / (N_STAT - 1)
    tr = want.diagonal().sum().item()
    err_c, err_m = (Cm - want).abs().max().item(), (mean - mu).abs().max().item()
    print('p_covariance: trace %.6g  max |C - ref| / trace %.3g  max |mean - ref| %.3g' % (tr, err_c / tr, err_m))
    assert Cm.dtype == torch.float64 and Cm.device.type == 'cpu' and Cm.shape == (512, 512)
    assert err_c <= 1e-10 * tr and err_m <= 1e-10 * tr ** 0.5
    # it is not the covariance of w
    torch.manual_seed(5)
    Cw, _ = ganspace.w_covariance(model, N_STAT, chunk_rows=4096)
    assert (Cw - Cm).abs().max().item() > 1e-3 * tr / 512


def test_stylegan2_prior_whitens_its_own_samples(problem, dev):
    import pix2latent_amd.loss_functions as LF
    model = problem[0]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        prior = _sg2_prior(model, num_components=512)
    K = prior.num_components
    print('kept K = %d of 512 (%s)' % (K, [str(r.message) for r in rec if 'LatentPrior' in str(r.message)]))
    assert prior.p_space is True and prior.dim == 512 and 1 <= K <= 512
    assert _sg2_prior(model, num_components=512).basis is prior.basis          # cached on the model
    torch.manual_seed(11)
    with torch.no_grad():
        w = model.mapping(torch.randn(N_STAT, 512)).contiguous()
    P = prior(w).double().cpu().numpy()                       # B = 16384 candidates, L = 1
    x = LF.to_p_space(w).double().cpu().numpy()
    bound = PR.rounding_bound(x, prior.basis.numpy(), prior.mean.numpy()).mean()
    diff = abs(P.mean() - (N_STAT - 1.0) / N_STAT)
    print('mean P - (N - 1) / N = %.3g, bound %.3g' % (diff, bound))
    assert bound < 1e-2
    assert diff <= bound


_DEFAULT = object()


def _start(model):
    """the two starting W+ candidates [2, n_latent, 512] and the starting noise [noise_total] (CPU)"""
    n_lat = model._desc.n_latent
    n_noise = sum(s[-2] * s[-1] for s in model.noise_shape)
    g = torch.Generator().manual_seed(4)
    z0 = model.latent_mean.cpu().view(1, 512).repeat(n_lat, 1) + 0.3 * torch.randn(n_lat, 512, generator=g)
    return torch.stack([z0, 1.25 * z0]), torch.randn(n_noise, generator=g)


def _steps(problem, dev, n_steps, use_graph, regularizer=_DEFAULT):
    """n_steps optimise steps of 2 candidates in W+ with optimised noise (an explicit variable: the model draws fresh
    noise otherwise); regularizer=_DEFAULT never passes the argument"""
    from pix2latent_amd import VariableManager
    from pix2latent_amd.optimizer import GradientOptimizer
    model, loss_fn, target, weight = problem
    z0, n0 = _start(model)
    vm = VariableManager(device=dev)
    kw = {} if regularizer is _DEFAULT else {'regularizer': regularizer}
    vm.register('z', tuple(z0.shape[1:]), 'input', learning_rate=0.05, default=z0[0], **kw)
    vm.register('noises', tuple(n0.shape), 'input', learning_rate=0.05, default=n0)
    vm.register('target', (3, SIZE, SIZE), 'output', requires_grad=False, default=target)
    vm.register('weight', (3, SIZE, SIZE), 'output', requires_grad=False, default=weight)
    opt = GradientOptimizer(model, vm, loss_fn, max_batch_size=9, use_graph=use_graph)
    variables = vm.initialize(num_samples=2)
    with torch.no_grad():
        variables.input.z.buf[1].copy_(z0[1])                 # two different candidates
    losses = []
    for i in range(n_steps):
        _, l, _ = opt.step(variables, optimize=True, transform=False)
        losses.append(np.array(l, dtype=np.float64))
    if use_graph:
        assert any(isinstance(v, tuple) for v in opt._graphs.values()), 'no graph was captured'
    return np.stack(losses), variables.input.z.buf.detach().cpu().clone(), opt


@pytest.fixture(scope='module')
def prior_weight(problem, dev):
    """the weight at which the term starts at about half the projection loss's O(1): 0.5 / mean P of the two
    starting candidates"""
    import pix2latent_amd.loss_functions as LF
    model = problem[0]
    p0 = LF.latent_prior(_start(model)[0].to(dev), _sg2_prior(model, num_components=512)).cpu()
    print('P of the starting candidates: %s' % p0.tolist())
    assert (p0 > 0).all()
    return 0.5 / p0.mean().item()


def test_closure_losses_contain_the_term(problem, dev, prior_weight):
    """the losses a step reports = loss_fn + weight P(z), recomputed from the tracked variables (no variable has a
    hook: tracked before the step is the value the step saw), to 1e-5 of the sum; both terms are visible at that bound"""
    import pix2latent_amd.loss_functions as LF
    model, loss_fn, target, weight = problem
    reg = _sg2_prior(model, num_components=512, weight=prior_weight)
    losses, _, opt = _steps(problem, dev, 2, False, regularizer=reg)
    for i in range(2):
        z, n = opt.tracked['z'][i].to(dev), opt.tracked['noises'][i].to(dev)
        with torch.no_grad():
            out = model(z=z, noises=n)
            t = target.to(dev).unsqueeze(0).expand(2, -1, -1, -1).contiguous()
            w = weight.to(dev).unsqueeze(0).expand(2, -1, -1, -1).contiguous()
            base = loss_fn(out, t, w).view(2, -1).mean(1).double().cpu().numpy()
            term = reg(z).double().cpu().numpy()
        ref = PR.reference(z.cpu().numpy(), reg.basis.numpy(), reg.mean.numpy(), None, True)
        print('step %d: loss_fn %s  weight P %s (reference %s)  reported %s'
              % (i, base, term, reg.weight * ref['P'], losses[i]))
        assert (np.abs(term - reg.weight * ref['P']) <= 1e-6 * term).all()
        assert (term > 0.01 * base).all() and (base > 0.01 * term).all()
        assert (np.abs(losses[i] - (base + term)) <= 1e-5 * (base + term)).all()


def test_closure_graph_replay_is_the_eager_trajectory(problem, dev, prior_weight):
    model = problem[0]
    make = lambda **kw: _sg2_prior(model, **dict(dict(num_components=512, weight=prior_weight), **kw))   # noqa: E731
    eager = _steps(problem, dev, 3, False, regularizer=make())
    graph = _steps(problem, dev, 3, True, regularizer=make())
    assert np.array_equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
    plain = _steps(problem, dev, 3, False)
    assert not torch.equal(plain[1], eager[1]) and (eager[0] > plain[0]).all()
    # the key of a captured step tells the priors apart
    opt = graph[2]
    (_, _, _, _, variables, _), = [v for v in opt._graphs.values() if isinstance(v, tuple)]
    k0 = opt._graph_key(variables, 0, 2)
    assert k0 in opt._graphs
    variables.input.z['regularizer'] = make(weight=2.0 * prior_weight)
    k1 = opt._graph_key(variables, 0, 2)
    variables.input.z['regularizer'] = make(num_components=64)
    k2 = opt._graph_key(variables, 0, 2)
    variables.input.z['regularizer'] = make()
    assert len({k0, k1, k2}) == 3 and opt._graph_key(variables, 0, 2) == k0


# ---- BigGAN: the class vector under the statistics of the class embeddings ------------------------------------------
def test_biggan_class_vector(dev):
    from pix2latent_amd import VariableManager
    from pix2latent_amd.optimizer import GradientOptimizer
    from pix2latent_amd.utils import synthetic as S
    from pix2latent_amd.model.biggan import BigGAN
    import pix2latent_amd.loss_functions as LF
    model = BigGAN(weights=S.biggan_weights(0), device=dev)
    loss_fn = LF.ProjectionLoss(lpips_net='vgg', weights=S.lpips_vgg_weights(1), device=dev)
    emb = model.embeddings.weight.t()
    assert tuple(emb.shape) == (1000, 128)
    g = torch.Generator().manual_seed(2)
    z0, c0 = torch.fmod(torch.randn(128, generator=g), 2.0), 0.05 * torch.randn(128, generator=g)
    unit = LF.LatentPrior.from_samples(emb, device=dev)
    p0 = unit(c0.view(1, 128).to(dev)).item()
    reg = LF.LatentPrior.from_samples(emb, weight=0.5 / p0, device=dev)
    assert reg.num_components == 128 and reg.p_space is False

    def step(**kw):
        vm = VariableManager(device=dev)
        vm.register('z', (128,), 'input', default=z0, learning_rate=0.05)
        vm.register('c', (128,), 'input', default=c0, learning_rate=0.01, **kw)
        vm.register('target', (3, 256, 256), 'output', requires_grad=False, default=S.synthetic_target(256, 1))
        vm.register('weight', (3, 256, 256), 'output', requires_grad=False, default=S.synthetic_weight_mask(256))
        opt = GradientOptimizer(model, vm, loss_fn, max_batch_size=9)
        variables = vm.initialize(num_samples=2)
        _, l, _ = opt.step(variables, optimize=True, transform=False)
        return (np.array(l, dtype=np.float64), torch.stack(list(variables.input.c.data)).detach().cpu(),
                torch.stack(list(variables.input.z.data)).detach().cpu())

    never, none, with_reg = step(), step(regularizer=None), step(regularizer=reg)
    assert np.array_equal(never[0], none[0]) and torch.equal(never[1], none[1]) and torch.equal(never[2], none[2])
    term = reg.weight * PR.reference(c0.view(1, 128).numpy(), reg.basis.numpy(), reg.mean.numpy(), None, False)['P'][0]
    print('BigGAN c: loss_fn %s  weight P(c) %.6g  reported %s' % (never[0], term, with_reg[0]))
    assert (term > 0.01 * never[0]).all() and (never[0] > 0.01 * term).all()
    assert (np.abs(with_reg[0] - (never[0] + term)) <= 1e-5 * (never[0] + term)).all()
    assert not torch.equal(with_reg[1], never[1])             # c moves differently
    assert torch.equal(with_reg[2], never[2])                 # z does not feel the term

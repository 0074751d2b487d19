"""The noise regulariser and the per-layer normalisation on the device (csrc/p2l_noise_reg.hip) against the
numpy reference of tests/_noise_ref.py, and the regulariser inside the fused closure and a replayed HIP graph.

Bounds.  corr: 1e-12 x the mean |product| of the level -- the two sides differ in the ORDER of an fp64 sum only
(at most a few hundred roundings of 1.1e-16 along any chain).  loss and dnoises: 1e-6 relative / of the largest
reference entry -- one fp32 rounding is 6e-8, a wrong level weight or a missing term is 1e-2 or more."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _noise_ref as NR  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE = 64


def _run(x, sizes, gloss=None, want_corr=True):
    from pix2latent_amd import ops
    loss, corr, ws = ops.noise_reg_fwd(x, sizes, want_corr=want_corr)
    dn = ops.noise_reg_bwd(x, sizes, ws, gloss)
    return loss, corr, dn, ws


def _check(x_np, sizes, got, what):
    """loss, corr, dnoises of the device against the reference, the bounds of the module docstring; prints first"""
    R, corr, grad, prod = NR.regularize(x_np, sizes)
    loss, c, dn = (t.cpu().numpy().astype(np.float64) for t in got[:3])
    e_corr = np.abs(c - corr) / np.maximum(prod, 1e-300)
    e_loss = np.abs(loss - R) / np.abs(R)
    gmax = np.abs(grad).max(1)
    e_grad = np.abs(dn - grad).max(1) / gmax
    print('%s: R %s  corr err / mean|prod| %.3g  loss rel %s  grad err / max %s'
          % (what, R, e_corr.max(), e_loss, e_grad))
    assert (np.abs(c - corr) <= 1e-12 * prod).all(), e_corr.max()
    assert (e_loss <= 1e-6).all(), e_loss
    assert (e_grad <= 1e-6).all(), e_grad
    return R, corr, grad


@pytest.fixture(scope='module')
def small(dev):
    """three candidates at the small layer list: white, planted horizontal correlation, white"""
    x = NR.white(3, NR.SMALL, seed=0)
    x[1] = NR.planted(x[1], NR.SMALL)
    xd = torch.from_numpy(x).to(dev)
    return x, xd, _run(xd, NR.SMALL)


def test_against_reference(small):
    x, xd, got = small
    R, _, _ = _check(x, NR.SMALL, got, 'small B=3')
    assert R[1] > R[0] + 1.0 and R[1] > R[2] + 1.0            # the planted candidate: ax = 0.48 at every level 0


def _one_layer(m, dev):
    s = m.shape[0]
    x = np.ascontiguousarray(m.reshape(1, -1), dtype=np.float32)
    return x, _run(torch.from_numpy(x).to(dev), [s])


@pytest.mark.parametrize('s', [16, 128])
def test_only_the_wrap_around_pair(dev, s):
    rs = np.random.RandomState(3)
    a, c = rs.randn(s).astype(np.float32), rs.randn(s).astype(np.float32)
    m = np.zeros((s, s), np.float32)
    m[:, 0], m[:, s - 1] = a, c
    x, got = _one_layer(m, dev)
    _, corr, _ = _check(x, [s], got, 'columns 0 and %d' % (s - 1))
    want = (a.astype(np.float64) * c.astype(np.float64)).sum() / (s * s)
    tol = 1e-12 * np.abs(a.astype(np.float64) * c).sum() / (s * s)
    assert abs(got[1][0, 0, 0].item() - want) <= tol and abs(want) > 0
    x, got = _one_layer(m.T, dev)
    _check(x, [s], got, 'rows 0 and %d' % (s - 1))
    assert abs(got[1][0, 0, 1].item() - want) <= tol


@pytest.mark.parametrize('s', [32, 256, 1024])
def test_checkerboard(dev, s):
    yy, xx = np.mgrid[0:s, 0:s]
    m = (1.0 - 2.0 * ((yy + xx) & 1)).astype(np.float32)
    x, (loss, corr, dn, ws) = _one_layer(m, dev)
    corr = corr.cpu().numpy()[0]
    assert (corr[0] == -1.0).all() and (corr[1:] == 0.0).all() and corr.shape[0] == len(NR._sides(s))
    assert loss.item() == 2.0
    from pix2latent_amd import ops
    assert (ops.noise_reg_ws_pooled(ws, [s], 1) == 0).all()
    # both neighbour sums are -2 n: g = (2 / s^2) ((-1)(-2 n) + (-1)(-2 n)) = 8 n / s^2, exactly
    assert torch.equal(dn.cpu(), torch.from_numpy(x * np.float32(8.0 / (s * s))))


def test_cells_pool_bit_for_bit(dev):
    s = 128
    cells = np.random.RandomState(5).randn(s // 2, s // 2).astype(np.float32)
    x, got = _one_layer(np.kron(cells, np.ones((2, 2), np.float32)), dev)
    _check(x, [s], got, '2x2 cells')
    from pix2latent_amd import ops
    pooled = ops.noise_reg_ws_pooled(got[3], [s], 1).cpu().numpy()[0]
    assert np.array_equal(pooled[:cells.size], cells.reshape(-1))
    want = np.concatenate([p.reshape(-1) for p in NR.pyramid(x.reshape(s, s))[1:]])
    assert np.array_equal(pooled, want)                       # every level, in fp32 with the stated association


def test_gloss(small, dev):
    x, xd, (_, _, dn, _) = small
    ones = _run(xd, NR.SMALL, torch.ones(3, device=dev))[2]
    assert torch.equal(ones, dn)                              # NULL = ones
    g = torch.tensor([0.0, 2.0, -1.0], device=dev)
    scaled = _run(xd, NR.SMALL, g)[2]
    assert (scaled[0] == 0).all()
    assert torch.equal(scaled[1], 2.0 * dn[1]) and torch.equal(scaled[2], -dn[2])
    # ... and through autograd
    import pix2latent_amd.loss_functions as LF
    t = xd.clone().requires_grad_(True)
    R = LF.noise_regularize(t, [[1, 1, s, s] for s in NR.SMALL])
    (R * g).sum().backward()
    assert torch.equal(t.grad, scaled) and torch.equal(R.detach(), small[2][0])


def test_bits(small, dev):
    x, xd, (loss, corr, dn, _) = small
    again = _run(xd, NR.SMALL)
    assert torch.equal(again[0], loss) and torch.equal(again[1], corr) and torch.equal(again[2], dn)
    for b in range(3):
        one = _run(xd[b:b + 1].contiguous(), NR.SMALL)
        assert torch.equal(one[0][0], loss[b]) and torch.equal(one[1][0], corr[b]) and torch.equal(one[2][0], dn[b]), b
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _run(xd, NR.SMALL)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(other[0], loss) and torch.equal(other[1], corr) and torch.equal(other[2], dn)


def test_ffhq_1024_layer_list(dev):
    x = NR.white(1, NR.FFHQ1024, seed=7)
    got = _run(torch.from_numpy(x).to(dev), NR.FFHQ1024)
    assert got[1].shape == (1, 73, 2)
    _check(x, NR.FFHQ1024, got, 'FFHQ-1024 B=1')


def test_noise_normalize(dev):
    from pix2latent_amd.utils import function_hooks as hook
    x = NR.white(3, NR.SMALL, seed=9) * np.float32(3.0) + np.float32(0.5)
    x[1] *= np.float32(0.01)
    h = hook.NoiseNormalize([[1, 1, s, s] for s in NR.SMALL])
    assert h.stochastic is False and h.graph_safe is True
    rows = torch.from_numpy(x).to(dev)
    h.apply_batched(rows)
    got = rows.cpu().numpy().astype(np.float64)
    ref = NR.normalize(x, NR.SMALL)
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print('normalise: err / max(1, |ref|) = %.3g (bound %.3g)' % (err.max(), 2.0 ** -22))
    assert err.max() <= 2.0 ** -22
    off = 0
    for s in NR.SMALL:
        n = got[:, off:off + s * s]
        mean = n.mean(1)
        std = np.sqrt(((n - mean[:, None]) ** 2).sum(1) / (s * s - 1))
        assert (np.abs(mean) <= 1e-6).all() and (np.abs(std - 1.0) <= 1e-6).all(), (s, mean, std)
        off += s * s
    for b in range(3):
        one = torch.from_numpy(x[b:b + 1]).to(dev)
        h.apply_batched(one)
        assert torch.equal(one[0], rows[b]), b
    per_sample = [torch.from_numpy(x[2]).to(dev)]
    h(per_sample)                                             # the reference's call form
    assert torch.equal(per_sample[0], rows[2])


# ---- the fused closure -------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def problem(dev):
    import warnings
    warnings.simplefilter('ignore')
    from pix2latent_amd.utils import synthetic as S
    from pix2latent_amd.model.stylegan2 import StyleGAN2
    import pix2latent_amd.loss_functions as LF
    W = S.stylegan2_weights(SIZE, 0, channels={4: 128, 8: 128, 16: 64, 32: 32, 64: 32})
    model = StyleGAN2(model='cars', search='w+', weights=W, size=SIZE, device=dev)
    loss_fn = LF.ProjectionLoss(lpips_net='vgg', weights=S.lpips_vgg_weights(1), device=dev)
    return model, loss_fn, S.synthetic_target(SIZE, 1), S.synthetic_weight_mask(SIZE)


_DEFAULT = object()


def _steps(problem, dev, n_steps, use_graph, regularizer=_DEFAULT, with_hook=True):
    """n_steps optimise steps of 2 candidates in W+ with optimised noise; regularizer=_DEFAULT never passes the
    argument"""
    from pix2latent_amd import VariableManager
    from pix2latent_amd.optimizer import GradientOptimizer
    from pix2latent_amd.utils import function_hooks as hook
    model, loss_fn, target, weight = problem
    n_lat = model._desc.n_latent
    n_noise = sum(s[-2] * s[-1] for s in model.noise_shape)
    g = torch.Generator().manual_seed(4)
    vm = VariableManager(device=dev)
    vm.register('z', (n_lat, 512), 'input', learning_rate=0.05,
                default=model.latent_mean.cpu().view(1, 512).repeat(n_lat, 1))
    kw = {} if regularizer is _DEFAULT else {'regularizer': regularizer}
    vm.register('noises', (n_noise,), 'input', learning_rate=0.05,
                default=torch.randn(n_noise, generator=g) * 1.5 + 0.1,
                hook_fn=hook.NoiseNormalize(model.noise_shape) if with_hook else None, **kw)
    vm.register('target', (3, SIZE, SIZE), 'output', requires_grad=False, default=target)
    vm.register('weight', (3, SIZE, SIZE), 'output', requires_grad=False, default=weight)
    opt = GradientOptimizer(model, vm, loss_fn, max_batch_size=9, use_graph=use_graph)
    variables = vm.initialize(num_samples=2)
    with torch.no_grad():
        variables.input.noises.buf[1].mul_(0.5).add_(torch.roll(variables.input.noises.buf[1], 1, 0))
    losses = []
    for i in range(n_steps):
        _, l, _ = opt.step(variables, optimize=True, transform=False)
        losses.append(np.array(l, dtype=np.float64))
    if use_graph:
        assert any(isinstance(v, tuple) for v in opt._graphs.values()), 'no graph was captured'
    return (np.stack(losses), variables.input.z.buf.detach().cpu().clone(),
            variables.input.noises.buf.detach().cpu().clone(), opt)


def test_fused_closure_losses_contain_the_term(problem, dev):
    """the losses a step reports = loss_fn + weight R(noises after the hook), recomputed from the tracked variables
    (tracked BEFORE the step's hook).  weight 1 here: both terms are O(1), so 1e-5 of the sum sees either"""
    import pix2latent_amd.loss_functions as LF
    from pix2latent_amd.utils import function_hooks as hook
    model, loss_fn, target, weight = problem
    reg = LF.NoiseRegularizer(model.noise_shape, weight=1.0)
    losses, _, _, opt = _steps(problem, dev, 2, False, regularizer=reg)
    tracked = opt.tracked
    for i in range(2):
        z, n = tracked['z'][i].to(dev), tracked['noises'][i].to(dev).clone()
        hook.NoiseNormalize(model.noise_shape).apply_batched(n)
        with torch.no_grad():
            out = model(z=z, noises=n)
            t = target.to(dev).unsqueeze(0).expand(2, -1, -1, -1).contiguous()
            w = weight.to(dev).unsqueeze(0).expand(2, -1, -1, -1).contiguous()
            base = loss_fn(out, t, w).view(2, -1).mean(1).double().cpu().numpy()
            term = LF.noise_regularize(n, model.noise_shape).double().cpu().numpy()
        R = NR.regularize(n.cpu().numpy(), [s[-1] for s in model.noise_shape])[0]
        print('step %d: loss_fn %s  R %s (reference %s)  reported %s' % (i, base, term, R, losses[i]))
        assert (np.abs(term - R) <= 1e-6 * R).all()
        assert (term > 0.01 * base).all()                       # the term is visible at the bound below
        assert (np.abs(losses[i] - (base + term)) <= 1e-5 * (base + term)).all()


def test_fused_closure_graph_replay_is_the_eager_trajectory(problem, dev):
    import pix2latent_amd.loss_functions as LF
    model = problem[0]
    eager = _steps(problem, dev, 3, False, regularizer=LF.NoiseRegularizer(model.noise_shape))
    graph = _steps(problem, dev, 3, True, regularizer=LF.NoiseRegularizer(model.noise_shape))
    assert np.array_equal(eager[0], graph[0])
    assert torch.equal(eager[1], graph[1]) and torch.equal(eager[2], graph[2])
    # the key of a captured step tells the regularisers apart
    opt = graph[3]
    from pix2latent_amd.variable_manager import slice_vars
    (_, _, _, _, variables, _), = [v for v in opt._graphs.values() if isinstance(v, tuple)]
    k0 = opt._graph_key(variables, 0, 2)
    variables.input.noises['regularizer'] = LF.NoiseRegularizer(model.noise_shape, weight=10.0)
    k1 = opt._graph_key(variables, 0, 2)
    variables.input.noises['regularizer'] = None
    assert k0 != k1 and k1 != opt._graph_key(variables, 0, 2) and k0 in opt._graphs


def test_regularizer_none_is_the_parent_behaviour(problem, dev):
    never = _steps(problem, dev, 3, False)
    none = _steps(problem, dev, 3, False, regularizer=None)
    assert np.array_equal(never[0], none[0])
    assert torch.equal(never[1], none[1]) and torch.equal(never[2], none[2])
    import pix2latent_amd.loss_functions as LF
    with_reg = _steps(problem, dev, 3, False, regularizer=LF.NoiseRegularizer(problem[0].noise_shape))
    assert not torch.equal(with_reg[2], never[2]) and (with_reg[0] > never[0]).all()

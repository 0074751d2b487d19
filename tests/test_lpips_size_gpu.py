"""`lpips_size` on the device: the three kernels of csrc/p2l_pool.hip against their definitions bit for bit, the
pooled loss against its composition from the parent path bit for bit and against the fp64 oracle, the default path
untouched, the caches, and the fused closure (graph replay, two lanes).

test_against_the_fp64_oracle prints what it measures; on the MI355X (vgg, 128^2 -> 64^2, B = 3): |loss - ref64|
1.48e-08 (bar 1e-3), LPIPS term 3.11e-11 (bar 1e-4), d loss / d out relative L2 to the fp64 oracle 1.96e-05 with the
fp32 oracle at 9.97e-08 (bar 3.0 x that + 2e-4)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# [B, C, H, W], f: non-square with quotient width 12; quotient width 5 (odd); f = 8; f = 16
SHAPES = [((2, 3, 8, 24), 2), ((3, 3, 16, 20), 4), ((1, 3, 32, 32), 8), ((2, 3, 64, 48), 16)]
# ... and f = 2 on a width that is no multiple of 4: the 8-byte path
SHAPES_ALL = SHAPES + [((2, 3, 6, 10), 2)]


def _inputs(shape, seed):
    """random in [-1, 1], plus one image of all -1.0 and one holding +-0.0 and denormals"""
    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, Cc, H, W, generator=g) * 2 - 1
    ones = torch.full((1, Cc, H, W), -1.0)
    pick = torch.randint(0, 6, (1, Cc, H, W), generator=g)
    vals = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -3e-39])
    assert (vals[2:].abs() < 1.1754944e-38).all() and (vals[2:] != 0).all()      # denormals, not flushed on the host
    return torch.cat([x, ones, vals[pick]])


def _expand(x, f):
    return x.repeat_interleave(f, 2).repeat_interleave(f, 3)


@pytest.mark.parametrize('shape,f', SHAPES_ALL)
def test_pool_kernels_are_the_definition(dev, shape, f):
    import pix2latent_amd.loss_functions as LF
    from pix2latent_amd import ops
    x = _inputs(shape, 10 + f)
    want = LF.area_pool_torch(x, f)                                   # on the CPU, fp32
    xd = x.to(dev)
    got = ops.area_pool_nchw(xd, f)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(torch.signbit(got.cpu()), torch.signbit(want))     # (-0.0 == +0.0 for torch.equal)
    packed = ops.area_pool3_to_nhwc16(xd, f).cpu()
    assert packed.shape == (x.size(0), shape[2] // f, shape[3] // f, 16)
    assert torch.equal(packed[..., :3].permute(0, 3, 1, 2), want)
    assert torch.equal(torch.signbit(packed[..., :3].permute(0, 3, 1, 2)), torch.signbit(want))
    assert (packed[..., 3:] == 0).all() and not torch.signbit(packed[..., 3:]).any()      # exactly +0.0
    # the product form, with a 0/1 mask
    m = (torch.rand(x.shape, generator=torch.Generator().manual_seed(f)) > 0.4).float()
    got_m = ops.area_pool_nchw(xd, f, mul=m.to(dev)).cpu()
    want_m = LF.area_pool_torch(x * m, f)
    assert torch.equal(got_m, want_m) and torch.equal(torch.signbit(got_m), torch.signbit(want_m))
    # an image's bits do not depend on the batch around it
    for b in range(x.size(0)):
        one = xd[b:b + 1].contiguous()
        assert torch.equal(ops.area_pool_nchw(one, f)[0], got[b]), b
        assert torch.equal(ops.area_pool3_to_nhwc16(one, f)[0].cpu(), packed[b]), b


@pytest.mark.parametrize('shape,f', SHAPES_ALL)
def test_unpool_kernel_is_its_definition(dev, shape, f):
    from pix2latent_amd import ops
    B, _, H, W = shape
    g = torch.Generator().manual_seed(20 + f)
    small = _inputs((B, 16, H // f, W // f), 30 + f).permute(0, 2, 3, 1).contiguous()      # [B+2, h, w, 16]
    Bn = small.size(0)
    full = torch.rand(Bn, H, W, 16, generator=g) * 2 - 1
    full[1, ..., :3] = 0.0
    s3 = _expand(small[..., :3].permute(0, 3, 1, 2), f) / float(f * f)
    want = full[..., :3].permute(0, 3, 1, 2) + s3
    got = ops.area_unpool16_add_nchw3(small.to(dev), full.to(dev), f).cpu()
    assert torch.equal(got, want) and torch.equal(torch.signbit(got), torch.signbit(want))
    # the second term alone: written, not accumulated into
    out = torch.full((Bn, 3, H, W), float('nan'), device=dev)
    ops.area_unpool16_add_nchw3(small.to(dev), None, f, out=out)
    assert torch.equal(out.cpu(), s3) and torch.equal(torch.signbit(out.cpu()), torch.signbit(s3))
    one = ops.area_unpool16_add_nchw3(small[1:2].to(dev).contiguous(), full[1:2].to(dev).contiguous(), f)
    assert torch.equal(one[0].cpu(), got[1])


# ---- the pooled loss -------------------------------------------------------------------------------------------
def _weights(net):
    from pix2latent_amd.utils import synthetic as S
    return {'vgg': S.lpips_vgg_weights, 'alex': S.lpips_alex_weights, 'squeeze': S.lpips_squeeze_weights}[net]()


_CASES = {}


def _case(size, B=3):
    """out, target, weight [B,3,size,size] on the CPU, made once per size"""
    if size not in _CASES:
        from pix2latent_amd.utils import synthetic as S
        g = torch.Generator().manual_seed(size)
        target = S.synthetic_target(size, 1).unsqueeze(0).repeat(B, 1, 1, 1)
        weight = S.synthetic_weight_mask(size).unsqueeze(0).repeat(B, 1, 1, 1)
        out = (target + 0.2 * torch.randn(B, 3, size, size, generator=g)).clamp(-1, 1)
        _CASES[size] = (out, target.contiguous(), weight.contiguous())
    return _CASES[size]


def _composition(dev, net, size, lpips_size, with_mask):
    import warnings
    warnings.simplefilter('ignore')
    import pix2latent_amd.loss_functions as LF
    from pix2latent_amd import ops
    f, beta = size // lpips_size, 10
    Wn = _weights(net)
    out0, target, weight = (t.to(dev) for t in _case(size))
    mask = None
    if with_mask:
        mask = (torch.rand(1, 1, size, size, generator=torch.Generator().manual_seed(9)) > 0.3).float().to(dev)
    loss_fn = LF.ProjectionLoss(lpips_net=net, weights=Wn, device=dev, lpips_size=lpips_size)
    out = out0.clone().requires_grad_(True)
    loss = loss_fn(out, target, weight, mask)
    loss.sum().backward()
    eng = loss_fn._engine
    last_l1, last_lp = eng.last_l1.clone(), eng.last_lpips.clone()

    # the parent path on the three natively pooled tensors, and the L1-only native path at full resolution
    mask3 = None if mask is None else mask.expand_as(weight).contiguous()
    po = ops.area_pool_nchw(out0, f).requires_grad_(True)
    pt, pw = ops.area_pool_nchw(target, f), ops.area_pool_nchw(weight, f, mul=mask3)
    lp = LF.PerceptualLoss(net=net, weights=Wn, device=dev)(po, pt, pw)
    (beta * lp).sum().backward()
    o1 = out0.clone().requires_grad_(True)
    l1 = LF.ReconstructionLoss()(o1, target, weight, mask)
    l1.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(last_lp, lp.detach())
    assert torch.equal(last_l1, l1.detach())
    small = _expand(po.grad.cpu(), f) / float(f * f)                 # (assembled on the CPU: IEEE, denormals kept)
    assert torch.equal(out.grad.cpu(), o1.grad.cpu() + small)
    assert po.grad.abs().max().item() > 0 and o1.grad.abs().max().item() > 0
    # the value: l1 + beta * lp, one or two roundings of fp32 whichever way the device forms it
    ref = l1.detach().double() + beta * lp.detach().double()
    assert ((loss.detach().double() - ref).abs() <= 2.0 ** -22 * ref.abs()).all()
    # PerceptualLoss(lpips_size=...) is the second term alone
    o2 = out0.clone().requires_grad_(True)
    per = LF.PerceptualLoss(net=net, weights=Wn, device=dev, lpips_size=lpips_size)
    lp2 = per(o2, target, weight, mask)
    (beta * lp2).sum().backward()
    assert torch.equal(lp2.detach(), lp.detach())
    assert torch.equal(o2.grad.cpu(), small)


@pytest.mark.parametrize('net', ['alex', 'vgg', 'squeeze'])
def test_composition_is_exact(dev, net):
    _composition(dev, net, 128, 64, False)


def test_composition_is_exact_f4_with_a_mask(dev):
    _composition(dev, 'alex', 256, 64, True)


def _rel(a, b):
    a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
    return ((a - b).norm() / b.norm()).item()


def test_against_the_fp64_oracle(dev):
    """reference: oracle.lpips_ref.reconstruction_loss + beta * perceptual_loss of F.avg_pool2d inputs; the bars of
    tests/test_model_gpu.py"""
    import warnings
    warnings.simplefilter('ignore')
    import pix2latent_amd.loss_functions as LF
    from oracle import lpips_ref as L
    Wv = _weights('vgg')
    out0, target, weight = _case(128)

    def oracle(dtype):
        W = {k: v.to(dtype) for k, v in Wv.items()}
        o = out0.to(dtype).clone().requires_grad_(True)
        t, w = target.to(dtype), weight.to(dtype)
        rec = L.reconstruction_loss(o, t, w)
        per = L.perceptual_loss(W, F.avg_pool2d(o, 2), F.avg_pool2d(t, 2), F.avg_pool2d(w, 2))
        loss = rec + 10 * per
        loss.mean().backward()
        return loss.detach(), per.detach(), o.grad
    loss64, per64, g64 = oracle(torch.float64)
    _, _, g32 = oracle(torch.float32)
    loss_fn = LF.ProjectionLoss(lpips_net='vgg', weights=Wv, device=dev, lpips_size=64)
    out = out0.to(dev).requires_grad_(True)
    loss = loss_fn(out, target.to(dev), weight.to(dev))
    loss.mean().backward()
    torch.cuda.synchronize()
    d_loss = (loss.detach().cpu().double() - loss64).abs().max().item()
    d_per = (loss_fn._engine.last_lpips.cpu().double() - per64).abs().max().item()
    dist, floor = _rel(out.grad, g64), _rel(g32, g64)
    print('lpips_size 128 -> 64, vgg: |loss - ref64| %.3g  LPIPS term %.3g  d loss / d out vs fp64: native %.3g, '
          'fp32 oracle %.3g' % (d_loss, d_per, dist, floor))
    assert d_loss < 1e-3
    assert d_per < 1e-4
    assert dist < 3.0 * floor + 2e-4


def test_none_and_full_size_are_the_parent_behaviour(dev):
    import warnings
    warnings.simplefilter('ignore')
    import pix2latent_amd.loss_functions as LF
    Wn = _weights('alex')
    out0, target, weight = (t.to(dev) for t in _case(64))

    def run(cls, **kw):
        fn = cls(weights=Wn, device=dev, **kw)
        o = out0.clone().requires_grad_(True)
        loss = fn(o, target, weight)
        loss.mean().backward()
        return loss.detach(), o.grad
    for cls in (LF.ProjectionLoss, LF.PerceptualLoss):
        base = run(cls)
        for s in (None, 64):
            got = run(cls, lpips_size=s)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (cls, s)


def test_caching(dev):
    import warnings
    warnings.simplefilter('ignore')
    import pix2latent_amd.loss_functions as LF
    loss_fn = LF.ProjectionLoss(lpips_net='alex', weights=_weights('alex'), device=dev, lpips_size=64)
    out0, target, weight = (t.to(dev).clone() for t in _case(128))
    eng = loss_fn._engine
    calls, inner = [], eng.f_prepare

    def counting(*a):
        calls.append(1)
        return inner(*a)
    eng.f_prepare = counting
    pooled_ptr = lambda: next(reversed(eng._pooled.values())).target.data_ptr()
    first = loss_fn(out0, target, weight)
    assert len(calls) == 1 and len(eng._pooled) == 1
    p0 = pooled_ptr()
    second = loss_fn(out0, target, weight)
    assert len(calls) == 1 and len(eng._pooled) == 1 and pooled_ptr() == p0
    assert torch.equal(first, second)
    target.mul_(0.5)                                            # in place: same storage, new version
    third = loss_fn(out0, target, weight)
    assert len(calls) == 2 and len(eng._pooled) == 2 and pooled_ptr() != p0
    assert not torch.equal(third, first)
    fresh = LF.ProjectionLoss(lpips_net='alex', weights=_weights('alex'), device=dev, lpips_size=64)
    assert torch.equal(fresh(out0, target, weight), third)


# ---- the fused closure -----------------------------------------------------------------------------------------
SIZE = 128


@pytest.fixture(scope='module')
def problem(dev):
    import warnings
    warnings.simplefilter('ignore')
    from pix2latent_amd.utils import synthetic as S
    from pix2latent_amd.model.stylegan2 import StyleGAN2
    import pix2latent_amd.loss_functions as LF
    W = S.stylegan2_weights(SIZE, 0, channels={4: 128, 8: 128, 16: 64, 32: 32, 64: 32, 128: 32})
    model = StyleGAN2(model='cars', search='w+', weights=W, size=SIZE, device=dev)
    loss_fn = LF.ProjectionLoss(lpips_net='vgg', weights=S.lpips_vgg_weights(1), device=dev, lpips_size=64)
    return model, loss_fn, S.synthetic_target(SIZE, 1), S.synthetic_weight_mask(SIZE)


def _steps(problem, dev, n_steps, use_graph, num_samples=2, max_batch_size=9, rows=None):
    """n_steps optimise steps of `num_samples` candidates in W+; candidate i starts from row rows[i] of one seeded
    set of latents"""
    from pix2latent_amd import VariableManager
    from pix2latent_amd.optimizer import GradientOptimizer
    model, loss_fn, target, weight = problem
    n_lat = model._desc.n_latent
    n_noise = sum(s[-2] * s[-1] for s in model.noise_shape)
    g = torch.Generator().manual_seed(4)
    noise0 = torch.randn(n_noise, generator=g)
    start = 0.3 * torch.randn(4, n_lat, 512, generator=g)
    vm = VariableManager(device=dev)
    vm.register('z', (n_lat, 512), 'input', learning_rate=0.05,
                default=model.latent_mean.cpu().view(1, 512).repeat(n_lat, 1))
    vm.register('noises', (n_noise,), 'input', learning_rate=0.05, default=noise0)
    vm.register('target', (3, SIZE, SIZE), 'output', requires_grad=False, default=target)
    vm.register('weight', (3, SIZE, SIZE), 'output', requires_grad=False, default=weight)
    opt = GradientOptimizer(model, vm, loss_fn, max_batch_size=max_batch_size, use_graph=use_graph)
    variables = vm.initialize(num_samples=num_samples)
    rows = list(range(num_samples)) if rows is None else rows
    with torch.no_grad():
        variables.input.z.buf.add_(start[rows].to(dev))
    losses = []
    for i in range(n_steps):
        _, l, _ = opt.step(variables, optimize=True, transform=False)
        losses.append(np.array(l, dtype=np.float64))
    if use_graph:
        assert any(isinstance(v, tuple) for v in opt._graphs.values()), 'no graph was captured'
    return np.stack(losses), variables.input.z.buf.detach().cpu().clone(), opt


def test_fused_closure_graph_replay_is_the_eager_trajectory(problem, dev):
    eager = _steps(problem, dev, 3, False)
    graph = _steps(problem, dev, 3, True)
    assert np.isfinite(eager[0]).all() and (eager[0][0, 0] != eager[0][0, 1])
    assert np.array_equal(eager[0], graph[0])
    assert torch.equal(eager[1], graph[1])
    # candidate 0 alone: its first loss (later ones follow an update scaled by another chunk size)
    alone = _steps(problem, dev, 1, False, num_samples=1, rows=[0])
    assert alone[0][0, 0] == eager[0][0, 0]
    # the key of a captured step tells two loss objects, and two sizes, apart
    opt = graph[2]
    (_, _, _, _, variables, _), = [v for v in opt._graphs.values() if isinstance(v, tuple)]
    k0 = opt._graph_key(variables, 0, 2)
    assert k0 in opt._graphs
    opt.loss_fn.lpips_size = 32
    assert opt._graph_key(variables, 0, 2) != k0
    opt.loss_fn.lpips_size = 64
    assert opt._graph_key(variables, 0, 2) == k0


def test_two_lanes_are_the_bits_of_one(problem, dev, monkeypatch):
    model, loss_fn = problem[0], problem[1]
    two = _steps(problem, dev, 3, False, num_samples=4, max_batch_size=2)
    assert len(loss_fn._engine._lanes) == 2 and loss_fn._engine._lanes[1].full16 is not None
    monkeypatch.setenv('P2L_STREAMS', '1')
    one = _steps(problem, dev, 3, False, num_samples=4, max_batch_size=2)
    assert np.array_equal(one[0], two[0]) and torch.equal(one[1], two[1])
    alone = _steps(problem, dev, 1, False, num_samples=1, rows=[0])
    assert alone[0][0, 0] == two[0][0, 0]
    # the side lane's scratch, the full-resolution staging included, goes with drop_side_scratch
    from pix2latent_amd import lanes
    gen = loss_fn._engine._scratch.generation
    lanes.drop_side_scratch(model, loss_fn._engine)
    assert list(loss_fn._engine._lanes) == [0] and loss_fn._engine._scratch.generation == gen + 1

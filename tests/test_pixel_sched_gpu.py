"""The weighted L2 pixel term (csrc/p2l_pixel.hip) and the scheduled Adam step (p2l_adam_step_sched) on the device
(DESIGN.md section 14): the kernels against the fp64 reference of tests/_pixel_sched_ref.py, their bits, their
argument checks, the term inside ProjectionLoss / ReconstructionLoss, and a schedule inside the closure and a replayed
HIP graph.

Bounds (u = 2^-24), derived and not measured.  Forward: every term w m (t - o)^2 is >= 0 and carries at most four
roundings, a sample's 3 H W terms are added with at most 3 H W - 1 roundings in any order, one division:
|loss - ref| <= (3 H W + 8) u ref.  Backward: (gscale / wsum) 2 (w m) (o - t) is six roundings (the division, w m,
o - t, three products), the bound allows seven: |d - ref| <= 7 u |ref| + 1e-37; accumulated onto q one more, u |q + ref|.  A missing mask, a wrong plane stride,
an unsquared difference or a missing factor 2 are 1e-2 or more at these inputs."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pixel_sched_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
G = 256                               # guard floats on either side of every output
SENT = 0x4EADBEEF                     # sentinel bit pattern (a finite float, ~1.46e9)
EINVAL = -1


class Out(object):
    """n floats between two guard bands, everything pre-filled with the sentinel (or, the n floats, with `prefill`)"""

    def __init__(self, n, dev, prefill=None):
        self.n = n
        self.full = torch.full((n + 2 * G,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
        self.t = self.full[G:G + n]
        if prefill is not None:
            self.t.copy_(prefill.reshape(-1))

    def guards_ok(self):
        torch.cuda.synchronize()
        bits = self.full.view(torch.int32)
        return bool((bits[:G] == SENT).all()) and bool((bits[G + self.n:] == SENT).all())

    def untouched(self):
        return self.guards_ok() and bool((self.t.view(torch.int32) == SENT).all())

    def numpy(self, *shape):
        assert self.guards_ok(), 'guard band written'
        return self.t.cpu().numpy().reshape(*shape)


@pytest.fixture(scope='module')
def lib():
    from pix2latent_amd import _native as N
    return N.lib()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Case(object):
    """operands of one (Bn, H, W, mask) case on the device; img16 carries random floats 3..15"""

    def __init__(self, Bn, H, W, with_mask, dev, seed=None):
        self.shape = (Bn, H, W)
        seed = Bn * 1000 + H * 10 + W + int(with_mask) if seed is None else seed
        self.np = R.make_case(Bn, H, W, with_mask, seed)
        out, target, weight, mask, wsum, gscale = self.np
        self.img16_np = R.pad16(out, rs=np.random.RandomState(seed + 1))
        d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)    # noqa: E731
        self.img16, self.target, self.weight, self.mask, self.wsum, self.gscale = (
            d(self.img16_np), d(target), d(weight), d(mask), d(wsum), d(gscale))
        self.dev = dev

    def rows(self, lo, hi):
        """samples [lo, hi) as a case of their own (contiguous copies)"""
        c = object.__new__(Case)
        c.shape, c.dev = (hi - lo,) + self.shape[1:], self.dev
        for k in ('img16', 'target', 'weight', 'mask', 'wsum', 'gscale'):
            t = getattr(self, k)
            setattr(c, k, None if t is None else t[lo:hi].clone())
        return c

    def fwd(self, lib, **kw):
        Bn, H, W = self.shape
        nblk = lib.p2l_l2_loss_nblk(H, W)
        loss, part = Out(Bn, self.dev), Out(Bn * nblk, self.dev)
        a = dict(img16=_p(self.img16), target=_p(self.target), weight=_p(self.weight), mask=_p(self.mask),
                 wsum=_p(self.wsum), loss=_p(loss.t), part=_p(part.t), Bn=Bn, H=H, W=W)
        a.update(kw)
        rc = lib.p2l_l2_loss_fwd(a['img16'], a['target'], a['weight'], a['mask'], a['wsum'], a['loss'], a['part'],
                                 a['Bn'], a['H'], a['W'], _stream())
        return rc, loss, part

    def bwd(self, lib, accumulate, prior=None, **kw):
        Bn, H, W = self.shape
        d = Out(Bn * H * W * 16, self.dev, prefill=prior)
        a = dict(img16=_p(self.img16), target=_p(self.target), weight=_p(self.weight), mask=_p(self.mask),
                 wsum=_p(self.wsum), gscale=_p(self.gscale), d=_p(d.t), Bn=Bn, H=H, W=W)
        a.update(kw)
        rc = lib.p2l_l2_loss_bwd(a['img16'], a['target'], a['weight'], a['mask'], a['wsum'], a['gscale'], a['d'],
                                 a['Bn'], a['H'], a['W'], accumulate, _stream())
        return rc, d


# (2,4,4) fewer pixels than a thread group's block; (3,17,15) 255 pixels, H W % 4 != 0: the 4-byte path with a ragged
# last thread; (2,16,20) 320 pixels: the 16-byte path; (1,64,64) several blocks; and, beyond the issue's four, a ragged
# last block on either path: (2,40,52) = 2080 pixels on the 16-byte path, (2,33,35) = 1155 on the 4-byte one
SHAPES = [(2, 4, 4), (3, 17, 15), (2, 16, 20), (1, 64, 64), (2, 40, 52), (2, 33, 35)]


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('Bn,H,W', SHAPES)
def test_l2_kernels_against_fp64(dev, lib, Bn, H, W, with_mask):
    c = Case(Bn, H, W, with_mask, dev)
    out, target, weight, mask, wsum, gscale = c.np
    ref_loss, ref_d = R.l2_reference(out, target, weight, mask, wsum, gscale)
    HW = H * W
    ref_rows = ref_d.reshape(Bn, 3, HW).transpose(0, 2, 1)                     # [B, HW, 3]
    assert (ref_loss > 1e-2).all() and (np.abs(ref_rows).max(axis=(1, 2)) > 0).all()
    assert (weight == 0).any() and (gscale < 0).any() == (Bn > 1)

    rc, loss, part = c.fwd(lib)
    assert rc == 0
    got = loss.numpy(Bn).astype(np.float64)
    assert part.guards_ok()
    tol = (3 * HW + 8) * U * ref_loss
    print('(%d, %d, %d) mask %d: loss %s  |loss - ref| / bound %.3g' % (Bn, H, W, with_mask, ref_loss,
                                                                       (np.abs(got - ref_loss) / tol).max()))
    assert (np.abs(got - ref_loss) <= tol).all()

    rc, d0 = c.bwd(lib, 0)
    assert rc == 0
    d = d0.numpy(Bn, HW, 16)
    tol_d = 7 * U * np.abs(ref_rows) + 1e-37
    err = np.abs(d[:, :, :3].astype(np.float64) - ref_rows)
    print('    backward: max |d - ref| / bound %.3g' % (err / tol_d).max())
    assert (err <= tol_d).all()
    assert (d[:, :, 3:] == 0).all()                                            # floats 3..15 exactly 0

    q = np.random.RandomState(7).uniform(-1e-3, 1e-3, (Bn, HW, 16)).astype(np.float32)
    rc, d1 = c.bwd(lib, 1, prior=torch.from_numpy(q))
    assert rc == 0
    a = d1.numpy(Bn, HW, 16)
    want = q[:, :, :3].astype(np.float64) + ref_rows
    tol_a = tol_d + U * np.abs(want)
    err = np.abs(a[:, :, :3].astype(np.float64) - want)
    print('    accumulate: max |d - (q + ref)| / bound %.3g' % (err / tol_a).max())
    assert (err <= tol_a).all()
    assert np.array_equal(a[:, :, 4:].view(np.int32), q[:, :, 4:].view(np.int32))     # 4..15 to the bit
    assert np.array_equal(a[:, :, 3], q[:, :, 3])                                        # 3 in value


@pytest.mark.parametrize('Bn,H,W', [(3, 17, 15), (3, 40, 52)])
def test_l2_bits(dev, lib, Bn, H, W):
    c = Case(Bn, H, W, True, dev)
    q = torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, (Bn, H * W, 16)).astype(np.float32))
    first = (c.fwd(lib)[1].numpy(Bn), c.bwd(lib, 0)[1].numpy(Bn, H * W, 16), c.bwd(lib, 1, q)[1].numpy(Bn, H * W, 16))
    again = (c.fwd(lib)[1].numpy(Bn), c.bwd(lib, 0)[1].numpy(Bn, H * W, 16), c.bwd(lib, 1, q)[1].numpy(Bn, H * W, 16))
    for x, y in zip(first, again):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    # the last sample of the batch of 3, alone
    b = Bn - 1
    one = c.rows(b, Bn)
    assert np.array_equal(one.fwd(lib)[1].numpy(1), first[0][b:])
    assert np.array_equal(one.bwd(lib, 0)[1].numpy(1, H * W, 16), first[1][b:])
    assert np.array_equal(one.bwd(lib, 1, q[b:])[1].numpy(1, H * W, 16), first[2][b:])
    # ... and on another stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = c.fwd(lib)[1]
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(other.numpy(Bn), first[0])


def test_l2_argument_checks(dev, lib):
    """each refusal returns P2L_EINVAL and launches nothing: the outputs still hold their sentinel fill"""
    c = Case(2, 16, 20, True, dev)
    for kw in (dict(img16=None), dict(target=None), dict(weight=None), dict(wsum=None), dict(loss=None),
               dict(part=None), dict(Bn=0), dict(Bn=65536), dict(H=0), dict(W=0), dict(H=-3)):
        rc, loss, part = c.fwd(lib, **kw)
        assert rc == EINVAL, kw
        assert loss.untouched() and part.untouched(), kw
    for kw in (dict(img16=None), dict(target=None), dict(weight=None), dict(wsum=None), dict(gscale=None),
               dict(d=None), dict(Bn=0), dict(Bn=65536), dict(H=0), dict(W=0)):
        for acc in (0, 1):
            rc, d = c.bwd(lib, acc, **kw)
            assert rc == EINVAL, kw
            assert d.untouched(), kw
    # the mask alone may be NULL
    c.mask = None
    assert c.fwd(lib)[0] == 0 and c.bwd(lib, 0)[0] == 0
    torch.cuda.synchronize()


# ---- the term in the Python losses ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def images(dev):
    """B = 3 outputs / targets / weights at 64^2 and 128^2, synthetic VGG weights"""
    warnings.simplefilter('ignore')
    from pix2latent_amd.utils import synthetic as S
    Wv = S.lpips_vgg_weights(1)
    sets = {}
    for size in (64, 128):
        g = torch.Generator().manual_seed(size)
        out = torch.tanh(torch.randn(3, 3, size, size, generator=g)).to(dev)
        target = torch.stack([S.synthetic_target(size, s) for s in (1, 2, 3)]).to(dev)
        weight = S.synthetic_weight_mask(size).unsqueeze(0).repeat(3, 1, 1, 1).to(dev)
        mask = (torch.rand(3, 3, size, size, generator=g) < 0.8).float().to(dev)
        sets[size] = (out, target, weight, mask)
    return Wv, sets


def _loss_and_grad(fn, out, *args):
    o = out.clone().requires_grad_(True)
    loss = fn(o, *args)
    g, = torch.autograd.grad(loss.sum(), o)
    return loss.detach(), g


@pytest.mark.parametrize('size,lpips_size,with_mask', [(64, None, False), (64, None, True), (128, 64, True)])
def test_projection_loss_l2_is_the_sum_of_its_terms(dev, images, size, lpips_size, with_mask):
    import pix2latent_amd.loss_functions as LF
    Wv, sets = images
    out, target, weight, mask = sets[size]
    args = (target, weight, mask) if with_mask else (target, weight)
    a, b = 0.37, 0.8
    proj = LF.ProjectionLoss(lpips_net='vgg', beta=b, weights=Wv, device=dev, lpips_size=lpips_size, pixel_loss='l2',
                             pixel_weight=a)
    rl2 = LF.ReconstructionLoss('l2')
    per = LF.PerceptualLoss(net='vgg', weights=Wv, device=dev, lpips_size=lpips_size)
    loss, grad = _loss_and_grad(proj, out, *args)
    l2, g2 = _loss_and_grad(lambda o, *r: a * rl2(o, *r), out, *args)
    lp, gp = _loss_and_grad(lambda o, *r: b * per(o, *r), out, *args)
    assert rl2._engine is not None                             # the native route
    ref = l2.double() + lp.double()
    print('%d^2 lpips_size %s: a L2 %s  b LPIPS %s  |loss - ref| / bound %.3g'
          % (size, lpips_size, l2.tolist(), lp.tolist(), ((loss.double() - ref).abs() / (2.0 ** -22 * ref)).max()))
    assert (l2 > 1e-3).all() and (lp > 1e-3).all()
    assert ((loss.double() - ref).abs() <= 2.0 ** -22 * ref).all()
    gref = g2.double() + gp.double()
    gtol = 2.0 ** -22 * (g2.double().abs() + gp.double().abs())
    print('    max |grad - ref| / bound %.3g' % ((grad.double() - gref).abs() / gtol.clamp_min(1e-300)).max())
    assert g2.abs().max() > 0 and gp.abs().max() > 0
    assert ((grad.double() - gref).abs() <= gtol).all()
    # `last_l1` holds the pixel term, whichever it is
    assert torch.equal(a * proj._engine.last_l1, l2)


def test_one_channel_weight_is_three_times(dev, images):
    import pix2latent_amd.loss_functions as LF
    Wv, sets = images
    out, target, weight, mask = sets[64]
    w1 = weight[:, :1].contiguous()
    rl2 = LF.ReconstructionLoss('l2')
    three, g3 = _loss_and_grad(rl2, out, target, weight)
    one, g1 = _loss_and_grad(rl2, out, target, w1)
    assert torch.equal(one, 3.0 * three)
    # (gscale = 3 enters the kernel in front of its three roundings; 3 * g3 has those and the product's: seven)
    assert ((g1.double() - 3.0 * g3.double()).abs() <= 7 * U * (3.0 * g3.double()).abs() + 1e-37).all()
    assert g3.abs().max() > 0
    # ... as the torch path does
    cpu = rl2(out.cpu(), target.cpu(), w1.cpu())
    assert ((cpu.double() - one.cpu().double()).abs() <= (3 * 64 * 64 + 8) * U * cpu.double()).all()
    # ... and inside ProjectionLoss the factor belongs to the pixel term alone
    a, b = 0.5, 0.8
    proj = LF.ProjectionLoss(lpips_net='vgg', beta=b, weights=Wv, device=dev, pixel_loss='l2', pixel_weight=a)
    per = LF.PerceptualLoss(net='vgg', weights=Wv, device=dev)
    with torch.no_grad():
        ref = a * one.double() + b * per(out, target, w1).double()
        got = proj(out, target, w1).double()
    assert ((got - ref).abs() <= 2.0 ** -22 * ref).all()


@pytest.mark.parametrize('size,lpips_size', [(64, None), (128, 64)])
def test_projection_loss_defaults_keep_their_bits(dev, images, size, lpips_size):
    import pix2latent_amd.loss_functions as LF
    Wv, sets = images
    out, target, weight, mask = sets[size]
    kw = dict(lpips_net='vgg', beta=10, weights=Wv, device=dev, lpips_size=lpips_size)
    first = _loss_and_grad(LF.ProjectionLoss(**kw), out, target, weight, mask)
    second = _loss_and_grad(LF.ProjectionLoss(**kw), out, target, weight, mask)
    explicit = _loss_and_grad(LF.ProjectionLoss(pixel_weight=1.0, pixel_loss='l1', **kw), out, target, weight, mask)
    for other in (second, explicit):
        assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])
    # a weighted L1 term: the sum of its terms, to the same bound
    a = 0.25
    half = _loss_and_grad(LF.ProjectionLoss(pixel_weight=a, **kw), out, target, weight, mask)
    l1 = _loss_and_grad(lambda o, *r: a * LF.ReconstructionLoss()(o, *r), out, target, weight, mask)
    per = LF.PerceptualLoss(net='vgg', weights=Wv, device=dev, lpips_size=lpips_size)
    lp = _loss_and_grad(lambda o, *r: 10 * per(o, *r), out, target, weight, mask)
    ref = l1[0].double() + lp[0].double()
    assert ((half[0].double() - ref).abs() <= 2.0 ** -22 * ref).all()
    gtol = 2.0 ** -22 * (l1[1].double().abs() + lp[1].double().abs())
    assert ((half[1].double() - (l1[1].double() + lp[1].double())).abs() <= gtol).all()


@pytest.mark.parametrize('with_mask', [False, True])
def test_native_l2_against_its_torch_expression(dev, images, with_mask):
    import pix2latent_amd.loss_functions as LF
    _, sets = images
    out, target, weight, mask = sets[64]
    m = mask if with_mask else None
    rl2 = LF.ReconstructionLoss('l2')
    gvec = torch.tensor([1.0, -0.5, 2.0], device=dev)

    def torch_expr(o):
        w = weight if m is None else m * weight
        return torch.sum(LF.l2_loss(o, target) * w, [1, 2, 3]) / torch.sum(w, [1, 2, 3])

    o1 = out.clone().requires_grad_(True)
    l_native = rl2(o1, target, weight, m)
    (l_native * gvec).sum().backward()
    o2 = out.clone().requires_grad_(True)
    l_torch = torch_expr(o2)
    (l_torch * gvec).sum().backward()
    assert rl2._engine is not None
    rel = ((l_native.double() - l_torch.double()).abs() / l_torch.double()).max().item()
    print('mask %d: loss %s  relative difference %.3g (bound %.3g)' % (with_mask, l_torch.tolist(), rel,
                                                                      (3 * 4096 + 8) * U))
    assert rel <= (3 * 4096 + 8) * U
    gref = o2.grad.double()
    gerr = (o1.grad.double() - gref).abs()
    print('    max |grad - ref| / bound %.3g' % (gerr / (2.0 ** -21 * gref.abs() + 1e-12)).max())
    assert gref.abs().max() > 0
    assert (gerr <= 2.0 ** -21 * gref.abs() + 1e-12).all()


# ---- p2l_adam_step_sched -------------------------------------------------------------------------------------------
N_ADAM = 18 * 128
BETAS_EPS = (0.9, 0.999, 1e-8)


def _adam_grads():
    """the operands of tests/test_kernels_gpu.py::test_adam_matches_torch"""
    g = torch.Generator().manual_seed(8)
    p0 = torch.randn(N_ADAM, generator=g)
    return p0, [torch.randn(N_ADAM, generator=g) * (10.0 ** (-step)) for step in range(1, 7)]


class AdamState(object):
    def __init__(self, p0, dev, counters=None):
        self.p = p0.clone().to(dev)
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.steps = torch.zeros(18, dtype=torch.int32, device=dev) if counters is None else \
            torch.tensor(counters, dtype=torch.int32, device=dev)

    def dev_step(self, lib, grad, lr):
        from pix2latent_amd import _native as N
        assert lib.p2l_adam_step_dev(_p(self.p), _p(grad), _p(self.m), _p(self.v), self.p.numel(), lr, *BETAS_EPS,
                                     _p(self.steps), self.steps.numel(), N.stream()) == 0

    def sched_step(self, lib, grad, table):
        from pix2latent_amd import _native as N
        assert lib.p2l_adam_step_sched(_p(self.p), _p(grad), _p(self.m), _p(self.v), self.p.numel(), _p(table),
                                       table.numel(), *BETAS_EPS, _p(self.steps), self.steps.numel(),
                                       N.stream()) == 0

    def same(self, other):
        return all(torch.equal(getattr(self, k), getattr(other, k)) for k in ('p', 'm', 'v', 'steps'))


def test_adam_sched_is_adam_dev_with_the_table_entry(dev, lib):
    p0, grads = _adam_grads()
    grads = [g.to(dev) for g in grads]
    # a table of three equal entries over six steps
    a, b = AdamState(p0, dev), AdamState(p0, dev)
    table = torch.full((3,), 0.05, device=dev)
    for g in grads:
        a.sched_step(lib, g, table)
        b.dev_step(lib, g, 0.05)
    assert a.same(b) and a.steps.tolist() == [6] * 18
    # [a, b, c] over five steps = a, b, c, c, c
    a, b = AdamState(p0, dev), AdamState(p0, dev)
    rates = [0.05, 0.02, 0.08]
    table = torch.tensor(rates, device=dev)
    for g, lr in zip(grads[:5], rates + rates[-1:] * 2):
        a.sched_step(lib, g, table)
        b.dev_step(lib, g, float(np.float32(lr)))
    assert a.same(b) and a.steps.tolist() == [5] * 18
    # the first counter of a chunk decides: counters 0 and 2 in one call use entry 0
    a, b = AdamState(p0, dev, [0, 2]), AdamState(p0, dev, [0, 2])
    a.sched_step(lib, grads[0], table)
    b.dev_step(lib, grads[0], float(np.float32(rates[0])))
    assert a.same(b) and a.steps.tolist() == [1, 3]
    c = AdamState(p0, dev, [2, 0])
    c.sched_step(lib, grads[0], table)
    assert not torch.equal(c.p, a.p) and c.steps.tolist() == [3, 1]


def test_adam_sched_matches_torch(dev, lib):
    p0, grads = _adam_grads()
    rates = [0.05, 0.025, 0.04]
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=rates[0])
    s = AdamState(p0, dev)
    table = torch.tensor(rates, device=dev)
    for i in range(5):
        opt.param_groups[0]['lr'] = float(np.float32(rates[min(i, 2)]))
        p_ref.grad = grads[i].clone()
        opt.step()
        s.sched_step(lib, grads[i].to(dev), table)
    diff = (s.p.cpu() - p_ref.detach()).abs().max().item()
    print('max |p - torch| = %.3g' % diff)
    assert diff < 1e-6


def test_adam_sched_argument_checks(dev, lib):
    from pix2latent_amd import _native as N
    p0, grads = _adam_grads()
    s = AdamState(p0, dev)
    g, table = grads[0].to(dev), torch.full((3,), 0.05, device=dev)

    def call(p=s.p, g=g, m=s.m, v=s.v, n=N_ADAM, table=table, n_lr=3, steps=s.steps, n_counters=18):
        return lib.p2l_adam_step_sched(_p(p), _p(g), _p(m), _p(v), n, _p(table), n_lr, *BETAS_EPS, _p(steps),
                                       n_counters, N.stream())

    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(table=None), dict(steps=None),
               dict(n=0), dict(n_lr=0), dict(n_counters=0)):
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert torch.equal(s.p.cpu(), p0) and s.steps.tolist() == [0] * 18 and not s.m.any() and not s.v.any()
    assert call() == 0
    assert s.steps.tolist() == [1] * 18


# ---- a schedule in the closure: the 64^2 synthetic StyleGAN2 of tests/test_latent_prior_gpu.py ---------------------
SIZE = 64


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


def _start(model):
    n_lat = model._desc.n_latent
    n_noise = sum(s[-2] * s[-1] for s in model.noise_shape)
    g = torch.Generator().manual_seed(4)
    z0 = model.latent_mean.cpu().view(1, 512).repeat(n_lat, 1) + 0.3 * torch.randn(n_lat, 512, generator=g)
    return torch.stack([z0, 1.25 * z0]), torch.randn(n_noise, generator=g)


def _setup(problem, dev, lr, use_graph):
    from pix2latent_amd import VariableManager
    from pix2latent_amd.optimizer import GradientOptimizer
    model, loss_fn, target, weight = problem
    z0, n0 = _start(model)
    vm = VariableManager(device=dev)
    vm.reuse_buffers = True
    vm.register('z', tuple(z0.shape[1:]), 'input', learning_rate=lr, default=z0[0])
    vm.register('noises', tuple(n0.shape), 'input', learning_rate=0.05, default=n0)
    vm.register('target', (3, SIZE, SIZE), 'output', requires_grad=False, default=target)
    vm.register('weight', (3, SIZE, SIZE), 'output', requires_grad=False, default=weight)
    opt = GradientOptimizer(model, vm, loss_fn, max_batch_size=9, use_graph=use_graph)
    return vm, opt, z0


def _init(vm, z0):
    variables = vm.initialize(num_samples=2)
    with torch.no_grad():
        variables.input.z.buf[1].copy_(z0[1])                 # two different candidates
    return variables


def _steps(problem, dev, n_steps, lr, use_graph):
    vm, opt, z0 = _setup(problem, dev, lr, use_graph)
    variables = _init(vm, z0)
    losses = []
    for i in range(n_steps):
        _, l, _ = opt.step(variables, optimize=True, transform=False)
        losses.append(np.array(l, dtype=np.float64))
    if use_graph:
        assert any(isinstance(v, tuple) for v in opt._graphs.values()), 'no graph was captured'
    return np.stack(losses), variables.input.z.buf.detach().cpu().clone(), opt, variables, vm


def test_closure_schedule_graph_replay_is_the_eager_trajectory(problem, dev):
    from pix2latent_amd import LRSchedule
    sched = LRSchedule.projector_ramp(0.1, 6)
    assert sched.value(0) == 0.0 and len(set(sched.values.tolist())) == 3
    graph = _steps(problem, dev, 7, sched, True)
    eager = _steps(problem, dev, 7, LRSchedule.projector_ramp(0.1, 6), False)
    assert np.array_equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
    const = _steps(problem, dev, 7, 0.1, False)
    assert np.array_equal(const[0][0], eager[0][0])            # the first step sees the starting point
    assert (const[0][1:] != eager[0][1:]).all() and not torch.equal(const[1], eager[1])
    for run in (graph, eager):
        opt = run[3].opt
        assert opt.state_steps('z') == [7, 7] and opt.state_steps('noises') == [7, 7]
        assert opt.current_lr('z') == [sched.value(7)] * 2 and opt.current_lr('noises') == [0.05] * 2
        groups = [g for g in opt.param_groups if g.get('lr_schedule') is not None]
        assert len(groups) == 2 and all(g['lr'] == 0.0 for g in groups)


def test_graph_key_holds_the_learning_rate(problem, dev):
    from pix2latent_amd import LRSchedule
    _, _, opt, variables, vm = _steps(problem, dev, 3, 0.05, True)
    z0 = _start(problem[0])[0]
    k0 = opt._graph_key(variables, 0, 2)
    assert k0 in opt._graphs
    addresses = lambda v: (v.input.z.buf.data_ptr(), v.opt.state_key()[0][:4], v.opt.state_key()[1][:4])  # noqa: E731
    a0 = addresses(variables)
    # lr 0.05 -> 0.1 between generations: every address stays, the key does not
    assert vm.edit_variable('z', {'learning_rate': 0.1})
    v1 = _init(vm, z0)
    k1 = opt._graph_key(v1, 0, 2)
    assert addresses(v1) == a0
    assert k1 != k0 and k1 not in opt._graphs
    # two schedules that differ in one table entry; equal tables share a key
    keys = []
    for table in ([0.0, 0.1, 0.05], [0.0, 0.1, 0.0501], [0.0, 0.1, 0.05]):
        assert vm.edit_variable('z', {'learning_rate': LRSchedule(table)})
        v = _init(vm, z0)
        assert addresses(v) == a0
        keys.append(opt._graph_key(v, 0, 2))
    assert keys[0] != keys[1] and keys[0] == keys[2] and k0 not in keys and k1 not in keys
    assert vm.edit_variable('z', {'learning_rate': 0.05})
    assert opt._graph_key(_init(vm, z0), 0, 2) == k0

"""Colour transformations on the MI355X (p2l_color_adjust, pix2latent_amd/csrc/p2l_color.hip):
every op and both chains bit-identical to tests/golden/color_transform.npz (Pillow through the
reference's torchvision wrappers) with a parameter per candidate, B from 1 to 22, 16^2 images
tiled to 256^2 and 1024^2, 37 x 53 and 1 x 1, out of place and in place; the device equals the host
restatement on random inputs; repeated calls are bit-identical; bad arguments are refused; and two
generations of TransformBasinCMAOptimizer search a spatial + hue + brightness chain on the device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_color_transform import gold, golden_cases, expected  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    return torch.device('cuda:0')


def _tile(a, reps):
    """[B,3,h,w] numpy -> tiled reps x reps times over H and W (the L mean, hence contrast, is unchanged)"""
    return np.tile(a, (1, 1, reps, reps))


def _run(CT, dev, ims, ops, ps, inplace):
    x = torch.from_numpy(np.ascontiguousarray(ims)).to(dev)
    params = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in ps]
    if inplace:
        y = CT.device_chain(x, ops, params, out=x)
        assert y.data_ptr() == x.data_ptr()
    else:
        y = CT.device_chain(x, ops, params)
        assert y.data_ptr() != x.data_ptr()
    return y.cpu()


@pytest.mark.parametrize('B', [1, 5, 12, 22])
def test_golden_16x16_all_ops_and_chains(dev, B):
    from pix2latent_amd.transform import color_transform as CT
    g = gold()
    idx = np.arange(B) % 12
    for s, key, ops, ps, k in golden_cases(g):
        if s != 'a':
            continue
        ims, ps, k = g['a_ims'][idx], ps[:, idx], k[idx]
        y = _run(CT, dev, ims, ops, ps, inplace=(B % 2 == 1))
        assert torch.equal(y, expected(k)), (key, B)


@pytest.mark.parametrize('reps', [16, 64])
def test_golden_tiled_to_256_and_1024(dev, reps):
    from pix2latent_amd.transform import color_transform as CT
    g = gold()
    B = 22 if reps == 16 else 6
    idx = (np.arange(B) * 5) % 12
    for s, key, ops, ps, k in golden_cases(g):
        if s != 'a' or (reps == 64 and not key.endswith(('_0', 'chain5', 'chain3'))):
            continue
        y = _run(CT, dev, _tile(g['a_ims'][idx], reps), ops, ps[:, idx], inplace=key.endswith('_1'))
        assert torch.equal(y, expected(_tile(k[idx], reps))), (key, reps)


@pytest.mark.parametrize('s', ['b', 'c'])
def test_golden_37x53_and_1x1(dev, s):
    """odd planes (37 x 53, 1 x 1): the one-pixel-per-thread path"""
    from pix2latent_amd.transform import color_transform as CT
    g = gold()
    for s_, key, ops, ps, k in golden_cases(g):
        if s_ != s:
            continue
        for inplace in (False, True):
            y = _run(CT, dev, g[s + '_ims'], ops, ps, inplace)
            assert torch.equal(y, expected(k)), (key, inplace)


@pytest.mark.parametrize('shape', [(3, 1, 1), (7, 37, 53), (2, 5, 6), (22, 64, 64), (4, 256, 256), (2, 1, 4)])
def test_device_equals_host_on_random_inputs(dev, shape):
    from pix2latent_amd.transform import color_transform as CT
    B, H, W = shape
    gen = torch.Generator().manual_seed(H * 1000 + W)
    ims = torch.rand(B, 3, H, W, generator=gen) * 2.1 - 1.05
    ranges = [(0.667, 1.5)] * 4 + [(-0.5 + 1e-6, 0.5 - 1e-6)]
    chains = [[o] for o in range(5)] + [[4, 3, 1, 0, 2], [2, 2, 4, 0], [3, 4, 2, 1, 0, 2, 4, 3]]
    for ops in chains:
        ps = [(torch.rand(B, generator=gen) * (ranges[o][1] - ranges[o][0]) + ranges[o][0]) for o in ops]
        want = CT.host_chain(ims, ops, [p.numpy() for p in ps])
        got = CT.device_chain(ims.to(dev), ops, [p.to(dev) for p in ps]).cpu()
        assert torch.equal(got, want), (shape, ops)


def test_unaligned_view_takes_the_scalar_path(dev):
    from pix2latent_amd.transform import color_transform as CT
    gen = torch.Generator().manual_seed(3)
    flat = (torch.rand(1 + 2 * 3 * 8 * 8, generator=gen) * 2 - 1).to(dev)
    ims = flat[1:].view(2, 3, 8, 8)                # 4-byte offset: no float4 access
    ps = [torch.tensor([0.8, 1.3]), torch.tensor([-0.2, 0.3])]
    want = CT.host_chain(ims.cpu(), [2, 4], [p.numpy() for p in ps])
    got = CT.device_chain(ims, [2, 4], [p.to(dev) for p in ps]).cpu()
    assert torch.equal(got, want)


def test_repeated_calls_are_bit_identical(dev):
    from pix2latent_amd.transform import color_transform as CT
    gen = torch.Generator().manual_seed(4)
    ims = (torch.rand(22, 3, 256, 256, generator=gen) * 2 - 1).to(dev)
    ops = [4, 3, 1, 0, 2]
    ps = [torch.full((22,), v).to(dev) + 0.01 * torch.arange(22, dtype=torch.float32, device=dev)
          for v in (-0.2, 0.8, 1.2, 0.9, 1.3)]
    first = CT.device_chain(ims, ops, ps)
    for _ in range(3):
        assert torch.equal(CT.device_chain(ims, ops, ps), first)


def test_bad_arguments_are_refused(dev):
    from pix2latent_amd import _native as N
    from pix2latent_amd.transform import color_transform as CT
    L = N.lib()
    x = torch.zeros(2, 3, 4, 4, device=dev)
    p = torch.ones(2, device=dev)
    lut = torch.zeros(2, 256, dtype=torch.uint8, device=dev)
    ws = torch.zeros(64, dtype=torch.int64, device=dev)

    def chain(ops, luts=True):
        ch = CT.P2LColorChain()
        ch.size = C.sizeof(CT.P2LColorChain)
        ch.n_ops = len(ops)
        for j, o in enumerate(ops):
            ch.ops[j].op = o
            ch.ops[j].param = p.data_ptr()
            ch.ops[j].lut = lut.data_ptr() if luts else None
        return ch

    def call(ch, Cn=3, H=4, W=4, B=2, src=N.ptr(x), nbytes=512):
        return L.p2l_color_adjust(C.byref(ch), src, N.ptr(x), B, Cn, H, W, C.c_void_p(ws.data_ptr()),
                                  C.c_size_t(nbytes), N.stream())

    assert call(chain([0, 2])) == 0
    assert call(chain([0]), Cn=4) == -1 and call(chain([0]), H=0) == -1 and call(chain([0]), B=0) == -1
    assert call(chain([5])) == -1 and call(chain([-1])) == -1
    too_long = chain([0] * 8)
    too_long.n_ops = 9
    assert call(chain([])) == -1 and call(too_long) == -1
    assert call(chain([3], luts=False)) == -1
    assert call(chain([0]), src=C.c_void_p(0)) == -1
    small = chain([0])
    small.size = 8
    assert call(small) == -1
    assert L.p2l_color_adjust(None, N.ptr(x), N.ptr(x), 2, 3, 4, 4, None, C.c_size_t(0), N.stream()) == -1
    assert L.p2l_color_adjust_ws_bytes(C.byref(chain([2, 0, 2])), 2) == 2 * 2 * 8
    assert L.p2l_color_adjust_ws_bytes(C.byref(chain([0, 4])), 2) == 0
    assert call(chain([2, 2]), nbytes=16) == -3                 # workspace too small
    assert call(chain([0, 4]), nbytes=0) == 0                   # no contrast: no workspace
    torch.cuda.synchronize()


class _Recording(object):
    """a transformation that records what it was given and what it returned"""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, ims, t, invert=False, **kw):
        out = self.fn(ims, t, invert=invert, **kw)
        self.calls.append((ims.detach().clone(), t.detach().clone(), invert, out.detach().clone()))
        return out


def _search(dev, monkeypatch):
    from _toy import ToyGenerator, toy_target, toy_weight, FakeCMAES
    from pix2latent_amd import VariableManager, distribution
    from pix2latent_amd.utils import function_hooks as hook
    from pix2latent_amd.transform import SpatialTransform, TransformBasinCMAOptimizer, ComposeTransform
    from pix2latent_amd.transform.color_transform import HueTransform, BrightnessTransform
    import pix2latent_amd.optimizer.base_cma_optimizer as BC
    from oracle.lpips_ref import reconstruction_loss
    FakeCMAES.log = []
    monkeypatch.setattr(BC, 'CMAEvolutionStrategy', FakeCMAES)
    vm = VariableManager(device=dev)
    vm.register('z', (6,), 'input', distribution=distribution.TruncatedNormalModulo(),
                learning_rate=0.05, hook_fn=hook.Clamp(1.5))
    vm.register('c', (4,), 'input', default=torch.linspace(-0.2, 0.2, 4), learning_rate=0.01)
    vm.register('target', (3, 4, 4), 'output', requires_grad=False, default=toy_target())
    vm.register('weight', (3, 4, 4), 'output', requires_grad=False, default=toy_weight())
    target_fn = ComposeTransform([(SpatialTransform(), 1.0), (HueTransform(), 5.0), (BrightnessTransform(), 5.0)])
    weight_fn = ComposeTransform([(SpatialTransform(), 1.0), (HueTransform(), 5.0), (BrightnessTransform(), 5.0)])
    vm.register('t', (5,), 'transform', requires_grad=False, grad_free=True,
                default=target_fn.get_param(as_tensor=True))
    model = ToyGenerator().to(dev)
    torch.manual_seed(45)
    opt = TransformBasinCMAOptimizer(model, vm, lambda o, target, weight: reconstruction_loss(o, target, weight),
                                     max_batch_size=4)
    rec_t = _Recording(target_fn)
    rec_w = _Recording(lambda ims, t, invert=False: weight_fn(ims, t, invert=invert, only_spatial=True))
    opt.register_transform(rec_t, 't', 'target')
    opt.register_transform(rec_w, 't', 'weight')
    opt.set_variable_propagation('z')
    variables, _, loss = opt.optimize(meta_steps=2, grad_steps=2)
    return opt, rec_t, rec_w, variables, loss


def test_transform_basincma_with_colour_chain(dev, monkeypatch):
    from pix2latent_amd.transform import ComposeTransform, SpatialTransform
    from pix2latent_amd.transform.color_transform import HueTransform, BrightnessTransform
    runs = [_search(dev, monkeypatch) for _ in range(2)]
    opt, rec_t, rec_w, variables, loss = runs[0]
    assert len(opt.transform_tracked) == 2 and opt.transform_tracked[0].shape[1] == 5
    assert np.isfinite(np.asarray(loss, dtype=np.float64)).all()
    fwd = [c for c in rec_t.calls if not c[2]]
    assert len(fwd) >= 2
    colour = ComposeTransform([(HueTransform(), 5.0), (BrightnessTransform(), 5.0)])
    spatial = SpatialTransform()
    for ims, t, _, out in fwd:
        assert out.is_cuda and t.shape[1] == 5
        # the targets each candidate sees: the device warp, then the host path of the colour part
        warped = spatial(ims, t[:, :3]).cpu()
        assert torch.equal(out.cpu(), colour(warped, t[:, 3:].cpu())), 'device colour chain != host path'
    for ims, t, _, out in rec_w.calls:
        assert torch.equal(out, spatial(ims, t[:, :3]))
    # two runs: bit-identical
    other = runs[1]
    for a, b in zip(opt.transform_tracked, other[0].transform_tracked):
        assert torch.equal(a, b)
    for a, b in zip(rec_t.calls, other[1].calls):
        assert torch.equal(a[3], b[3])
    assert torch.equal(torch.stack(list(variables.output.target.data)),
                       torch.stack(list(other[3].output.target.data)))

"""The noise regulariser and its plumbing without a GPU: the torch restatement against the numpy
reference, the host guards of the native entry points, `register(regularizer=...)` through the
VariableManager, and the generic closure path with a spy regulariser."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _noise_ref as NR  # noqa: E402
from _toy import ToyGenerator, toy_target, toy_weight  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(ROOT, 'pix2latent_amd', 'libp2l_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from pix2latent_amd import _native as N
    return N.lib()


def test_reference_level_counts():
    assert NR.total(NR.SMALL) == 43664
    assert NR.n_levels(NR.FFHQ1024) == 73 and NR.total(NR.FFHQ1024) == 2796176
    cars512 = [4] + [r for k in range(3, 10) for r in (2 ** k, 2 ** k)]
    assert NR.n_levels(cars512) == 57


def test_cpu_path_against_reference():
    import pix2latent_amd.loss_functions as LF
    x = NR.white(3, NR.SMALL, seed=1)
    x[1] = NR.planted(x[1], NR.SMALL)
    R, _, grad, _ = NR.regularize(x, NR.SMALL)
    assert R[1] > R[0] + 1.0                                # planted: ax = 0.48 at level 0 of every layer
    t = torch.from_numpy(x).requires_grad_(True)
    got = LF.noise_regularize(t, [[1, 1, s, s] for s in NR.SMALL])
    assert got.dtype == torch.float32 and got.shape == (3,)
    assert np.abs(got.detach().numpy().astype(np.float64) - R).max() <= 1e-6 * np.abs(R).max()
    assert (np.abs(got.detach().numpy().astype(np.float64) - R) <= 1e-6 * np.abs(R)).all()
    got.sum().backward()
    err = np.abs(t.grad.numpy().astype(np.float64) - grad).max(1)
    assert (err <= 1e-6 * np.abs(grad).max(1)).all(), (err, np.abs(grad).max(1))
    # the list of [B,1,h,w] maps is the same variable
    maps, off = [], 0
    for s in NR.SMALL:
        maps.append(torch.from_numpy(x[:, off:off + s * s]).reshape(3, 1, s, s))
        off += s * s
    assert torch.equal(LF.noise_regularize(maps, NR.SMALL), got.detach())
    reg = LF.NoiseRegularizer(NR.SMALL)
    assert reg.weight == 1e5
    assert torch.equal(reg(t.detach()), 1e5 * got.detach())
    # and the alias package carries the same objects
    import pix2latent.loss_functions as LFA
    from pix2latent.utils import function_hooks as hookA
    from pix2latent_amd.utils import function_hooks as hook
    assert LFA.NoiseRegularizer is LF.NoiseRegularizer and LFA.noise_regularize is LF.noise_regularize
    assert hookA.NoiseNormalize is hook.NoiseNormalize


def test_noise_normalize_hook_cpu():
    from pix2latent_amd.utils import function_hooks as hook
    sizes = [4, 8, 16]
    x = NR.white(2, sizes, seed=2) * 3.0 + 0.5
    h = hook.NoiseNormalize([[1, 1, s, s] for s in sizes])
    assert h.stochastic is False and h.graph_safe is True
    rows = torch.from_numpy(x.copy())
    h.apply_batched(rows)
    ref = NR.normalize(x, sizes)
    assert np.abs(rows.numpy() - ref).max() < 1e-5
    one = [torch.from_numpy(x[1].copy())]
    h(one)                                                  # the reference's per-sample call form
    assert torch.allclose(one[0], rows[1], atol=1e-6)


def test_host_guards(lib):
    """everything below returns before any launch: no device is needed (fake non-null pointers)"""
    from pix2latent_amd import _native as N
    fake = C.c_void_p(4096)
    arr = lambda v: (C.c_int32 * len(v))(*v)
    small = arr(NR.SMALL)
    n = len(NR.SMALL)
    levels = NR.n_levels(NR.SMALL)
    # workspace: corr + one partial pair per item (fp64), then the pooled levels (fp32)
    items = sum(max(1, (s >> k) ** 2 // 4096) for s in NR.SMALL for k in range(len(NR._sides(s))))
    pooled = sum(sum(v * v for v in NR._sides(s)[1:]) for s in NR.SMALL)
    one = lib.p2l_sg2_noise_reg_ws_bytes(small, n, 1)
    assert one == -(-((levels + items) * 16 + pooled * 4) // 16) * 16
    assert lib.p2l_sg2_noise_reg_ws_bytes(small, n, 3) >= 3 * ((levels + items) * 16 + pooled * 4)
    ffhq = lib.p2l_sg2_noise_reg_ws_bytes(arr(NR.FFHQ1024), len(NR.FFHQ1024), 1)
    assert 0.33 * 4 * NR.total(NR.FFHQ1024) < ffhq < 0.36 * 4 * NR.total(NR.FFHQ1024)
    for bad in ([], [3], [2], [2048], [4, 12], [4] * 33):
        assert lib.p2l_sg2_noise_reg_ws_bytes(arr(bad) if bad else None, len(bad), 1) == 0, bad
    assert lib.p2l_sg2_noise_reg_ws_bytes(small, n, 0) == 0
    assert lib.p2l_sg2_noise_reg_ws_bytes(None, n, 1) == 0
    big = C.c_size_t(1 << 30)
    fwd, bwd, nrm = lib.p2l_sg2_noise_reg_fwd, lib.p2l_sg2_noise_reg_bwd, lib.p2l_sg2_noise_normalize
    assert fwd(None, small, n, 1, fake, None, fake, big, None) == -1
    assert fwd(fake, None, n, 1, fake, None, fake, big, None) == -1
    assert fwd(fake, small, n, 1, None, None, fake, big, None) == -1
    assert fwd(fake, small, n, 0, fake, None, fake, big, None) == -1
    assert fwd(fake, small, 0, 1, fake, None, fake, big, None) == -1
    assert fwd(fake, arr([4, 24]), 2, 1, fake, None, fake, big, None) == -1
    assert fwd(C.c_void_p(4100), small, n, 1, fake, None, fake, big, None) == -1          # misaligned
    assert fwd(fake, small, n, 1, fake, None, None, big, None) == -3
    assert fwd(fake, small, n, 1, fake, None, fake, C.c_size_t(one - 16), None) == -3
    assert bwd(None, small, n, 1, None, fake, fake, big, None) == -1
    assert bwd(fake, small, n, 1, None, None, fake, big, None) == -1
    assert bwd(fake, small, n, -2, None, fake, fake, big, None) == -1
    assert bwd(fake, arr([4096]), 1, 1, None, fake, fake, big, None) == -1
    assert bwd(fake, small, n, 1, None, fake, None, big, None) == -3
    assert bwd(fake, small, n, 1, None, fake, fake, C.c_size_t(8), None) == -3
    assert nrm(None, small, n, 1, fake, big, None) == -1
    assert nrm(fake, small, n, 0, fake, big, None) == -1
    assert nrm(fake, arr([5]), 1, 1, fake, big, None) == -1
    assert nrm(fake, small, n, 1, None, big, None) == -3
    assert nrm(fake, small, n, 1, fake, C.c_size_t(one - 16), None) == -3
    assert N.ABI_VERSION == lib.p2l_version() == 101


def _spy(x):
    return (x ** 2).mean(1)


def test_register_carries_the_regularizer():
    from pix2latent_amd import VariableManager
    from pix2latent_amd.variable_manager import split_vars
    vm = VariableManager(device='cpu')
    vm.register('z', (6,), 'input', learning_rate=0.1, regularizer=_spy)
    vm.register('c', (4,), 'input', learning_rate=0.1)
    assert vm.variable_info['z']['regularizer'] is _spy and vm.variable_info['c']['regularizer'] is None
    v = vm.initialize(num_samples=5)
    assert v.input.z.regularizer is _spy and v.input.c.regularizer is None
    chunks = split_vars(v, size=2)
    assert [c.num_samples for c in chunks] == [2, 2, 1]
    assert all(c.input.z.regularizer is _spy and c.input.c.regularizer is None for c in chunks)
    other = lambda x: x.abs().sum(1)
    assert vm.edit_variable('z', {'regularizer': other})
    assert vm.initialize(num_samples=2).input.z.regularizer is other
    assert vm.edit_variable('z', {'regularizer': None})
    assert vm.initialize(num_samples=2).input.z.regularizer is None


def test_generic_closure_adds_the_regularizer():
    """CPU tensors take the reference's own sequence (torch.optim.Adam, `opt.step(closure)`): the losses
    handed back are loss_fn + r, and x moves as torch.optim.Adam moves it on the summed objective"""
    from pix2latent_amd import VariableManager
    from pix2latent_amd.optimizer.closure import step
    import pix2latent_amd.loss_functions as LF
    model = ToyGenerator()
    for p in model.parameters():
        p.requires_grad_(False)
    loss_fn = LF.ReconstructionLoss()

    def make():
        vm = VariableManager(device='cpu')
        g = torch.Generator().manual_seed(11)
        vm.register('z', (6,), 'input', learning_rate=0.05, default=torch.randn(6, generator=g), regularizer=_spy)
        vm.register('c', (4,), 'input', learning_rate=0.02, default=torch.randn(4, generator=g))
        vm.register('target', (3, 4, 4), 'output', requires_grad=False, default=toy_target())
        vm.register('weight', (3, 4, 4), 'output', requires_grad=False, default=toy_weight())
        v = vm.initialize(num_samples=3)
        with torch.no_grad():
            for i in range(3):                      # three different candidates
                v.input.z.data[i].add_(0.1 * i)
        return v

    def objective(z, c):
        out = model(z=z, c=c)
        t = toy_target().unsqueeze(0).expand(3, -1, -1, -1)
        w = toy_weight().unsqueeze(0).expand(3, -1, -1, -1)
        return loss_fn(out, t, w).view(3, -1).mean(1) + _spy(z)

    v = make()
    z0 = torch.stack(list(v.input.z.data)).detach().clone()
    c0 = torch.stack(list(v.input.c.data)).detach().clone()
    want = objective(z0, c0)
    # forward-only pass: the term is in the losses, nothing moves
    _, losses, _ = step(model, v, loss_fn, optimize=False, max_batch_size=3)
    assert np.allclose(np.asarray(losses, dtype=np.float64), want.numpy(), rtol=1e-6, atol=0)
    assert torch.equal(torch.stack(list(v.input.z.data)), z0)
    plain = loss_fn(model(z=z0, c=c0), toy_target().unsqueeze(0).expand(3, -1, -1, -1),
                    toy_weight().unsqueeze(0).expand(3, -1, -1, -1)).view(3, -1).mean(1)
    assert (want - plain).min() > 0.05              # the term is not a rounding error
    # one Adam step
    _, losses, _ = step(model, v, loss_fn, optimize=True, max_batch_size=3)
    assert np.allclose(np.asarray(losses, dtype=np.float64), want.numpy(), rtol=1e-6, atol=0)
    zr, cr = z0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    ref = torch.optim.Adam([{'params': [zr], 'lr': 0.05}, {'params': [cr], 'lr': 0.02}])
    objective(zr, cr).mean().backward()
    ref.step()
    assert torch.allclose(torch.stack(list(v.input.z.data)), zr.detach(), rtol=0, atol=1e-6)
    assert torch.allclose(torch.stack(list(v.input.c.data)), cr.detach(), rtol=0, atol=1e-6)
    # without the regulariser z moves elsewhere: the comparison above can tell
    zr2 = z0.clone().requires_grad_(True)
    ref2 = torch.optim.Adam([zr2], lr=0.05)
    (objective(zr2, c0).mean() - _spy(zr2).mean()).backward()
    ref2.step()
    assert (zr2.detach() - zr.detach()).abs().max() > 1e-3

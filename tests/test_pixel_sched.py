"""Learning-rate schedules and the pixel-term options of the losses, on the host: the schedule
tables against tests/_pixel_sched_ref.py, a scheduled run of the generic (torch) optimizer path against a hand loop,
the CPU route of the L2 loss, and the names of the new entry points.  CPU only."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pixel_sched_ref as R  # noqa: E402
from _toy import ToyGenerator, toy_target, toy_weight  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- schedule values -----------------------------------------------------------------------------------------------
def test_exported_from_both_packages():
    import pix2latent
    import pix2latent_amd
    from pix2latent_amd.lr_schedule import LRSchedule
    assert pix2latent_amd.LRSchedule is LRSchedule and pix2latent.LRSchedule is LRSchedule
    assert 'LRSchedule' in pix2latent_amd.__all__


def test_projector_ramp_values():
    from pix2latent_amd import LRSchedule
    s = LRSchedule.projector_ramp(0.1, 1000)
    assert len(s) == 1000 and s.values.dtype == np.float32
    assert s.value(0) == 0.0
    assert F32(s.value(400)) == F32(0.1) and F32(s.value(50)) == F32(0.1) and F32(s.value(750)) == F32(0.1)
    assert R.ulps(s.value(25), F32(0.05)) <= 1                # half the ramp-up
    assert R.ulps(s.value(875), F32(0.05)) <= 1               # half-way down the cosine
    assert np.array_equal(s.values, R.fp32(R.projector_ramp(0.1, 1000)))
    # up over the first 5 %, flat, down over the last 25 %
    v = s.values
    assert (np.diff(v[:51]) > 0).all() and (v[50:751] == F32(0.1)).all() and (np.diff(v[750:]) < 0).all()
    assert 0 < v[-1] < 1e-5
    # other ramps, and the docstring names the formula as unpinned
    assert np.array_equal(LRSchedule.projector_ramp(0.02, 37, 0.5, 0.1).values, R.fp32(R.projector_ramp(0.02, 37, 0.5, 0.1)))
    assert 'unpinned' in LRSchedule.projector_ramp.__doc__.lower()


def test_cosine_constant_and_the_end_of_a_table():
    from pix2latent_amd import LRSchedule
    c = LRSchedule.cosine(0.05, 101, final=0.01)
    assert F32(c.value(0)) == F32(0.05) and F32(c.value(100)) == F32(0.01)
    assert R.ulps(c.value(50), F32(0.03)) <= 1
    assert np.abs(c.values.astype(np.float64) - np.asarray(R.cosine(0.05, 101, 0.01))).max() <= 2.0 ** -24 * 0.05
    assert (np.diff(c.values) < 0).all()
    assert F32(LRSchedule.cosine(0.05, 10).value(9)) == 0.0
    # after its end the last value holds
    assert c.value(101) == c.value(100) == c.value(10 ** 9)
    k = LRSchedule.constant(0.05)
    assert len(k) == 1 and [k.value(i) for i in (0, 1, 77)] == [float(F32(0.05))] * 3
    t = LRSchedule([0.1, 0.2, 0.3])
    assert [F32(t.value(i)) for i in range(5)] == [F32(0.1), F32(0.2), F32(0.3), F32(0.3), F32(0.3)]
    with pytest.raises(ValueError):
        LRSchedule([])
    with pytest.raises(ValueError):
        LRSchedule([0.1, float('nan')])


def test_graph_key():
    from pix2latent_amd import LRSchedule
    a, b = LRSchedule([0.1, 0.2, 0.3]), LRSchedule([0.1, 0.2, 0.3])
    c = LRSchedule([0.1, 0.2, float(np.nextafter(F32(0.3), F32(1.0)))])
    assert a.graph_key() == b.graph_key() and a.graph_key()[0] == 'LRSchedule'
    assert a.graph_key() != c.graph_key()
    assert LRSchedule([0.1]).graph_key() != LRSchedule([0.1, 0.1]).graph_key()
    # the device copy is made once per device
    assert a.device_table('cpu') is a.device_table(torch.device('cpu'))
    assert a.device_table('cpu').dtype == torch.float32 and a.device_table('cpu').tolist() == a.values.tolist()


# ---- a scheduled variable on the generic path ----------------------------------------------------------------------
def test_generic_path_follows_the_schedule():
    """five steps of GradientOptimizer over CPU variables (torch.optim.Adam underneath) = a hand loop that sets
    group['lr'] per step: both are torch, to the bit"""
    from pix2latent_amd import VariableManager, LRSchedule
    from pix2latent_amd.optimizer import GradientOptimizer
    import pix2latent_amd.loss_functions as LF
    sched = LRSchedule.projector_ramp(0.1, 4, rampdown=0.5)    # 0, 0.1, 0.1, 0.05; holds its last value at step 5
    assert len(set(sched.values.tolist())) >= 3
    z0 = torch.linspace(-0.5, 0.5, 6)
    c0 = torch.linspace(-0.2, 0.2, 4)
    target, weight = toy_target(), toy_weight()
    loss_fn = LF.ReconstructionLoss('l2')

    def run(lr):
        vm = VariableManager(device='cpu')
        vm.register('z', (6,), 'input', default=z0, learning_rate=lr)
        vm.register('c', (4,), 'input', default=c0, learning_rate=0.01)
        vm.register('target', (3, 4, 4), 'output', requires_grad=False, default=target)
        vm.register('weight', (3, 4, 4), 'output', requires_grad=False, default=weight)
        opt = GradientOptimizer(ToyGenerator(), vm, loss_fn, max_batch_size=9)
        variables = vm.initialize(num_samples=2)
        with torch.no_grad():
            variables.input.z.data[1].mul_(-1.5)
        assert isinstance(variables.opt, torch.optim.Adam)
        losses = []
        for _ in range(5):
            _, l, _ = opt.step(variables, optimize=True, transform=False)
            losses.append(np.array(l, dtype=np.float64))
        return (np.stack(losses), torch.stack(list(variables.input.z.data)).detach().clone(),
                torch.stack(list(variables.input.c.data)).detach().clone(), variables.opt)

    losses, z, c, opt = run(sched)
    assert [g.get('lr_schedule') for g in opt.param_groups] == [sched, sched, None, None]
    assert opt.param_groups[0]['lr'] == sched.value(4) and opt.param_groups[2]['lr'] == 0.01

    # the hand loop
    model = ToyGenerator()
    zs = [z0.clone().requires_grad_(True), (z0 * -1.5).requires_grad_(True)]
    cs = [c0.clone().requires_grad_(True) for _ in range(2)]
    ref = torch.optim.Adam([{'params': p, 'lr': sched.value(0)} for p in zs] + [{'params': p, 'lr': 0.01} for p in cs])
    t2, w2 = torch.stack([target, target]), torch.stack([weight, weight])
    ref_losses = []
    for i in range(5):
        for g in ref.param_groups[:2]:
            g['lr'] = sched.value(i)
        ref.zero_grad()
        loss = loss_fn(model(z=torch.stack(zs), c=torch.stack(cs)), target=t2, weight=w2).view(2, -1).mean(1)
        loss.mean().backward()
        ref.step()
        ref_losses.append(loss.detach().double().numpy())
    assert np.array_equal(losses, np.stack(ref_losses))
    assert torch.equal(z, torch.stack(zs).detach()) and torch.equal(c, torch.stack(cs).detach())
    # lr 0 at the first step: z has not moved after it, c has; and a constant rate is another trajectory
    assert sched.value(0) == 0.0
    const = run(0.1)
    assert not torch.equal(const[1], z) and losses[1, 0] != const[0][1, 0]
    assert torch.equal(run(LRSchedule.constant(0.1))[1], const[1])


def test_generic_path_follows_the_schedule_with_sgd():
    """an optimizer class that keeps no step count of its own (torch.optim.SGD), two chunks of one sample: five steps
    = a hand loop that sets group['lr'] per step and steps sample by sample, to the bit"""
    from pix2latent_amd import VariableManager, LRSchedule
    from pix2latent_amd.optimizer import GradientOptimizer
    import pix2latent_amd.loss_functions as LF
    sched = LRSchedule.projector_ramp(0.1, 4, rampdown=0.5)    # 0, 0.1, 0.1, 0.05, 0.05, ...
    z0 = torch.linspace(-0.5, 0.5, 6)
    c0 = torch.linspace(-0.2, 0.2, 4)
    target, weight = toy_target(), toy_weight()
    loss_fn = LF.ReconstructionLoss('l2')

    def run(lr):
        vm = VariableManager(device='cpu')
        vm.register('z', (6,), 'input', default=z0, learning_rate=lr, optimizer=torch.optim.SGD)
        vm.register('c', (4,), 'input', default=c0, learning_rate=0.01, optimizer=torch.optim.SGD)
        vm.register('target', (3, 4, 4), 'output', requires_grad=False, default=target)
        # (the optimizer class is the one of the LAST registered variable, as in the reference)
        vm.register('weight', (3, 4, 4), 'output', requires_grad=False, default=weight, optimizer=torch.optim.SGD)
        opt = GradientOptimizer(ToyGenerator(), vm, loss_fn, max_batch_size=1)
        variables = vm.initialize(num_samples=2)
        with torch.no_grad():
            variables.input.z.data[1].mul_(-1.5)
        assert isinstance(variables.opt, torch.optim.SGD)
        for _ in range(5):
            opt.step(variables, optimize=True, transform=False)
        return torch.stack(list(variables.input.z.data)).detach().clone(), variables.opt

    z, opt = run(sched)
    assert [g.get('lr_step') for g in opt.param_groups] == [5, 5, None, None]
    assert opt.param_groups[0]['lr'] == sched.value(4)

    model = ToyGenerator()
    zs = [z0.clone().requires_grad_(True), (z0 * -1.5).requires_grad_(True)]
    cs = [c0.clone().requires_grad_(True) for _ in range(2)]
    ref = torch.optim.SGD([{'params': p, 'lr': sched.value(0)} for p in zs] + [{'params': p, 'lr': 0.01} for p in cs])
    for i in range(5):
        for s in range(2):
            for g in ref.param_groups[:2]:
                g['lr'] = sched.value(i)
            ref.zero_grad()
            out = model(z=torch.stack([zs[s]]), c=torch.stack([cs[s]]))
            loss_fn(out, target=target.unsqueeze(0), weight=weight.unsqueeze(0)).view(1, -1).mean(1).mean().backward()
            ref.step()
    assert torch.equal(z, torch.stack(zs).detach())
    # the ramp is followed: not the trajectory of its first entry (0: z would not move), nor of a constant rate
    assert not torch.equal(z, torch.stack([z0, z0 * -1.5])) and not torch.equal(run(0.1)[0], z)


# ---- the losses on CPU tensors -------------------------------------------------------------------------------------
def test_l2_on_cpu_tensors_is_the_torch_expression():
    import pix2latent_amd.loss_functions as LF
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'losses.npz'), allow_pickle=False)
    o, t, w, m = (torch.from_numpy(g[k]) for k in ('o', 't', 'w', 'm'))
    rl2 = LF.ReconstructionLoss('l2')
    assert np.array_equal(rl2(o, t, w).numpy(), g['rec_l2_w'])
    assert rl2._engine is None                                 # (no native engine for CPU tensors)
    want = torch.sum((t - o) ** 2 * (m * w), [1, 2, 3]) / torch.sum(m * w, [1, 2, 3])
    assert torch.equal(rl2(o, t, w, m), want)
    # the one-channel-weight quirk: the numerator runs over three channels, the denominator over one
    w1 = w[:, :1]
    three = rl2(o, t, w1.expand(-1, 3, -1, -1).contiguous())
    assert torch.allclose(rl2(o, t, w1), 3.0 * three, rtol=1e-6, atol=0)


def test_projection_loss_arguments():
    import pix2latent_amd.loss_functions as LF
    with pytest.raises(ValueError, match='pixel_loss'):
        LF.ProjectionLoss(pixel_loss='l3')
    with pytest.raises(ValueError, match='pixel_weight'):
        LF.ProjectionLoss(pixel_loss='l2', pixel_weight=-1.0)
    with pytest.raises(ValueError, match='pixel_weight'):
        LF.ProjectionLoss(pixel_weight=float('nan'))


# ---- the boundary --------------------------------------------------------------------------------------------------
NEW = ('p2l_l2_loss_nblk', 'p2l_l2_loss_fwd', 'p2l_l2_loss_bwd', 'p2l_adam_step_sched')


def test_new_entry_points_are_declared_and_exported():
    from pix2latent_amd import _native as N
    header = open(os.path.join(ROOT, 'include', 'p2l.h')).read()
    declared = set(re.findall(r'\b(p2l_[a-z0-9_]+)\s*\(', header))
    lib = N.lib()
    for name in NEW:
        assert name in declared, name
        assert name in N.EXPORTS and hasattr(lib, name), name
    assert lib.p2l_version() == 101
    # the argument-checked list of the header names them
    checked = header[header.index('Host-side argument checks'):header.index('Every OTHER entry point')]
    assert 'p2l_l2_loss_fwd/_bwd' in checked and 'p2l_adam_step_sched' in checked
    # sizes are shape arithmetic: no device needed
    assert lib.p2l_l2_loss_nblk(4, 4) == 1 and lib.p2l_l2_loss_nblk(32, 32) == 1
    assert lib.p2l_l2_loss_nblk(32, 33) == 2 and lib.p2l_l2_loss_nblk(1024, 1024) == 1024
    assert lib.p2l_l2_loss_nblk(0, 4) == 0

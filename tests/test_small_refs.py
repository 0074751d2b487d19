"""The float64 references of tests/_small_refs.py against independent formulations of the same operations (runs on
a CPU-only machine): a reference that is wrong would make every kernel test built on it worthless."""
import pytest
import torch
import torch.nn.functional as F

import _small_refs as R
from oracle import lpips_ref, stylegan2_ref

D = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize('h,w', [(1, 1), (4, 4), (3, 5), (16, 16)])
def test_rgb_up_is_a_transposed_conv(h, w):
    """upfirdn2d(up=2, pad=(2,1)) with the 4x4 FIR == conv_transpose2d(stride 2, padding 1) with the same kernel;
    and == the oracle's own upfirdn2d."""
    x = torch.randn(2, 4, h, w, generator=_g(1), dtype=D)
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=D)
    k = torch.outer(k1, k1) / 16.0
    want = F.conv_transpose2d(x.reshape(8, 1, h, w), k.view(1, 1, 4, 4), stride=2, padding=1).view(2, 4, 2 * h, 2 * w)
    got = R.upfirdn2d_up2(x)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < 1e-14
    ora = stylegan2_ref.upfirdn2d(x, stylegan2_ref.make_kernel([1, 3, 3, 1]).double() * 4, up=2, pad=(2, 1))
    assert (got - ora).abs().max().item() < 1e-14
    # the NHWC16 wrapper: channels 4..15 zero, and its vjp is the adjoint (<up(x), g> == <x, up^T g>)
    x16 = torch.randn(2, h, w, 16, generator=_g(2), dtype=D)
    g16 = torch.randn(2, 2 * h, 2 * w, 16, generator=_g(3), dtype=D)
    up = R.rgb_up(x16)
    assert torch.equal(up[..., 4:], torch.zeros_like(up[..., 4:]))
    dsk = R.rgb_up_bwd(g16, h, w)
    assert abs((up * g16).sum().item() - (x16 * dsk).sum().item()) < 1e-10
    assert torch.equal(dsk[..., 4:], torch.zeros_like(dsk[..., 4:]))


def test_pixelnorm_and_demod_gradcheck():
    z = torch.randn(3, 7, generator=_g(4), dtype=D, requires_grad=True)
    assert torch.autograd.gradcheck(R.pixelnorm, (z,))
    s = (0.5 + torch.rand(3, 6, generator=_g(5), dtype=D)).requires_grad_(True)
    Wsq = torch.rand(6, 5, generator=_g(6), dtype=D)
    assert torch.autograd.gradcheck(lambda s_: R.demod(s_, Wsq), (s,))
    # and the vjp helpers against the hand-derived forms in the kernel comments' algebra
    dy = torch.randn(3, 7, generator=_g(7), dtype=D)
    zz = z.detach()
    r = torch.rsqrt((zz * zz).mean(1, keepdim=True) + 1e-8)
    hand = r * dy - zz * r ** 3 * (zz * dy).sum(1, keepdim=True) / 7
    assert (R.vjp(R.pixelnorm, [zz], dy) - hand).abs().max().item() < 1e-13
    dd = torch.randn(3, 5, generator=_g(8), dtype=D)
    d = R.demod(s.detach(), Wsq)
    hand = 2 * s.detach() * ((dd * -0.5 * d ** 3) @ Wsq.t())
    assert (R.demod_bwd(s.detach(), Wsq, dd) - hand).abs().max().item() < 1e-12


def test_l1_is_the_reference_expression():
    g = _g(9)
    B, H, W = 3, 6, 10
    out = torch.randn(B, 3, H, W, generator=g, dtype=D)
    target = torch.randn(B, 3, H, W, generator=g, dtype=D)
    weight = torch.rand(B, 3, H, W, generator=g, dtype=D)
    mask = (torch.rand(B, 3, H, W, generator=g) > 0.3).double()
    img16 = R.nchw3_to_nhwc16(out)
    for m in (None, mask):
        want = lpips_ref.reconstruction_loss(out, target, weight=weight, loss_mask=m, loss_type='l1')
        assert (R.l1_loss(img16, target, weight, m) - want).abs().max().item() < 1e-14
        assert (R.weight_sum(weight, m) - (weight if m is None else weight * m).sum((1, 2, 3))).abs().max() < 1e-12
    # backward: sign(o - t) * w / sum w * gscale, zero where o == t
    out[0, 0, 0, 0] = target[0, 0, 0, 0]
    img16 = R.nchw3_to_nhwc16(out)
    gs = torch.randn(B, generator=g, dtype=D)
    got = R.l1_loss_bwd(img16, target, weight, mask, gs)
    w = weight * mask
    hand = torch.sign(out - target) * w / w.sum((1, 2, 3), keepdim=True) * gs.view(B, 1, 1, 1)
    assert (R.nhwc16_to_nchw3(got) - hand).abs().max().item() < 1e-14
    assert got[0, 0, 0, 0].item() == 0.0
    assert torch.equal(got[..., 3:], torch.zeros_like(got[..., 3:]))


def test_cbn_fold_is_batchnorm_with_conditional_gain():
    g = _g(10)
    B, C = 4, 9
    x = torch.randn(B, C, 5, 5, generator=g, dtype=D)
    mean, var = torch.randn(C, generator=g, dtype=D), 0.5 + torch.rand(C, generator=g, dtype=D)
    rstd = torch.rsqrt(var + 1e-4)
    g_raw, b_raw = torch.randn(B, C, generator=g, dtype=D), torch.randn(B, C, generator=g, dtype=D)
    s, t = R.cbn_fold(g_raw, b_raw, mean, rstd)
    bn = F.batch_norm(x, mean, var, None, None, False, 0.0, 1e-4)        # (x - mean) * rstd
    want = bn * (1 + g_raw).view(B, C, 1, 1) + b_raw.view(B, C, 1, 1)
    got = x * s.view(B, C, 1, 1) + t.view(B, C, 1, 1)
    assert (got - want).abs().max().item() < 1e-12
    ds, dt = torch.randn(B, C, generator=g, dtype=D), torch.randn(B, C, generator=g, dtype=D)
    dg, db = R.cbn_fold_bwd(ds, dt, mean, rstd)
    assert (dg - (ds * rstd - dt * mean * rstd)).abs().max().item() < 1e-13         # the header's formula
    assert torch.equal(db, dt)


def test_activation_edges_and_styled_act():
    z = torch.tensor([0.0, -0.0, 1.0, -1.0, 1e-30, -1e-30], dtype=D)
    assert torch.equal(R.lrelu(z), torch.tensor([0.0, -0.0, 1.0, -0.2, 1e-30, -0.2e-30], dtype=D))
    gy = R.lrelu_bwd(z, torch.ones_like(z))
    assert torch.allclose(gy, torch.tensor([.2, .2, 1, .2, 1, .2], dtype=D) * R.SQRT2, rtol=0, atol=1e-15)
    assert torch.equal(R.relu_mask(z, torch.ones_like(z)), torch.tensor([0, 0, 1, 0, 1, 0], dtype=D))
    x16 = torch.zeros(1, 1, 2, 16, dtype=D)
    x16[0, 0, 0, :3] = torch.tensor([1.0, -1.0, 1.0 + 1e-9], dtype=D)
    x16[0, 0, 1, :3] = torch.tensor([-1.0 - 1e-9, 0.5, -0.0], dtype=D)
    dx = R.clamp16_bwd(x16, torch.ones_like(x16))
    assert dx[0, 0, 0, :4].tolist() == [1, 1, 0, 0] and dx[0, 0, 1, :4].tolist() == [0, 1, 1, 0]
    # styled activation backward against fused_leaky_relu of the oracle + hand-derived sums
    g = _g(11)
    B, P, C = 2, 9, 4
    c, d = torch.randn(B, P, C, generator=g, dtype=D), 0.5 + torch.rand(B, C, generator=g, dtype=D)
    noise, bias = torch.randn(B, P, generator=g, dtype=D), torch.randn(C, generator=g, dtype=D)
    dy = torch.randn(B, P, C, generator=g, dtype=D)
    pre = c * d[:, None] + 0.3 * noise[:, :, None]
    want_y = stylegan2_ref.fused_leaky_relu(pre.permute(0, 2, 1).reshape(B, C, 3, 3), bias)
    y = R.styled_act(c, d, noise, 0.3, bias)
    assert (y.permute(0, 2, 1).reshape(B, C, 3, 3) - want_y).abs().max().item() < 1e-14
    gd, dd, dn = R.styled_act_bwd(dy, c, d, noise, 0.3, bias)
    g1 = dy * torch.where(y > 0, torch.tensor(R.SQRT2, dtype=D), torch.tensor(R.SLOPE * R.SQRT2, dtype=D))
    assert (gd - g1 * d[:, None]).abs().max().item() < 1e-14
    assert (dd - (g1 * c).sum(1)).abs().max().item() < 1e-13
    assert (dn - 0.3 * g1.sum(2)).abs().max().item() < 1e-13


def test_adam_reference_restarts_at_a_step():
    g = _g(12)
    p0 = torch.randn(50, generator=g)
    grads = [torch.randn(50, generator=g) for _ in range(4)]
    full = R.adam_reference(p0, grads, 0.05)
    # hand formula of torch.optim.Adam for step 1: p - lr * g / (|g| + eps)
    want = p0 - 0.05 * grads[0] / (grads[0].abs() + 1e-8)
    assert (full[0] - want).abs().max().item() < 1e-6
    # restarting from the state after two steps reproduces steps 3 and 4
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=0.05)
    for gr in grads[:2]:
        p.grad = gr.clone()
        opt.step()
    st = opt.state[p]
    tail = R.adam_reference(p.detach(), grads[2:], 0.05, first_step=3, m0=st['exp_avg'], v0=st['exp_avg_sq'])
    assert torch.equal(tail[-1], full[-1])


def test_layout_and_misc():
    g = _g(13)
    src = torch.randn(2, 3, 4, 5, generator=g, dtype=D)
    i16 = R.nchw3_to_nhwc16(src)
    assert torch.equal(R.nhwc16_to_nchw3(i16), src) and torch.equal(i16[..., 3:], torch.zeros(2, 4, 5, 13, dtype=D))
    img = torch.tanh(torch.randn(2, 4, 5, 16, generator=g, dtype=D))
    dimg = torch.randn(2, 4, 5, 16, generator=g, dtype=D)
    got = R.tanh_bwd16(img, dimg)
    assert (got[..., :3] - dimg[..., :3] * (1 - img[..., :3] ** 2)).abs().max().item() < 1e-12
    assert torch.equal(got[..., 4:], dimg[..., 4:]) and got[..., 3].abs().max().item() == 0
    part, div = torch.randn(3, 17, generator=g, dtype=D), 1 + torch.rand(3, generator=g, dtype=D)
    assert torch.allclose(R.reduce_rows(part, 0.5, div), 0.5 * part.sum(1) / div, rtol=1e-15, atol=0)
    W = torch.randn(8, 6, generator=g, dtype=D)
    dy = torch.randn(3, 6, generator=g, dtype=D)
    assert (R.linear_bwd(dy, W) - dy @ W.t()).abs().max().item() < 1e-13

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


# ---- LPIPS loss path ---------------------------------------------------------------------------------------------
def test_lpips_tap_bwd_closed_form_is_autograd_and_finite_at_zero():
    g = _g(20)
    B, P, C = 3, 11, 8
    f = F.relu(torch.randn(B, P, C, generator=g, dtype=D))
    f[1, 4] *= 1e-10                                                     # the eps matters here
    f[2, 0] = 0
    f[2, 0, 3] = 1e-10
    ft = F.relu(torch.randn(B, P, C, generator=g, dtype=D))
    ft[0, 2] = 0
    nft = R.lpips_normalize(ft)
    assert torch.equal(nft[0, 2], torch.zeros(C, dtype=D))               # 0 / (0 + 1e-10)
    assert abs(nft[1, 1].norm().item() - 1) < 1e-9
    lin, wt = torch.rand(C, generator=g, dtype=D), torch.rand(B, P, generator=g, dtype=D)
    gs = torch.tensor([0.7, -1.3, 0.4], dtype=D)
    # the forward is the oracle's expression (lpips_ref.normalize_tensor over the channel axis of NCHW)
    nchw = lambda t: t.view(B, 1, P, C).permute(0, 3, 1, 2)
    d = ((lpips_ref.normalize_tensor(nchw(f)) - nchw(nft)) ** 2 * lin.view(1, C, 1, 1)).sum(1)[:, 0]
    assert (R.lpips_tap(f, nft, lin, wt) - (d * wt).sum(1)).abs().max().item() < 1e-14
    got = R.lpips_tap_bwd(f, nft, lin, wt, gs)
    auto = R.vjp(lambda f_: R.lpips_tap(f_, nft, lin, wt), [f], gs)
    assert bool(torch.isfinite(auto).all())
    scale = auto.abs().amax(dim=2, keepdim=True) + 1e-300
    assert ((got - auto).abs() / scale).max().item() < 1e-9
    # a shared target: nft [P, C], wt [P]
    shared = R.lpips_tap_bwd(f, nft[0], lin, wt[0], gs)
    assert torch.equal(shared, R.lpips_tap_bwd(f, nft[:1].expand(B, P, C), lin, wt[:1].expand(B, P), gs))
    # an all-zero pixel: autograd is NaN there (and only there), the closed form is gscale wt u / eps
    f[0, 5] = 0
    auto = R.vjp(lambda f_: R.lpips_tap(f_, nft, lin, wt), [f], gs)
    nan = torch.isnan(auto).any(dim=2)
    assert bool(nan[0, 5]) and int(nan.sum()) == 1
    got = R.lpips_tap_bwd(f, nft, lin, wt, gs)
    assert bool(torch.isfinite(got).all())
    want = gs[0] * wt[0, 5] * 2 * lin * (0 - nft[0, 5]) / 1e-10
    assert torch.allclose(got[0, 5], want, rtol=1e-14, atol=0)
    keep = ~nan
    assert ((got - auto).abs() / scale)[keep].max().item() < 1e-9


def _upsample_matrix(n_out, n_in):
    """[n_out, n_in] weights of bilinear interpolation along one axis, align_corners=False"""
    U = torch.zeros(n_out, n_in, dtype=D)
    for p in range(n_out):
        src = max((p + 0.5) * n_in / n_out - 0.5, 0.0)
        i0 = int(src)
        i1 = min(i0 + 1, n_in - 1)
        U[p, i0] += 1 - (src - i0)
        U[p, i1] += src - i0
    return U


@pytest.mark.parametrize('H,W,h,w', [(8, 8, 8, 8), (16, 8, 4, 4), (64, 48, 7, 3), (37, 53, 9, 20), (16, 16, 1, 1)])
def test_bilinear_adjoint_is_the_transposed_dense_matrix(H, W, h, w):
    wsrc = torch.randn(2, H, W, generator=_g(21), dtype=D)
    Uy, Ux = _upsample_matrix(H, h), _upsample_matrix(W, w)
    m = torch.randn(2, 1, h, w, generator=_g(22), dtype=D)
    up = F.interpolate(m, size=(H, W), mode='bilinear', align_corners=False)[:, 0]
    assert (up - Uy @ m[:, 0] @ Ux.t()).abs().max().item() < 1e-13       # the matrix is the upsampling
    want = Uy.t() @ wsrc @ Ux
    got = R.bilinear_adjoint(wsrc, h, w)
    assert got.shape == (2, h, w) and (got - want).abs().max().item() < 1e-12


@pytest.mark.parametrize('H,W,Co,K,S,pad', [(3, 3, 4, 3, 2, 0), (19, 16, 8, 3, 2, 0), (37, 50, 4, 11, 4, 2), (5, 5, 4, 1, 2, 0)])
def test_conv1_dgrad_is_autograd_of_conv2d(H, W, Co, K, S, pad):
    g = _g(23)
    w = torch.randn(Co, 3, K, K, generator=g, dtype=D)
    x = torch.randn(2, 3, H, W, generator=g, dtype=D)
    y = F.conv2d(x, w, None, stride=S, padding=pad)
    dy = torch.randn(y.shape, generator=g, dtype=D)
    want = R.vjp(lambda x_: F.conv2d(x_, w, None, stride=S, padding=pad), [x], dy)
    w_t3 = w.permute(2, 3, 1, 0).reshape(K * K, 3, Co).contiguous()
    got = R.conv1_dgrad(dy.permute(0, 2, 3, 1).contiguous(), w_t3, H, W, K, S, pad)
    assert got.shape == (2, H, W, 16) and torch.equal(got[..., 3:], torch.zeros(2, H, W, 13, dtype=D))
    assert (got[..., :3] - want.permute(0, 2, 3, 1)).abs().max().item() < 1e-12
    # pixels that no window covers: exactly zero
    cov_y = torch.zeros(H + 2 * pad, dtype=torch.bool)
    cov_x = torch.zeros(W + 2 * pad, dtype=torch.bool)
    for o in range(y.shape[2]):
        cov_y[o * S:o * S + K] = True
    for o in range(y.shape[3]):
        cov_x[o * S:o * S + K] = True
    cov = cov_y[pad:pad + H, None] & cov_x[None, pad:pad + W]
    assert bool((got[:, ~cov] == 0).all())
    if (H + 2 * pad - K) % S or K < S:
        assert not bool(cov.all())


def test_pool_references_on_hand_written_ties():
    """ATen's rule, written out: the first maximum in row-major scan order of the window takes the gradient"""
    # 2x2: one quad per channel; value 5 at the listed positions, 1 elsewhere; expected winner = the first listed
    pats = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3), (0, 1, 2, 3)]
    y = torch.ones(1, 2, 2, len(pats), dtype=D)
    for c, pat in enumerate(pats):
        for s in pat:
            y[0, s >> 1, s & 1, c] = 5.0
    dyp = torch.arange(1, len(pats) + 1, dtype=D).view(1, 1, 1, -1)
    got = R.maxpool2_bwd(y, dyp)
    want = torch.zeros_like(y)
    for c, pat in enumerate(pats):
        want[0, pat[0] >> 1, pat[0] & 1, c] = c + 1
    assert torch.equal(got, want)
    add = torch.full_like(y, 0.5)
    assert torch.equal(R.maxpool2_bwd(y, dyp, add), want + 0.5)
    y0 = y.clone()
    y0[0, 0, 0, :] = 0.0                                                 # masked where y == 0, after the add
    got = R.maxpool2_bwd(y0, dyp, add, True)
    assert torch.equal(got[0, 0, 0], torch.zeros(len(pats), dtype=D)) and torch.equal(got[0, 1, 1], R.maxpool2_bwd(y0, dyp, add)[0, 1, 1])
    # 3x3 / stride 2 on an all-equal 5x5: four windows, each sends its gradient to its first element
    x = torch.full((1, 5, 5, 1), 2.0, dtype=D)
    gp = torch.tensor([[1.0, 2.0], [4.0, 8.0]], dtype=D).view(1, 2, 2, 1)
    assert torch.equal(R.maxpool3s2(x), torch.full((1, 2, 2, 1), 2.0, dtype=D))
    want = torch.zeros(5, 5, dtype=D)
    want[0, 0], want[0, 2], want[2, 0], want[2, 2] = 1, 2, 4, 8
    assert torch.equal(R.maxpool3s2_bwd(x, gp)[0, :, :, 0], want)
    # ties at scan positions 4 and 8 of window (0, 0); position 8 is position 0 of window (1, 1) and its only maximum
    x = torch.ones(1, 5, 5, 1, dtype=D)
    x[0, 1, 1, 0] = x[0, 2, 2, 0] = 3.0
    want = torch.zeros(5, 5, dtype=D)
    want[1, 1], want[2, 2] = 1, 8                                        # windows (0,1) and (1,0) hold (2,2) alone
    want[2, 2] += 2 + 4
    assert torch.equal(R.maxpool3s2_bwd(x, gp)[0, :, :, 0], want)
    gt = torch.full((1, 5, 5, 1), 0.25, dtype=D)
    x[0, 2, 2, 0] = 0.0                                                  # (1,1) now wins all of window (0,0); (2,2) is masked
    got = R.maxpool3s2_bwd(x, gp, gt)[0, :, :, 0]
    assert got[1, 1].item() == 1.25 and got[2, 2].item() == 0.0 and got[4, 4].item() == 0.25
    # even sizes: the last row / column lies in no window and receives gtap only
    x = torch.rand(1, 6, 8, 2, generator=_g(24), dtype=D) + 0.1
    gp = torch.randn(1, 2, 3, 2, generator=_g(25), dtype=D)
    gt = torch.randn(1, 6, 8, 2, generator=_g(26), dtype=D)
    got = R.maxpool3s2_bwd(x, gp, gt)
    assert torch.equal(got[:, 5], gt[:, 5]) and torch.equal(got[:, :, 7], gt[:, :, 7])
    # the composition: tap backward + pool backward + mask
    f = F.relu(torch.randn(2, 4, 6, 8, generator=_g(27), dtype=D))
    nft = R.lpips_normalize(F.relu(torch.randn(2, 24, 8, generator=_g(28), dtype=D)))
    lin, wt = torch.rand(8, generator=_g(29), dtype=D), torch.rand(2, 24, generator=_g(30), dtype=D)
    gs, dyp = torch.tensor([0.5, -2.0], dtype=D), torch.randn(2, 2, 3, 8, generator=_g(31), dtype=D)
    tap = R.lpips_tap_bwd(f.view(2, 24, 8), nft, lin, wt, gs).view(2, 4, 6, 8)
    pooled = R.vjp(lambda f_: F.max_pool2d(f_.permute(0, 3, 1, 2), 2), [f], dyp.permute(0, 3, 1, 2))
    assert torch.equal(R.lpips_tap_pool_bwd(f, nft, lin, wt, gs, dyp), (pooled + tap) * (f > 0))


# ---- the glue kernels' references (tests/test_glue_kernels_gpu.py) -------------------------------------------------
@pytest.mark.parametrize('akm,bkm', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_layouts_and_pitches(akm, bkm):
    """both operand layouts at pitches above the row, junk in the gap: == a triple loop written as einsum on the
    dense operands, one B shared by the batch (leading dimension 1), alpha and the added C"""
    g = _g(60 + 2 * akm + bkm)
    bt, M, Nn, K = 3, 8, 6, 10
    a = torch.randn(bt, M, K, generator=g, dtype=D)
    b = torch.randn(bt, Nn, K, generator=g, dtype=D)
    c0 = torch.randn(bt, M, Nn, generator=g, dtype=D)

    def pitched(t, ld):
        o = torch.full(t.shape[:-1] + (ld,), 1e30, dtype=D)
        o[..., :t.shape[-1]] = t
        return o
    A = pitched(a.transpose(1, 2).contiguous(), M + 4) if akm else pitched(a, K + 8)
    B = pitched(b.transpose(1, 2).contiguous(), Nn + 12) if bkm else pitched(b, K + 4)
    want = torch.einsum('bmk,bnk->bmn', a, b)
    assert (R.gemm(A, B, M, Nn, K, akm, bkm) - want).abs().max().item() < 1e-13
    got = R.gemm(A, B, M, Nn, K, akm, bkm, -0.37, pitched(c0, Nn + 4))
    assert (got - (-0.37 * want + c0)).abs().max().item() < 1e-13
    shared = R.gemm(A, B[1:2], M, Nn, K, akm, bkm)
    assert (shared - torch.einsum('bmk,nk->bmn', a, b[1])).abs().max().item() < 1e-13


def test_softmax_rows_and_its_backward():
    g = _g(61)
    S = torch.randn(5, 32, generator=g, dtype=D) * 4
    S[1] = 2.5                                                   # all equal
    S[2] += 1e4                                                  # only the max subtraction keeps it finite
    S[3, 7] += 800.0                                             # the others underflow to exactly 0
    P = R.softmax_rows(S)
    assert (P - torch.softmax(S, dim=-1)).abs().max().item() < 1e-15
    assert (P.sum(-1) - 1).abs().max().item() < 1e-14
    assert torch.equal(P[1], torch.full((32,), 1.0 / 32, dtype=D))
    assert float(P[3, 7]) == 1.0 and float(P[3].sum()) == 1.0
    dP = torch.randn(5, 32, generator=g, dtype=D)
    want = R.vjp(R.softmax_rows, [S], dP)
    assert (R.softmax_rows_bwd(P, dP) - want).abs().max().item() < 1e-14
    # ... and the closed form is linear in P: on probabilities that do not sum to 1 (the fp32-rounded ones the kernel
    # is handed) it is the expression of the header, not the gradient at some other logits
    P2 = P * 1.25
    assert (R.softmax_rows_bwd(P2, dP) - P2 * (dP - (P2 * dP).sum(-1, keepdim=True))).abs().max().item() == 0.0


@pytest.mark.parametrize('skip_kind', ['none', 'same', 'half', 'zero', 'ups'])
def test_affine_relu_bwd_is_the_written_out_formula(skip_kind):
    g = _g(62)
    Bn, H, W, C = 2, 3, 5, 8
    P = H * W
    x = torch.randn(Bn, P, C, generator=g, dtype=D)
    s = torch.randn(Bn, C, generator=g, dtype=D)
    t = torch.randn(Bn, C, generator=g, dtype=D)
    da = torch.randn(Bn, P, C, generator=g, dtype=D)
    x[0, 0, 0], s[0, 0], t[0, 0] = 2.0, 0.5, -1.0                # x s + t == +0: masked off
    x[0, 1, 0] = -2.0
    t[1, 3] = -100.0                                             # a whole channel masked off
    a = R.affine_relu_fwd(x, s, t)
    assert float(a[0, 0, 0]) == 0 and bool((a[1, :, 3] == 0).all())
    m = ((x * s[:, None] + t[:, None]) > 0).to(D)
    skip, skip_C, ups = None, 0, False
    if skip_kind in ('same', 'half', 'zero'):
        skip, skip_C = torch.randn(Bn, P, C + 4, generator=g, dtype=D), {'same': C, 'half': C // 2, 'zero': 0}[skip_kind]
    elif skip_kind == 'ups':
        skip, skip_C, ups = torch.randn(Bn, 2 * H, 2 * W, C, generator=g, dtype=D), C // 2, True
    dx, ds, dt = R.affine_relu_bwd(da, x, s, t, skip, skip_C, ups, H, W)
    want = m * da * s[:, None]
    if skip_kind in ('same', 'half', 'zero'):
        want[:, :, :skip_C] += skip[:, :, :skip_C]
    elif ups:
        for yy in range(H):
            for xx in range(W):
                kids = skip[:, 2 * yy:2 * yy + 2, 2 * xx:2 * xx + 2, :skip_C].sum(dim=(1, 2))
                want[:, yy * W + xx, :skip_C] += kids
    assert (dx - want).abs().max().item() < 1e-13
    assert (ds - (m * da * x).sum(1)).abs().max().item() < 1e-13
    assert (dt - (m * da).sum(1)).abs().max().item() < 1e-13
    assert float(ds[1, 3]) == 0 and float(dt[1, 3]) == 0
    if skip_kind == 'none':
        assert float(dx[0, 0, 0]) == 0


def _random_thetas(g, Bn, scale=0.35):
    return (torch.eye(2, 3, dtype=D).view(1, 6) + scale * torch.randn(Bn, 6, generator=g, dtype=D))


@pytest.mark.parametrize('C,H,W', [(1, 8, 8), (3, 16, 32), (3, 24, 40), (1, 37, 53)])
def test_affine_warp_is_affine_grid_plus_grid_sample(C, H, W):
    g = _g(63)
    Bn = 4
    src = torch.randn(Bn, C, H, W, generator=g, dtype=D)
    theta = _random_thetas(g, Bn)
    theta[0] = torch.tensor([1.0, 0, 0, 0, 1.0, 0], dtype=D)                  # identity: the image itself
    theta[1] = torch.tensor([0.0, 0, 5.0, 0, 0.0, 0], dtype=D)                # every sample outside: exactly 0
    dout = torch.randn(Bn, C, H, W, generator=g, dtype=D)

    def torch_warp(s_, th_):
        grid = F.affine_grid(th_.view(-1, 2, 3), list(s_.shape), align_corners=False)
        return F.grid_sample(s_, grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    got, want = R.affine_warp(src, theta), torch_warp(src, theta)
    assert (got - want).abs().max().item() < 1e-12
    assert (got[0] - src[0]).abs().max().item() < 1e-13 and bool((got[1] == 0).all())
    dsrc, dth = R.affine_warp_bwd(src, theta, dout)
    wsrc, wth = R.vjp(torch_warp, [src, theta], dout)
    assert (dsrc - wsrc).abs().max().item() < 1e-12
    # (not image 0: with every sample ON a pixel centre the warp has a kink in theta at each of them, and which side
    #  a formulation differentiates depends on the last bit of its coordinate; d src has no such kink)
    assert ((dth - wth).abs() / (1 + wth.abs()))[1:].max().item() < 1e-11
    # the corner weights of a sample add up to 1, corner values outside the image are zero
    cs = R.warp_corners(torch.ones_like(src), theta)
    assert (sum(w for _, w in cs) - 1).abs().max().item() < 1e-13
    assert bool((cs[0][0][1] == 0).all())


@pytest.mark.parametrize('H,W', [(4, 4), (4, 8), (8, 4), (8, 12), (16, 4)])
def test_sg2_blur_is_conv2d_and_the_oracles_upfirdn(H, W):
    g = _g(64)
    Bn, C = 2, 4
    u = torch.randn(Bn, H + 2, W + 2, C, generator=g, dtype=D)
    u[:, H + 1] = 0
    u[:, :, W + 1] = 0
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=D)
    k = torch.outer(k1, k1) / 16.0                                           # [1 3 3 1]^2 / 64 * 4
    real = u[:, :H + 1, :W + 1].permute(0, 3, 1, 2)                          # the transposed conv's result
    want = F.conv2d(F.pad(real, [1, 1, 1, 1]).reshape(Bn * C, 1, H + 3, W + 3), k.view(1, 1, 4, 4))
    want = want.view(Bn, C, H, W).permute(0, 2, 3, 1)
    got = R.blur4(u)
    assert got.shape == (Bn, H, W, C) and (got - want).abs().max().item() < 1e-13
    ora = stylegan2_ref.upfirdn2d(real, stylegan2_ref.make_kernel([1, 3, 3, 1]).double() * 4, pad=(1, 1))
    assert (got - ora.permute(0, 2, 3, 1)).abs().max().item() < 1e-13
    # the activation around it: the oracle's noise injection and fused leaky ReLU
    d = torch.rand(Bn, C, generator=g, dtype=D) + 0.5
    noise = torch.randn(Bn, H * W, generator=g, dtype=D)
    bias = torch.randn(C, generator=g, dtype=D)
    for nz, nw in ((noise, 0.3), (noise, 0.0), (None, 0.3)):
        y = R.sg2_blur_fwd(u, d, nz, nw, bias)
        pre = want.permute(0, 3, 1, 2) * d[:, :, None, None]
        if nz is not None:
            pre = pre + nw * nz.view(Bn, 1, H, W)
        assert (y.permute(0, 3, 1, 2) - stylegan2_ref.fused_leaky_relu(pre, bias)).abs().max().item() < 1e-13
    # the transpose: <blur(u), g> == <u, blur^T g> for a FULL frame u; row H+1 and column W+1 of du are reached from
    # the last real row and column and are not zero
    gr = torch.randn(Bn, H, W, C, generator=g, dtype=D)
    du = R.sg2_blur_bwd(gr, H, W)
    full = torch.randn(Bn, H + 2, W + 2, C, generator=g, dtype=D)
    assert abs((R.blur4(full) * gr).sum().item() - (full * du).sum().item()) < 1e-10
    assert bool((du[:, H + 1, 1:] != 0).all()) and bool((du[:, 1:, W + 1] != 0).all())
    assert (du[:, H + 1, W + 1] - gr[:, H - 1, W - 1] / 16).abs().max().item() < 1e-15


def test_warp_general_seeds_stay_under_the_exclusion_cap():
    """the thetas tests/test_glue_kernels_gpu.py draws for its general warp cases leave fewer than 1 % of the samples
    within the coordinate bound of an integer -- on the reference alone, before any kernel is asked"""
    import _pin
    import test_glue_kernels_gpu as T
    try:
        for Cc, H, W in T.WARP_GENERAL:
            for sd in range(_pin.SEEDS + 3):
                _pin._DRAW['seed'] = sd
                theta = T._general_thetas(T._gen(208, Cc, H, W)).to(D)
                near, bx, by = T._near_integer(theta, H, W)
                assert float(near.float().mean(dim=(1, 2)).max()) < T.WARP_CAP, (Cc, H, W, sd)
                assert float(bx.max()) < 4096 and float(by.max()) < 4096           # the bound itself: < 2^-12 pixels
    finally:
        _pin._DRAW['seed'] = 0


# ---- 1x1 convs: the references, splits, packers and cases of tests/test_pw_kernels_gpu.py ---------------------------
@pytest.mark.parametrize('pro,pro_b', [(0, 1), (1, 1), (2, 0)])
@pytest.mark.parametrize('epi', range(len(R.EPI)))
def test_conv1x1_is_conv2d_with_the_epilogue(epi, pro, pro_b):
    """conv1x1 in fp64 == F.conv2d on NCHW + the header's epilogue written out once more, term by term"""
    c = R._pwc('A', (4, 6), 3, 16, 32, **dict(R.EPI[epi], pro=pro, pro_b=pro_b, n_store=24))
    i = {k: (v.to(D) if torch.is_tensor(v) else v) for k, v in R.pw_inputs(_g(50 + epi), c).items()}
    got = R.conv1x1(i['x'], i['w'], **R.pw_kwargs(c, i, D))
    a = i['x'].permute(0, 3, 1, 2)
    if pro:
        a = a * i['s'].expand(3, -1)[:, :, None, None] + i['t'].expand(3, -1)[:, :, None, None]
        a = F.relu(a) if pro == R.PRO_AFFINE_RELU else a
    v = c['alpha'] * F.conv2d(a, i['w'][:, :, None, None])
    if c['oscale']:
        v = v * i['oscale'][:, :, None, None]
    if c['noise']:
        v = v + i['noise_w'] * i['noise'][:, None]
    if c['bias']:
        v = v + i['bias'][None, :, None, None]
    if c['res']:
        r = i['res'].permute(0, 3, 1, 2)
        v = v + (F.interpolate(r, scale_factor=2, mode='nearest') if c['res'] == 'ups' else r)
    v = {0: lambda u: u, 1: F.relu, 2: torch.tanh, 3: lambda u: F.leaky_relu(u, 0.2) * R.SQRT2}[c['act']](v)
    if c['mask']:
        v = v * (i['mask'].permute(0, 3, 1, 2) > 0)
    v = v[:, :24]
    assert (got['y'].permute(0, 3, 1, 2) - v).abs().max().item() < 1e-12 * v.abs().max().item()
    if c['pool']:
        p = F.max_pool2d(v, 2) if c['pool'] == R.POOL_MAX else F.avg_pool2d(v, 2) * 4
        assert (got['yp'].permute(0, 3, 1, 2) - p).abs().max().item() < 1e-12 * v.abs().max().item()
    # the denominator: the same expression on absolute values -- it bounds the result, and equals it where no term
    # is negative (no activation, no mask)
    assert bool((got['y'].abs() <= got['den'] * (1 + 1e-12) * (R.SQRT2 if c['act'] == 3 else 1)).all())
    pos = {k: (v_.abs() if torch.is_tensor(v_) else abs(v_) if k == 'noise_w' else v_) for k, v_ in i.items()}
    kw = dict(R.pw_kwargs(c, pos, D), act=R.ACT_NONE, mask=None)
    assert (R.conv1x1(pos['x'], pos['w'], **kw)['y'] - got['den']).abs().max().item() < 1e-12 * got['den'].max().item()


@pytest.mark.parametrize('v', range(len(R.ARB_VARIANTS)))
def test_conv1x1_arb_is_autograd_through_the_forward(v):
    """dx, ds, dt of conv1x1_arb == autograd in fp64 through relu(x s + t) -> up2 -> the forward 1x1 conv, with the
    shortcut's gradient added; inputs kept away from the decision x s + t = 0"""
    c = R._arbc('A', (4, 6), 2, 16, 32, **R.ARB_VARIANTS[v])
    i = {k: t.to(D) for k, t in R.arb_inputs(_g(70 + v), c).items()}
    pre = i['ax'] * i['as'][:, None, None] + i['at'][:, None, None]
    i['ax'] = torch.where(pre.abs() < 1e-3 * i['at'].abs()[:, None, None], i['ax'] + 1.0, i['ax'])
    kw = dict(pool_sum=c['pool_sum'], nomask=c['nomask'], skip=i.get('skip'), skip_C=16 if c['skip'] else 0,
              skip_ups=c['skip'] == 'ups')
    got = R.conv1x1_arb(i['x'], i['w'], i['ax'], i['as'], i['at'], **kw)

    def fwd(x, s, t):                                   # the consumer: dy's conv maps its [.., Cout] to [.., Cin]
        a = x * s[:, None, None] + t[:, None, None]
        a = a if c['nomask'] else torch.relu(a)
        a = R.up2(a) if c['pool_sum'] else a
        return a @ i['w']
    dx, ds, dt = R.vjp(fwd, [i['ax'], i['as'], i['at']], i['x'])
    if c['skip']:
        sk = i['skip'][..., :16]
        dx[..., :16] += sk.reshape(2, dx.shape[1], 2, dx.shape[2], 2, 16).sum(dim=(2, 4)) if c['skip'] == 'ups' else sk
    for name, want in (('dx', dx), ('ds', ds), ('dt', dt)):
        assert (got[name] - want).abs().max().item() < 1e-12 * want.abs().max().item(), name
    assert bool((got['dx'].abs() <= got['den_dx'] * (1 + 1e-12)).all())


def test_splits_and_scales():
    g = _g(90)
    x = torch.randn(4096, generator=g) * 2.0 ** torch.randint(-30, 30, (4096,), generator=g).float()
    h, m, l = R.split3(x)
    assert bool(((h.double() + m.double() + l.double() - x.double()).abs() <= 2.0 ** -24 * x.double().abs()).all())
    for p in (h, m, l):
        assert torch.equal(p.bfloat16().float(), p)
    # fp16 x 2 on a scaled operand (maximum in [2^12, 2^13)): 2^-22 relative from 2^-3 upwards, 2^-25 absolute below
    v = torch.cat([torch.randn(4096, generator=g) * 2.0 ** torch.randint(-3, 13, (4096,), generator=g).float(),
                   torch.randn(4096, generator=g) * 2.0 ** torch.randint(-30, -3, (4096,), generator=g).float()])
    v = v[v.abs() < 2.0 ** 13]
    h, m = R.split2(v)
    err = (h.double() + m.double() - v.double()).abs()
    big = v.abs() >= 2.0 ** -3
    assert bool(big.any()) and bool((~big).any())
    assert bool((err[big] <= 2.0 ** -22 * v.double().abs()[big]).all()) and bool((err[~big] <= 2.0 ** -25).all())
    # h2_scales: a maximum with exponent 40 .. 254 lands in [2^12, 2^13); the two factors are inverse powers of two
    E = torch.arange(40, 255, dtype=torch.int32)
    for mant in (0, 1, 0x7fffff):
        mx = ((E << 23) | mant).view(torch.float32)
        sc, inv = R.h2_scales(mx)
        assert bool(((mx * sc >= 2.0 ** 12) & (mx * sc < 2.0 ** 13)).all()) and bool((sc * inv == 1.0).all())
    sc, _ = R.h2_scales(torch.tensor([0.0, 1e-30, float(2.0 ** 127) * 1.5]))        # clamped below and above
    assert sc.tolist() == [2.0 ** 99, 2.0 ** 99, 2.0 ** -115]


@pytest.mark.parametrize('N,K,N_pad,K_pad', [(40, 24, 64, 32), (64, 48, 64, 48), (96, 160, 96, 160)])
def test_host_packers_round_trip(N, K, N_pad, K_pad):
    """every element read back through the header's index formulas, one at a time: the fp32 layout gives the weight,
    the three bf16 pieces add up to it, the two fp16 pieces to the scaled weight; the padding is +0"""
    w = torch.randn(N, K, generator=_g(91)) / 7
    words = R.pack_pw(w, N_pad, K_pad)
    tot = N_pad * K_pad
    assert words.numel() == tot + tot * 3 // 2 + tot + 4
    f32 = words[:tot].view(torch.float32)
    bf = words[tot:tot + tot * 3 // 2].view(torch.int16).view(torch.bfloat16).float()
    h2 = words[tot + tot * 3 // 2:-4].view(torch.int16).view(torch.float16).float()
    tail = words[-4:]
    assert tail[1:].tolist() == [0, 0, 0] and tail[:1].view(torch.float32).item() == w.abs().max().item()
    scale = float(R.h2_scales(w.abs().max().reshape(1))[0])
    kc = 32 if K_pad % 32 == 0 else 16
    h3, m3, l3 = R.split3(w)
    for n in range(0, N_pad, 3):
        for k in range(0, K_pad, 5):
            want = float(w[n, k]) if n < N and k < K else 0.0
            assert float(f32[((k // kc) * N_pad + n) * kc + k % kc]) == want
            r, hi, lo = n % 32, (k % 16) // 8, k % 8
            row = ((k // 16) * (N_pad // 32) + n // 32) * 32 + r
            pieces = [float(bf[row * 48 + (((2 * p + hi) ^ ((r >> 3) & 1)) * 8) + lo]) for p in range(3)]
            if n < N and k < K:
                assert pieces == [float(h3[n, k]), float(m3[n, k]), float(l3[n, k])]
            else:
                assert pieces == [0.0, 0.0, 0.0]
            hm = [float(h2[row * 32 + (((2 * p + hi) ^ ((r >> 2) & 3)) * 8) + lo]) for p in range(2)]
            assert abs(hm[0] + hm[1] - want * scale) <= 2.0 ** -22 * abs(want * scale) + 2.0 ** -25
    if N < N_pad or K < K_pad:                                                    # +0, not -0: no bit set at all
        pad = torch.ones(N_pad, K_pad, dtype=torch.bool)
        pad[:N, :K] = False
        assert int(R.pack_f32(w, N_pad, K_pad).view(torch.int32)[R.pack_f32(pad.float(), N_pad, K_pad) > 0].abs().sum()) == 0
    zero = R.pack_pw(torch.zeros(N, K), N_pad, K_pad)                              # an all-zero weight: no bit set
    assert int(zero.abs().sum()) == 0


def _draws(fn):
    import _pin
    try:
        for sd in range(_pin.SEEDS):
            _pin._DRAW['seed'] = sd
            fn(_pin._gen)
    finally:
        _pin._DRAW['seed'] = 0


def _fig(got, ref, den):
    ok = den > 0
    return float(((got.double() - ref).abs()[ok] / den[ok]).max()) / R.U if bool(ok.any()) else 0.0


@pytest.mark.parametrize('case', R.PW_FWD_CASES, ids=R.pw_id)
def test_forward_restatements_stay_under_a_quarter_of_k(case):
    """for every case's generator and shape the fp32 restatement of its route -- and of route A on the same inputs --
    is within k / 4 of the fp64 reference: the 4 x restatement bar a kernel meets is attainable.  A condition on the
    inputs, not a measurement of a kernel."""
    def body(gen):
        i = R.pw_inputs(gen('pw', R.pw_id(case)), case)
        for route in sorted(set([case['route'], 'A'])):
            r64, r32 = R.pw_refs(case, i, route)
            for out, den, pooled in (('y', 'den', False), ('yp', 'denp', True)):
                if r64[out] is not None:
                    f = _fig(r32[out], r64[out], r64[den])
                    assert f <= R.pw_k(case, route, pooled) / 4.0, (route, out, f, R.pw_k(case, route, pooled))
    _draws(body)


@pytest.mark.parametrize('case', R.PW_ARB_CASES, ids=R.arb_id)
def test_dgrad_restatements_stay_under_a_quarter_of_k(case):
    """dx on the signed inputs, ds and dt on the positive ones (arb_positive); on the signed ones the restatement's ds
    and dt are inside the a-priori bound"""
    def body(gen):
        i = R.arb_inputs(gen('arb', R.arb_id(case)), case)
        kdx, kds, kdt = R.arb_k(case)
        r64, r32 = R.arb_refs(case, i)
        f = _fig(r32['dx'], r64['dx'], r64['den_dx'])
        assert f <= kdx / 4.0, ('dx', f, kdx)
        for name, bound in zip(('ds', 'dt'), R.arb_bound(case, r64, i['ax'])):
            assert bool(((r32[name].double() - r64[name]).abs() <= bound * R.U).all()), name
        p64, p32 = R.arb_refs(case, R.arb_positive(i))
        for name, k in (('ds', kds), ('dt', kdt)):
            f = _fig(p32[name], p64[name], p64['den_' + name])
            assert f <= k / 4.0, (name, f, k)
    _draws(body)


# ---- Winograd 3x3 convs: the references, restatements and cases of tests/test_wino_kernels_gpu.py -------------------
@pytest.mark.parametrize('pro,pro_b', [(0, 1), (1, 1), (2, 0)])
@pytest.mark.parametrize('epi', range(len(R.EPI)))
def test_conv3x3_is_conv2d_with_the_epilogue(epi, pro, pro_b):
    """conv3x3 in fp64 == F.conv2d(padding=1) on the prologue's result + the epilogue written out once more; den_d is
    the same expression on absolute values; den_w is the transform-domain sum written with the matrices B^T, G, A^T
    on unfolded patches, and bounds the result"""
    c = R._wc('W8', (4, 6), 3, 16, 32, **dict(R.EPI[epi], pro=pro, pro_b=pro_b, n_store=24))
    i = {k: (v.to(D) if torch.is_tensor(v) else v) for k, v in R.wino_inputs(_g(150 + epi), c).items()}
    got = R.conv3x3(i['x'], i['w'], **R.pw_kwargs(c, i, D))
    a = i['x'].permute(0, 3, 1, 2)
    if pro:
        a = a * i['s'].expand(3, -1)[:, :, None, None] + i['t'].expand(3, -1)[:, :, None, None]
        a = F.relu(a) if pro == R.PRO_AFFINE_RELU else a
    v = c['alpha'] * F.conv2d(a, i['w'], padding=1)
    if c['oscale']:
        v = v * i['oscale'][:, :, None, None]
    if c['noise']:
        v = v + i['noise_w'] * i['noise'][:, None]
    if c['bias']:
        v = v + i['bias'][None, :, None, None]
    if c['res']:
        r = i['res'].permute(0, 3, 1, 2)
        v = v + (F.interpolate(r, scale_factor=2, mode='nearest') if c['res'] == 'ups' else r)
    v = {0: lambda u: u, 1: F.relu, 2: torch.tanh, 3: lambda u: F.leaky_relu(u, 0.2) * R.SQRT2}[c['act']](v)
    if c['mask']:
        v = v * (i['mask'].permute(0, 3, 1, 2) > 0)
    v = v[:, :24]
    assert (got['y'].permute(0, 3, 1, 2) - v).abs().max().item() < 1e-12 * v.abs().max().item()
    if c['pool']:
        p = F.max_pool2d(v, 2) if c['pool'] == R.POOL_MAX else F.avg_pool2d(v, 2) * 4
        assert (got['yp'].permute(0, 3, 1, 2) - p).abs().max().item() < 1e-12 * v.abs().max().item()
    lr = R.SQRT2 if c['act'] == 3 else 1
    for den in ('den', 'den_d'):
        assert bool((got['y'].abs() <= got[den] * (1 + 1e-12) * lr).all()), den
    pos = {k: (v_.abs() if torch.is_tensor(v_) else abs(v_) if k == 'noise_w' else v_) for k, v_ in i.items()}
    kw = dict(R.pw_kwargs(c, pos, D), act=R.ACT_NONE, mask=None)
    assert (R.conv3x3(pos['x'], pos['w'], **kw)['y'] - got['den_d']).abs().max().item() < 1e-12 * got['den_d'].max().item()
    # den_w of the bare conv, patch by patch with the matrices
    BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=D).abs()
    AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=D).abs()
    aabs = F.pad(got['aabs'].permute(0, 3, 1, 2), (1, 1, 1, 1))
    d = aabs.unfold(2, 4, 2).unfold(3, 4, 2)                                          # [B, K, Hq, Wq, 4, 4]
    Vm = torch.einsum('ip,bkyxpq,jq->bkyxij', BT, d, BT)
    Um = torch.einsum('ia,nkab,jb->nkij', R.WINO_G, i['w'], R.WINO_G).abs()
    Ym = torch.einsum('ui,bnyxij,vj->byuxvn', AT, torch.einsum('bkyxij,nkij->bnyxij', Vm, Um), AT).reshape(3, 4, 6, 32)
    assert (R.wino_den(got['aabs'], i['w']) - Ym).abs().max().item() < 1e-12 * Ym.max().item()


@pytest.mark.parametrize('v', range(len(R.ARB_VARIANTS)))
def test_conv3x3_arb_is_autograd_through_the_forward(v):
    """dx, ds, dt of conv3x3_arb == autograd in fp64 through relu(x s + t) -> up2 -> the 3x3 conv whose input gradient
    the launch computes (the launch applies the transposed, mirrored kernel), shortcut added"""
    c = R._wac('W8', (4, 6), 2, 16, 32, **R.ARB_VARIANTS[v])
    i = {k: t.to(D) for k, t in R.wino_arb_inputs(_g(170 + v), c).items()}
    pre = i['ax'] * i['as'][:, None, None] + i['at'][:, None, None]
    i['ax'] = torch.where(pre.abs() < 1e-3 * i['at'].abs()[:, None, None], i['ax'] + 1.0, i['ax'])
    kw = dict(pool_sum=c['pool_sum'], nomask=c['nomask'], skip=i.get('skip'), skip_C=16 if c['skip'] else 0,
              skip_ups=c['skip'] == 'ups')
    got = R.conv3x3_arb(i['x'], i['w'], i['ax'], i['as'], i['at'], **kw)
    wf = i['w'].permute(1, 0, 2, 3).flip(2, 3)            # the forward conv [Cin, Cout, 3, 3] of this input gradient

    def fwd(x, s, t):
        a = x * s[:, None, None] + t[:, None, None]
        a = a if c['nomask'] else torch.relu(a)
        a = R.up2(a) if c['pool_sum'] else a
        return F.conv2d(a.permute(0, 3, 1, 2), wf, padding=1).permute(0, 2, 3, 1)
    dx, ds, dt = R.vjp(fwd, [i['ax'], i['as'], i['at']], i['x'])
    if c['skip']:
        sk = i['skip'][..., :16]
        dx[..., :16] += sk.reshape(2, dx.shape[1], 2, dx.shape[2], 2, 16).sum(dim=(2, 4)) if c['skip'] == 'ups' else sk
    for name, want in (('dx', dx), ('ds', ds), ('dt', dt)):
        assert (got[name] - want).abs().max().item() < 1e-12 * want.abs().max().item(), name
    assert bool((got['dx'].abs() <= got['den_dx'] * (1 + 1e-12)).all())
    assert bool((got['dx'].abs() <= got['den_dx_d'] * (1 + 1e-12)).all())


@pytest.mark.parametrize('case', R.WINO_FWD_CASES, ids=R.wino_id)
def test_winograd_forward_restatements_stay_under_a_quarter_of_k(case):
    """for every case's generator and shape the fp32 restatement of its route is within k / 4 of the fp64 reference on
    den_w: k and the fp16 x 2 floor were not set from the kernels.  Under PRO_AFFINE padding in FRONT of the prologue
    would be more than 100 bars off at the border"""
    def body(gen):
        i = R.wino_inputs(gen('wino', R.wino_id(case)), case)
        r64, r32 = R.wino_refs(case, i)
        for out, den, pooled in (('y', 'den', False), ('yp', 'denp', True)):
            if r64[out] is not None:
                f = _fig(r32[out], r64[out], r64[den])
                assert f <= R.wino_k(case, None, pooled) / 4.0, (out, f, R.wino_k(case, None, pooled))
        if case['pro'] == R.PRO_AFFINE and case['act'] == R.ACT_NONE and not case['mask']:
            kw = R.pw_kwargs(case, i, D)
            a, _ = R.pw_prologue(i['x'].double(), case['pro'], i['s'].double(), i['t'].double())
            t_ = i['t'].double().expand(case['B'], -1)[:, None, None, :]
            ap = F.pad(a - t_, (0, 0, 1, 1, 1, 1)) + t_                   # x s padded, t added after: the halo holds t
            wrong = F.conv2d(ap.permute(0, 3, 1, 2), i['w'].double()).permute(0, 2, 3, 1) * case['alpha']
            wrong = R.conv_epilogue(wrong, r64['den'], **{k: v for k, v in kw.items() if k not in ('pro', 's', 't', 'alpha')})
            for out, den, pooled in (('y', 'den', False), ('yp', 'denp', True)):
                if r64[out] is None:
                    continue
                err = (wrong[out] - r64[out]).abs() / r64[den] / R.U
                border = torch.ones(err.shape[1:3], dtype=torch.bool)
                border[1:-1, 1:-1] = False
                xmax = i['x'].abs().amax(dim=(1, 2, 3))
                b0 = int(torch.where(xmax > 0, xmax, xmax.max()).argmin())    # (a shared t is scaled to this image)
                live = r64[den][b0][border] > 0
                bar = min(R.wino_k(case, None, pooled), 4.0 * _fig(r32[out], r64[out], r64[den]))
                assert float(err[b0][border][live].median()) > 100 * bar, (out, bar)
                assert float(err[:, ~border].max()) < 1e-3
    _draws(body)


@pytest.mark.parametrize('case', R.WINO_ARB_CASES, ids=R.wino_arb_id)
def test_winograd_dgrad_restatements_stay_under_a_quarter_of_k(case):
    def body(gen):
        i = R.wino_arb_inputs(gen('warb', R.wino_arb_id(case)), case)
        kdx, kds, kdt = R.arb_k(case, R.wino_k)
        r64, r32 = R.wino_arb_refs(case, i)
        f = _fig(r32['dx'], r64['dx'], r64['den_dx'])
        assert f <= kdx / 4.0, ('dx', f, kdx)
        for name, bound in zip(('ds', 'dt'), R.arb_bound(case, r64, i['ax'], R.wino_k)):
            assert bool(((r32[name].double() - r64[name]).abs() <= bound * R.U).all()), name
        p64, p32 = R.wino_arb_refs(case, R.arb_positive(i))
        for name, k in (('ds', kds), ('dt', kdt)):
            f = _fig(p32[name], p64[name], p64['den_' + name])
            assert f <= k / 4.0, (name, f, k)
    _draws(body)


@pytest.mark.parametrize('tap', range(9))
def test_winograd_one_hot_inputs_are_exact_in_every_restatement(tap):
    """single power-of-two pixels and weights go through G g G^T, B^T d B, the bf16 x 3 / fp16 x 2 pieces and A^T M A
    without a rounding: all three restatements give the fp64 result bit for bit, and it is not all zero"""
    for route, shape, kw in (('W8', '16x32', {}), ('H', '16x32', {}), ('HS', 'hs2', dict(splitk=2))):
        c = R._wsh(route, shape, **kw)
        for seed in range(3):
            i = R.wino_onehot(c, tap, seed)
            r64, r32 = R.wino_refs(c, i)
            assert torch.equal(r32['y'].double(), r64['y']), (route, seed)
            assert int((r64['y'] != 0).sum()) >= 3, (route, seed)


def test_winograd_headroom_of_the_fp16_scales():
    """an image maximum nextafter(2^e, 0) in the +, -, -, + pattern that drives B^T d B to 4 max: times the image's
    power of two the transformed value stays below 2^15, finite in fp16, and the two pieces hold it to 2^-22; U = G g
    G^T stays below 2.25 max |w|"""
    m = torch.tensor(2.0 ** 5).nextafter(torch.tensor(0.0))
    x = torch.zeros(1, 8, 16, 16)
    x[0, 1, 1, 3], x[0, 1, 3, 3], x[0, 3, 1, 3], x[0, 3, 3, 3] = m, -m, -m, m
    xs, _ = R.h2_scales(x.abs().amax(dim=(1, 2, 3)))
    V = R.wino_V(x * xs.view(-1, 1, 1, 1))
    assert float(V.abs().max()) == float(4 * m * xs[0]) < 2.0 ** 15
    h, l = R.split2(V)
    assert bool(torch.isfinite(h).all()) and bool(((h.double() + l.double() - V.double()).abs() <= 2.0 ** -22 * V.abs().double()).all())
    w = torch.full((64, 16, 3, 3), 0.7)
    assert float(R.wino_U(w).abs().max()) <= 2.25 * 0.7 * (1 + 1e-12)


def test_winograd_case_tables():
    """every EPI term on every route; both H blocks and all three sources of its maxima; the HS slice counts"""
    for route in ('W8', 'W16', 'H', 'HS'):
        cs = [c for c in R.WINO_FWD_CASES if c['route'] == route]
        for e in R.EPI:
            assert any(all(c[k] == v for k, v in e.items()) for c in cs), (route, e)
        assert any(c['n_store'] < c['Cout'] for c in cs) and any(c['pro'] and not c['pro_b'] for c in cs)
    hs = [c for c in R.WINO_FWD_CASES if c['route'] == 'H']
    assert set((c['blk'], c['amax']) for c in hs) >= set([(8, None), (16, 'true'), (8, 'raw'), (16, 'applied')])
    assert len(set(R.wino_id(c) for c in R.WINO_FWD_CASES)) == len(R.WINO_FWD_CASES)
    assert len(set(R.wino_arb_id(c) for c in R.WINO_ARB_CASES)) == len(R.WINO_ARB_CASES)


# ---- direct 3x3 convs: the references, restatements and cases of tests/test_direct_kernels_gpu.py -------------------
@pytest.mark.parametrize('pro,pro_b', [(0, 1), (1, 1), (2, 0)])
@pytest.mark.parametrize('epi', range(len(R.EPI)))
def test_conv3x3_ups_is_nearest_interpolate_plus_conv2d(epi, pro, pro_b):
    """ups = 1 in fp64: the prologue on the low-resolution x, F.interpolate(mode='nearest'), F.conv2d(padding=1), the
    epilogue written out once more (res_ups and the pool on the output grid); den_d is the same expression on
    absolute values"""
    c = R._dc('F', (8, 12), 3, 16, 32, **dict(R.EPI[epi], pro=pro, pro_b=pro_b, n_store=24, ups=1))
    i = {k: (v.to(D) if torch.is_tensor(v) else v) for k, v in R.direct_inputs(_g(190 + epi), c).items()}
    assert i['x'].shape == (3, 4, 6, 16)
    got = R.conv3x3(i['x'], i['w'], ups=True, den_w=False, **R.pw_kwargs(c, i, D))
    a = i['x'].permute(0, 3, 1, 2)
    if pro:
        a = a * i['s'].expand(3, -1)[:, :, None, None] + i['t'].expand(3, -1)[:, :, None, None]
        a = F.relu(a) if pro == R.PRO_AFFINE_RELU else a
    v = c['alpha'] * F.conv2d(F.interpolate(a, scale_factor=2, mode='nearest'), i['w'], padding=1)
    if c['oscale']:
        v = v * i['oscale'][:, :, None, None]
    if c['noise']:
        v = v + i['noise_w'] * i['noise'][:, None]
    if c['bias']:
        v = v + i['bias'][None, :, None, None]
    if c['res']:
        r = i['res'].permute(0, 3, 1, 2)
        v = v + (F.interpolate(r, scale_factor=2, mode='nearest') if c['res'] == 'ups' else r)
    v = {0: lambda u: u, 1: F.relu, 2: torch.tanh, 3: lambda u: F.leaky_relu(u, 0.2) * R.SQRT2}[c['act']](v)
    if c['mask']:
        v = v * (i['mask'].permute(0, 3, 1, 2) > 0)
    v = v[:, :24]
    assert got['y'].shape == (3, 8, 12, 24)
    assert (got['y'].permute(0, 3, 1, 2) - v).abs().max().item() < 1e-12 * v.abs().max().item()
    if c['pool']:
        p = F.max_pool2d(v, 2) if c['pool'] == R.POOL_MAX else F.avg_pool2d(v, 2) * 4
        assert (got['yp'].permute(0, 3, 1, 2) - p).abs().max().item() < 1e-12 * v.abs().max().item()
    lr = R.SQRT2 if c['act'] == 3 else 1
    assert torch.equal(got['den'], got['den_d'])
    assert bool((got['y'].abs() <= got['den_d'] * (1 + 1e-12) * lr).all())
    pos = {k: (v_.abs() if torch.is_tensor(v_) else abs(v_) if k == 'noise_w' else v_) for k, v_ in i.items()}
    kw = dict(R.pw_kwargs(c, pos, D), act=R.ACT_NONE, mask=None)
    den = R.conv3x3(pos['x'], pos['w'], ups=True, den_w=False, **kw)['y']
    assert (den - got['den_d']).abs().max().item() < 1e-12 * got['den_d'].max().item()


@pytest.mark.parametrize('v', range(len(R.ARB_VARIANTS)))
def test_conv3x3_arb_ups_is_autograd_through_the_forward(v):
    """ups = 1 on the fused input gradient: da = conv3x3(up2(dy)) is the gradient of relu(x s + t) -> [up2 ->] the 3x3
    conv -> 2x2 sum pool w.r.t. the conv's input; dx, ds, dt == autograd in fp64"""
    c = R._dac('F', (4, 6), 2, 16, 32, **R.ARB_VARIANTS[v])
    i = {k: t.to(D) for k, t in R.direct_arb_inputs(_g(210 + v), c).items()}
    pre = i['ax'] * i['as'][:, None, None] + i['at'][:, None, None]
    i['ax'] = torch.where(pre.abs() < 1e-3 * i['at'].abs()[:, None, None], i['ax'] + 1.0, i['ax'])
    dy = i['x'][:, ::2, ::2].contiguous()                 # the low-resolution gradient the launch reads
    kw = dict(pool_sum=c['pool_sum'], nomask=c['nomask'], skip=i.get('skip'), skip_C=16 if c['skip'] else 0,
              skip_ups=c['skip'] == 'ups')
    got = R.conv3x3_arb(dy, i['w'], i['ax'], i['as'], i['at'], ups=True, den_w=False, **kw)
    wf = i['w'].permute(1, 0, 2, 3).flip(2, 3)

    def fwd(x, s, t):
        a = x * s[:, None, None] + t[:, None, None]
        a = a if c['nomask'] else torch.relu(a)
        a = R.up2(a) if c['pool_sum'] else a
        return R.quad_sum(F.conv2d(a.permute(0, 3, 1, 2), wf, padding=1).permute(0, 2, 3, 1))
    dx, ds, dt = R.vjp(fwd, [i['ax'], i['as'], i['at']], dy)
    if c['skip']:
        sk = i['skip'][..., :16]
        dx[..., :16] += sk.reshape(2, dx.shape[1], 2, dx.shape[2], 2, 16).sum(dim=(2, 4)) if c['skip'] == 'ups' else sk
    for name, want in (('dx', dx), ('ds', ds), ('dt', dt)):
        assert (got[name] - want).abs().max().item() < 1e-12 * want.abs().max().item(), name
    assert bool((got['dx'].abs() <= got['den_dx'] * (1 + 1e-12)).all())
    assert torch.equal(got['den_dx'], got['den_dx_d'])


def test_direct_im2col_order_and_the_generalised_accumulators():
    """direct_cols / direct_wmat: column ((chunk * 9 + tap) * 16 + channel) holds pixel (y + dy - 1, x + dx - 1) of
    channel 16 chunk + channel and w[n, k, dy, dx]; their fp64 product is F.conv2d(padding=1); a chunk is 144
    columns, so splitk_slices on them are the launch's slices of whole 16-channel chunks; with the default chunk
    sizes acc_fp32 / acc_bf3 / acc_h2 are what they were for the 1x1 routes"""
    g = _g(230)
    a, w = torch.randn(2, 6, 4, 48, generator=g, dtype=D), torch.randn(32, 48, 3, 3, generator=g, dtype=D)
    cols, wm = R.direct_cols(a), R.direct_wmat(w)
    want = F.conv2d(a.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    assert (cols @ wm.t() - want).abs().max().item() < 1e-12
    for chunk, tap, ch, y, x in ((0, 0, 0, 0, 0), (1, 5, 3, 2, 1), (2, 8, 15, 5, 3), (2, 2, 7, 0, 3), (1, 6, 9, 5, 0)):
        col, dy, dx = (chunk * 9 + tap) * 16 + ch, tap // 3, tap % 3
        assert torch.equal(wm[:, col], w[:, 16 * chunk + ch, dy, dx])
        yy, xx = y + dy - 1, x + dx - 1
        inside = 0 <= yy < 6 and 0 <= xx < 4
        assert torch.equal(cols[:, y, x, col], a[:, yy, xx, 16 * chunk + ch] if inside else torch.zeros(2, dtype=D))
    assert R.splitk_slices(9 * 128, 144, 3) == [(0, 432), (432, 864), (864, 1152)]          # 8 chunks: 3 + 3 + 2
    assert R.splitk_slices(9 * 256, 144, 8) == [(z * 288, (z + 1) * 288) for z in range(8)]
    a32, w32 = torch.randn(2, 4, 4, 96, generator=g), torch.randn(64, 96, generator=g)
    assert torch.equal(R.acc_fp32(a32, w32, 2), R.acc_fp32(a32, w32, 2, 32))
    assert torch.equal(R.acc_bf3(a32, w32), R.acc_bf3(a32, w32, 1, 96))
    amax, wmax = a32.abs().amax(dim=(1, 2, 3)), w32.abs().max()
    assert torch.equal(R.acc_h2(a32, w32, amax, wmax, 3), R.acc_h2(a32, w32, amax, wmax, 3, 32))
    assert R.direct_tile(4, 4) == (4, 4, 8) and R.direct_tile(8, 8) == (8, 8, 2) and R.direct_tile(32, 4) == (4, 32, 1)
    assert R.direct_tile(6, 6) == (8, 8, 2) and R.direct_tile(12, 20) == (16, 8, 1) and R.direct_tile(64, 64) == (16, 8, 1)


@pytest.mark.parametrize('case', R.DIRECT_FWD_CASES, ids=R.direct_id)
def test_direct_forward_restatements_stay_under_a_quarter_of_k(case):
    """for every case's generator and shape the fp32 restatement of its route is within k / 4 of the fp64 reference on
    den_d (H, R: plus direct_h2_floor): k and the floor were not set from the kernels.  Under PRO_AFFINE zero padding
    applied in FRONT of the prologue would be more than 100 bars off at the border, so the cases see that mistake"""
    def body(gen):
        i = R.direct_inputs(gen('direct', R.direct_id(case)), case)
        r64, r32 = R.direct_refs(case, i)
        for out, den, pooled in (('y', 'den', False), ('yp', 'denp', True)):
            if r64[out] is not None:
                f = _fig(r32[out], r64[out], r64[den])
                assert f <= R.direct_k(case, None, pooled) / 4.0, (out, f, R.direct_k(case, None, pooled))
        if case['pro'] == R.PRO_AFFINE and case['act'] == R.ACT_NONE and not case['mask']:
            kw = R.pw_kwargs(case, i, D)
            a, _ = R.pw_prologue(i['x'].double(), case['pro'], i['s'].double(), i['t'].double())
            t_ = i['t'].double().expand(case['B'], -1)[:, None, None, :]
            xs = R.up2(a - t_) if case['ups'] else a - t_
            ap = F.pad(xs, (0, 0, 1, 1, 1, 1)) + t_                       # x s padded, t added after: the halo holds t
            wrong = F.conv2d(ap.permute(0, 3, 1, 2), i['w'].double()).permute(0, 2, 3, 1) * case['alpha']
            wrong = R.conv_epilogue(wrong, r64['den'], **{k: v for k, v in kw.items() if k not in ('pro', 's', 't', 'alpha')})
            for out, den, pooled in (('y', 'den', False), ('yp', 'denp', True)):
                if r64[out] is None:
                    continue
                err = (wrong[out] - r64[out]).abs() / r64[den] / R.U
                border = torch.ones(err.shape[1:3], dtype=torch.bool)
                border[1:-1, 1:-1] = False
                xmax = i['x'].abs().amax(dim=(1, 2, 3))
                b0 = int(torch.where(xmax > 0, xmax, xmax.max()).argmin())    # (a shared t is scaled to this image)
                live = r64[den][b0][border] > 0
                bar = min(R.direct_k(case, None, pooled), 4.0 * _fig(r32[out], r64[out], r64[den]))
                assert float(err[b0][border][live].median()) > 100 * bar, (out, bar)
                assert float(err[:, ~border].max()) < 1e-3
    _draws(body)


@pytest.mark.parametrize('case', R.DIRECT_ARB_CASES, ids=R.direct_arb_id)
def test_direct_dgrad_restatements_stay_under_a_quarter_of_k(case):
    def body(gen):
        i = R.direct_arb_inputs(gen('darb', R.direct_arb_id(case)), case)
        kdx, kds, kdt = R.arb_k(case, R.direct_k)
        r64, r32 = R.direct_arb_refs(case, i)
        f = _fig(r32['dx'], r64['dx'], r64['den_dx'])
        assert f <= kdx / 4.0, ('dx', f, kdx)
        for name, bound in zip(('ds', 'dt'), R.arb_bound(case, r64, i['ax'], R.direct_k)):
            assert bool(((r32[name].double() - r64[name]).abs() <= bound * R.U).all()), name
        p64, p32 = R.direct_arb_refs(case, R.arb_positive(i))
        for name, k in (('ds', kds), ('dt', kdt)):
            f = _fig(p32[name], p64[name], p64['den_' + name])
            assert f <= k / 4.0, (name, f, k)
    _draws(body)


@pytest.mark.parametrize('tap', range(9))
def test_direct_one_hot_inputs_are_exact_in_every_restatement(tap):
    """single power-of-two pixels and weights go through the fp32 chain, the bf16 x 3 and the fp16 x 2 pieces and the
    slices without a rounding: all three restatements give the fp64 result bit for bit, and it is not all zero"""
    for c in (R._dsh('F', '12x20'), R._dsh('B', '6x6'), R._dsh('H', '8x8'), R._dsh('R', '16x32'),
              R._dsh('F', '16x16', ups=1), R._dsh('B', '8x8', ups=1, wfmt='bf3w'), R._dsh('H', 'k3', splitk=3),
              R._dsh('B', 'k4s', splitk=4), R._dsh('F', 'k8', splitk=8)):
        for seed in range(3):
            i = R.direct_onehot(c, tap, seed)
            r64, r32 = R.direct_refs(c, i)
            assert torch.equal(r32['y'].double(), r64['y']), (R.direct_id(c), seed)
            assert int((r64['y'] != 0).sum()) >= 3, (R.direct_id(c), seed)


def test_direct_case_tables():
    """every EPI term, n_store < Cout, both prologues and the shared one on every route; ups = 1 on F and B unsplit
    and sliced; H and R with all three sources of their maxima; the K slices on F, B and H through both finish
    kernels; every shape the tile, channel-tile and slice rules distinguish; the images of a launch 3e10 apart"""
    for route in 'FBHR':
        cs = [c for c in R.DIRECT_FWD_CASES if c['route'] == route]
        for e in R.EPI:
            assert any(all(c[k] == v for k, v in e.items()) for c in cs), (route, e)
        assert any(c['n_store'] < c['Cout'] for c in cs) and any(c['pro'] and not c['pro_b'] for c in cs)
        assert set(c['pro'] for c in cs) == set([0, 1, 2])
        if route in 'FB':
            assert any(c['ups'] and c['splitk'] == 1 for c in cs) and any(c['ups'] and c['splitk'] > 1 for c in cs)
        if route in 'HR':
            assert set(c['amax'] for c in cs) == set([None, 'true', 'raw', 'applied'])
            assert not any(c['ups'] for c in cs)
        if route != 'R':
            assert set(len(R.splitk_slices(9 * c['Cin'], 144, c['splitk'])) for c in cs) >= set([1, 3, 4, 8])
            assert any(c['finish'] == 'scalar' for c in cs)
            assert set(R.direct_tile(c['H'], c['W']) for c in cs) >= set([(4, 4, 8), (8, 8, 2), (4, 32, 1), (16, 8, 1)])
            assert any(c['H'] % R.direct_tile(c['H'], c['W'])[1] and R.direct_tile(c['H'], c['W'])[2] > 1 for c in cs)
            assert any(c['Cout'] == 96 for c in cs) and any(c['B'] * c['H'] * c['W'] // 128 * (c['Cout'] // 64) >= 320 for c in cs)
    b = [c for c in R.DIRECT_FWD_CASES if c['route'] == 'B']
    assert set(R.direct_form(c)[0] for c in b) == set([R.WFMT_BF16X3, R.WFMT_BF16X3W])
    assert len(set(R.direct_id(c) for c in R.DIRECT_FWD_CASES)) == len(R.DIRECT_FWD_CASES)
    assert len(set(R.direct_arb_id(c) for c in R.DIRECT_ARB_CASES)) == len(R.DIRECT_ARB_CASES)
    i = R.direct_inputs(_g(240), R._dsh('F', '8x8', **R.EPI[0]))
    m = i['x'].abs().amax(dim=(1, 2, 3))
    assert float(m[2] / m[0]) > 1e13 and float(i['res'][2].abs().max() / i['res'][0].abs().max()) > 1e9


# ---- sub-pixel 3x3 convs (tests/test_subpix_kernels_gpu.py) --------------------------------------------------------
def _sp_operands(g, ups, ext, B=2, H=8, W=12, Ci=16, Co=32):
    """fp64 operands of one mode: the forward's OIHW weight and the launch's input (ups = 3: the gradient frame)"""
    wf = torch.randn(Co, Ci, 3, 3, generator=g, dtype=D) if ups == 2 else torch.randn(Ci, Co, 3, 3, generator=g, dtype=D)
    if ups == 2:
        return torch.randn(B, H // 2, W // 2, Ci, generator=g, dtype=D), wf
    a = torch.randn(B, H + 2 * ext, W + 2 * ext, Ci, generator=g, dtype=D)
    if ext:
        a[:, -1], a[:, :, -1] = 0.0, 0.0
    return a, wf


def test_subpix_references_agree_with_independent_formulations():
    """ups = 2, ext = 0 == F.interpolate(nearest) + F.conv2d; ext = 1 == F.conv_transpose2d(stride 2) in rows / columns
    0 .. H of the frame, row / column H + 1 +0; ups = 3 == autograd through those, the frame's last row ignored"""
    g = _g(300)
    nchw, nhwc = (lambda v: v.permute(0, 3, 1, 2)), (lambda v: v.permute(0, 2, 3, 1))
    x, w = _sp_operands(g, 2, 0)
    want = nhwc(F.conv2d(F.interpolate(nchw(x), scale_factor=2, mode='nearest'), w, padding=1))
    assert (R.subpix_map(x, w, 2, 0) - want).abs().max().item() < 1e-12
    dy = torch.randn(want.shape, generator=g, dtype=D)
    xr = x.clone().requires_grad_(True)
    nhwc(F.conv2d(F.interpolate(nchw(xr), scale_factor=2, mode='nearest'), w, padding=1)).backward(dy)
    assert (R.subpix_map(dy, w, 3, 0) - xr.grad).abs().max().item() < 1e-12
    got = R.subpix_map(x, w, 2, 1)
    tc = nhwc(F.conv_transpose2d(nchw(x), w.transpose(0, 1), stride=2))
    assert got.shape[1:3] == (10, 14) and tc.shape[1:3] == (9, 13)
    assert (got[:, :9, :13] - tc).abs().max().item() < 1e-12
    assert bool((got[:, 9].view(torch.int64) == 0).all()) and bool((got[:, :, 13].view(torch.int64) == 0).all())
    du = torch.randn(got.shape, generator=g, dtype=D)                        # (junk in row / column H + 1: ignored)
    xr = x.clone().requires_grad_(True)
    (nhwc(F.conv_transpose2d(nchw(xr), w.transpose(0, 1), stride=2)) * du[:, :9, :13]).sum().backward()
    assert (R.subpix_map(du, w, 3, 1) - xr.grad).abs().max().item() < 1e-12
    # the out[2 p + k] += x[p] w[k] of the header, element by element on one pixel
    one = torch.zeros(1, 4, 6, 16, dtype=D)
    one[0, 2, 3, 5] = 1.0
    u = R.subpix_map(one, w, 2, 1)
    assert torch.equal(u[0, 4:7, 6:9], w[:, 5].permute(1, 2, 0)) and float(u.abs().sum()) == float(w[:, 5].abs().sum())


@pytest.mark.parametrize('ups,ext', [(2, 0), (2, 1), (3, 0), (3, 1)])
def test_subpix_slab_table_is_tied_to_its_definition(ups, ext):
    """SP_TAPS / subpix_slabs / subpix_windows restate the kernels; subpix_map does not know them.  For each of the
    nine ORIGINAL taps alone, and for a dense weight, the sum over phases (planes) of slab (*) low-resolution window ==
    the plain reference: every one of the 16 slabs of the mode and flip holds exactly the taps the definition gives
    it.  Mode 1 leaves 7 of the 16 slabs empty (the taps sp_skip leaves out), mode 0 none; every original tap sits in
    exactly one slab per phase of mode 0 forward (4 slabs), in 4 of the gradient's, and in one slab of mode 1"""
    g = _g(310 + 2 * ups + ext)
    a, w = _sp_operands(g, ups, ext)

    def by_slabs(wt):
        sl, wins = R.subpix_slabs(wt, ext, ups == 3), R.subpix_windows(a, ups, ext)
        parts = [R.subpix_cols(wins[p]) @ R.subpix_wmat(sl[4 * p:4 * p + 4]).t() for p in range(4)]
        if ups == 3:
            return sum(parts)
        out = torch.zeros(a.shape[0], 2 * parts[0].shape[1], 2 * parts[0].shape[2], parts[0].shape[3], dtype=D)
        for p in range(4):
            out[:, p >> 1::2, p & 1::2] = parts[p]
        return out
    assert (by_slabs(w) - R.subpix_map(a, w, ups, ext)).abs().max().item() < 1e-12
    member = torch.zeros(16, 9, dtype=torch.int64)
    for tap in range(9):
        wt = torch.zeros_like(w)
        wt[:, :, tap // 3, tap % 3] = w[:, :, tap // 3, tap % 3]
        want = R.subpix_map(a, wt, ups, ext)
        assert float(want.abs().max()) > 0 and (by_slabs(wt) - want).abs().max().item() < 1e-12, tap
        member[:, tap] = (R.subpix_slabs(wt, ext, ups == 3).abs().sum(dim=(1, 2)) > 0).long()
    empty = int((member.sum(1) == 0).sum())
    assert empty == (7 if ext else 0)
    per_tap = member.sum(0)
    assert bool((per_tap == (1 if ext else 4)).all()), per_tap
    if not ext:
        assert int(member.sum(1).max()) == 4 and int(member.sum(1).min()) == 1     # 2 x 2 sums down to single taps
    # the window of every slab, read as a position: tap t of phase | plane p at grid point (1, 1)
    T = R.SP_TAPS[(ext, int(ups == 3))]
    for p in range(4):
        for t in range(4):
            assert int(member[4 * p + t].sum()) == len(T[p >> 1][t >> 1]) * len(T[p & 1][t & 1])


def _sp_wrong_prologue(case, i):
    """the mistake the plan's t = 0 launch cannot see: the prologue applied AFTER the padding of the H/2 + 1 grid -- the
    out-of-range window positions p - 1 < 0 and p = H/2 read t (relu(t)) in place of 0 -- in fp64, through the epilogue"""
    i64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in i.items()}
    kw = R.pw_kwargs(case, i, D)
    a, _ = R.pw_prologue(F.pad(i64['x'], (0, 0, 1, 1, 1, 1)), case['pro'], i64['s'], i64['t'])
    u = F.conv_transpose2d(a.permute(0, 3, 1, 2), i64['w'].transpose(0, 1), stride=2).permute(0, 2, 3, 1)
    H, W = case['H'], case['W']
    v = u[:, 2:2 + H + 2, 2:2 + W + 2] * case['alpha']
    r64 = R.subpix_refs(case, i, restate=False)[0]
    return R.conv_epilogue(v, torch.zeros_like(v), **{k: x for k, x in kw.items() if k not in ('pro', 's', 't', 'alpha')}), r64


@pytest.mark.parametrize('case', R.SUBPIX_FWD_CASES + R.SUBPIX_BWD_CASES, ids=R.subpix_id)
def test_subpix_restatements_stay_under_a_quarter_of_k(case):
    """for every case's generator and shape the fp32 restatement of its route is within k / 4 of the fp64 reference on
    sum |a| |w_tap| (H, P: plus subpix_h2_floor): k and the floor were not set from the kernels.  Two negative
    controls.  (1) ext = 1 forward under a prologue: with t = 0 -- the only launch the StyleGAN2 plan makes -- a
    prologue applied after the padding of the H/2 + 1 grid IS the right answer, bit for bit; on the t != 0 draws it
    misses the bar by more than 100 x in the frame's rows / columns 0 and H (and H + 1, which must hold the epilogue of
    0).  (2) cancel: on weights whose taps nearly cancel inside a slab the restatement held to a denominator on |sum
    w_tap| -- sum |a| |slab| -- misses its bar by more than 100 x, and passes on sum |a| |w_tap|"""
    def body(gen):
        i = R.subpix_inputs(gen('subpix', R.subpix_id(case)), case)
        r64, r32 = R.subpix_refs(case, i)
        f = _fig(r32['y'], r64['y'], r64['den'])
        k = R.subpix_k(case)
        assert f <= k / 4.0, (f, k)
        bar = min(k, 4.0 * f)
        if case['ups'] == 2 and case['ext'] and case['pro'] != R.PRO_NONE:
            wrong, _ = _sp_wrong_prologue(case, i)
            err = (wrong['y'] - r64['y']).abs()
            if case['t0']:
                assert float(err.max()) == 0.0
            else:
                H, W = case['H'], case['W']
                edge = torch.zeros(err.shape[1:3], dtype=torch.bool)
                edge[0], edge[H], edge[:, 0], edge[:, W] = True, True, True, True
                edge[H + 1], edge[:, W + 1] = False, False
                rel = err / r64['den'].clamp_min(1e-300) / R.U
                xmax = i['x'].abs().amax(dim=(1, 2, 3))
                b0 = int(torch.where(xmax > 0, xmax, xmax.max()).argmin()) if not case['pro_b'] else case['B'] - 1
                live = (r64['den'][b0] > 0) & edge[..., None]
                miss = float(rel[b0][live].median()) / bar
                print('%s: prologue after the padding misses the bar %.3g x' % (R.subpix_id(case), miss))
                assert miss > 100, miss
                assert float(err[:, 1:H, 1:W].max()) == 0.0                  # (the interior cannot tell)
                assert float(err[:, H + 1].max()) > 0                        # t W[1] where the frame must hold +0
        if case['cancel'] and case['route'] in 'FB':
            # (H, P: the fp16 x 2 floor, 2^-13 of the maxima, stands above a slab cancelled to 2^-18 in either denominator)
            a = r64['aabs']
            sl = R.subpix_slabs(i['w'].double(), case['ext'], case['ups'] == 3).abs()
            wins = R.subpix_windows(a, case['ups'], case['ext'])
            parts = [R.subpix_cols(wins[p]) @ R.subpix_wmat(sl[4 * p:4 * p + 4]).t() for p in range(4)]
            if case['ups'] == 3:
                den_slab = sum(parts)
            else:
                den_slab = torch.zeros_like(r64['den'])
                for p in range(4):
                    den_slab[:, p >> 1::2, p & 1::2] = parts[p]
            miss = _fig(r32['y'], r64['y'], den_slab * abs(case['alpha'])) / bar
            print('%s: a denominator on |sum w_tap| misses the bar %.3g x' % (R.subpix_id(case), miss))
            assert miss > 100, miss
    _draws(body)


@pytest.mark.parametrize('case', R.SUBPIX_ARB_CASES, ids=R.subpix_arb_id)
def test_subpix_dgrad_restatements_stay_under_a_quarter_of_k(case):
    def body(gen):
        i = R.subpix_arb_inputs(gen('sarb', R.subpix_arb_id(case)), case)
        kdx, kds, kdt = R.subpix_arb_k(case)
        r64, r32 = R.subpix_arb_refs(case, i)
        f = _fig(r32['dx'], r64['dx'], r64['den_dx'])
        assert f <= kdx / 4.0, ('dx', f, kdx)
        for name, bound in zip(('ds', 'dt'), R.subpix_arb_bound(case, r64, i['ax'])):
            assert bool(((r32[name].double() - r64[name]).abs() <= bound * R.U).all()), name
        p64, p32 = R.subpix_arb_refs(case, R.arb_positive(i))
        for name, k in (('ds', kds), ('dt', kdt)):
            f = _fig(p32[name], p64[name], p64['den_' + name])
            assert f <= k / 4.0, (name, f, k)
    _draws(body)
    # against autograd through relu(x s + t) -> the forward of the mode, once
    i = R.subpix_arb_inputs(_g(330), case)
    got = R.subpix_arb_refs(case, i)[0]
    x64, s64, t64 = i['ax'].double(), i['as'].double(), i['at'].double()

    def fwd(x, s, t):
        a = x * s[:, None, None, :] + t[:, None, None, :]
        return R.subpix_map(a if case['nomask'] else torch.relu(a), i['w'].double(), 2, case['ext'])
    dx, ds, dt = R.vjp(fwd, [x64, s64, t64], i['x'].double())
    if case['skip_g']:
        C2 = case['Cout'] // 2
        sk = i['skip'].double()[..., :C2]
        dx[..., :C2] += R.quad_sum(sk) if case['skip_g'] == 'ups' else sk
    for name, want in (('dx', dx), ('ds', ds), ('dt', dt)):
        assert (got[name] - want).abs().max().item() <= 1e-11 * want.abs().max().item(), name


@pytest.mark.parametrize('tap', range(9))
def test_subpix_one_hot_inputs_are_exact_in_every_restatement(tap):
    """single power-of-two pixels and a single power-of-two weight on one original tap go through the slab sums, the
    fp32 chain, the bf16 x 3 and the fp16 x 2 pieces and the slices without a rounding: every restatement gives the
    fp64 result bit for bit, and it is not all zero"""
    for c in (R._ssh('F', 2, 0, '32x32'), R._ssh('B', 2, 1, '16x16'), R._ssh('H', 2, 1, '8x8'), R._ssh('P', 2, 0, '4x4'),
              R._ssh('F', 3, 1, '16x16'), R._ssh('B', 3, 0, '8x8'), R._ssh('H', 3, 0, '16x64'),
              R._ssh('H', 3, 1, 's4', splitk=4), R._ssh('H', 3, 1, 's8', splitk=8)):
        for seed in range(2):
            i = R.subpix_onehot(c, tap, seed)
            r64, r32 = R.subpix_refs(c, i)
            assert torch.equal(r32['y'].double(), r64['y']), (R.subpix_id(c), seed)
            assert torch.equal(r64['y'], R.subpix_map(i['x'].double(), i['w'].double(), c['ups'], c['ext']))
            assert int((r64['y'] != 0).sum()) >= 3, (R.subpix_id(c), seed)


def _choose_bn(c):
    """choose_bn of csrc/p2l_conv.hip for a sub-pixel case"""
    (gh, gw), (TW, TH, TB) = R.subpix_grid(c)
    n_mtiles = R.cdiv(gw, TW) * R.cdiv(gh, TH) * R.cdiv(c['B'], TB)
    if c['Cout'] % 64:
        return 32
    ph = 4 if c['ups'] == 2 else 1
    n64, n32 = n_mtiles * (c['Cout'] // 64) * ph, n_mtiles * (c['Cout'] // 32) * ph
    if n64 < 256:
        return 32
    return 32 if R.cdiv(n32, 256) * 32.0 * 1.06 < 0.93 * R.cdiv(n64, 256) * 64.0 else 64


def test_subpix_case_tables():
    """the slice counts of the issue against the restatement of subpix_bwd_split; the tiles each shape reaches
    (choose_tile on the low-resolution grid); 64-channel tiles at the two bn64 shapes only; every route in all four
    modes with every epilogue term of its mode; H with all sources of its maxima; the images of a launch 3e10 apart"""
    assert R.subpix_bwd_split(16, 16, 128, 64) == 4 and R.subpix_bwd_split(16, 16, 256, 32) == 8
    assert R.subpix_bwd_split(32, 32, 256, 32) == 4 and R.subpix_bwd_split(16, 16, 64, 64) == 1
    for c in R.SUBPIX_BWD_CASES + R.SUBPIX_ARB_CASES:
        if c['splitk'] > 1:
            assert c['route'] == 'H' and c['ext'] and R.subpix_bwd_split(c['H'], c['W'], c['Cin'], c['Cout']) == c['splitk']
            assert len(R.subpix_slices(c)) == c['splitk']
    assert R.subpix_slices(R._ssh('H', 3, 1, 's4', splitk=4)) == [(z * 512, (z + 1) * 512) for z in range(4)]
    tiles = {}
    for c in R.SUBPIX_FWD_CASES + R.SUBPIX_BWD_CASES:
        tiles.setdefault((c['ups'], c['ext']), set()).add(R.subpix_grid(c))
    assert tiles[(2, 0)] >= set([((8, 16), (16, 8, 1)), ((16, 16), (16, 8, 1)), ((8, 32), (16, 8, 1)), ((4, 4), (4, 4, 8)),
                                 ((2, 2), (2, 8, 8)), ((8, 8), (8, 8, 2))])
    assert tiles[(2, 1)] >= set([((5, 5), (8, 8, 2)), ((9, 9), (16, 8, 1)), ((17, 17), (16, 8, 1)), ((9, 17), (16, 8, 1)),
                                 ((3, 3), (4, 4, 8))])
    assert tiles[(3, 1)] >= set([((8, 16), (16, 8, 1)), ((16, 16), (16, 8, 1)), ((4, 4), (4, 4, 8)), ((2, 2), (2, 8, 8))])
    for c in R.SUBPIX_FWD_CASES + R.SUBPIX_BWD_CASES:
        name = [n for n, v in R.SUBPIX_SHAPES.items() if v == ((c['H'], c['W']), c['B'], c['Cin'], c['Cout'])][0]
        assert _choose_bn(c) == (64 if name.startswith('bn64') else 32), R.subpix_id(c)
    for route in 'FBH':
        for ups, ext, epi in ((2, 0, R.SP_EPI_E0), (2, 1, R.SP_EPI_E1), (3, 0, R.SP_EPI_G), (3, 1, R.SP_EPI_G)):
            cs = [c for c in R.SUBPIX_FWD_CASES + R.SUBPIX_BWD_CASES if (c['route'], c['ups'], c['ext']) == (route, ups, ext)]
            for e in epi:
                assert any(all(c[k] == v for k, v in e.items()) for c in cs), (route, ups, ext, e)
            assert any(c['n_store'] < c['Cout'] for c in cs), (route, ups, ext)
    for ext in (0, 1):
        assert any((c['route'], c['ext']) == ('P', ext) for c in R.SUBPIX_FWD_CASES)
    h = [c for c in R.SUBPIX_FWD_CASES if c['route'] in 'HP']
    assert set(c['amax'] for c in h) == set([None, 'true', 'raw', 'applied'])
    assert len(set(R.subpix_id(c) for c in R.SUBPIX_FWD_CASES + R.SUBPIX_BWD_CASES)) == \
        len(R.SUBPIX_FWD_CASES + R.SUBPIX_BWD_CASES)
    assert len(set(R.subpix_arb_id(c) for c in R.SUBPIX_ARB_CASES)) == len(R.SUBPIX_ARB_CASES)
    i = R.subpix_inputs(_g(340), R._ssh('H', 2, 1, '8x8', pro=R.PRO_AFFINE))
    m = i['x'].abs().amax(dim=(1, 2, 3))
    assert float(m[2] / m[0]) > 1e13 and not bool(i['x'][1].any())
    w = R.subpix_inputs(_g(341), R._ssh('F', 2, 0, '32x32', cancel=True))['w']
    sl, big = R.subpix_slabs(w.double(), 0, False), R.subpix_slabs(w.double().abs(), 0, False)
    assert float((sl[3].abs() / big[3]).median()) < 2.0 ** -16          # phase (0, 0), tap (1, 1): {1, 2} x {1, 2}
    off = (R.subpix_slabs(w, 0, False)[3].double() - sl[3]).abs()          # ... and fp32 cannot follow the chain
    assert float((off / sl[3].abs()).median()) > 2.0 ** -10 and float((off / big[3]).max()) <= 3 * R.U


# ---- generic gather conv: the references, restatements and cases of tests/test_gconv_kernels_gpu.py -----------------
GCONV_ALL = R.GCONV_CASES + list(R.GCONV_PAIR)


def test_gconv_reference_geometry_and_im2col_order():
    """R.gconv against a conv written out tap by tap on the padded tensor (stride, padding, floor division, KH != KW);
    column (tap, chunk, j, h) of gconv_cols holds channel 16 chunk + 8 h + j of pixel (oy s - p + ky, ox s - p + kx);
    cols x wmat is the conv; a dgrad case's vjp is the launch's conv with the transposed, tap-reversed weight"""
    for n, c in enumerate(GCONV_ALL):
        i = R.gconv_inputs(_g(400 + n), c)
        x, w = i['x'].double(), R.gconv_weight(c, i, D)
        s, p, KH, KW = c['stride'], c['pad'], c['KH'], c['KW']
        Ho, Wo = R.gconv_out(c)
        assert (Ho - 1) * s + KH <= c['Hi'] + 2 * p < Ho * s + KH and (Wo - 1) * s + KW <= c['Wi'] + 2 * p < Wo * s + KW
        xp = torch.zeros(c['B'], c['Hi'] + 2 * p, c['Wi'] + 2 * p, c['Cin'], dtype=D)
        a = x * i['pro_s'].double() + i['pro_t'].double() if c['pro'] else x
        xp[:, p:p + c['Hi'], p:p + c['Wi']] = a
        want = torch.zeros(c['B'], Ho, Wo, c['n_store'], dtype=D)
        for ky in range(KH):
            for kx in range(KW):
                win = xp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s]
                want += win @ w[:, :, ky, kx].t()
        plain = R.gconv(x, w, s, p, i.get('pro_s'), i.get('pro_t'))
        assert float((plain['y'] - want).abs().max()) <= 1e-12 * float(plain['den'].max())
        cols, wm = R.gconv_cols(a, c), R.gconv_wmat(w)
        assert float((cols @ wm.t() - want).abs().max()) <= 1e-12 * float(plain['den'].max())
        tap, ch, j, h = KH * KW - 1, c['Cin'] // 16 - 1, 3, 1
        col = ((tap * (c['Cin'] // 16) + ch) * 8 + j) * 2 + h
        assert torch.equal(cols[..., col], xp[:, KH - 1:KH + (Ho - 1) * s:s, KW - 1:KW + (Wo - 1) * s:s, 16 * ch + 8 * h + j])
        assert torch.equal(wm[:, col], w[:, 16 * ch + 8 * h + j, KH - 1, KW - 1])
        r64, _ = R.gconv_refs(c, i)
        full = R.gconv(x, w, **R._gconv_kwargs(c, i, D))
        if c['dgrad']:
            assert float((r64['y'] - full['y']).abs().max()) <= 1e-12 * float(full['den'].max())
        else:
            assert torch.equal(r64['y'], full['y'])
        if c['mask']:
            dead = ~(i['mask'] > 0)
            assert bool(dead.any()) and bool((r64['y'][dead] == 0).all())
            assert bool((i['mask'] < 0).any()) and bool(torch.signbit(i['mask'][i['mask'] == 0]).any())


@pytest.mark.parametrize('case', GCONV_ALL, ids=R.gconv_id)
def test_gconv_restatements_stay_under_a_quarter_of_k(case):
    """for every case's generator and shape the fp32 restatement is within k / 4 of the fp64 reference on the issue's
    denominator: the bar min(k, 4 x restatement) is attainable and k was not set from the kernel.  Zero padding
    applied in FRONT of the prologue is far outside the bar at the border of every case with a prologue and
    padding"""
    def body(gen):
        i = R.gconv_inputs(gen('gconv', R.gconv_id(case)), case)
        r64, r32 = R.gconv_refs(case, i)
        f = _fig(r32['y'], r64['y'], r64['den'])
        assert f <= R.gconv_k(case) / 4.0, (f, R.gconv_k(case))
        if case['pro'] and case['pad'] and not case['relu']:
            x = i['x'].double()
            p = case['pad']
            xs = F.pad(x * i['pro_s'].double(), (0, 0, p, p, p, p)) + i['pro_t'].double()     # the halo holds pro_t
            w = R.gconv_weight(case, i, D)
            acc = F.conv2d(xs.permute(0, 3, 1, 2), w, stride=case['stride']).permute(0, 2, 3, 1)
            wrong = R.gconv(x, w, acc=acc, **R._gconv_kwargs(case, i, D))
            err = (wrong['y'] - r64['y']).abs() / r64['den'] / R.U
            assert float(err[:, 0].median()) > 100 * min(R.gconv_k(case), 4.0 * f)
    _draws(body)


def test_gconv_one_hot_inputs_are_exact_in_the_restatement():
    for KH, KW, s, p in R.gconv_geometries():
        c = R._gc('onehot', (KH, KW), s, p, (max(KH, 7) + 2 * s, max(KW, 6) + 2 * s + 1), 2, 16, 64)
        for n, spot in enumerate(R.gconv_spots(c)):
            i = R.gconv_onehot(c, spot, n)
            r64, r32 = R.gconv_refs(c, i)
            assert torch.equal(r32['y'].double(), r64['y']), (KH, KW, s, p, spot)
            # one product per output: the quotient by x is the weight of the one tap and channel that reached it
            xv = float(i['x'][spot][(5 * n) % 16])
            nz = r64['y'] != 0
            vals = set((r64['y'][nz] / xv).tolist())
            assert vals <= set(i['w'][:, (5 * n) % 16].double().reshape(-1).tolist()), (KH, KW, s, p, spot)
    assert len(R.gconv_geometries()) >= 10


@pytest.mark.parametrize('taps_hw', [(1, 1), (2, 3), (3, 3), (5, 5), (11, 11)])
@pytest.mark.parametrize('flip', [False, True])
def test_gconv_pack_is_the_written_out_layout(taps_hw, flip):
    KH, KW = taps_hw
    O, I, N_pad, K_pad = (16, 3, 64, 16) if not flip else (35, 16, 64, 48)
    w = torch.randn(O, I, KH, KW, generator=_g(430))
    got = R.gconv_pack(w, N_pad, K_pad, flip).view(KH * KW, K_pad // 16, N_pad, 16)
    N, K = (I, O) if flip else (O, I)
    want = torch.zeros_like(got)
    for tap in range(KH * KW):
        for k in range(K):
            for n in range(N):
                v = w[k, n].reshape(-1)[KH * KW - 1 - tap] if flip else w[n, k].reshape(-1)[tap]
                want[tap, k // 16, n, k % 16] = v
    assert torch.equal(got, want)


def test_gconv_case_table():
    """the mechanisms the issue names, each in at least one case"""
    cs = R.GCONV_CASES
    M = lambda c: c['B'] * R.gconv_out(c)[0] * R.gconv_out(c)[1]
    assert set([1, 63, 64, 65, 128, 40, 105]) <= set(M(c) for c in cs)
    assert any(c['Cin'] == 48 and not c['dgrad'] for c in cs) and any(c['Cin'] == 48 and c['dgrad'] for c in cs)
    assert set(c['n_store'] for c in cs if c['tight']) >= set([16, 48])
    assert set(c['n_store'] for c in cs if c['dgrad'] and c['aux_tight']) == set([16, 32, 48])
    d = [c for c in cs if c['dgrad']]
    assert set((c['res'], c['mask']) for c in d) == set([(True, True), (True, False), (False, True), (False, False)])
    assert any(c['x_off'] for c in d) and any(c['KH'] == 5 and c['Cin'] == 192 for c in d)
    assert any(c['KH'] != c['KW'] for c in cs) and any(c['stride'] > c['KH'] for c in cs)
    assert any(c['pad'] >= c['KH'] and c['pro'] for c in cs)
    assert all(max(c['Hi'], c['Wi']) <= 24 for c in cs + list(R.GCONV_PAIR))
    assert len(set(R.gconv_id(c) for c in GCONV_ALL)) == len(GCONV_ALL)
    assert [c['col'] for c in R.GCONV_PAIR] == [0, 64] and all(c['y_ld'] == 128 for c in R.GCONV_PAIR)


# ---- thin 3x3 convs ---------------------------------------------------------------------------------------------------
def _thin_route(case):
    """the route a forward case's own launch takes and, where it is a thin one, B beside it"""
    return [case['route']] + (['B'] if case['route'] != 'B' else [])


@pytest.mark.parametrize('case', R.THIN_FWD_CASES, ids=R.thin_id)
def test_thin_forward_reference_is_conv2d_and_the_walks_are_the_conv(case):
    """from the definition alone: the fp64 reference of a case is F.conv2d(padding = 1) of the prologue's result on
    the REAL channels with the real weight, through the epilogue; and the walk of either thin kernel (27 tap-channel
    columns as one K | Z columns and the nine-tap sum), run with a plain fp64 matrix product, is that conv"""
    i = R.thin_inputs(_g(400), case)
    ri, ro = R.thin_real(case)
    kw = R.pw_kwargs(case, i, D)
    r64, _ = R.thin_refs(case, i, restate=False)
    x, s, t = i['x'].double()[..., :ri], kw['s'], kw['t']
    a = x if case['pro'] == R.PRO_NONE else x * s[:, None, None, :ri] + t[:, None, None, :ri]
    a = torch.relu(a) if case['pro'] == R.PRO_AFFINE_RELU else a
    v = F.conv2d(a.permute(0, 3, 1, 2), i['w'].double()[:ro, :ri], padding=1).permute(0, 2, 3, 1)
    full = torch.zeros(v.shape[:3] + (case['Cout'],), dtype=D)
    full[..., :ro] = v
    want = R.conv_epilogue(full * case['alpha'], torch.ones_like(full),
                           **{k: u for k, u in kw.items() if k not in ('pro', 's', 't', 'alpha')})
    for out in ('y', 'yp'):
        if r64[out] is not None:
            scale = r64['den' if out == 'y' else 'denp'].clamp_min(1e-300)
            assert float(((want[out] - r64[out]).abs() / scale).max()) < 1e-12, out
    assert bool(torch.isfinite(r64['y']).all()) and bool(torch.isfinite(r64['den']).all())   # (the junk of s, t shows nowhere)
    kind = R.thin_kind(case)
    if kind >= 0:
        i64 = {k: (u.double() if torch.is_tensor(u) else u) for k, u in i.items()}
        walk = R.thin_acc32(case, i64, 'TI' if kind else 'TO', mm=lambda p, q: p @ q.t())
        den = F.conv2d(a.abs().permute(0, 3, 1, 2), i['w'].double()[:ro, :ri].abs(), padding=1).permute(0, 2, 3, 1)
        assert float(((walk[..., :ro] - v).abs() / den.clamp_min(1e-300)).max()) < 1e-12
        assert bool((walk[..., ro:] == 0).all())


@pytest.mark.parametrize('case', R.THIN_FWD_CASES, ids=R.thin_id)
def test_thin_forward_restatements_stay_under_a_quarter_of_k(case):
    """for every case's generator and shape the fp32 restatement of its route -- and of route B on the same inputs --
    is within k / 4 of the fp64 reference on den_d.  Under a prologue with t != 0 (relu(t) > 0 on channel 0) zero
    padding applied in FRONT of the prologue is more than 100 bars off at the border of the thin cases."""
    def body(gen):
        i = R.thin_inputs(gen('thin', R.thin_id(case)), case)
        for route in _thin_route(case):
            r64, r32 = R.thin_refs(case, i, route)
            for out, den, pooled in (('y', 'den', False), ('yp', 'denp', True)):
                if r64[out] is not None:
                    f = _fig(r32[out], r64[out], r64[den])
                    assert f <= R.thin_k(case, route, pooled) / 4.0, (route, out, f, R.thin_k(case, route, pooled))
        if case['pro'] != R.PRO_NONE:
            t = i['t']
            assert bool((t[:, 0] > 0).all()) and bool((t[:, 1] < 0).all())          # relu(t) > 0 somewhere, t != 0
        if case['pro'] != R.PRO_NONE and case['act'] == R.ACT_NONE and not case['mask'] and case['route'] != 'B':
            kw = R.pw_kwargs(case, i, D)
            r64, r32 = R.thin_refs(case, i)
            a, _ = R.pw_prologue(i['x'].double(), case['pro'], i['s'].double(), i['t'].double())
            halo, _ = R.pw_prologue(torch.zeros_like(i['x'][:, :1, :1]).double(), case['pro'], i['s'].double(), i['t'].double())
            ap = F.pad(a - halo, (0, 0, 1, 1, 1, 1)) + halo                      # the halo holds prologue(0)
            wrong = F.conv2d(ap.permute(0, 3, 1, 2), i['w'].double()).permute(0, 2, 3, 1) * case['alpha']
            wrong = R.conv_epilogue(wrong, torch.ones_like(wrong), **{k: v for k, v in kw.items() if k not in ('pro', 's', 't', 'alpha')})
            ro = R.thin_real(case)[1]
            for out, den, pooled in (('y', 'den', False), ('yp', 'denp', True)):
                if r64[out] is None:
                    continue
                err = ((wrong[out] - r64[out]).abs() / r64[den].clamp_min(1e-300) / R.U)[..., :min(ro, case['n_store'])]
                border = torch.ones(err.shape[1:3], dtype=torch.bool)
                border[1:-1, 1:-1] = False
                bar = min(R.thin_k(case, None, pooled), 4.0 * _fig(r32[out], r64[out], r64[den]))
                assert float(err[:, border].median()) > 100 * bar, (out, bar)
                assert float(err[:, ~border].max()) < 1e-3
    _draws(body)


@pytest.mark.parametrize('case', R.THIN_ARB_CASES, ids=R.thin_arb_id)
def test_thin_dgrad_reference_is_autograd_and_restatements_stay_under_a_quarter_of_k(case):
    """da of the fp64 reference is autograd through F.conv2d of the FORWARD conv whose OIHW tensor the packer is handed
    for its transpose_flip copy (thin_weight(flip = True)); dx, ds, dt of the restatement as in the direct module"""
    kfn = lambda cc, route=None, pooled=False: R.thin_k(cc, case['route'], pooled)

    def body(gen):
        i = R.thin_arb_inputs(gen('tarb', R.thin_arb_id(case)), case)
        kdx, kds, kdt = R.arb_k(case, kfn)
        r64, r32 = R.thin_arb_refs(case, i)
        f = _fig(r32['dx'], r64['dx'], r64['den_dx'])
        assert f <= kdx / 4.0, ('dx', f, kdx)
        for name, bound in zip(('ds', 'dt'), R.arb_bound(case, r64, i['ax'], kfn)):
            assert bool(((r32[name].double() - r64[name]).abs() <= bound * R.U).all()), name
        p64, p32 = R.thin_arb_refs(case, R.arb_positive(i))
        for name, k in (('ds', kds), ('dt', kdt)):
            f = _fig(p32[name], p64[name], p64['den_' + name])
            assert f <= k / 4.0, (name, f, k)
        if not case['nomask'] and not case['skip']:
            assert bool((r64['g'] == 0).any()) and bool((r64['g'] != 0).any())       # masked-off elements exist
    _draws(body)
    # the flip, from the definition: the launch's weight applied as a correlation == the input gradient of the forward conv
    i = R.thin_arb_inputs(_g(410), case)
    ri, ro = R.thin_real(case)
    wf = R.thin_weight(case, i, flip=True).double()                           # forward conv: [O = ri, I = ro, 3, 3]
    assert wf.shape == (ri, ro, 3, 3)
    dy = i['x'].double()[..., :ri].permute(0, 3, 1, 2)
    xin = torch.zeros(case['B'], ro, case['H'], case['W'], dtype=D, requires_grad=True)
    F.conv2d(xin, wf, padding=1).backward(dy)
    da = R.conv3x3(i['x'].double(), i['w'].double(), den_w=False)['y']
    assert float((da[..., :ro] - xin.grad.permute(0, 2, 3, 1)).abs().max()) < 1e-12 * float(da.abs().max())
    assert bool((da[..., ro:] == 0).all())


def test_thin_arb_sums_and_dead_units():
    """thin_arb_sums32, restated from the thin-input kernel (butterfly over lanes >= 8, (0 + 1) + (2 + 3), one partial
    per 8 x 16 block), gives the bits of arb_sums32's unsplit order on whole 8 x 16 tiles; its fp64 value is the plain
    sum; the gradient inputs hold a dead unit (a channel of an image with no live pixel)"""
    g = _g(420)
    for H, W, pool_sum in ((16, 32, False), (24, 16, True), (8, 48, False)):
        Ho, Wo = (H // 2, W // 2) if pool_sum else (H, W)
        gg, xx = torch.randn(2, Ho, Wo, 8, generator=g), torch.randn(2, Ho, Wo, 8, generator=g)
        a, b = R.thin_arb_sums32(gg, xx, H, W, pool_sum), R.arb_sums32(gg, xx, H, W, pool_sum, False)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert float((a[0].double() - (gg.double() * xx.double()).sum(dim=(1, 2))).abs().max()) < 1e-4
    dead = 0
    for case in R.THIN_ARB_CASES:
        if case['nomask']:
            continue
        i = R.thin_arb_inputs(_g(421), case)
        r64, _ = R.thin_arb_refs(case, i)
        live = (R.fma(i['ax'], i['as'][:, None, None], i['at'][:, None, None]) > 0)
        dead += int((~live).all(dim=1).all(dim=1).sum())
        assert bool((r64['g'][~live] == 0).all())
    assert dead > 0


@pytest.mark.parametrize('tap', range(9))
def test_thin_one_hot_inputs_are_exact_in_every_restatement(tap):
    for c in (R._tsh('TI', 'i16x32'), R._tsh('TI', 'i24x16'), R._tsh('TO', 'o16x32'), R._tsh('TO', 'o24x16'),
              R._tsh('B', 'n12x20')):
        for seed in range(3):
            i = R.thin_onehot(c, tap, seed)
            for route in _thin_route(c):
                r64, r32 = R.thin_refs(c, i, route)
                assert torch.equal(r32['y'].double(), r64['y']), (R.thin_id(c), route, seed)
            assert int((r64['y'] != 0).sum()) >= 3, (R.thin_id(c), seed)


def test_thin_case_tables_and_spots():
    """every width, chunk count, n_store and prologue the issue names is in the tables; every launch-side fallback of
    thin_takes; the spot lists cover each seam, wave boundary and quad boundary on both sides; a masked-off element
    exists; nothing is larger than 24 x 16 ... 16 x 32 ... 8 x 48 pixels"""
    cs = R.THIN_FWD_CASES
    ti = [c for c in cs if c['route'] == 'TI']
    to = [c for c in cs if c['route'] == 'TO']
    b = [c for c in cs if c['route'] == 'B']
    assert all(R.thin_kind(c) == 1 for c in ti) and all(R.thin_kind(c) == 0 for c in to)
    assert not any(R.thin_falls_back(c) for c in ti + to)
    assert set(c['Cout'] for c in ti) == set([64, 96])
    assert set(c['n_store'] for c in ti if c['Cout'] == 64) >= set([16, 36, 64])
    assert set(c['Cin'] // 16 for c in to) == set([2, 3, 4])
    assert set((c['n_store'], c['y_gap']) for c in to) >= set([(4, 4), (16, 0), (16, 4), (32, 4)])
    for group in (ti, to):
        assert set((c['pro'], c['pro_b']) for c in group if c['pro']) == set([(1, 0), (1, 1), (2, 0), (2, 1)])
        assert any(c['pro'] == R.PRO_NONE for c in group)
        assert set((c['B'], c['H'], c['W']) for c in group) >= set([(1, 8, 16), (2, 16, 32), (3, 24, 16), (2, 8, 48)])
    assert set(c['act'] for c in to) == set([0, 1, 2, 3]) and any(c['alpha'] != 1.0 for c in to)
    assert any(c['bias'] for c in to) and any(not c['bias'] for c in to)
    for e in R.EPI:
        assert any(all(c[k] == v for k, v in e.items()) for c in ti + b if R.thin_kind(c) == 1), e
    # the two product combinations of either kernel
    assert any(c['pro'] == R.PRO_AFFINE and not c['pro_b'] and c['bias'] and c['act'] == R.ACT_RELU for c in ti)
    assert any(c['pro'] == R.PRO_AFFINE_RELU and not c['pro_b'] and c['bias'] and c['act'] == R.ACT_TANH and
               (c['n_store'], c['y_gap']) == (16, 0) for c in to)
    assert any(c['Cin'] == 64 and c['pro'] == 0 and not c['bias'] and (c['n_store'], c['y_gap']) == (16, 0) for c in to)
    # the fallbacks of thin_takes, and the shapes thin_shape leaves
    fb = [c for c in b if R.thin_falls_back(c)]
    for kind, key in ((0, 'res'), (0, 'mask'), (0, 'oscale'), (0, 'noise'), (1, 'oscale'), (1, 'noise')):
        assert any(R.thin_kind(c) == kind and c[key] for c in fb), (kind, key)
    assert any(R.thin_kind(c) == 0 and c['pool'] and c['want_y'] for c in fb)
    assert any(R.thin_kind(c) == 0 and c['pool'] and not c['want_y'] for c in fb)
    assert all(R.thin_form(c) == (4, 0) for c in cs) and all(R.thin_form(c, 'B') == (4, 16) for c in ti + to)
    nt = [c for c in b if R.thin_kind(c) < 0]
    assert set((c['H'], c['W']) for c in nt) >= set([(12, 20), (8, 8)]) and any((c['Cin'], c['Cout']) == (16, 32) for c in nt)
    assert all(c['H'] * c['W'] <= 512 for c in cs + R.THIN_ARB_CASES)
    assert len(set(R.thin_id(c) for c in cs)) == len(cs)
    assert len(set(R.thin_arb_id(c) for c in R.THIN_ARB_CASES)) == len(R.THIN_ARB_CASES)
    arb = [c for c in R.THIN_ARB_CASES if c['route'] == 'TI']
    for v in R.ARB_VARIANTS:
        for amax_out in (False, True):
            assert any(all(c[k] == u for k, u in v.items()) and c['amax_out'] == amax_out and
                       (c['skip'] is None) == ('skip' not in v) for c in arb), (v, amax_out)
    assert any(c['route'] == 'B' and R.thin_kind(c) == 0 for c in R.THIN_ARB_CASES)
    # a masked-off element; images 3e14 apart; the real channels alone are non-zero
    mc = [c for c in cs if c['mask']][0]
    i = R.thin_inputs(_g(430), mc)
    assert bool((i['mask'] <= 0).any()) and bool((i['mask'] > 0).any())
    i = R.thin_inputs(_g(431), R._tsh('TI', 'i24x16'))
    m = i['x'].abs().amax(dim=(1, 2, 3))
    assert float(m[2] / m[0]) > 1e13 and bool((i['x'][..., 3:] == 0).all()) and bool((i['w'][:, 3:] == 0).all())
    # spots: both sides of every seam / wave boundary / quad boundary
    for H, W, B in ((8, 16, 1), (16, 32, 2), (24, 16, 3), (8, 48, 2)):
        sp = R.thin_spots(H, W, B)
        rows, cols = set(s[1] for s in sp if s[0] == 0), set(s[2] for s in sp if s[0] == 0)
        assert all(0 <= s[0] < B and 0 <= s[1] < H and 0 <= s[2] < W for s in sp)
        for ys in range(8, H, 8):
            assert ys - 1 in rows and ys in rows
        for xs in range(16, W, 16):
            assert xs - 1 in cols and xs in cols
        for wv in range(3):
            assert 2 * wv + 1 in rows and 2 * wv + 2 in rows
        assert any(s[2] % 2 == 1 and (s[0], s[1], s[2] + 1) in sp for s in sp)
        assert set([(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1)]) <= set(sp)
        if B > 1:
            assert (1, 0, 0) in sp and (1, H - 1, W - 1) in sp


def test_thin_size_queries_on_the_host():
    """pure host functions of the descriptor (no device call): a thin shape never takes K slices --
    p2l_conv_suggest_splitk is 1 and p2l_conv_workspace_bytes 0 whatever d.splitk says; a shape thin_shape leaves
    is sized for d.splitk as it stands; the maxima slots are blocks x 4 for thin input and 0 for thin output"""
    import ctypes as C
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, 'pix2latent_amd', 'libp2l_hip.so')):
        import __graft_entry__ as g
        g.build()
    from pix2latent_amd import _native as N
    lib = N.lib()
    for c in R.THIN_FWD_CASES:
        for splitk in (1, 4):
            d = N.P2LConv()
            d.B, d.H, d.W, d.Cin, d.Cout, d.taps, d.ups = c['B'], c['H'], c['W'], c['Cin'], c['Cout'], 9, 0
            d.x_ld, d.alpha, d.splitk, d.wfmt, d.form = c['Cin'] + c['x_gap'], 1.0, splitk, R.WFMT_BF16X3T, 0
            d.n_store = d.y_ld = c['n_store']
            kind = R.thin_kind(c)
            if kind >= 0:
                assert lib.p2l_conv_workspace_bytes(C.byref(d)) == 0, (R.thin_id(c), splitk)
                assert lib.p2l_conv_suggest_splitk(C.byref(d)) == 1
                blocks = (c['H'] // 8) * (c['W'] // 16)
                assert lib.p2l_conv_amax_slots(C.byref(d)) == (blocks * 4 if kind == 1 else 0), R.thin_id(c)
            elif splitk == 4:
                # a shape thin_shape leaves is a direct launch: the query sizes the slices of d.splitk as it stands
                assert lib.p2l_conv_workspace_bytes(C.byref(d)) == 4 * c['B'] * c['H'] * c['W'] * c['Cout'] * 4

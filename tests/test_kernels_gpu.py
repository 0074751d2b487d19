"""Per-kernel parity: every HIP kernel of libp2l_hip against plain PyTorch-CPU
fp32 ops (the oracle's building blocks) on seeded inputs.  Tolerances are
fp32-summation-order level and written per test."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def nhwc(t, dev):          # NCHW cpu -> NHWC device
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def nchw(t):               # NHWC device -> NCHW cpu
    return t.detach().cpu().permute(0, 3, 1, 2).contiguous()


def relerr(a, b):
    return ((a - b).abs().max() / (b.abs().max() + 1e-20)).item()


@pytest.fixture(scope='module')
def O(dev):
    from pix2latent_amd import ops
    return ops


def test_mfma_probe_layout(dev, O):
    """asymmetric A/B so that a transposed fragment map cannot pass."""
    g = torch.Generator().manual_seed(0)
    A = torch.randn(32, 8, generator=g)
    B = torch.randn(8, 32, generator=g)
    Cm = O.mfma_probe(A.to(dev), B.to(dev)).cpu()
    assert relerr(Cm, A @ B) < 1e-5


CONV_CASES = [
    # B, H, Cin, Cout, taps, extras
    dict(B=2, H=16, Cin=64, Cout=64, taps=9),
    dict(B=3, H=32, Cin=32, Cout=96, taps=9, bias=True),               # BN=32 path
    dict(B=2, H=16, Cin=64, Cout=128, taps=1, bias=True),
    dict(B=2, H=32, Cin=64, Cout=64, taps=9, pro='affine_relu', bias=True),
    dict(B=2, H=32, Cin=64, Cout=64, taps=9, pro='affine_relu', ups=True, bias=True),
    dict(B=3, H=4, Cin=128, Cout=64, taps=9, pro='affine_relu', bias=True),      # TB=8 tile, split-K
    dict(B=3, H=8, Cin=128, Cout=64, taps=9, pro='affine_relu', ups=True, bias=True),  # TB=2
    dict(B=9, H=4, Cin=256, Cout=64, taps=1, pro='affine_relu', bias=True),
    dict(B=2, H=16, Cin=64, Cout=64, taps=9, act='relu', pool='max', bias=True),
    dict(B=2, H=16, Cin=64, Cout=64, taps=9, pool='sum', want_y=False),
    dict(B=3, H=8, Cin=128, Cout=64, taps=9, pool='sum', want_y=False, splitk=4),
    dict(B=2, H=16, Cin=64, Cout=128, taps=1, res='same', alpha=0.5),
    dict(B=2, H=16, Cin=64, Cout=64, taps=1, res='ups', bias=True, pro='affine_relu'),
    dict(B=2, H=16, Cin=64, Cout=64, taps=9, mask=True),
    dict(B=2, H=32, Cin=16, Cout=64, taps=9, pro='affine', act='relu', bias=True),   # VGG conv0 form
    dict(B=2, H=32, Cin=64, Cout=32, taps=9, act='tanh', n_store=16, bias=True),     # rgb form
    dict(B=1, H=64, Cin=64, Cout=64, taps=9, splitk=2, bias=True),
    # shapes the Winograd form takes (H % 16 == 0, Cout % 64 == 0) with every epilogue family
    dict(B=2, H=32, Cin=32, Cout=128, taps=9, pro='affine_relu', bias=True, act='relu', pool='max'),
    dict(B=1, H=48, Cin=48, Cout=64, taps=9, res='same', alpha=0.5, bias=True),
    dict(B=2, H=16, Cin=128, Cout=64, taps=9, mask=True, pro='affine'),
    dict(B=2, H=32, Cin=16, Cout=64, taps=9, res='ups', bias=True),
    # 1x1 shapes the bf16x3 pointwise kernel takes (>= 32x32, Cin and Cout multiples of 64)
    dict(B=2, H=32, Cin=64, Cout=64, taps=1, bias=True),
    dict(B=2, H=32, Cin=256, Cout=128, taps=1, pro='affine_relu', bias=True, res='same', alpha=0.5),
    dict(B=3, H=32, Cin=128, Cout=64, taps=1, res='ups', bias=True, pro='affine_relu'),
    dict(B=2, H=64, Cin=128, Cout=64, taps=1, act='relu', pool='max'),
    dict(B=2, H=32, Cin=64, Cout=128, taps=1, pool='sum', want_y=False, pro='affine'),
    # channel-expanding 1x1 shapes (64 / 128 inputs: one to four 32-channel stages)
    dict(B=2, H=32, Cin=128, Cout=256, taps=1, pro='affine_relu', bias=True, res='same', alpha=0.5),
    dict(B=3, H=32, Cin=64, Cout=256, taps=1, res='ups', bias=True, pro='affine_relu'),
    dict(B=1, H=64, Cin=128, Cout=512, taps=1, act='relu', pool='max', pro='affine'),
    dict(B=9, H=64, Cin=64, Cout=192, taps=1, mask=True, bias=True),
]


# P2L_WFMT_F32 (exact fp32 MFMA), P2L_WFMT_BF16X3 (3-way bf16 split, 6 products, direct kernel),
# P2L_WFMT_BF16X3W (same arithmetic; eligible shapes run in the Winograd F(2x2,3x3) form)
# P2L_WFMT_PW (1x1 convs: fp32 layout + bf16x3 image; layers >= 32x32 run in the bf16x3 arithmetic)
# (4 = P2L_WFMT_BF16X3W again, with the 16x16-pixel / 8-wave Winograd kernel forced wherever H, W allow)
# (5 = P2L_WFMT_BF16X3W, 16x16-pixel kernel in its default fp16 x 2 arithmetic; 4 keeps bf16 x 3)
WFMTS = [0, 1, 2, 3, 4, 5]
WFMT_IDS = ['f32', 'bf16x3', 'bf16x3-winograd', 'pw-bf16x3', 'bf16x3-winograd16', 'f16x2-winograd16']


def _skip_unless_format_applies(wfmt, taps, H=None, ups=False):
    if (taps == 9 and wfmt == 3) or (taps != 9 and wfmt in (1, 2, 4, 5)):
        pytest.skip('weight format does not apply to this kernel size')
    if wfmt in (4, 5) and (ups or H is None or H % 16):
        pytest.skip('the 16x16-pixel Winograd kernel does not take this shape')


def _fmt(wfmt):
    """test id 4 -> the real weight format (2) with the 16x16-pixel block shape forced"""
    if wfmt in (4, 5):
        from pix2latent_amd import _native as N, ops as O
        O.DEFAULT_FORM = N.FORM_WINO_ANY | (N.FORM_WINO_BF3 if wfmt == 4 else 0)
        return 2
    return wfmt


@pytest.fixture(autouse=True)
def _force_winograd_for_small_grids(dev):
    """the default only sends layers with >= 64 blocks per image to the Winograd kernel; the test
    shapes are small, so ask for it on every eligible shape (P2LConv.form, per launch: the
    8x16-pixel kernel here, the 16x16-pixel one under format id 4) and restore the default"""
    from pix2latent_amd import _native as N, ops as O
    O.DEFAULT_FORM = N.FORM_WINO_ANY | N.FORM_WINO_8X16
    yield
    O.DEFAULT_FORM = N.FORM_AUTO


@pytest.mark.parametrize('wfmt', WFMTS, ids=WFMT_IDS)
@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: '-'.join('%s%s' % (k, v) for k, v in c.items()))
def test_conv_fwd(dev, O, case, wfmt):
    """both weight formats must meet the SAME tolerance: bf16x3 is an fp32-equivalent
    arithmetic (include/p2l.h P2L_WFMT_BF16X3), not a reduced-precision mode"""
    from pix2latent_amd import _native as N
    _skip_unless_format_applies(wfmt, case['taps'], case['H'], case.get('ups', False))
    wfmt = _fmt(wfmt)
    g = torch.Generator().manual_seed(1)
    B, H, Cin, Cout, taps = case['B'], case['H'], case['Cin'], case['Cout'], case['taps']
    k = 3 if taps == 9 else 1
    ups = case.get('ups', False)
    Hin = H // 2 if ups else H
    x = torch.randn(B, Cin, Hin, Hin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    bias = torch.randn(Cout, generator=g) * 0.1 if case.get('bias') else None
    a = x
    pro, ps, pt = N.PRO_NONE, None, None
    if case.get('pro'):
        s = 0.5 + torch.rand(B, Cin, generator=g)
        t = torch.randn(B, Cin, generator=g) * 0.3
        a = x * s.view(B, Cin, 1, 1) + t.view(B, Cin, 1, 1)
        if case['pro'] == 'affine_relu':
            a = F.relu(a)
            pro = N.PRO_AFFINE_RELU
        else:
            pro = N.PRO_AFFINE
        ps, pt = s.to(dev), t.to(dev)
    if ups:
        a = F.interpolate(a, scale_factor=2, mode='nearest')
    ref = F.conv2d(a, w, None, padding=k // 2) * case.get('alpha', 1.0)
    if bias is not None:
        ref = ref + bias.view(1, -1, 1, 1)
    res_t = None
    if case.get('res') == 'same':
        r = torch.randn(B, Cout, H, H, generator=g)
        ref = ref + r
        res_t = nhwc(r, dev)
    elif case.get('res') == 'ups':
        r = torch.randn(B, Cout + 32, H // 2, H // 2, generator=g)      # channel-truncated + nearest x2
        ref = ref + F.interpolate(r[:, :Cout], scale_factor=2, mode='nearest')
        res_t = nhwc(r, dev)
    act = N.ACT_NONE
    if case.get('act') == 'relu':
        ref, act = F.relu(ref), N.ACT_RELU
    elif case.get('act') == 'tanh':
        ref, act = torch.tanh(ref), N.ACT_TANH
    mask_t = None
    if case.get('mask'):
        m = torch.randn(B, Cout, H, H, generator=g)
        ref = ref * (m > 0).float()
        mask_t = nhwc(m, dev)
    pool = {None: N.POOL_NONE, 'max': N.POOL_MAX, 'sum': N.POOL_SUM}[case.get('pool')]
    n_store = case.get('n_store')
    kc = 16 if taps == 9 else 32
    assert Cin % kc == 0
    wp = O.pack_conv_weight(w.to(dev), taps, Cout, Cin, wfmt=wfmt)
    y, yp = O.conv(nhwc(x, dev), wp, B, H, H, Cin, Cout, taps, wfmt=wfmt,
                   bias=bias.to(dev) if bias is not None else None, pro=pro, pro_s=ps, pro_t=pt,
                   pro_bstride=Cin if ps is not None else 0, ups=ups,
                   alpha=case.get('alpha', 1.0), act=act, pool=pool, res=res_t,
                   res_ups=case.get('res') == 'ups', mask=mask_t, n_store=n_store,
                   want_y=case.get('want_y', True), splitk=case.get('splitk'))
    torch.cuda.synchronize()
    tol = 2e-5
    if y is not None:
        got = nchw(y)
        exp = ref if n_store is None else ref[:, :n_store]
        assert relerr(got, exp) < tol, 'y'
    if pool:
        got = nchw(yp)
        exp = F.max_pool2d(ref, 2, 2) if case['pool'] == 'max' else F.avg_pool2d(ref, 2, 2) * 4
        assert relerr(got, exp) < tol, 'pooled'


@pytest.mark.parametrize('wfmt', WFMTS, ids=WFMT_IDS)
@pytest.mark.parametrize('Cin,Cout', [(64, 64), (128, 96)])
def test_conv_subpixel_forward_and_dgrad(dev, O, Cin, Cout, wfmt):
    _skip_unless_format_applies(wfmt, 9, None, True)
    """3x3 conv on a nearest-x2 upsampled input in sub-pixel form (ups=2) and its
    input-gradient (ups=3) against F.interpolate + F.conv2d and autograd."""
    from pix2latent_amd import _native as N
    g = torch.Generator().manual_seed(13)
    B, h = 2, 16
    x = torch.randn(B, Cin, h, h, generator=g)
    s = 0.5 + torch.rand(B, Cin, generator=g)
    t = torch.randn(B, Cin, generator=g) * 0.3
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(Cout, generator=g) * 0.1
    a = F.relu(x * s.view(B, Cin, 1, 1) + t.view(B, Cin, 1, 1)).requires_grad_(True)
    y_ref = F.conv2d(F.interpolate(a, scale_factor=2, mode='nearest'), w, bias, padding=1)
    dy = torch.randn(B, Cout, 2 * h, 2 * h, generator=g)
    y_ref.backward(dy)
    wsp = O.pack_conv_weight_subpix(w.to(dev), Cout, Cin, wfmt=wfmt)
    y, _ = O.conv(nhwc(x, dev), wsp, B, 2 * h, 2 * h, Cin, Cout, 9, bias=bias.to(dev), wfmt=wfmt,
                  pro=N.PRO_AFFINE_RELU, pro_s=s.to(dev), pro_t=t.to(dev), pro_bstride=Cin, ups=2)
    torch.cuda.synchronize()
    assert relerr(nchw(y), y_ref.detach()) < 2e-5
    wtsp = O.pack_conv_weight_subpix(w.to(dev), Cin, Cout, flip=True, wfmt=wfmt)
    da, _ = O.conv(nhwc(dy, dev), wtsp, B, 2 * h, 2 * h, Cout, Cin, 9, ups=3, wfmt=wfmt)
    torch.cuda.synchronize()
    assert relerr(nchw(da), a.grad) < 2e-5


def test_packed_weight_buffer_of_another_format_is_refused(dev, O):
    """VERDICT r5 #7 / ADVICE r4: the packed formats are not tagged on the device.  A sub-pixel launch
    of format P2L_WFMT_BF16X3W reads the fp16 x 2 image BEHIND the bf16 x 3 one, so a buffer packed by
    p2l_pack_conv_weight_subpix_bf3 (bf16 x 3 only) would be read past its end.  With the buffer length
    stated in P2LConv.w_floats (the wrappers always state it) the library refuses the call (P2L_EINVAL)
    and launches nothing; the properly packed buffer runs; w_floats = 0 keeps the unchecked contract."""
    from pix2latent_amd import _native as N
    g = torch.Generator().manual_seed(77)
    B, h, Cin, Cout = 2, 16, 64, 64
    x = nhwc(torch.randn(B, Cin, h, h, generator=g), dev)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)).to(dev)
    w_bf3 = O.pack_conv_weight_subpix(w, Cout, Cin, wfmt=N.WFMT_BF16X3)      # bf16 x 3 image only
    w_h2 = O.pack_conv_weight_subpix(w, Cout, Cin, wfmt=N.WFMT_BF16X3W)      # + fp16 x 2 image
    assert w_bf3.numel() < w_h2.numel() == N.lib().p2l_packed_subpix_weight_floats(Cout, Cin, N.WFMT_BF16X3W)
    with pytest.raises(N.NativeError, match='rc=-1'):
        O.conv(x, w_bf3, B, 2 * h, 2 * h, Cin, Cout, 9, ups=2, wfmt=N.WFMT_BF16X3W)
    y_ok, _ = O.conv(x, w_h2, B, 2 * h, 2 * h, Cin, Cout, 9, ups=2, wfmt=N.WFMT_BF16X3W)
    y_bf3, _ = O.conv(x, w_bf3, B, 2 * h, 2 * h, Cin, Cout, 9, ups=2, wfmt=N.WFMT_BF16X3)
    torch.cuda.synchronize()
    assert relerr(y_ok, y_bf3) < 2e-5
    # plain 3x3: a P2L_WFMT_BF16X3 buffer (no Winograd / fp16 x 2 images behind it) handed to a BF16X3W launch
    w3_bf3 = O.pack_conv_weight(w, 9, Cout, Cin, wfmt=N.WFMT_BF16X3)
    with pytest.raises(N.NativeError, match='rc=-1'):
        O.conv(x, w3_bf3, B, h, h, Cin, Cout, 9, wfmt=N.WFMT_BF16X3W)
    # and the input-gradient wrapper states the length too
    xs = nhwc(torch.randn(B, Cout, h, h, generator=g), dev)
    one = torch.ones(B, Cout, device=dev)
    with pytest.raises(N.NativeError, match='rc=-1'):
        O.conv_dgrad_arb(x, w3_bf3, B, h, h, Cin, Cout, 9, xs, one, one, Cout, wfmt=N.WFMT_BF16X3W)


@pytest.mark.parametrize('wfmt', WFMTS, ids=WFMT_IDS)
def test_conv_subpixel_dgrad_fused_arb(dev, O, wfmt):
    _skip_unless_format_applies(wfmt, 9, None, True)
    g = torch.Generator().manual_seed(14)
    B, C, Co, h = 2, 64, 64, 16
    x = torch.randn(B, C, h, h, generator=g, requires_grad=True)
    s = (0.5 + torch.rand(B, C, generator=g)).requires_grad_(True)
    t = (torch.randn(B, C, generator=g) * 0.3).requires_grad_(True)
    w = torch.randn(Co, C, 3, 3, generator=g) / math.sqrt(C * 9)
    dy = torch.randn(B, Co, 2 * h, 2 * h, generator=g)
    a = F.interpolate(F.relu(x * s.view(B, C, 1, 1) + t.view(B, C, 1, 1)), scale_factor=2, mode='nearest')
    F.conv2d(a, w, None, padding=1).backward(dy)
    wt = O.pack_conv_weight_subpix(w.to(dev), C, Co, flip=True, wfmt=wfmt)
    dx, ds, dt = O.conv_dgrad_arb(nhwc(dy, dev), wt, B, 2 * h, 2 * h, Co, C, 9, nhwc(x.detach(), dev),
                                  s.detach().to(dev), t.detach().to(dev), C, subpix=True, wfmt=wfmt)
    torch.cuda.synchronize()
    assert relerr(nchw(dx), x.grad) < 2e-5
    assert relerr(ds.cpu(), s.grad) < 5e-5
    assert relerr(dt.cpu(), t.grad) < 5e-5


@pytest.mark.parametrize('taps,Cin,Cout,H', [(9, 64, 128, 16), (1, 128, 64, 16), (9, 3, 64, 32), (9, 128, 3, 32)])
def test_conv_dgrad_matches_autograd(dev, O, taps, Cin, Cout, H):
    """the transpose_flip packing turns the same kernel into the input-gradient."""
    g = torch.Generator().manual_seed(2)
    k = 3 if taps == 9 else 1
    B = 2
    x = torch.randn(B, Cin, H, H, generator=g, requires_grad=True)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    dy = torch.randn(B, Cout, H, H, generator=g)
    F.conv2d(x, w, None, padding=k // 2).backward(dy)
    kc = 16 if taps == 9 else 32
    K_pad = (Cout + kc - 1) // kc * kc
    N_pad = (Cin + 31) // 32 * 32
    wt = O.pack_conv_weight(w.to(dev), taps, N_pad, K_pad, flip=True)
    dyp = torch.zeros(B, K_pad, H, H)
    dyp[:, :Cout] = dy
    dx, _ = O.conv(nhwc(dyp, dev), wt, B, H, H, K_pad, N_pad, taps)
    torch.cuda.synchronize()
    assert relerr(nchw(dx)[:, :Cin], x.grad) < 2e-5


@pytest.mark.parametrize('splitk', [1, 4], ids=['epilogue', 'splitk-finish'])
@pytest.mark.parametrize('wfmt', WFMTS, ids=WFMT_IDS)
@pytest.mark.parametrize('taps,ups,skip', [(9, False, None), (9, True, None), (1, False, 'same'),
                                           (1, False, 'ups')])
def test_conv_dgrad_fused_affine_relu_bwd(dev, O, taps, ups, skip, wfmt, splitk):
    """dgrad conv with the consumer's CBN+ReLU backward (and GenBlock shortcut gradient)
    fused into its epilogue - or, split over K, into the deterministic finish kernel - vs
    autograd through relu(x*s+t) -> (nearest x2) -> conv."""
    g = torch.Generator().manual_seed(12)
    B, C, Co, H = 3, 64, 128, 16           # x: [B,C,H,H] ; y: [B,Co,Ho,Ho]
    k = 3 if taps == 9 else 1
    Ho = 2 * H if ups else H
    x = torch.randn(B, C, H, H, generator=g, requires_grad=True)
    s = (0.5 + torch.rand(B, C, generator=g)).requires_grad_(True)
    t = (torch.randn(B, C, generator=g) * 0.3).requires_grad_(True)
    w = torch.randn(Co, C, k, k, generator=g) / math.sqrt(C * k * k)
    dy = torch.randn(B, Co, Ho, Ho, generator=g)
    a = F.relu(x * s.view(B, C, 1, 1) + t.view(B, C, 1, 1))
    if ups:
        a = F.interpolate(a, scale_factor=2, mode='nearest')
    F.conv2d(a, w, None, padding=k // 2).backward(dy)
    exp_dx = x.grad.clone()
    sk_t, skip_C = None, 0
    if skip == 'same':
        sk = torch.randn(B, C, H, H, generator=g)
        exp_dx = exp_dx + sk
        sk_t, skip_C = nhwc(sk, dev), C
    elif skip == 'ups':
        sk = torch.randn(B, C // 2, 2 * H, 2 * H, generator=g)
        exp_dx[:, :C // 2] += F.avg_pool2d(sk, 2, 2) * 4
        sk_t, skip_C = nhwc(sk, dev), C // 2
    _skip_unless_format_applies(wfmt, taps, Ho, False)
    wfmt = _fmt(wfmt)
    wt = O.pack_conv_weight(w.to(dev), taps, C, Co, flip=True, wfmt=wfmt)
    dx, ds, dt = O.conv_dgrad_arb(nhwc(dy, dev), wt, B, Ho, Ho, Co, C, taps, nhwc(x.detach(), dev),
                                  s.detach().to(dev), t.detach().to(dev), C, pool_sum=ups, wfmt=wfmt,
                                  skip=sk_t, skip_C=skip_C, skip_ups=(skip == 'ups'), splitk=splitk)
    torch.cuda.synchronize()
    assert relerr(nchw(dx), exp_dx) < 2e-5
    assert relerr(ds.cpu(), s.grad) < 5e-5
    assert relerr(dt.cpu(), t.grad) < 5e-5


@pytest.mark.parametrize('C,Co', [(128, 64), (256, 128), (512, 64), (64, 256)],
                         ids=['64to128', '128to256', '64to512', '256to64'])
@pytest.mark.parametrize('skip', [None, 'same', 'ups'])
def test_pointwise_bf16x3_dgrad_fused_affine_relu_bwd(dev, O, skip, C, Co):
    """the 1x1 input-gradient conv in the bf16x3 arithmetic (csrc/p2l_pw.hip) with the fused
    backward of relu(x*s+t) and the GenBlock shortcut gradient, 1 to 8 stages of 32 channels"""
    g = torch.Generator().manual_seed(14)
    B, H = 2, 32
    x = torch.randn(B, C, H, H, generator=g, requires_grad=True)
    s = (0.5 + torch.rand(B, C, generator=g)).requires_grad_(True)
    t = (torch.randn(B, C, generator=g) * 0.3).requires_grad_(True)
    w = torch.randn(Co, C, 1, 1, generator=g) / math.sqrt(C)
    dy = torch.randn(B, Co, H, H, generator=g)
    F.conv2d(F.relu(x * s.view(B, C, 1, 1) + t.view(B, C, 1, 1)), w).backward(dy)
    exp_dx = x.grad.clone()
    sk_t, skip_C = None, 0
    if skip == 'same':
        sk = torch.randn(B, C, H, H, generator=g)
        exp_dx = exp_dx + sk
        sk_t, skip_C = nhwc(sk, dev), C
    elif skip == 'ups':
        sk = torch.randn(B, C // 2, 2 * H, 2 * H, generator=g)
        exp_dx[:, :C // 2] += F.avg_pool2d(sk, 2, 2) * 4
        sk_t, skip_C = nhwc(sk, dev), C // 2
    wt = O.pack_conv_weight(w.to(dev), 1, C, Co, flip=True, wfmt=3)
    dx, ds, dt = O.conv_dgrad_arb(nhwc(dy, dev), wt, B, H, H, Co, C, 1, nhwc(x.detach(), dev),
                                  s.detach().to(dev), t.detach().to(dev), C, wfmt=3,
                                  skip=sk_t, skip_C=skip_C, skip_ups=(skip == 'ups'))
    torch.cuda.synchronize()
    assert relerr(nchw(dx), exp_dx) < 2e-5
    assert relerr(ds.cpu(), s.grad) < 5e-5
    assert relerr(dt.cpu(), t.grad) < 5e-5


def test_winograd_f16x2_scales(dev, O):
    """the fp16 x 2 arithmetic of the 16x16 Winograd kernel lives on per-image (activations) and
    per-layer (weights) power-of-two scales: images of wildly different magnitude in one launch
    (zeros, gradient-sized 1e-12, 1e+6, one with a 1e4 outlier pixel), tiny and huge weights --
    every image meets the tolerance of the fp32-grade kernels RELATIVE TO ITS OWN output, an
    all-zero image gives exact zeros, and no image's bits depend on what else is in the batch."""
    from pix2latent_amd import _native as N
    O.DEFAULT_FORM = N.FORM_WINO_ANY                  # 16x16 kernel, default (fp16 x 2) arithmetic
    g = torch.Generator().manual_seed(5)
    H, Cin, Cout = 32, 64, 64
    x = torch.randn(5, Cin, H, H, generator=g)
    x[0] = 0.0
    x[1] *= 1e-12
    x[2] *= 1e6
    x[3, 7, 11, 13] = 1e4
    x[4] = x[4].abs() * 3.0                           # (a ReLU-like image)
    for wscale in (1.0, 1e-4, 1e3):
        w = wscale * torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
        ref = F.conv2d(x.double(), w.double(), None, padding=1)
        wp = O.pack_conv_weight(w.to(dev), 9, Cout, Cin, wfmt=2)
        y, _ = O.conv(nhwc(x, dev), wp, 5, H, H, Cin, Cout, 9, wfmt=2)
        y = nchw(y).double()
        assert torch.isfinite(y).all()
        assert (y[0] == 0).all()
        for b in range(1, 5):
            err = (y[b] - ref[b]).abs().max().item() / ref[b].abs().max().item()
            assert err < 1e-5, (wscale, b, err)
        for b in (1, 3):
            y1, _ = O.conv(nhwc(x[b:b + 1], dev), wp, 1, H, H, Cin, Cout, 9, wfmt=2)
            assert torch.equal(nchw(y1)[0].double(), y[b]), 'result depends on the batch composition'
    # the same launch in the bf16 x 3 arithmetic: the two agree to fp32 rounding of the products
    O.DEFAULT_FORM = N.FORM_WINO_ANY | N.FORM_WINO_BF3
    y3, _ = O.conv(nhwc(x, dev), wp, 5, H, H, Cin, Cout, 9, wfmt=2)
    y3 = nchw(y3).double()
    for b in range(1, 5):
        assert (y3[b] - y[b]).abs().max().item() <= 1e-5 * ref[b].abs().max().item()


def test_winograd_f16x2_maxima_handed_over(dev, O):
    """P2LAmax: an (unsplit 16x16 Winograd) launch writes one partial maximum of |y| (and of the
    pooled |yp|) per block; the launch that reads the tensor takes its per-image power of two from
    them instead of running its own max-|x| pass.  The partials reduce to the exact per-image
    maxima; a consumer without prologue gives the same bits either way; with a fused prologue it
    scales by the bound max|s| max|x| + max|t| -- a different power of two at most, same values."""
    from pix2latent_amd import _native as N
    O.DEFAULT_FORM = N.FORM_WINO_ANY
    g = torch.Generator().manual_seed(9)
    B, H, C1, C2 = 3, 32, 64, 128
    x = torch.randn(B, C1, H, H, generator=g)
    x[1] *= 1e-5
    w1 = torch.randn(C2, C1, 3, 3, generator=g) / math.sqrt(9 * C1)
    w2 = torch.randn(C1, C2, 3, 3, generator=g) / math.sqrt(9 * C2)
    b1 = 0.1 * torch.randn(C2, generator=g)
    wp1 = O.pack_conv_weight(w1.to(dev), 9, C2, C1, wfmt=2)
    wp2 = O.pack_conv_weight(w2.to(dev), 9, C1, C2, wfmt=2)
    y, yp, (am, amp) = O.conv(nhwc(x, dev), wp1, B, H, H, C1, C2, 9, wfmt=2, bias=b1.to(dev), act=N.ACT_RELU,
                              pool=N.POOL_MAX, want_amax=True)
    assert am is not None and am.shape == (B, (H // 16) ** 2 * (C2 // 64) * 8)      # (one partial per wave)
    assert torch.equal(am.amax(dim=1), y.abs().amax(dim=(1, 2, 3)))
    assert torch.equal(amp.amax(dim=1), yp.abs().amax(dim=(1, 2, 3)))
    # consumer without prologue: bit-identical with and without the hand-over
    z0, _ = O.conv(y, wp2, B, H, H, C2, C1, 9, wfmt=2)
    z1, _ = O.conv(y, wp2, B, H, H, C2, C1, 9, wfmt=2, amax_in=am)
    assert torch.equal(z0, z1)
    ref = F.conv2d(F.relu(F.conv2d(x, w1, b1, padding=1)), w2, None, padding=1)
    assert relerr(nchw(z1), ref) < 2e-5
    # consumer with a fused affine + ReLU prologue: the bound replaces the exact maximum
    s = 0.5 + torch.rand(B, C2, generator=g)
    t = 0.3 * torch.randn(B, C2, generator=g)
    kw = dict(wfmt=2, pro=N.PRO_AFFINE_RELU, pro_s=s.to(dev), pro_t=t.to(dev), pro_bstride=C2)
    p0, _ = O.conv(y, wp2, B, H, H, C2, C1, 9, **kw)
    p1, _ = O.conv(y, wp2, B, H, H, C2, C1, 9, amax_in=am, **kw)
    assert (p0 - p1).abs().max().item() <= 1e-6 * p0.abs().max().item()
    # the pooled tensor feeds a conv at half resolution (16^2: the 16x16 kernel under WINO_ANY)
    q0, _ = O.conv(yp, wp2, B, H // 2, H // 2, C2, C1, 9, wfmt=2)
    q1, _ = O.conv(yp, wp2, B, H // 2, H // 2, C2, C1, 9, wfmt=2, amax_in=amp)
    assert torch.equal(q0, q1)
    # a pointwise (1x1) consumer takes the fp16 x 2 form when -- and only when -- the maxima come with
    # the tensor; without them it stays bf16 x 3; both fp32-grade
    w21 = torch.randn(C1, C2, 1, 1, generator=g) / math.sqrt(C2)
    wp21 = O.pack_conv_weight(w21.to(dev), 1, C1, C2, wfmt=3)
    for kwp in (dict(), dict(pro=N.PRO_AFFINE_RELU, pro_s=s.to(dev), pro_t=t.to(dev), pro_bstride=C2)):
        u0, _ = O.conv(y, wp21, B, H, H, C2, C1, 1, wfmt=3, **kwp)
        u1, _ = O.conv(y, wp21, B, H, H, C2, C1, 1, wfmt=3, amax_in=am, **kwp)
        yin = F.relu(F.conv2d(x, w1, b1, padding=1))
        if kwp:
            yin = F.relu(yin * s.view(B, C2, 1, 1) + t.view(B, C2, 1, 1))
        refu = F.conv2d(yin, w21)
        for bb in range(B):
            sc = refu[bb].abs().max().item()
            assert (nchw(u1)[bb] - refu[bb]).abs().max().item() < 2e-5 * sc
            assert (nchw(u0)[bb] - nchw(u1)[bb]).abs().max().item() < 1e-5 * sc
    # other producers: the kernels that end in the vector epilogue -- 1x1 (bf16x3 pointwise and exact
    # fp32), direct 3x3, sub-pixel (upsample-fused) 3x3 with its four output phases
    w11 = torch.randn(C2, C1, 1, 1, generator=g) / math.sqrt(C1)
    for wf in (3, 0):
        wp11 = O.pack_conv_weight(w11.to(dev), 1, C2, C1, wfmt=wf)
        y11, _, (am11, _) = O.conv(nhwc(x, dev), wp11, B, H, H, C1, C2, 1, wfmt=wf, bias=b1.to(dev), want_amax=True)
        assert am11 is not None and torch.equal(am11.amax(dim=1), y11.abs().amax(dim=(1, 2, 3)))
        r0, _ = O.conv(y11, wp2, B, H, H, C2, C1, 9, wfmt=2)
        r1, _ = O.conv(y11, wp2, B, H, H, C2, C1, 9, wfmt=2, amax_in=am11)
        assert torch.equal(r0, r1)
    wpd = O.pack_conv_weight(w1.to(dev), 9, C2, C1, wfmt=1)
    yd, _, (amd, _) = O.conv(nhwc(x, dev), wpd, B, H, H, C1, C2, 9, wfmt=1, act=N.ACT_RELU, want_amax=True,
                             splitk=1)   # (a split-K launch ends in the finish kernel: no maxima)
    assert amd is not None and torch.equal(amd.amax(dim=1), yd.abs().amax(dim=(1, 2, 3)))
    xs = torch.randn(B, C1, H // 2, H // 2, generator=g)
    yu, _, (amu, _) = O.conv(nhwc(xs, dev), wpd, B, H, H, C1, C2, 9, wfmt=1, ups=True, want_amax=True, splitk=1)
    if amu is not None:
        assert torch.equal(amu.amax(dim=1), yu.abs().amax(dim=(1, 2, 3)))
    # the three-channel image conv (first VGG conv) and the max-pool backward kernel leave theirs too
    x3 = torch.randn(B, 3, H, H, generator=g)
    w3 = torch.randn(C1, 3, 3, 3, generator=g) / math.sqrt(27)
    wp3 = O.pack_conv_weight(w3.to(dev), 9, C1, 16, wfmt=4)
    y3, _, (am3, _) = O.conv(_pad_c(x3, 16).to(dev), wp3, B, H, H, 16, C1, 9, wfmt=4, act=N.ACT_RELU, want_amax=True)
    assert am3 is not None and am3.shape[1] == (H // 8) * (H // 16) * 4
    assert torch.equal(am3.amax(dim=1), y3.abs().amax(dim=(1, 2, 3)))
    dyp = torch.randn(B, H // 2, H // 2, C2, generator=g).to(dev)
    ns = N.lib().p2l_maxpool2_bwd_amax_slots(H, H, C2)
    amm = torch.full((B, ns), -1.0, device=dev)
    dy = torch.empty(B, H, H, C2, device=dev)
    N.check(N.lib().p2l_maxpool2_bwd_amax(N.ptr(y), C2, N.ptr(dyp), C2, None, 0, N.ptr(dy), C2, B, H, H, C2, 1,
                                          N.ptr(amm), N.stream()), 'maxpool2_bwd_amax')
    assert torch.equal(amm.amax(dim=1), dy.abs().amax(dim=(1, 2, 3)))
    assert torch.equal(dy, O.maxpool2_bwd(y, dyp, relu_mask=True))


@pytest.mark.parametrize('shape', [(32, 256, 256, 2), (16, 512, 512, 4), (32, 512, 256, 2)],
                         ids=['32x32-256to256', '16x16-512to512', '32x32-512to256'])
def test_winograd_k_sliced_small_grid_layers(dev, O, shape):
    """small-grid 3x3 layers (16..63 blocks of 8x16x64 per image) run the 16x16 Winograd kernel
    with the input channels cut into slices -- a count that depends on the LAYER SHAPE only -- and
    the deterministic split-K finish kernel: same numbers as torch, forward and the input-gradient
    form with the fused activation backward; and a candidate's result does not depend on how many
    others share the launch (bit for bit)."""
    from pix2latent_amd import _native as N
    H, Cin, Cout, slices = shape
    O.DEFAULT_FORM = N.FORM_AUTO                      # the product's own choice for this shape
    d = N.P2LConv()
    d.B, d.H, d.W, d.Cin, d.Cout, d.taps, d.x_ld, d.wfmt, d.splitk = 3, H, H, Cin, Cout, 9, Cin, 2, 1
    assert N.lib().p2l_conv_suggest_splitk(C.byref(d)) == slices
    d.B = 18
    assert N.lib().p2l_conv_suggest_splitk(C.byref(d)) == slices      # ... whatever the batch
    g = torch.Generator().manual_seed(31)
    B = 3
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    bias = 0.1 * torch.randn(Cout, generator=g)
    s = 0.5 + torch.rand(B, Cin, generator=g)
    t = 0.3 * torch.randn(B, Cin, generator=g)
    ref = F.conv2d(F.relu(x * s.view(B, Cin, 1, 1) + t.view(B, Cin, 1, 1)), w, bias, padding=1)
    wp = O.pack_conv_weight(w.to(dev), 9, Cout, Cin, wfmt=2)
    y, _, (am, _) = O.conv(nhwc(x, dev), wp, B, H, H, Cin, Cout, 9, wfmt=2, bias=bias.to(dev),
                           pro=N.PRO_AFFINE_RELU, pro_s=s.to(dev), pro_t=t.to(dev), pro_bstride=Cin,
                           want_amax=True)
    assert relerr(nchw(y), ref) < 2e-5
    if slices > 1:      # (the finish kernel of a K-sliced launch leaves the maxima of what it wrote: P2LAmax)
        assert am is not None and torch.equal(am.amax(dim=1), y.abs().amax(dim=(1, 2, 3)))
    y1, _ = O.conv(nhwc(x[1:2], dev), wp, 1, H, H, Cin, Cout, 9, wfmt=2, bias=bias.to(dev),
                   pro=N.PRO_AFFINE_RELU, pro_s=s[1:2].to(dev), pro_t=t[1:2].to(dev), pro_bstride=Cin)
    assert torch.equal(y1[0], y[1]), 'result depends on the batch composition'
    # input-gradient form Cout -> Cin with the fused backward of relu(xa*s+t), K-sliced finish
    xa = torch.randn(B, Cin, H, H, generator=g, requires_grad=True)
    sa = (0.5 + torch.rand(B, Cin, generator=g)).requires_grad_(True)
    ta = (0.3 * torch.randn(B, Cin, generator=g)).requires_grad_(True)
    dy = torch.randn(B, Cout, H, H, generator=g)
    F.conv2d(F.relu(xa * sa.view(B, Cin, 1, 1) + ta.view(B, Cin, 1, 1)), w, None, padding=1).backward(dy)
    wt = O.pack_conv_weight(w.to(dev), 9, Cin, Cout, flip=True, wfmt=2)
    dd = N.P2LConv()
    dd.B, dd.H, dd.W, dd.Cin, dd.Cout, dd.taps, dd.x_ld, dd.wfmt, dd.splitk = B, H, H, Cout, Cin, 9, Cout, 2, 1
    sk = N.lib().p2l_conv_suggest_splitk(C.byref(dd))
    assert sk == N.lib().p2l_wino_split_factor(H, H, Cout, Cin)      # (1 for 32^2 256->512: a full-grid layer)
    dx, ds, dt = O.conv_dgrad_arb(nhwc(dy, dev), wt, B, H, H, Cout, Cin, 9, nhwc(xa.detach(), dev),
                                  sa.detach().to(dev), ta.detach().to(dev), Cin, wfmt=2, splitk=sk)
    torch.cuda.synchronize()
    assert relerr(nchw(dx), xa.grad) < 2e-5
    assert relerr(ds.cpu(), sa.grad) < 5e-5 and relerr(dt.cpu(), ta.grad) < 5e-5


def test_two_host_threads_two_streams_bit_identical(dev, O):
    """the library is re-entrant.  Two host threads drive the same conv layers (direct,
    Winograd 8x16 / 16x16, pointwise: the form travels in P2LConv) on two streams at the same time,
    with the (process-wide, mutex-guarded, opt-in) launch profiler running; every result equals
    the single-threaded one bit for bit and every launch of both threads got its own slot."""
    import threading
    from pix2latent_amd import _native as N
    g = torch.Generator().manual_seed(77)
    B, H = 4, 32
    cases = []
    for Cin, Cout, taps, wf, form in ((64, 128, 9, 1, 0), (64, 128, 9, 2, N.FORM_WINO_ANY | N.FORM_WINO_8X16),
                                      (64, 128, 9, 2, N.FORM_WINO_ANY), (128, 64, 1, 3, 0)):
        k = 3 if taps == 9 else 1
        x = torch.randn(B, H, H, Cin, generator=g).to(dev)
        w = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(k * k * Cin)).to(dev)
        cases.append((x, O.pack_conv_weight(w, taps, Cout, Cin, wfmt=wf), Cin, Cout, taps, wf, form))

    def run_all(reps):
        outs = []
        for _ in range(reps):
            outs = [O.conv(x, wp, B, H, H, Cin, Cout, taps, wfmt=wf, form=form)[0]
                    for x, wp, Cin, Cout, taps, wf, form in cases]
        return outs
    ref = [y.clone() for y in run_all(1)]
    torch.cuda.synchronize()
    results, errors = {}, []

    def worker(name):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                outs = run_all(20)
                st.synchronize()
            results[name] = [y.clone() for y in outs]
        except Exception as e:          # noqa: BLE001
            errors.append(e)
    N.check(N.lib().p2l_prof_begin(512), 'prof_begin')
    th = [threading.Thread(target=worker, args=('a',)), threading.Thread(target=worker, args=('b',))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    T = N.prof_end()
    f, m, c = T.flops, T.ms, T.count
    assert not errors, errors
    assert c[0] + c[1] == 2 * 20 * len(cases)
    for name in ('a', 'b'):
        for y, r in zip(results[name], ref):
            assert torch.equal(y, r)


@pytest.mark.parametrize('arb', [False, True], ids=['forward', 'dgrad-fused-arb'])
def test_winograd_block_shapes_bit_identical(dev, O, arb):
    """the 8x16-pixel / 4-wave and the 16x16-pixel / 8-wave Winograd kernels do the same
    additions and products in the same order when both run the bf16 x 3 arithmetic: not a single
    bit differs"""
    from pix2latent_amd import _native as N
    g = torch.Generator().manual_seed(21)
    B, H, Cin, Cout = 3, 32, 48, 128
    outs = []
    x = torch.randn(B, H, H, Cin, generator=g).to(dev)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).to(dev)
    s = (0.5 + torch.rand(B, Cout if arb else Cin, generator=g)).to(dev)
    t = (0.3 * torch.randn(B, Cout if arb else Cin, generator=g)).to(dev)
    bias = (0.1 * torch.randn(Cout, generator=g)).to(dev)
    res = torch.randn(B, H, H, Cout, generator=g).to(dev)
    xa = torch.randn(B, H, H, Cout, generator=g).to(dev)
    for form in (N.FORM_WINO_ANY | N.FORM_WINO_8X16, N.FORM_WINO_ANY | N.FORM_WINO_BF3, N.FORM_WINO_ANY):
        O.DEFAULT_FORM = form
        if not arb:
            wp = O.pack_conv_weight(w, 9, Cout, Cin, wfmt=2)
            y, _ = O.conv(x, wp, B, H, H, Cin, Cout, 9, wfmt=2, bias=bias, pro=N.PRO_AFFINE_RELU,
                          pro_s=s, pro_t=t, pro_bstride=Cin, res=res, alpha=0.5)
            outs.append((y.clone(),))
        else:
            # input-gradient form Cin -> Cout of a conv Cout -> Cin, fused backward of relu(xa*s+t)
            wt = O.pack_conv_weight(w.permute(1, 0, 2, 3).contiguous(), 9, Cout, Cin, flip=True, wfmt=2)
            dx, ds, dt = O.conv_dgrad_arb(x, wt, B, H, H, Cin, Cout, 9, xa, s, t, Cout, wfmt=2,
                                          skip=res, skip_C=Cout)
            outs.append((dx.clone(), ds.clone(), dt.clone()))
    torch.cuda.synchronize()
    for a, b, h in zip(*outs):
        assert torch.equal(a, b)
        # the 16x16 kernel's default arithmetic (fp16 x 2, per-image power-of-two scales) is a
        # different rounding of the same fp32-grade products
        assert (h - a).abs().max().item() <= 2e-5 * a.abs().max().item()


@pytest.mark.parametrize('H', [16, 128])
def test_arb_finish_deferred_group(dev, O, H):
    """p2l_arb_defer_begin/flush: the second reduction stage of several activation-backwards
    in ONE launch gives exactly what the per-layer launches give (H = 128: more partial rows than
    segments, both chains of a segment in use)."""
    from pix2latent_amd import _native as N
    g = torch.Generator().manual_seed(21)
    B = 2
    cases = []
    for C, Co, taps in ((64, 128, 9), (128, 64, 1), (96, 64, 1)):
        k = 3 if taps == 9 else 1
        x = torch.randn(B, H, H, C, generator=g).to(dev)
        s = (0.5 + torch.rand(B, C, generator=g)).to(dev)
        t = (0.3 * torch.randn(B, C, generator=g)).to(dev)
        w = torch.randn(Co, C, k, k, generator=g) / math.sqrt(C * k * k)
        dy = torch.randn(B, H, H, Co, generator=g).to(dev)
        wt = O.pack_conv_weight(w.to(dev), taps, C, Co, flip=True)
        cases.append((dy, wt, Co, C, taps, x, s, t))

    keep = []                      # partial buffers must outlive the deferred flush

    def run_all():
        return [O.conv_dgrad_arb(dy, wt, B, H, H, Co, C, taps, x, s, t, C, keep=keep)
                for dy, wt, Co, C, taps, x, s, t in cases]

    ref = run_all()
    torch.cuda.synchronize()
    N.lib().p2l_arb_defer_begin()
    try:
        got = run_all()            # ds / dt are not written yet
        N.check(N.lib().p2l_arb_defer_flush(N.stream()), 'arb_defer_flush')
    finally:
        N.lib().p2l_arb_defer_cancel()
    torch.cuda.synchronize()
    for (dx0, ds0, dt0), (dx1, ds1, dt1) in zip(ref, got):
        assert torch.equal(dx0, dx1) and torch.equal(ds0, ds1) and torch.equal(dt0, dt1)


def test_conv_profiler_sampling(dev, O):
    """p2l_prof_step(i, period): launch n of step i is timed iff n % period == i % period"""
    import ctypes as C
    from pix2latent_amd import _native as N
    lib = N.lib()
    x = torch.randn(1, 16, 16, 32, device=dev)
    w = O.pack_conv_weight(torch.randn(32, 32, 1, 1, device=dev), 1, 32, 32)
    N.check(lib.p2l_prof_begin(64), 'prof_begin')
    for step in range(4):
        N.check(lib.p2l_prof_step(step, 4), 'prof_step')
        for _ in range(8):
            O.conv(x, w, 1, 16, 16, 32, 32, 1)
    torch.cuda.synchronize()
    T = N.prof_end()
    f, m, c = T.flops, T.ms, T.count
    assert c[1] == 8 and c[0] == 0          # 4 steps x 8 launches, every 4th timed
    assert m[1] > 0 and f[1] == 8 * 2.0 * 16 * 16 * 32 * 32


@pytest.mark.parametrize('akm,bkm', [(False, False), (False, True), (True, False), (True, True)])
def test_gemm_layouts(dev, O, akm, bkm):
    g = torch.Generator().manual_seed(3)
    batch, M, Nn, K = 2, 256, 96, 80
    A = torch.randn(batch, M, K, generator=g)
    Bm = torch.randn(batch, Nn, K, generator=g)
    ref = torch.bmm(A, Bm.transpose(1, 2)) * 0.7
    Ad = (A.transpose(1, 2) if akm else A).contiguous().to(dev)
    Bd = (Bm.transpose(1, 2) if bkm else Bm).contiguous().to(dev)
    Cm = O.gemm(Ad, Bd, batch, M, Nn, K, a_kmajor=akm, b_kmajor=bkm, alpha=0.7)
    torch.cuda.synchronize()
    assert relerr(Cm.cpu(), ref) < 2e-5
    C2 = O.gemm(Ad, Bd, batch, M, Nn, K, a_kmajor=akm, b_kmajor=bkm, alpha=0.7, Cacc=Cm.clone())
    torch.cuda.synchronize()
    assert relerr(C2.cpu(), 2 * ref) < 2e-5


@pytest.mark.parametrize('akm,bkm', [(False, False), (True, True)])
def test_gemm_splitk(dev, O, akm, bkm):
    # deep K, few output tiles: the K range is split over blocks and summed in a fixed order
    from pix2latent_amd import _native as N
    import ctypes as C
    g = torch.Generator().manual_seed(5)
    batch, M, Nn, K = 2, 256, 64, 2048
    d = N.P2LGemm()
    d.batch, d.M, d.N, d.K = batch, M, Nn, K
    assert N.lib().p2l_gemm_ws_bytes(C.byref(d)) > 0
    A = torch.randn(batch, M, K, generator=g)
    Bm = torch.randn(batch, Nn, K, generator=g)
    ref = torch.bmm(A.double(), Bm.double().transpose(1, 2)) * 0.5
    Ad = (A.transpose(1, 2) if akm else A).contiguous().to(dev)
    Bd = (Bm.transpose(1, 2) if bkm else Bm).contiguous().to(dev)
    Cm = O.gemm(Ad, Bd, batch, M, Nn, K, a_kmajor=akm, b_kmajor=bkm, alpha=0.5)
    C1 = O.gemm(Ad, Bd, batch, M, Nn, K, a_kmajor=akm, b_kmajor=bkm, alpha=0.5)
    torch.cuda.synchronize()
    assert relerr(Cm.cpu().double(), ref) < 2e-5
    assert torch.equal(Cm, C1)                         # deterministic
    C2 = O.gemm(Ad, Bd, batch, M, Nn, K, a_kmajor=akm, b_kmajor=bkm, alpha=0.5, Cacc=Cm.clone())
    torch.cuda.synchronize()
    assert relerr(C2.cpu().double(), 2 * ref) < 2e-5


@pytest.mark.parametrize('Bn', [1, 9, 18, 24, 40])
def test_linear_fwd_bwd(dev, O, Bn):
    g = torch.Generator().manual_seed(4)
    K, Nn = 256, 1000  # Nn % 4 == 0
    x = torch.randn(Bn, K, generator=g)
    W = torch.randn(K, Nn, generator=g) / 16
    b = torch.randn(Nn, generator=g)
    y = O.linear_fwd(x.to(dev), W.to(dev), b.to(dev))
    assert relerr(y.cpu(), x @ W + b) < 1e-5
    dy = torch.randn(Bn, Nn, generator=g)
    dx = O.linear_bwd(dy.to(dev), W.to(dev))
    assert relerr(dx.cpu(), dy @ W.t()) < 1e-5
    dx2 = O.linear_bwd(dy.to(dev), W.to(dev), dx=dx.clone())
    assert relerr(dx2.cpu(), 2 * (dy @ W.t())) < 1e-5
    # a row's bits do not depend on the rows it shares a pass over W with (groups of 16 | 24 rows)
    r = Bn - 1
    assert torch.equal(O.linear_fwd(x[r:].to(dev), W.to(dev), b.to(dev))[0], y[r])
    assert torch.equal(O.linear_bwd(dy[r:].to(dev), W.to(dev))[0], dx[r])


@pytest.mark.parametrize('skip', [None, 'same', 'ups'])
def test_affine_relu_bwd(dev, O, skip):
    g = torch.Generator().manual_seed(5)
    B, C, H = 3, 128, 16
    x = torch.randn(B, C, H, H, generator=g, requires_grad=True)
    s = (0.5 + torch.rand(B, C, generator=g)).requires_grad_(True)
    t = (torch.randn(B, C, generator=g) * 0.3).requires_grad_(True)
    da = torch.randn(B, C, H, H, generator=g)
    a = F.relu(x * s.view(B, C, 1, 1) + t.view(B, C, 1, 1))
    a.backward(da)
    exp_dx = x.grad.clone()
    sk_t, skip_C = None, 0
    if skip == 'same':
        sk = torch.randn(B, C, H, H, generator=g)
        exp_dx = exp_dx + sk
        sk_t, skip_C = nhwc(sk, dev), C
    elif skip == 'ups':
        sk = torch.randn(B, C // 2, 2 * H, 2 * H, generator=g)
        add = F.avg_pool2d(sk, 2, 2) * 4
        exp_dx[:, :C // 2] += add
        sk_t, skip_C = nhwc(sk, dev), C // 2
    dx, ds, dt = O.affine_relu_bwd(nhwc(da, dev), nhwc(x.detach(), dev), s.detach().to(dev),
                                   t.detach().to(dev), C, skip=sk_t, skip_C=skip_C,
                                   skip_ups=(skip == 'ups'))
    torch.cuda.synchronize()
    assert relerr(nchw(dx), exp_dx) < 1e-5
    assert relerr(ds.cpu(), s.grad) < 2e-5
    assert relerr(dt.cpu(), t.grad) < 2e-5


def test_softmax_fwd_bwd(dev, O):
    g = torch.Generator().manual_seed(6)
    S = (torch.randn(2, 64, 1024, generator=g) * 5).requires_grad_(True)
    P = torch.softmax(S, -1)
    dP = torch.randn(2, 64, 1024, generator=g)
    P.backward(dP)
    Pd = O.softmax_fwd(S.detach().to(dev))
    assert relerr(Pd.cpu(), P.detach()) < 1e-5
    dS = O.softmax_bwd(Pd, dP.to(dev))
    assert relerr(dS.cpu(), S.grad) < 1e-4


def test_maxpool2_bwd(dev, O):
    g = torch.Generator().manual_seed(7)
    B, C, H = 2, 64, 16
    pre = torch.randn(B, C, H, H, generator=g, requires_grad=True)
    y = F.relu(pre)
    yp = F.max_pool2d(y, 2, 2)
    dyp = torch.randn_like(yp)
    add = torch.randn(B, C, H, H, generator=g)
    (yp * dyp).sum().backward(retain_graph=True)
    g_pool = pre.grad.clone()          # pool backward through relu mask
    pre.grad = None
    (y * add).sum().backward()
    exp = g_pool + pre.grad
    got = O.maxpool2_bwd(nhwc(y.detach(), dev), nhwc(dyp, dev), add=nhwc(add, dev), relu_mask=True)
    assert relerr(nchw(got), exp) < 1e-6


def test_adam_matches_torch(dev, O):
    g = torch.Generator().manual_seed(8)
    p0 = torch.randn(18 * 128, generator=g)
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=0.05)
    p = p0.clone().to(dev)
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    for step in range(1, 6):
        grad = torch.randn(18 * 128, generator=g) * (10.0 ** (-step))
        p_ref.grad = grad.clone()
        opt.step()
        O.adam_step(p, grad.to(dev), m, v, 0.05, step)
    assert (p.cpu() - p_ref.detach()).abs().max().item() < 1e-6


@pytest.mark.parametrize('h', [256, 128, 64, 32, 16])
def test_bilinear_adjoint(dev, O, h):
    g = torch.Generator().manual_seed(9)
    B, H = 2, 256
    wsrc = torch.rand(B, H, H, generator=g)
    m = torch.randn(B, 1, h, h, generator=g, requires_grad=True)
    up = F.interpolate(m, size=(H, H), mode='bilinear', align_corners=False)
    (up[:, 0] * wsrc).sum().backward()
    wt = O.bilinear_adjoint(wsrc.to(dev), h, h)
    assert relerr(wt.cpu(), m.grad[:, 0]) < 1e-5


@pytest.mark.parametrize('C', [64, 128, 256, 512])
def test_lpips_tap(dev, O, C):
    g = torch.Generator().manual_seed(10)
    B, h = 2, 16
    f = F.relu(torch.randn(B, C, h, h, generator=g)).requires_grad_(True)
    ft = F.relu(torch.randn(B, C, h, h, generator=g))
    lin = torch.rand(C, generator=g) / C
    wt = torch.rand(B, h, h, generator=g)
    wsum = torch.tensor([3.0, 5.0])

    def norm(a):
        return a / (torch.sqrt((a ** 2).sum(1, keepdim=True)) + 1e-10)
    d = ((norm(f) - norm(ft)) ** 2 * lin.view(1, C, 1, 1)).sum(1)
    loss = (d * wt).sum((1, 2)) / wsum
    gl = torch.tensor([0.7, -1.3])
    (loss * gl).sum().backward()
    nft = O.lpips_normalize(nhwc(ft, dev))
    assert relerr(nchw(nft), norm(ft)) < 1e-5
    got = O.lpips_tap_fwd(nhwc(f.detach(), dev), nft, lin.to(dev), wt.to(dev), wsum.to(dev))
    assert relerr(got.cpu(), loss.detach()) < 1e-5
    df = O.lpips_tap_bwd(nhwc(f.detach(), dev), nft, lin.to(dev), wt.to(dev), (gl / wsum).to(dev))
    assert relerr(nchw(df), f.grad) < 1e-4


@pytest.mark.parametrize('C', [64, 128, 256, 512])
def test_lpips_tap_pool_bwd(dev, O, C):
    """Round 5: the gradient of a VGG tap that relu -> 2x2 max pool follows, in ONE pass
    (p2l_lpips_tap_pool_bwd) = tap backward, then pool backward + ReLU mask (the two kernels of rounds 1-4)
    bit for bit, and = autograd of the torch composition; the partial maxima cover what was written.  (The only ties
    in this data are quads of ReLU zeros, and the f > 0 mask erases whichever pixel won them: the first-maximum rule
    is pinned with equal POSITIVE maxima in tests/test_loss_kernels_gpu.py.)"""
    g = torch.Generator().manual_seed(12)
    B, h = 3, 32
    pre = torch.randn(B, C, h, h, generator=g).requires_grad_(True)     # conv output before the ReLU
    ft = F.relu(torch.randn(B, C, h, h, generator=g))
    lin = torch.rand(C, generator=g) / C
    wt = torch.rand(B, h, h, generator=g)
    gs = torch.tensor([0.7, -1.3, 0.4])
    dyp = torch.randn(B, C, h // 2, h // 2, generator=g)

    def norm(a):
        return a / (torch.sqrt((a ** 2).sum(1, keepdim=True)) + 1e-10)
    f = F.relu(pre)
    d = ((norm(f) - norm(ft)) ** 2 * lin.view(1, C, 1, 1)).sum(1)
    ((d * wt).sum((1, 2)) * gs).sum().backward(retain_graph=True)
    (F.max_pool2d(f, 2) * dyp).sum().backward()
    fd = nhwc(f.detach(), dev)
    nft = O.lpips_normalize(nhwc(ft, dev))
    args = (fd, nft, lin.to(dev), wt.to(dev), gs.to(dev))
    two = O.maxpool2_bwd(fd, nhwc(dyp, dev), add=O.lpips_tap_bwd(*args), relu_mask=True)
    one, am = O.lpips_tap_pool_bwd(*args, nhwc(dyp, dev), want_amax=True)
    assert torch.equal(one, two), 'the one-pass form differs from tap backward + pool backward'
    assert relerr(nchw(one), pre.grad) < 1e-4
    assert bool((am >= 0).all()), 'a promised maxima slot was not written'
    assert torch.equal(am.amax(dim=1), one.abs().amax(dim=(1, 2, 3)))
    # wrong geometry is refused, not computed
    from pix2latent_amd import _native as N
    with pytest.raises(N.NativeError):
        O.lpips_tap_pool_bwd(fd[:, :31].contiguous(), nft, lin.to(dev), wt.to(dev), gs.to(dev), nhwc(dyp, dev))


def test_affine_grid_sample_kernel(dev):
    """fused affine-grid + bilinear grid-sample vs the two torch ops the reference calls"""
    from pix2latent_amd.transform import SpatialTransform
    g = torch.Generator().manual_seed(15)
    ims = torch.rand(4, 3, 64, 64, generator=g) * 2 - 1
    t = torch.tensor([[1.0, 0.0, 0.0], [0.8, 0.1, -0.2], [1.3, -0.25, 0.15], [0.6, 0.4, 0.4]])
    st = SpatialTransform()
    ref_f, ref_i = st.transform(ims, t), st.invert_transform(ims, t)
    got_f, got_i = st.transform(ims.to(dev), t.to(dev)), st.invert_transform(ims.to(dev), t.to(dev))
    # interpolation weights come from coordinates of magnitude ~W: fp32 rounding ~1e-5
    assert (got_f.cpu() - ref_f).abs().max().item() < 5e-5
    assert (got_i.cpu() - ref_i).abs().max().item() < 5e-5


def test_conv_non_pow2_grid(dev, O):
    """grid that is not a multiple of the 8x16 tile (partial border tiles)"""
    g = torch.Generator().manual_seed(16)
    B, C, Co, H = 2, 32, 64, 24
    x = torch.randn(B, C, H, H, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / math.sqrt(C * 9)
    bias = torch.randn(Co, generator=g) * 0.1
    y, _ = O.conv(nhwc(x, dev), O.pack_conv_weight(w.to(dev), 9, Co, C), B, H, H, C, Co, 9,
                  bias=bias.to(dev), splitk=1)
    torch.cuda.synchronize()
    assert relerr(nchw(y), F.conv2d(x, w, bias, padding=1)) < 2e-5


def test_styled_conv_epilogue_terms(dev, O):
    """StyleGAN2 styled conv: modulation prologue, demod scale, noise, bias, lrelu*sqrt2"""
    from pix2latent_amd import _native as N
    g = torch.Generator().manual_seed(17)
    B, C, Co, H = 2, 64, 64, 16
    x = torch.randn(B, C, H, H, generator=g)
    s = 0.5 + torch.rand(B, C, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / math.sqrt(C * 9)
    d = 0.5 + torch.rand(B, Co, generator=g)
    noise = torch.randn(B, 1, H, H, generator=g)
    bias = torch.randn(Co, generator=g) * 0.1
    ref = F.conv2d(x * s.view(B, C, 1, 1), w, None, padding=1) * d.view(B, Co, 1, 1) + 0.3 * noise + bias.view(1, -1, 1, 1)
    ref = F.leaky_relu(ref, 0.2) * math.sqrt(2)
    y, _ = O.conv(nhwc(x, dev), O.pack_conv_weight(w.to(dev), 9, Co, C), B, H, H, C, Co, 9,
                  bias=bias.to(dev), pro=N.PRO_AFFINE, pro_s=s.to(dev), pro_t=torch.zeros(B, C, device=dev),
                  pro_bstride=C, act=N.ACT_LRELU_SQRT2, oscale=d.to(dev),
                  noise=noise.view(B, H * H).contiguous().to(dev), noise_w=0.3, splitk=1)
    torch.cuda.synchronize()
    assert relerr(nchw(y), ref) < 2e-5


@pytest.mark.parametrize('h,Cin,Cout', [(8, 64, 64), (16, 128, 64), (4, 64, 64)])
def test_transposed_conv_subpixel(dev, O, h, Cin, Cout):
    """stride-2 transposed 3x3 conv (StyleGAN2 up-conv) as 4 phase convs on the low-res grid
    of h+1 points (ups=2, ext=1) and its input-gradient (ups=3, ext=1)."""
    g = torch.Generator().manual_seed(18)
    B = 2
    x = torch.randn(B, Cin, h, h, generator=g, requires_grad=True)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    u_ref = F.conv_transpose2d(x, w.transpose(0, 1), stride=2)            # [B,Cout,2h+1,2h+1]
    du = torch.randn_like(u_ref)
    u_ref.backward(du)
    H = 2 * h
    wsp = O.pack_conv_weight_subpix(w.to(dev), Cout, Cin, mode=1)
    u, _ = O.conv(nhwc(x.detach(), dev), wsp, B, H, H, Cin, Cout, 9, ups=2, ext=1, splitk=1)
    torch.cuda.synchronize()
    got = nchw(u)
    assert got.shape[-1] == H + 2
    assert relerr(got[:, :, :H + 1, :H + 1], u_ref.detach()) < 2e-5
    assert got[:, :, H + 1].abs().max().item() == 0.0 and got[:, :, :, H + 1].abs().max().item() == 0.0
    dup = torch.zeros(B, Cout, H + 2, H + 2)
    dup[:, :, :H + 1, :H + 1] = du
    wtsp = O.pack_conv_weight_subpix(w.to(dev), Cin, Cout, flip=True, mode=1)
    dx, _ = O.conv(nhwc(dup, dev), wtsp, B, H, H, Cout, Cin, 9, ups=3, ext=1, splitk=1)
    torch.cuda.synchronize()
    assert relerr(nchw(dx), x.grad) < 2e-5


@pytest.mark.parametrize('B,h,Cin,Cout', [(2, 8, 64, 64), (3, 16, 128, 64), (2, 32, 64, 128), (9, 4, 64, 64),
                                          (1, 64, 32, 32)])
def test_transposed_conv_fp16x2_skips_its_zero_taps_bit_identically(dev, O, B, h, Cin, Cout):
    """The fp16 x 2 sub-pixel kernel on the weights of a stride-2 transposed conv (ext = 1): 7 of the 16 (phase,
    window tap) slabs are zero by construction (pack_subpix_kernel mode 1) and their products are skipped -- 9 matrix
    products per 2x2 output quad instead of 16.  Same bits as multiplying them (P2L_FORM_NO_SP_SKIP), forward and
    input gradient, K slices included; and right against F.conv_transpose2d / autograd."""
    from pix2latent_amd import _native as N
    g = torch.Generator().manual_seed(B * 100 + h)
    x = torch.randn(B, Cin, h, h, generator=g, requires_grad=True)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    u_ref = F.conv_transpose2d(x, w.transpose(0, 1), stride=2)
    du = torch.randn_like(u_ref)
    u_ref.backward(du)
    H = 2 * h
    wsp = O.pack_conv_weight_subpix(w.to(dev), Cout, Cin, mode=1, wfmt=2)
    wtsp = O.pack_conv_weight_subpix(w.to(dev), Cin, Cout, flip=True, mode=1, wfmt=2)
    dup = torch.zeros(B, Cout, H + 2, H + 2)
    dup[:, :, :H + 1, :H + 1] = du
    xd, dud = nhwc(x.detach(), dev), nhwc(dup, dev)
    outs = {}
    for form in (0, N.FORM_SP_PAIR, N.FORM_NO_SP_SKIP | N.FORM_SP_PAIR, N.FORM_NO_SP_PAIR, N.FORM_NO_SP_SKIP | N.FORM_NO_SP_PAIR):
        # (FORM_NO_SP_PAIR: one output phase per block of the forward launch instead of two on one staged patch)
        (u, _), mm_f = _mfma_products(N, lambda: O.conv(xd, wsp, B, H, H, Cin, Cout, 9, ups=2, ext=1, splitk=1, wfmt=2,
                                                     form=form))
        dxs = []
        for sk in (1, None):               # (None: the shape's own slice count -- 8^2 ... 32^2 gradients are sliced)
            (dx, _), mm_b = _mfma_products(N, lambda: O.conv(dud, wtsp, B, H, H, Cout, Cin, 9, ups=3, ext=1,
                                                           splitk=sk, wfmt=2, form=form))
            dxs.append(dx)
        torch.cuda.synchronize()
        assert abs(mm_f - 3) < 1e-6 and abs(mm_b - 3) < 1e-6       # the fp16 x 2 arithmetic ran
        outs[form] = (u, dxs[0], dxs[1])
    for form in outs:
        for a, b in zip(outs[0], outs[form]):
            assert torch.equal(a, b), form
    u, dx, dx_sliced = outs[0]
    assert relerr(nchw(u)[:, :, :H + 1, :H + 1], u_ref.detach()) < 2e-5
    assert relerr(nchw(dx), x.grad) < 2e-5 and relerr(nchw(dx_sliced), x.grad) < 2e-5


# ---- 3-channel image convs (csrc/p2l_thin.hip, P2L_WFMT_BF16X3T) --------------------------------
def _pad_c(x, C):
    """[B,c,H,W] -> NHWC with the channels zero-padded to C"""
    B, c, H, W = x.shape
    out = torch.zeros(B, H, W, C)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out


@pytest.mark.parametrize('B,H,Cout', [(2, 32, 64), (3, 64, 128), (1, 16, 96)])
def test_thin_input_conv(dev, O, B, H, Cout):
    """first VGG conv form: 3 real input channels (stored as 16), LPIPS scaling layer as the
    prologue, bias + ReLU + 2x2 max pool: 27 tap-channel products as one K dimension"""
    from pix2latent_amd import _native as N
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, 3, H, H, generator=g)
    w = torch.randn(Cout, 3, 3, 3, generator=g) / math.sqrt(27)
    bias = torch.randn(Cout, generator=g) * 0.1
    s16, t16 = torch.zeros(16), torch.zeros(16)
    s16[:3] = 0.5 + torch.rand(3, generator=g)
    t16[:3] = torch.randn(3, generator=g) * 0.3
    ref = F.relu(F.conv2d(x * s16[:3].view(1, 3, 1, 1) + t16[:3].view(1, 3, 1, 1), w, bias, padding=1))
    wp = O.pack_conv_weight(w.to(dev), 9, Cout, 16, wfmt=4)
    y, yp = O.conv(_pad_c(x, 16).to(dev), wp, B, H, H, 16, Cout, 9, wfmt=4, bias=bias.to(dev),
                   pro=N.PRO_AFFINE, pro_s=s16.to(dev), pro_t=t16.to(dev), pro_bstride=0,
                   act=N.ACT_RELU, pool=N.POOL_MAX)
    torch.cuda.synchronize()
    assert relerr(nchw(y), ref) < 2e-5
    assert relerr(nchw(yp), F.max_pool2d(ref, 2, 2)) < 2e-5


@pytest.mark.parametrize('skip', [None, 'same'])
def test_thin_input_dgrad_fused_affine_relu_bwd(dev, O, skip):
    """conv_to_rgb input gradient: dY has 3 real channels, the result 128, with the backward of
    relu(x*s+t) fused into the epilogue (per-tile partial sums reduced across the 4 waves)"""
    g = torch.Generator().manual_seed(32)
    B, C, H = 2, 128, 32
    x = torch.randn(B, C, H, H, generator=g, requires_grad=True)
    s = (0.5 + torch.rand(B, C, generator=g)).requires_grad_(True)
    t = (torch.randn(B, C, generator=g) * 0.3).requires_grad_(True)
    w = torch.randn(3, C, 3, 3, generator=g) / math.sqrt(C * 9)
    dy = torch.randn(B, 3, H, H, generator=g)
    F.conv2d(F.relu(x * s.view(B, C, 1, 1) + t.view(B, C, 1, 1)), w, None, padding=1).backward(dy)
    exp_dx = x.grad.clone()
    sk_t, skip_C = None, 0
    if skip == 'same':
        sk = torch.randn(B, C, H, H, generator=g)
        exp_dx = exp_dx + sk
        sk_t, skip_C = nhwc(sk, dev), C
    wt = O.pack_conv_weight(w.to(dev), 9, C, 16, flip=True, wfmt=4)
    dx, ds, dt = O.conv_dgrad_arb(_pad_c(dy, 16).to(dev), wt, B, H, H, 16, C, 9, nhwc(x.detach(), dev),
                                  s.detach().to(dev), t.detach().to(dev), C, wfmt=4, skip=sk_t,
                                  skip_C=skip_C)
    torch.cuda.synchronize()
    assert relerr(nchw(dx), exp_dx) < 2e-5
    assert relerr(ds.cpu(), s.grad) < 5e-5
    assert relerr(dt.cpu(), t.grad) < 5e-5


@pytest.mark.parametrize('B,H,Cin', [(2, 32, 128), (3, 64, 64), (1, 16, 48)])
def test_thin_output_conv_and_dgrad(dev, O, B, H, Cin):
    """conv_to_rgb form (CBN+ReLU prologue, bias, tanh, 3 of 16 stored channels) and the first
    VGG conv's input gradient (64 -> 3): pointwise product onto 27 columns + 9-tap gather"""
    from pix2latent_amd import _native as N
    g = torch.Generator().manual_seed(33)
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(3, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    b32 = torch.zeros(32)
    b32[:3] = torch.randn(3, generator=g) * 0.1
    s = 0.5 + torch.rand(B, Cin, generator=g)
    t = torch.randn(B, Cin, generator=g) * 0.3
    a = F.relu(x * s.view(B, Cin, 1, 1) + t.view(B, Cin, 1, 1))
    ref = torch.tanh(F.conv2d(a, w, None, padding=1) * 0.7 + b32[:3].view(1, 3, 1, 1))
    wp = O.pack_conv_weight(w.to(dev), 9, 32, Cin, wfmt=4)
    y, _ = O.conv(nhwc(x, dev), wp, B, H, H, Cin, 32, 9, wfmt=4, bias=b32.to(dev), alpha=0.7,
                  pro=N.PRO_AFFINE_RELU, pro_s=s.to(dev), pro_t=t.to(dev), pro_bstride=Cin,
                  act=N.ACT_TANH, n_store=16, y_ld=16)
    torch.cuda.synchronize()
    got = nchw(y)
    assert relerr(got[:, :3], ref) < 2e-5
    assert got[:, 3:].abs().max().item() == 0.0
    # input gradient of a conv 3 -> Cin: dY [B,Cin,H,H] -> d img [B,3,H,H]
    wf = torch.randn(Cin, 3, 3, 3, generator=g) / math.sqrt(27)
    img = torch.randn(B, 3, H, H, generator=g, requires_grad=True)
    dy = torch.randn(B, Cin, H, H, generator=g)
    F.conv2d(img, wf, None, padding=1).backward(dy)
    wt = O.pack_conv_weight(wf.to(dev), 9, 32, Cin, flip=True, wfmt=4)
    di, _ = O.conv(nhwc(dy, dev), wt, B, H, H, Cin, 32, 9, wfmt=4, n_store=16, y_ld=16)
    torch.cuda.synchronize()
    assert relerr(nchw(di)[:, :3], img.grad) < 2e-5


@pytest.mark.parametrize('shape', [(2, 3, 32, 32), (1, 2, 24, 40), (3, 1, 64, 48)])
def test_affine_grid_sample_backward(dev, shape):
    """p2l_affine_grid_sample_bwd: d src (gather-form adjoint) and d theta of the fused warp against
    autograd through the two torch ops the reference calls (F.affine_grid + F.grid_sample,
    /root/reference pix2latent/transform/spatial_transform.py:69-104) on the CPU in fp64 -- scale +
    shift as SpatialTransform builds them, and general matrices (rotation / shear / out-of-range
    shifts: zero padding on every side)."""
    from pix2latent_amd.transform.spatial_transform import _warp, SpatialTransform
    g = torch.Generator().manual_seed(17)
    B, C, H, W = shape
    x = torch.randn(B, C, H, W, generator=g)
    probe = torch.randn(B, C, H, W, generator=g)
    thetas = []
    st = SpatialTransform()
    # (no identity: there every sample sits exactly ON a pixel centre, the kink of the bilinear kernel,
    #  and which one-sided derivative d theta gets is decided by the last bit of ix)
    t = torch.tensor([[1.3, 0.2, -0.1], [0.7, -0.4, 0.3], [1.07, 0.03, -0.05]])[:B]
    thetas.append(st._theta(t[:, 0], t[:, 1:]))
    thetas.append(torch.eye(2, 3).unsqueeze(0).repeat(B, 1, 1) + 0.35 * torch.randn(B, 2, 3, generator=g))
    for theta in thetas:
        xr = x.double().requires_grad_(True)
        tr = theta.double().requires_grad_(True)
        ref = F.grid_sample(xr, F.affine_grid(tr, [B, C, H, W], align_corners=False), align_corners=False)
        (ref * probe.double()).sum().backward()
        xd = x.to(dev).requires_grad_(True)
        td = theta.to(dev).requires_grad_(True)
        out = _warp(xd, td)
        (out * probe.to(dev)).sum().backward()
        torch.cuda.synchronize()
        assert relerr(out.detach().cpu(), ref.detach()) < 1e-5
        assert relerr(xd.grad.cpu(), xr.grad) < 1e-5
        # d theta sums B*C*H*W products whose per-pixel sign changes at every cell border: compare
        # against the fp64 value with an fp32-accumulation tolerance
        assert relerr(td.grad.cpu(), tr.grad) < 2e-4, (td.grad.cpu(), tr.grad)
        # only the image is differentiable / only theta
        x2 = x.to(dev).requires_grad_(True)
        _warp(x2, theta.to(dev)).mul(probe.to(dev)).sum().backward()
        assert torch.equal(x2.grad, xd.grad)
        t2 = theta.to(dev).requires_grad_(True)
        _warp(x.to(dev), t2).mul(probe.to(dev)).sum().backward()
        assert torch.equal(t2.grad, td.grad)


def test_invertibility_loss_runs_native_on_the_device(dev):
    """loss_functions.invertibility_loss (/root/reference pix2latent/loss_functions.py:30-38)
    differentiates through transform + invert_transform: both warps and both backward passes are
    the native kernels (no ATen grid_sampler in the graph)"""
    import pix2latent_amd.loss_functions as LF
    from pix2latent_amd.transform.spatial_transform import SpatialTransform, _WarpFn
    g = torch.Generator().manual_seed(3)
    ims = torch.randn(2, 3, 32, 32, generator=g)
    t = torch.tensor([[1.2, 0.1, -0.2], [0.9, 0.0, 0.15]])
    st = SpatialTransform()
    ims_d = ims.to(dev).requires_grad_(True)
    out = st.invert_transform(st.transform(ims_d, t.to(dev)), t.to(dev))
    names = []
    fn = out.grad_fn
    while fn is not None and len(names) < 8:
        names.append(type(fn).__name__)
        fn = fn.next_functions[0][0] if fn.next_functions else None
    assert names[0].startswith('_WarpFn') and not any('GridSampler' in n for n in names), names
    out.sum().backward()
    ims_c = ims.double().requires_grad_(True)
    ref = st.invert_transform(st.transform(ims_c, t.double()), t.double())
    ref.sum().backward()
    assert relerr(out.detach().cpu(), ref.detach()) < 1e-5 and relerr(ims_d.grad.cpu(), ims_c.grad) < 1e-5


def _mfma_products(N, fn):
    """run fn() under the launch profiler -> 16-bit MFMA products per fp32 product of its 3x3 launches
    (6 = bf16 x 3, 3 = fp16 x 2)"""
    lib = N.lib()
    N.check(lib.p2l_prof_begin(64), 'p2l_prof_begin')
    lib.p2l_prof_step(0, 1)
    out = fn()
    torch.cuda.synchronize()
    T = N.prof_end()
    assert T.count[0] >= 1
    return out, T.mfma_flops[0] / T.exec_flops[0]


H2_DIRECT_CASES = [
    # (the Winograd kernel takes none of these: H not a multiple of 16 / sub-pixel / small grids in split-K slices)
    dict(B=2, H=24, Cin=64, Cout=64, pro='affine_relu', bias=True, splitk=1),      # partial tiles (never split)
    dict(B=3, H=8, Cin=256, Cout=64, bias=True, res='same', alpha=0.5),            # two images per tile, split-K
    dict(B=5, H=4, Cin=128, Cout=128, pro='affine', act='relu'),                    # eight images per tile
    dict(B=2, H=48, Cin=32, Cout=32, act='relu', pool='max'),                       # BN = 32
    dict(B=2, H=40, Cin=48, Cout=96, act='relu', splitk=1),                         # partial tiles
    dict(B=2, H=16, Cin=512, Cout=64, splitk=1),                                    # forced unsplit, one image per tile
]


@pytest.mark.parametrize('case', H2_DIRECT_CASES, ids=lambda c: '-'.join('%s%s' % kv for kv in c.items()))
def test_direct_kernel_fp16x2(dev, O, case):
    """conv_h2_kernel (csrc/p2l_h2.hip): the direct 3x3 kernel in the fp16 x 2 arithmetic -- default for
    every P2L_WFMT_BF16X3W launch the Winograd kernel does not take -- against torch in fp64 at the
    tolerance of the fp32-grade kernels, next to the bf16 x 3 form of the same launch
    (P2L_FORM_WINO_BF3); the launch profiler confirms which arithmetic ran."""
    from pix2latent_amd import _native as N
    g = torch.Generator().manual_seed(21)
    B, H, Cin, Cout = case['B'], case['H'], case['Cin'], case['Cout']
    x = torch.randn(B, Cin, H, H, generator=g)
    x[0] *= 1e-6                                        # images of very different magnitude in one launch
    if B > 2:
        x[2] *= 3e4
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    bias = 0.1 * torch.randn(Cout, generator=g) if case.get('bias') else None
    kw = dict(wfmt=2)
    a = x.double()
    if case.get('pro'):
        s = 0.5 + torch.rand(B, Cin, generator=g)
        t = 0.3 * torch.randn(B, Cin, generator=g) * x.abs().amax(dim=(1, 2, 3)).view(B, 1)
        a = a * s.double().view(B, Cin, 1, 1) + t.double().view(B, Cin, 1, 1)
        if case['pro'] == 'affine_relu':
            a = F.relu(a)
        kw.update(pro=N.PRO_AFFINE_RELU if case['pro'] == 'affine_relu' else N.PRO_AFFINE,
                  pro_s=s.to(dev), pro_t=t.to(dev), pro_bstride=Cin)
    alpha = case.get('alpha', 1.0)
    ref = alpha * F.conv2d(a, w.double(), None, padding=1)
    if bias is not None:
        ref = ref + bias.double().view(1, Cout, 1, 1)
        kw['bias'] = bias.to(dev)
    if case.get('res'):
        r = torch.randn(B, Cout, H, H, generator=g) * ref.abs().amax(dim=(1, 2, 3)).view(B, 1, 1, 1).float()
        ref = ref + r.double()
        kw['res'] = nhwc(r, dev)
    if case.get('act') == 'relu':
        ref = F.relu(ref)
        kw['act'] = N.ACT_RELU
    if case.get('pool') == 'max':
        kw['pool'] = N.POOL_MAX
    if 'splitk' in case:
        kw['splitk'] = case['splitk']
    kw['alpha'] = alpha
    wp = O.pack_conv_weight(w.to(dev), 9, Cout, Cin, wfmt=2)
    xs = nhwc(x, dev)
    O.DEFAULT_FORM = N.FORM_NO_WINO
    (y, yp), mm = _mfma_products(N, lambda: O.conv(xs, wp, B, H, H, Cin, Cout, 9, **kw))
    assert abs(mm - 3.0) < 1e-6, 'expected the fp16 x 2 kernel, got %g products' % mm
    O.DEFAULT_FORM = N.FORM_NO_WINO | N.FORM_WINO_BF3
    (y3, _), mm3 = _mfma_products(N, lambda: O.conv(xs, wp, B, H, H, Cin, Cout, 9, **kw))
    assert abs(mm3 - 6.0) < 1e-6
    y, y3 = nchw(y).double(), nchw(y3).double()
    for b in range(B):
        sc = ref[b].abs().max().item()
        assert (y[b] - ref[b]).abs().max().item() < 2e-5 * sc, (b, (y[b] - ref[b]).abs().max().item() / sc)
        assert (y3[b] - y[b]).abs().max().item() < 2e-5 * sc
    if yp is not None:
        assert relerr(nchw(yp), F.max_pool2d(ref, 2)) < 2e-5
    # a candidate's bits do not depend on who shares its launch (same split-K request)
    kw1 = dict(kw)
    for key in ('pro_s', 'pro_t', 'res'):
        if key in kw1:
            kw1[key] = kw1[key][1:2].contiguous()
    if 'splitk' not in kw1:
        d = N.P2LConv()
        d.B, d.H, d.W, d.Cin, d.Cout, d.taps, d.wfmt, d.x_ld = B, H, H, Cin, Cout, 9, 2, Cin
        d.n_store = d.y_ld = Cout
        d.form = N.FORM_NO_WINO
        kw1['splitk'] = N.lib().p2l_conv_suggest_splitk(C.byref(d))
    O.DEFAULT_FORM = N.FORM_NO_WINO
    ya, _ = O.conv(xs, wp, B, H, H, Cin, Cout, 9, **dict(kw, splitk=kw1['splitk']))
    y1, _ = O.conv(xs[1:2].contiguous(), wp, 1, H, H, Cin, Cout, 9, **kw1)
    assert torch.equal(y1[0], ya[1]), 'result depends on the batch composition'


# (the last two have more tiles than CUs: persistent blocks walk over 4-5 tiles each, ranges straddle images)
H2R_CASES = [(3, 32, 32), (2, 24, 48), (5, 16, 16), (9, 128, 128), (2, 256, 256)]


@pytest.mark.parametrize('mode', ['plain', 'pro-relu-maxima', 'pool-max-res', 'mask', 'own-amax-pass', 'fast-mask',
                                  'fast-pool-max-maxima',
                                  'dgrad-fused-arb', 'dgrad-fused-arb-skip-pool-sum'])
@pytest.mark.parametrize('case', H2R_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_register_resident_64ch_kernel_bit_identical(dev, O, case, mode):
    """conv_h2r_kernel (csrc/p2l_h2r.hip, round 6): the 64 -> 64 channel 3x3 layers with their weights resident
    in registers, persistent blocks walking over tiles.  Same operand pieces, same per-output summation order as
    the chunked direct kernel (P2L_FORM_NO_H2R keeps that one): outputs, pooled outputs, handed-over maxima and
    the partial sums of the fused activation backward are EQUAL bit for bit, for images of very different
    magnitude in one launch, tiles on every border, blocks that change image mid-range, non-power-of-two grids;
    and the result agrees with torch in fp64 at the tolerance of the fp32-grade kernels."""
    from pix2latent_amd import _native as N
    B, H, W = case
    Cin = Cout = 64
    g = torch.Generator().manual_seed(61)
    x = torch.randn(B, Cin, H, W, generator=g)
    x[0] *= 1e-5
    if B > 2:
        x[2] *= 3e3
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    bias = 0.1 * torch.randn(Cout, generator=g)
    s = 0.5 + torch.rand(B, Cin, generator=g)
    t = 0.3 * torch.randn(B, Cin, generator=g) * x.abs().amax(dim=(1, 2, 3)).view(B, 1)
    xs = nhwc(x, dev)
    forms = (N.FORM_NO_WINO, N.FORM_NO_WINO | N.FORM_NO_H2R)
    fam_new, fam_old = 6, 2                  # P2L_PROF_FAM_DIRECT_H2R / _DIRECT_H2

    def family(fn):
        N.check(N.lib().p2l_prof_begin(64), 'p2l_prof_begin')
        out = fn()
        torch.cuda.synchronize()
        T = N.prof_totals()
        return out, [i for i in range(8) if T.fam_count[i]]

    if mode.startswith('dgrad'):
        wt = O.pack_conv_weight(w.to(dev), 9, Cin, Cout, flip=True, wfmt=2)
        dy = nhwc(torch.randn(B, Cout, H, W, generator=g), dev)
        skip = pool = None
        Hx, Wx = H, W
        if 'pool-sum' in mode:
            Hx, Wx, pool = H // 2, W // 2, True
        xa = nhwc(torch.randn(B, Cin, Hx, Wx, generator=g), dev)
        kw = dict(wfmt=2)
        if 'skip' in mode:
            kw.update(skip=nhwc(torch.randn(B, 32, Hx, Wx, generator=g), dev), skip_C=32)
        res = []
        # (a fused activation backward stays on the chunked kernel by default -- the resident one cannot pipeline
        #  that epilogue --: forced here, so that the shared-item form of the new kernel is held to the same bits)
        _, fams = family(lambda: O.conv_dgrad_arb(dy, wt, B, H, W, Cout, Cin, 9, xa, s.to(dev), t.to(dev), Cin,
                                                  pool_sum=bool(pool), form=N.FORM_NO_WINO, **kw))
        assert fams == [fam_old]
        for form, fam in zip((N.FORM_NO_WINO | N.FORM_H2R_SEQ_EPI, forms[1]), (fam_new, fam_old)):
            out, fams = family(lambda: O.conv_dgrad_arb(dy, wt, B, H, W, Cout, Cin, 9, xa, s.to(dev), t.to(dev), Cin,
                                                        pool_sum=bool(pool), form=form, **kw))
            assert fams == [fam], (fams, fam)
            res.append(out)
        for a, b_, what in zip(res[0], res[1], ('dx', 'ds', 'dt')):
            assert torch.equal(a, b_), what
        return
    kw = dict(wfmt=2, bias=bias.to(dev))
    a = x.double()
    ref_act = None
    if mode == 'plain':
        kw['amax_in'] = xs.abs().reshape(B, -1, 64).amax(dim=2).contiguous()
    if mode == 'pro-relu-maxima':
        a = F.relu(a * s.double().view(B, Cin, 1, 1) + t.double().view(B, Cin, 1, 1))
        # maxima of |x| handed in (as the producer of x would leave them: here per 64-element pieces) and out
        am_in = xs.abs().reshape(B, -1, 64).amax(dim=2).contiguous()
        kw.update(pro=N.PRO_AFFINE_RELU, pro_s=s.to(dev), pro_t=t.to(dev), pro_bstride=Cin, amax_in=am_in,
                  want_amax=True, act=N.ACT_RELU, amax_next=(s.to(dev), t.to(dev), Cin))
        ref_act = 'relu'
    elif mode == 'pool-max-res':
        kw.update(pool=N.POOL_MAX, res=nhwc(torch.randn(B, Cout, H, W, generator=g), dev), act=N.ACT_RELU,
                  want_amax=True)
    elif mode == 'mask':
        kw.update(mask=nhwc(torch.randn(B, Cout, H, W, generator=g), dev), alpha=0.5)
    elif mode == 'fast-mask':                           # (the VGG input-gradient launches: pipelined epilogue 2)
        kw.update(mask=nhwc(torch.randn(B, Cout, H, W, generator=g), dev), want_amax=True)
        kw.pop('bias')
    elif mode == 'fast-pool-max-maxima':                # (VGG conv1_2 forward: pipelined epilogue 3)
        kw.update(pool=N.POOL_MAX, act=N.ACT_RELU, want_amax=True)
    wp = O.pack_conv_weight(w.to(dev), 9, Cout, Cin, wfmt=2)
    outs = []
    slow = mode in ('pool-max-res', 'mask')           # (residual / alpha: not the pipelined epilogue)
    for form, fam in zip(((forms[0] | N.FORM_H2R_SEQ_EPI) if slow else forms[0], forms[1]), (fam_new, fam_old)):
        out, fams = family(lambda: O.conv(xs, wp, B, H, W, Cin, Cout, 9, form=form, **kw))
        assert fams == [fam], (fams, fam)
        outs.append(out)
    if mode == 'plain':                                 # ... and the two epilogues of the new kernel against each other
        (y_seq, _), _ = family(lambda: O.conv(xs, wp, B, H, W, Cin, Cout, 9, form=forms[0] | N.FORM_H2R_SEQ_EPI, **kw))
        assert torch.equal(y_seq, outs[0][0])
    y_new, y_old = outs[0][0], outs[1][0]
    assert torch.equal(y_new, y_old), 'outputs differ: %g' % (y_new - y_old).abs().max().item()
    if outs[0][1] is not None:
        assert torch.equal(outs[0][1], outs[1][1]), 'pooled outputs differ'
    if kw.get('want_amax'):
        # the two kernels tile the channels differently (64 per block | 32 or 64): the per-image maxima agree
        for m_new, m_old in zip(outs[0][2], outs[1][2]):
            if m_new is not None:
                assert torch.equal(m_new.amax(dim=1), m_old.amax(dim=1))
                assert (m_new >= 0).all(), 'a promised maxima slot was not written'
    if mode in ('plain', 'pro-relu-maxima', 'own-amax-pass'):
        ref = F.conv2d(a, w.double(), bias.double(), padding=1)
        if ref_act:
            ref = F.relu(ref)
        got = nchw(y_new).double()
        for b_ in range(B):
            sc = ref[b_].abs().max().item()
            assert (got[b_] - ref[b_]).abs().max().item() < 2e-5 * sc, b_
    # a candidate's bits do not depend on who shares its launch, nor on which block's range it falls into
    if mode == 'plain' and B > 1:
        kw['amax_in'] = kw['amax_in'][1:2].contiguous()
        y1, _ = O.conv(xs[1:2].contiguous(), wp, 1, H, W, Cin, Cout, 9, form=forms[0], **kw)
        assert torch.equal(y1[0], y_new[1])


def test_direct_kernel_fp16x2_subpixel_and_maxima(dev, O):
    """the sub-pixel forms (nearest-x2 up-conv forward, its input gradient) in the fp16 x 2 arithmetic,
    and the maxima a split-K launch now leaves through its finish kernel (P2LAmax): exact per-image
    maxima, and a consumer that takes them gives the bits of the consumer that ran its own pass."""
    from pix2latent_amd import _native as N
    g = torch.Generator().manual_seed(23)
    B, H, Cin, Cout = 2, 32, 64, 64
    x = torch.randn(B, Cin, H // 2, H // 2, generator=g)
    x[1] *= 1e3
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode='nearest'), w.double(), None, padding=1)
    wsp = O.pack_conv_weight_subpix(w.to(dev), Cout, Cin, wfmt=2)
    O.DEFAULT_FORM = N.FORM_AUTO
    (y, _), mm = _mfma_products(N, lambda: O.conv(nhwc(x, dev), wsp, B, H, H, Cin, Cout, 9, wfmt=2, ups=2))
    assert abs(mm - 3.0) < 1e-6
    for b in range(B):
        assert (nchw(y)[b].double() - ref[b]).abs().max().item() < 2e-5 * ref[b].abs().max().item()
    # two output phases per block (the default of the forward launch) = one phase per block, bit for bit; also with
    # a prologue, bias + ReLU, 32-channel tiles, multi-image tiles, and the maxima the launch leaves
    for Bp, hp, ci, co, kw in ((2, 16, 64, 64, dict(bias=True, act=N.ACT_RELU, want_amax=True)),
                               (3, 32, 128, 32, dict(pro=N.PRO_AFFINE_RELU)),
                               (9, 4, 64, 128, dict(bias=True)), (2, 64, 32, 64, dict(want_amax=True))):
        xp = nhwc(torch.randn(Bp, ci, hp, hp, generator=g), dev)
        wq = O.pack_conv_weight_subpix((torch.randn(co, ci, 3, 3, generator=g) / math.sqrt(9 * ci)).to(dev), co, ci, wfmt=2)
        kw = dict(kw)
        if kw.pop('bias', False):
            kw['bias'] = torch.randn(co, generator=g).to(dev)
        if kw.get('pro'):
            kw.update(pro_s=(0.5 + torch.rand(Bp, ci, generator=g)).to(dev), pro_t=torch.randn(Bp, ci, generator=g).to(dev),
                      pro_bstride=ci)
        pair = O.conv(xp, wq, Bp, 2 * hp, 2 * hp, ci, co, 9, wfmt=2, ups=2, form=N.FORM_SP_PAIR, **kw)
        single = O.conv(xp, wq, Bp, 2 * hp, 2 * hp, ci, co, 9, wfmt=2, ups=2, form=N.FORM_NO_SP_PAIR, **kw)
        torch.cuda.synchronize()
        assert torch.equal(pair[0], single[0]), (Bp, hp, ci, co)
        if kw.get('want_amax') and pair[2][0] is not None:
            assert torch.equal(pair[2][0], single[2][0])
            assert torch.equal(pair[2][0].amax(dim=1), pair[0].abs().amax(dim=(1, 2, 3)))
    # input-gradient form: dx[low res] of the same conv for a gradient dy at high resolution
    dy = torch.randn(B, Cout, H, H, generator=g)
    xr = x.double().requires_grad_(True)
    F.conv2d(F.interpolate(xr, scale_factor=2, mode='nearest'), w.double(), None, padding=1).backward(dy.double())
    wtsp = O.pack_conv_weight_subpix(w.to(dev), Cin, Cout, flip=True, wfmt=2)
    (dx, _), mm = _mfma_products(N, lambda: O.conv(nhwc(dy, dev), wtsp, B, H, H, Cout, Cin, 9, wfmt=2, ups=3))
    assert abs(mm - 3.0) < 1e-6
    assert relerr(nchw(dx), xr.grad) < 2e-5
    # split-K launch -> finish kernel -> maxima
    Hs, Ci, Co = 8, 256, 128
    xs = torch.randn(3, Ci, Hs, Hs, generator=g)
    xs[2] *= 1e-4
    ws = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)
    wps = O.pack_conv_weight(ws.to(dev), 9, Co, Ci, wfmt=2)
    ys, _, (am, _) = O.conv(nhwc(xs, dev), wps, 3, Hs, Hs, Ci, Co, 9, wfmt=2, act=N.ACT_RELU, want_amax=True)
    assert am is not None and torch.equal(am.amax(dim=1), ys.abs().amax(dim=(1, 2, 3)))
    w2 = torch.randn(Co, Co, 3, 3, generator=g) / math.sqrt(9 * Co)
    wp2 = O.pack_conv_weight(w2.to(dev), 9, Co, Co, wfmt=2)
    z0, _ = O.conv(ys, wp2, 3, Hs, Hs, Co, Co, 9, wfmt=2)
    z1, _ = O.conv(ys, wp2, 3, Hs, Hs, Co, Co, 9, wfmt=2, amax_in=am)
    assert torch.equal(z0, z1)


PW_SMALL_CASES = [
    dict(B=3, H=8, Cin=512, Cout=128, pro='affine_relu', bias=True),                 # two images per tile
    dict(B=5, H=4, Cin=256, Cout=64, bias=True, res='same', alpha=0.5),              # eight images per tile
    dict(B=2, H=16, Cin=128, Cout=256, act='relu', pro='affine'),                    # one image per tile (2 tiles)
    dict(B=3, H=8, Cin=1024, Cout=64, splitk=4),
]


@pytest.mark.parametrize('case', PW_SMALL_CASES, ids=lambda c: '-'.join('%s%s' % kv for kv in c.items()))
def test_pointwise_small_grid_fp16x2(dev, O, case):
    """pw_h2_kernel<.., SM> (csrc/p2l_pw.hip): the 1x1 convs of the 4^2 ... 16^2 layers in the fp16 x 2
    arithmetic -- tiles that span several images, each on its own power of two, split-K slices summed by
    the deterministic finish kernel -- against torch in fp64 and against the exact-fp32 MFMA kernel
    (P2L_FORM_NO_PW), with and without handed-over maxima; a candidate's bits do not depend on the batch."""
    from pix2latent_amd import _native as N
    g = torch.Generator().manual_seed(31)
    B, H, Cin, Cout = case['B'], case['H'], case['Cin'], case['Cout']
    x = torch.randn(B, Cin, H, H, generator=g)
    x[0] *= 1e-5
    x[B - 1] *= 2e3
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / math.sqrt(Cin)
    kw = dict(wfmt=3)
    a = x.double()
    if case.get('pro'):
        s = 0.5 + torch.rand(B, Cin, generator=g)
        t = 0.3 * torch.randn(B, Cin, generator=g) * x.abs().amax(dim=(1, 2, 3)).view(B, 1)
        a = a * s.double().view(B, Cin, 1, 1) + t.double().view(B, Cin, 1, 1)
        if case['pro'] == 'affine_relu':
            a = F.relu(a)
        kw.update(pro=N.PRO_AFFINE_RELU if case['pro'] == 'affine_relu' else N.PRO_AFFINE,
                  pro_s=s.to(dev), pro_t=t.to(dev), pro_bstride=Cin)
    alpha = case.get('alpha', 1.0)
    ref = alpha * F.conv2d(a, w.double())
    if case.get('bias'):
        bias = 0.1 * torch.randn(Cout, generator=g)
        ref = ref + bias.double().view(1, Cout, 1, 1)
        kw['bias'] = bias.to(dev)
    if case.get('res'):
        r = torch.randn(B, Cout, H, H, generator=g) * ref.abs().amax(dim=(1, 2, 3)).view(B, 1, 1, 1).float()
        ref = ref + r.double()
        kw['res'] = nhwc(r, dev)
    if case.get('act') == 'relu':
        ref = F.relu(ref)
        kw['act'] = N.ACT_RELU
    kw['alpha'] = alpha
    if 'splitk' in case:
        kw['splitk'] = case['splitk']
    wp = O.pack_conv_weight(w.to(dev), 1, Cout, Cin, wfmt=3)
    xs = nhwc(x, dev)

    def products(fn):
        lib = N.lib()
        N.check(lib.p2l_prof_begin(64), 'p2l_prof_begin')
        lib.p2l_prof_step(0, 1)
        out = fn()
        torch.cuda.synchronize()
        T = N.prof_end()
        return out, T.mfma_flops[1] / T.exec_flops[1]

    O.DEFAULT_FORM = N.FORM_AUTO
    (y, _), mm = products(lambda: O.conv(xs, wp, B, H, H, Cin, Cout, 1, **kw))
    assert abs(mm - 3.0) < 1e-6, 'expected the fp16 x 2 small-grid kernel, got %g products' % mm
    O.DEFAULT_FORM = N.FORM_NO_PW
    (y32, _), mm32 = products(lambda: O.conv(xs, wp, B, H, H, Cin, Cout, 1, **kw))
    assert abs(mm32 - 16.0) < 1e-6
    O.DEFAULT_FORM = N.FORM_AUTO
    am = x.abs().amax(dim=(1, 2, 3)).view(B, 1).contiguous().to(dev)      # maxima handed over
    yh, _ = O.conv(xs, wp, B, H, H, Cin, Cout, 1, amax_in=am, **kw)
    y, y32, yh = nchw(y).double(), nchw(y32).double(), nchw(yh).double()
    for b in range(B):
        sc = ref[b].abs().max().item()
        assert (y[b] - ref[b]).abs().max().item() < 2e-5 * sc, (b, (y[b] - ref[b]).abs().max().item() / sc)
        assert (yh[b] - ref[b]).abs().max().item() < 2e-5 * sc
        assert (y32[b] - y[b]).abs().max().item() < 2e-5 * sc
    # batch composition (same split-K request)
    d = N.P2LConv()
    d.B, d.H, d.W, d.Cin, d.Cout, d.taps, d.wfmt, d.x_ld = B, H, H, Cin, Cout, 1, 3, Cin
    d.n_store = d.y_ld = Cout
    sk = kw.get('splitk', N.lib().p2l_conv_suggest_splitk(C.byref(d)))
    kw1 = dict(kw, splitk=sk)
    for key in ('pro_s', 'pro_t', 'res'):
        if key in kw1:
            kw1[key] = kw1[key][1:2].contiguous()
    ya, _ = O.conv(xs, wp, B, H, H, Cin, Cout, 1, **dict(kw, splitk=sk))
    y1, _ = O.conv(xs[1:2].contiguous(), wp, 1, H, H, Cin, Cout, 1, **kw1)
    assert torch.equal(y1[0], ya[1]), 'result depends on the batch composition'


AMAX_SLOT_CASES = [
    # taps, B, H, Cin, Cout, wfmt  (the launches of a BigGAN / VGG step that leave maxima, at the batch
    # sizes whose grids make choose_bn pick 32-channel tiles: 9 and 18 candidates)
    (1, 9, 16, 256, 1024, 3),      # small-grid pointwise kernel, unsplit (the round-5 finding)
    (1, 18, 16, 256, 1024, 3),
    (1, 2, 16, 256, 1024, 3),      # ... in split-K slices (finish kernel)
    (1, 9, 8, 512, 2048, 3),
    (1, 3, 32, 256, 1024, 3),      # full-tile pointwise kernel
    (9, 9, 16, 256, 256, 2),       # direct 3x3, split-K
    (9, 9, 64, 64, 64, 2),         # direct 3x3, one image per tile
    (9, 5, 32, 128, 96, 2),        # ... 32-channel tiles
    (9, 2, 32, 256, 256, 2),       # Winograd in K slices
    (9, 2, 64, 128, 128, 2),       # Winograd
]


@pytest.mark.parametrize('case', AMAX_SLOT_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_every_promised_maxima_slot_is_written(dev, O, case):
    """P2LAmax: the reader of a tensor takes its power of two from ALL p2l_conv_amax_slots(d) partial maxima
    per image, so the launch has to write every one of them (round 5: the small-grid pointwise kernel wrote
    half of what was promised where choose_bn said 32 -- the other half was whatever the ring set held
    before, and the first re-score after an optimising step differed from the following ones by an ulp)."""
    from pix2latent_amd import _native as N
    taps, B, H, Cin, Cout, wfmt = case
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, 3 if taps == 9 else 1, 3 if taps == 9 else 1, generator=g) / math.sqrt(taps * Cin)
    wp = O.pack_conv_weight(w.to(dev), taps, Cout, Cin, wfmt=wfmt)
    O.DEFAULT_FORM = N.FORM_AUTO
    y, _, (am, _) = O.conv(nhwc(x, dev), wp, B, H, H, Cin, Cout, taps, wfmt=wfmt, want_amax=True)
    assert am is not None, 'this launch was expected to leave maxima'
    assert bool((am >= 0).all()), '%d of %d promised slots were not written' % (int((am < 0).sum()), am.numel())
    assert torch.equal(am.amax(dim=1), y.abs().amax(dim=(1, 2, 3)))


H2_BLOCK_CASES = [
    # B, H, Cin, Cout, base form: 'auto' = what the plans run (K slices where the layer shape asks for them),
    # 'any' = P2L_FORM_WINO_ANY (Winograd form for a shape the default leaves to the direct kernel)
    (2, 32, 512, 512, 'auto'),     # a 32^2 layer of the generator at 2 local candidates (64 blocks of 16x16)
    (3, 64, 256, 128, 'auto'),     # 64^2, 2 N-tiles
    (2, 32, 256, 256, 'auto'),     # K-sliced small-grid layer (2 slices + finish kernel)
    (1, 16, 512, 512, 'auto'),     # 16^2: 4 slices
    (5, 48, 128, 64, 'any'),       # H not a power of two, odd batch
]


@pytest.mark.parametrize('mode', ['forward', 'forward-pool-max', 'dgrad-fused-arb', 'dgrad-fused-arb-pool-sum'])
@pytest.mark.parametrize('case', H2_BLOCK_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_winograd_f16x2_block_shapes_bit_identical(dev, O, case, mode):
    """Round 5: the 8x16-pixel / 4-wave block of the hand-scheduled fp16 x 2 Winograd kernel (the
    small-batch form: twice the blocks, one wave per SIMD) against its 16x16-pixel / 8-wave block.
    Re-tiling along M changes no output's summation order, so the launcher may pick the shape from the
    GRID SIZE: outputs, pooled outputs, the fused activation-backward sums (d s, d t) and the partial
    maxima handed to the next launch -- slot for slot -- are bit-identical, with and without K slices,
    and so is the consumer that reads those maxima."""
    from pix2latent_amd import _native as N
    B, H, Cin, Cout, base = case
    base = N.FORM_WINO_ANY if base == 'any' else N.FORM_AUTO
    g = torch.Generator().manual_seed(33)
    x = torch.randn(B, H, H, Cin, generator=g)
    x[0] *= 1e-3
    x = x.to(dev)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).to(dev)
    arb = mode.startswith('dgrad')
    s = (0.5 + torch.rand(B, Cout if arb else Cin, generator=g)).to(dev)
    t = (0.3 * torch.randn(B, Cout if arb else Cin, generator=g)).to(dev)
    bias = (0.1 * torch.randn(Cout, generator=g)).to(dev)
    res = torch.randn(B, H, H, Cout, generator=g).to(dev)
    pooled = mode.endswith('pool-sum')
    Ho = H // 2 if pooled else H
    xa = torch.randn(B, Ho, Ho, Cout, generator=g).to(dev)
    skip = torch.randn(B, Ho, Ho, Cout, generator=g).to(dev)
    outs = []
    for form in (base | N.FORM_WINO_H2_16X16, base | N.FORM_WINO_H2_8X16, base):
        O.DEFAULT_FORM = form
        if not arb:
            wp = O.pack_conv_weight(w, 9, Cout, Cin, wfmt=2)
            kw = dict(wfmt=2, bias=bias, pro=N.PRO_AFFINE_RELU, pro_s=s, pro_t=t, pro_bstride=Cin, alpha=0.5,
                      want_amax=True)
            if mode == 'forward':
                kw['res'] = res
            else:
                kw.update(pool=N.POOL_MAX, act=N.ACT_RELU)
            (y, yp, (am, amp)), mm = _mfma_products(N, lambda: O.conv(x, wp, B, H, H, Cin, Cout, 9, **kw))
            assert abs(mm - 3.0) < 1e-6, 'expected the fp16 x 2 Winograd kernel'
            assert am is not None and bool((am >= 0).all())
            # the consumer of the maxima
            w2 = O.pack_conv_weight((torch.randn(64, Cout, 3, 3, generator=torch.Generator().manual_seed(1)) / math.sqrt(9 * Cout)).to(dev), 9, 64, Cout, wfmt=2)
            z, _ = O.conv(y, w2, B, H, H, Cout, 64, 9, wfmt=2, amax_in=am)
            outs.append([y.clone(), am.clone(), z.clone()] + ([yp.clone(), amp.clone()] if yp is not None else []))
        else:
            wt = O.pack_conv_weight(w.permute(1, 0, 2, 3).contiguous(), 9, Cout, Cin, flip=True, wfmt=2)
            dd = N.P2LConv()
            dd.B, dd.H, dd.W, dd.Cin, dd.Cout, dd.taps, dd.wfmt, dd.x_ld, dd.form = B, H, H, Cin, Cout, 9, 2, Cin, form
            dd.n_store = dd.y_ld = dd.yp_ld = Cout
            dd.pool = N.POOL_SUM if pooled else N.POOL_NONE
            dx, ds, dt = O.conv_dgrad_arb(x, wt, B, H, H, Cin, Cout, 9, xa, s, t, Cout, wfmt=2, skip=skip, skip_C=Cout,
                                          pool_sum=pooled, splitk=N.lib().p2l_conv_suggest_splitk(C.byref(dd)))
            outs.append([dx.clone(), ds.clone(), dt.clone()])
    torch.cuda.synchronize()
    for a, b, c in zip(*outs):
        assert torch.equal(a, b), 'the 8x16 block differs from the 16x16 block'
        assert torch.equal(a, c), 'the block shape picked from the grid differs'

"""The non-conv kernels of the LPIPS loss path (csrc/p2l_loss_shell.h and the three plans chain them between the
convs) against the float64 references of tests/_small_refs.py, called through ctypes with the harness, the metric
and the bars of tests/test_small_kernels_gpu.py (tests/_pin.py):

    p2l_lpips_normalize, p2l_lpips_tap_fwd / _bwd / _pool_bwd, p2l_bilinear_adjoint, p2l_maxpool2_bwd(_amax),
    p2l_maxpool3s2_fwd / _bwd, p2l_conv1_dgrad.

Exact kernels (the pool forward, a pool backward that adds nothing, every zero the contract promises) are compared
bit for bit; rounded outputs are held to |got - r64| / sum|terms| <= min(k, 4 x fp32 restatement) x 2^-24 with the
denominators written next to each `hold`, so that a weak pixel or a converged one (nf ~ nft: a difference of nearly
equal numbers) is measured against its own terms and not against the largest output of the tensor.  Every image of a
batch has a magnitude of its own.  The LPIPS inputs hold, next to ordinary relu(randn) pixels, all-zero pixels (in f,
in the target, in both), a pixel whose only non-zero channel is 1e-10, pixels scaled by 1e-10 and 1e-6 (where the
1e-10 of the normalisation decides the result), pixels with f equal to the target features, pixels of weight 0 and
negative gscales; the pool inputs hold 2, 3 and 4 equal POSITIVE maxima at every scan position of a window, which
no ReLU mask hides.  P2L_LOSS_ERR_FILE=<path> records the figures (profiles/loss_kernels_err.txt)."""
import math

import pytest
import torch
import torch.nn.functional as F

import _small_refs as R
from _pin import D64, N, Out, _gen, _record_file, d64, draw, hold, is_sentinel, randn, seeded  # noqa: F401

pytestmark = pytest.mark.gpu
EINVAL, EUNSUP = -1, -4
PB = {64: 16, 128: 8, 192: 16, 256: 4, 384: 8, 512: 4}        # LPIPS width -> pixels per block of the tap kernels


def _mags(Bn):
    """one magnitude per image: a value or a maxima slot that leaks between images shows"""
    return 10.0 ** torch.linspace(-1.0, 1.0, Bn) if Bn > 1 else torch.tensor([3.0])


def _pitched(t, ld, dev):
    """[..., C] -> the same rows at pitch ld on the device, junk in the gap columns"""
    o = torch.full(t.shape[:-1] + (ld,), 7.0)
    o[..., :t.shape[-1]] = t
    return o.to(dev)


# =====================================================================================================================
# LPIPS: normalise, tap forward, tap backward
# =====================================================================================================================
def _lanes(C):
    """lanes that share a pixel (the largest power of two in C / 4, at most a wave) and float4s per lane"""
    lp = 1
    while lp < 64 and (C // 4) % (2 * lp) == 0:
        lp *= 2
    return lp, C // (4 * lp)


def _k_lpips(C):
    """roundings on the longest chain of nf, of the forward sum and of the backward, from the header's formulas and
    the summation the width fixes: a lane sums its float4s' squares ((x^2 + y^2) + (z^2 + w^2), one accumulation
    per float4), log2(lanes) shuffles finish the pixel"""
    lp, vpl = _lanes(C)
    k_sum = 2 + vpl + int(math.log2(lp))             # a channel sum: the float4's tree, the lane's chain, the shuffles
    k_ss = 1 + k_sum                                 # ... of squares
    k_nrm = k_ss / 2 + 1                             # the square root halves the error and rounds once
    k_inv = k_nrm + 2 + 1                            # + 1e-10 and that constant's own rounding to fp32; 1 / x
    k_nf = k_inv + 1                                 # f * inv
    # forward: e = nf - nft carries k_nf + 1 against |nf| + |nft|; lin e e doubles that and multiplies twice; the
    # channel sum; * wt; the wave tree (6) and the four waves (2)
    k_fwd = 2 * (k_nf + 1) + 2 + k_sum + 1 + 6 + 2
    # backward: u = 2 lin e: k_nf + 2 (the 2 is exact); u . f: a product and the channel sum; c2 = (u . f) inv inv /
    # nrm: twice inv's error, nrm's, three operations; c2 f, the subtraction from u inv (the shorter chain);
    # gscale * wt and the product with it
    k_bwd = (k_nf + 2) + 1 + k_sum + 2 * k_inv + k_nrm + 3 + 1 + 1 + 2
    return k_nf, k_fwd, k_bwd


KINDS = 12


def _lpips_case(g, Bn, P, C, shared=False):
    """f, nft [Bn, P, C], lin [C], wt [Bn, P], gscale [Bn].  Pixel p of image b is of kind (p + 5 b + 7 draw) % 12:
    1 f all zero, 2 target all zero, 3 both, 4 f = 1e-10 in one channel, 5 / 6 f scaled by 1e-10 / 1e-6, 7 / 8 f equal
    to the target features (8: up to a factor the normalisation removes), 9 weight 0, the others ordinary."""
    mag = _mags(Bn)
    f = F.relu(randn(g, Bn, P, C)) * mag.view(Bn, 1, 1)
    ft = F.relu(randn(g, Bn, P, C))
    wt = torch.rand(Bn, P, generator=g) * mag.flip(0).view(Bn, 1)
    lin = torch.rand(C, generator=g) / C
    gs = randn(g, Bn).abs() + 0.1
    gs[::2] *= -1.0                                                      # image 0 (and 2): a negative gscale
    gs = gs * mag
    kind = (torch.arange(P)[None, :] + 5 * torch.arange(Bn)[:, None] + 7 * draw()) % KINDS
    ft[(kind == 2) | (kind == 3)] = 0.0
    if shared:                                                           # one target for the batch: the last image's
        ft, wt = ft[-1:].repeat(Bn, 1, 1), wt[-1:].repeat(Bn, 1)
        kind_t = kind[-1:].repeat(Bn, 1)
    else:
        kind_t = kind
    f[(kind == 1) | (kind_t == 3)] = 0.0
    hot = torch.zeros(C)
    hot[int(torch.randint(C, (1,), generator=g))] = 1e-10
    f[kind == 4] = hot
    f[kind == 5] *= 1e-10                                                # ||f|| ~ 6e-11 x magnitude: >= 1e-12
    f[kind == 6] *= 1e-6
    conv = (kind == 7) & (kind_t != 3)
    f[conv] = ft[conv]
    conv = (kind == 8) & (kind_t != 3)
    f[conv] = 3.0 * ft[conv]
    wt[kind_t == 9] = 0.0
    nrm = f.to(D64).pow(2).sum(-1).sqrt()
    assert bool(((nrm == 0) | (nrm >= 1e-12)).all())
    nft = R.lpips_normalize(ft.to(D64)).float()                          # the cached target features the kernels read
    return f, nft, lin, wt, gs


def _tap_run(dev, N, f, nft, lin, wt, gs, nft_shared=False, wt_shared=False):
    """-> nf [Bn, P, C], partial [Bn, nblk], df [Bn, P, C]; a shared target is handed over once, with stride 0"""
    lib = N.lib()
    Bn, P, C = f.shape
    nblk = lib.p2l_lpips_tap_nblk(P, C)
    assert nblk == -(-P // PB[C])
    fd, lind, gsd = f.contiguous().to(dev), lin.to(dev), gs.contiguous().to(dev)
    nftd = (nft[0] if nft_shared else nft).contiguous().to(dev)
    wtd = (wt[0] if wt_shared else wt).contiguous().to(dev)
    ns, ws = N.i64(0 if nft_shared else P * C), N.i64(0 if wt_shared else P)
    nf, part, df = Out(dev, Bn * P * C), Out(dev, Bn * nblk), Out(dev, Bn * P * C)
    N.check(lib.p2l_lpips_normalize(N.ptr(fd), N.ptr(nf.t), N.i64(Bn * P), C, N.stream()), 'lpips_normalize')
    N.check(lib.p2l_lpips_tap_fwd(N.ptr(fd), N.ptr(nftd), ns, N.ptr(lind), N.ptr(wtd), ws, N.ptr(part.t), Bn, P, C,
                                  N.stream()), 'lpips_tap_fwd')
    N.check(lib.p2l_lpips_tap_bwd(N.ptr(fd), N.ptr(nftd), ns, N.ptr(lind), N.ptr(wtd), ws, N.ptr(gsd), N.ptr(df.t),
                                  Bn, P, C, N.stream()), 'lpips_tap_bwd')
    return nf.cpu(Bn, P, C), part.cpu(Bn, nblk), df.cpu(Bn, P, C)


def _tap_denominators(f6, nft6, lin6, wt6, gs6):
    """forward [Bn]: sum_p |wt| sum_c lin_c (|nf| + |nft|)^2.  Backward, channel j:
    |gscale wt| (2 lin_j inv (|nf_j| + |nft_j|) + |f_j| inv^2 / nrm * sum_c 2 lin_c (|nf_c| + |nft_c|) |f_c|)"""
    nrm = f6.pow(2).sum(-1, keepdim=True).sqrt()
    inv = 1.0 / (nrm + 1e-10)
    a = lin6 * ((f6 * inv).abs() + nft6.abs())
    den_fwd = (wt6.abs() * (a * ((f6 * inv).abs() + nft6.abs())).sum(-1)).sum(-1)
    s = (2 * a * f6.abs()).sum(-1, keepdim=True)
    t2 = torch.where(nrm > 0, f6.abs() * inv * inv / torch.where(nrm > 0, nrm, torch.ones_like(nrm)) * s,
                     torch.zeros_like(f6))
    den_bwd = (gs6.view(-1, 1) * wt6).abs()[..., None] * (2 * a * inv + t2)
    return den_fwd, den_bwd


def _all_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('Bn', [1, 3])
@pytest.mark.parametrize('Pi', range(5))
@pytest.mark.parametrize('C', sorted(PB))
@seeded
def test_lpips_normalize_tap_fwd_bwd(dev, N, C, Pi, Bn):
    P = [1, PB[C] - 1, PB[C], PB[C] + 1, 225][Pi]
    g = _gen(101, C, P, Bn)
    case = 'Bn=%d P=%d C=%d' % (Bn, P, C)
    f, nft, lin, wt, gs = _lpips_case(g, Bn, P, C)
    nf, part, df = got = _tap_run(dev, N, f, nft, lin, wt, gs)
    assert _all_equal(got, _tap_run(dev, N, f, nft, lin, wt, gs))
    alone = _tap_run(dev, N, f[-1:], nft[-1:], lin, wt[-1:], gs[-1:])        # an image does not depend on its batch
    assert _all_equal([t[0] for t in alone], [t[-1] for t in got])
    f6, nft6, lin6, wt6, gs6 = d64(f, nft, lin, wt, gs)
    k_nf, k_fwd, k_bwd = _k_lpips(C)
    ref = R.lpips_normalize(f6)
    hold('p2l_lpips_normalize:nf', case, nf, ref, ref.abs(), R.lpips_normalize(f), k_nf)
    den_fwd, den_bwd = _tap_denominators(f6, nft6, lin6, wt6, gs6)
    # the fp64 host sum of the partials: what p2l_reduce_rows adds is held in test_small_kernels_gpu.py
    hold('p2l_lpips_tap_fwd:partial', case, part.to(D64).sum(1), R.lpips_tap(f6, nft6, lin6, wt6), den_fwd,
         R.lpips_tap(f, nft, lin, wt), k_fwd)
    ref = R.lpips_tap_bwd(f6, nft6, lin6, wt6, gs6)
    assert bool(torch.isfinite(df).all())                                    # ||f|| == 0: c2 = 0, not 0 / 0
    hold('p2l_lpips_tap_bwd:df', case, df, ref, den_bwd, R.lpips_tap_bwd(f, nft, lin, wt, gs), k_bwd)
    # one target for the whole batch (stride 0) == the same target replicated per image, bit for bit
    f, nft, lin, wt, gs = _lpips_case(g, Bn, P, C, shared=True)
    want = _tap_run(dev, N, f, nft, lin, wt, gs)
    for nft_shared, wt_shared in ((True, False), (False, True), (True, True)):
        assert _all_equal(_tap_run(dev, N, f, nft, lin, wt, gs, nft_shared, wt_shared), want), (nft_shared, wt_shared)
    f6, nft6, lin6, wt6, gs6 = d64(f, nft, lin, wt, gs)
    den_fwd, den_bwd = _tap_denominators(f6, nft6, lin6, wt6, gs6)
    hold('p2l_lpips_tap_fwd:partial', case + ' shared', want[1].to(D64).sum(1), R.lpips_tap(f6, nft6[0], lin6, wt6[0]),
         den_fwd, R.lpips_tap(f, nft[0], lin, wt[0]), k_fwd)
    hold('p2l_lpips_tap_bwd:df', case + ' shared', want[2], R.lpips_tap_bwd(f6, nft6[0], lin6, wt6[0], gs6), den_bwd,
         R.lpips_tap_bwd(f, nft[0], lin, wt[0], gs), k_bwd)


# =====================================================================================================================
# 2x2 max pool backward, alone and inside the tap backward
# =====================================================================================================================
# the scan positions (row-major in the quad) that hold the quad's maximum: every pair, every triple, all four
PATS2 = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3), (0, 1, 2, 3)]


def _write_quad_ties(y, mag, alternate=False):
    """in place, y [Bn, H, W, C]: in the first and the last quad of every image the first 22 channels hold a positive
    maximum (8 .. 11 x the image's magnitude, above anything drawn) at the positions of a pattern and half of it at
    the others; the pattern moves with channel, image, quad and draw.  alternate: the first quad on even draws, the
    last on odd ones and none where that is the first again, so that on a grid of one or two quads the pixels
    drawn for the other quad survive"""
    Bn, H, W, C = y.shape
    quads = sorted({(0, 0), (H // 2 - 1, W // 2 - 1)})
    for b in range(Bn):
        for qi, (qy, qx) in enumerate(quads):
            if alternate and qi != (draw() % 2 if len(quads) > 1 else 2 * (draw() % 2)):
                continue
            for c in range(min(C, 22)):
                pat = PATS2[(c + 3 * b + 5 * qi + 7 * draw()) % len(PATS2)]
                v = (8.0 + c % 4) * float(mag[b])
                for s in range(4):
                    y[b, 2 * qy + (s >> 1), 2 * qx + (s & 1), c] = v if s in pat else 0.5 * v


def _amax_ok(am, dy):
    """every slot written (the buffer held -1), the per-image maximum is that of |dy| exactly"""
    assert bool((am >= 0).all()), 'a promised maxima slot was not written'
    assert torch.equal(am.amax(dim=1), dy.abs().flatten(1).amax(dim=1))


def _pool2_run(dev, N, y, dyp, add, relu_mask, ld, amax):
    lib = N.lib()
    Bn, H, W, C = y.shape
    slots = lib.p2l_maxpool2_bwd_amax_slots(H, W, C)
    assert slots == -(-((H // 2) * (W // 2) * (C // 4)) // 256) * 4
    dy = Out(dev, Bn * H * W * ld)
    am = Out(dev, Bn * slots, prefill=torch.full((Bn * slots,), -1.0))
    args = [N.ptr(_pitched(y, ld, dev)), ld, N.ptr(_pitched(dyp, ld, dev)), ld,
            N.ptr(_pitched(add, ld, dev)) if add is not None else None, ld, N.ptr(dy.t), ld, Bn, H, W, C, relu_mask]
    if amax is None:
        N.check(lib.p2l_maxpool2_bwd(*(args + [N.stream()])), 'maxpool2_bwd')
    else:
        N.check(lib.p2l_maxpool2_bwd_amax(*(args + [N.ptr(am.t) if amax else None, N.stream()])), 'maxpool2_bwd_amax')
    got = dy.cpu(Bn, H, W, ld)
    assert ld == C or is_sentinel(got[..., C:]), 'gap columns of the pitched dy written'
    got = got[..., :C].contiguous()
    amc = am.cpu(Bn, slots)
    if amax:
        _amax_ok(amc, got)
    else:
        assert bool((amc == -1).all())
    return got


@pytest.mark.parametrize('relu_mask', [0, 1])
@pytest.mark.parametrize('add_on', [0, 1])
@pytest.mark.parametrize('Bn,H,W,C,ld', [(1, 2, 2, 4, 4), (3, 6, 10, 12, 20), (2, 18, 14, 20, 20), (2, 16, 16, 64, 72)])
@seeded
def test_maxpool2_bwd_amax(dev, N, Bn, H, W, C, ld, add_on, relu_mask):
    """the un-pooled tensor holds negative values, zeros (a quad of zeros is a tie that relu_mask = 0 shows) and the
    hand-written positive ties"""
    g = _gen(102, Bn, H, W, C)
    mag = _mags(Bn)
    y = randn(g, Bn, H, W, C) * mag.view(Bn, 1, 1, 1)
    y[torch.rand(Bn, H, W, C, generator=g) < 0.3] = 0.0
    _write_quad_ties(y, mag)
    dyp = randn(g, Bn, H // 2, W // 2, C) * mag.flip(0).view(Bn, 1, 1, 1)
    add = randn(g, Bn, H, W, C) * mag.flip(0).view(Bn, 1, 1, 1) if add_on else None
    got = _pool2_run(dev, N, y, dyp, add, relu_mask, ld, None)
    for amax in (None, False, True):                         # p2l_maxpool2_bwd, _amax(NULL), _amax(buffer): same bits
        assert torch.equal(_pool2_run(dev, N, y, dyp, add, relu_mask, ld, amax), got)
    alone = _pool2_run(dev, N, y[-1:], dyp[-1:], None if add is None else add[-1:], relu_mask, ld, True)
    assert torch.equal(alone[0], got[-1])
    y6, dyp6, add6 = d64(y, dyp, add)
    ref = R.maxpool2_bwd(y6, dyp6, add6, relu_mask)
    if not add_on:
        assert torch.equal(got.to(D64), ref)                 # a selection and a mask: exact
        return
    den = R.maxpool2_bwd(y6, dyp6.abs(), add6.abs(), relu_mask)
    # one addition
    hold('p2l_maxpool2_bwd:dy', 'Bn=%d %dx%d C=%d ld=%d mask=%d' % (Bn, H, W, C, ld, relu_mask), got, ref, den,
         R.maxpool2_bwd(y, dyp, add, relu_mask), 1)


@pytest.mark.parametrize('big', [0, 1])
@pytest.mark.parametrize('C', sorted(PB))
@seeded
def test_lpips_tap_pool_bwd(dev, N, C, big):
    lib = N.lib()
    half = PB[C] // 2
    Bn, (H, W) = 3, ((6, 3 * half if half != 2 else 10) if big else (2, half))
    P = H * W
    g = _gen(103, C, H, W)
    case = 'Bn=%d %dx%d C=%d' % (Bn, H, W, C)
    mag = _mags(Bn)
    f, nft, lin, wt, gs = _lpips_case(g, Bn, P, C)
    f = f.view(Bn, H, W, C)
    _write_quad_ties(f, mag, alternate=True)                 # (2, half) is one or two quads: keep the eps pixels
    dyp = randn(g, Bn, H // 2, W // 2, C) * mag.flip(0).view(Bn, 1, 1, 1)
    nblk = lib.p2l_lpips_tap_nblk(P, C)

    def run(sl, amax):
        b = sl.stop - sl.start
        df = Out(dev, b * P * C)
        am = Out(dev, b * nblk, prefill=torch.full((b * nblk,), -1.0))
        N.check(lib.p2l_lpips_tap_pool_bwd(N.ptr(f[sl].contiguous().to(dev)), N.ptr(nft[sl].contiguous().to(dev)),
                                           N.i64(P * C), N.ptr(lin.to(dev)), N.ptr(wt[sl].contiguous().to(dev)), N.i64(P),
                                           N.ptr(gs[sl].contiguous().to(dev)), N.ptr(dyp[sl].contiguous().to(dev)),
                                           N.ptr(df.t), N.ptr(am.t) if amax else None, b, H, W, C, N.stream()),
                'lpips_tap_pool_bwd')
        got, amc = df.cpu(b, H, W, C), am.cpu(b, nblk)
        if amax:
            _amax_ok(amc, got)
        else:
            assert bool((amc == -1).all())
        return got
    got = run(slice(0, Bn), True)
    assert torch.equal(run(slice(0, Bn), True), got) and torch.equal(run(slice(0, Bn), False), got)
    assert torch.equal(run(slice(Bn - 1, Bn), True)[0], got[-1])
    # = the tap backward, then the pool backward with the tap gradient as its additive term, bit for bit (p2l.h)
    tap = _tap_run(dev, N, f.view(Bn, P, C), nft, lin, wt, gs)[2].view(Bn, H, W, C)
    assert torch.equal(_pool2_run(dev, N, f, dyp, tap, 1, C, True), got)
    f6, nft6, lin6, wt6, gs6, dyp6 = d64(f, nft, lin, wt, gs, dyp)
    _, den_tap = _tap_denominators(f6.view(Bn, P, C), nft6, lin6, wt6, gs6)
    den = R.maxpool2_bwd(f6, dyp6.abs(), den_tap.view(Bn, H, W, C), True)
    # the tap backward's chain and the addition of the pooled gradient
    hold('p2l_lpips_tap_pool_bwd:df', case, got, R.lpips_tap_pool_bwd(f6, nft6, lin6, wt6, gs6, dyp6), den,
         R.lpips_tap_pool_bwd(f, nft, lin, wt, gs, dyp), _k_lpips(C)[2] + 1)


# =====================================================================================================================
# 3x3 / stride 2 max pool
# =====================================================================================================================
# scan positions of a 3x3 window that hold its maximum: 2, 3 and 4 of them, starting at every position
PATS3 = [tuple(sorted({(t + 2 * j) % 9 for j in range(n)})) for n in (2, 3, 4) for t in range(9)]


def _write_window_ties(x, mag):
    """in place, x [Bn, Hi, Wi, C]: in the first and the last window of every image the first 27 channels hold a
    positive maximum (above anything drawn) at the positions of a pattern; the windows next to them see it too"""
    Bn, Hi, Wi, C = x.shape
    Ho, Wo = (Hi - 3) // 2 + 1, (Wi - 3) // 2 + 1
    for b in range(Bn):
        for wi, (oy, ox) in enumerate(sorted({(0, 0), (Ho - 1, Wo - 1)})):
            for c in range(min(C, 27)):
                pat = PATS3[(c + C * b + 5 * wi + 7 * draw()) % len(PATS3)]
                for t in pat:
                    x[b, 2 * oy + t // 3, 2 * ox + t % 3, c] = (8.0 + c % 4) * float(mag[b])


@pytest.mark.parametrize('gtap_on', [0, 1])
@pytest.mark.parametrize('Bn,Hi,Wi,C', [(1, 3, 3, 4), (2, 7, 15, 8), (2, 8, 6, 12), (3, 31, 15, 64)])
@seeded
def test_maxpool3s2_fwd_bwd(dev, N, Bn, Hi, Wi, C, gtap_on):
    lib, g = N.lib(), _gen(104, Bn, Hi, Wi, C)
    Ho, Wo = (Hi - 3) // 2 + 1, (Wi - 3) // 2 + 1
    mag = _mags(Bn)
    x = F.relu(randn(g, Bn, Hi, Wi, C)) * mag.view(Bn, 1, 1, 1)
    _write_window_ties(x, mag)
    if gtap_on:
        gp = randn(g, Bn, Ho, Wo, C) * mag.flip(0).view(Bn, 1, 1, 1)
        gt = randn(g, Bn, Hi, Wi, C) * mag.flip(0).view(Bn, 1, 1, 1)
    else:
        # a pixel is the first maximum of up to four windows; multiples of 1/8 below 8, times a power of two per
        # image, add up without rounding, so that the backward without gtap is exact
        gp = torch.randint(-63, 64, (Bn, Ho, Wo, C), generator=g).float() / 8.0
        gp = gp * (2.0 ** (3 * torch.arange(Bn))).view(Bn, 1, 1, 1)
        gt = None

    def run(sl):
        b = sl.stop - sl.start
        y, dx = Out(dev, b * Ho * Wo * C), Out(dev, b * Hi * Wi * C)
        xd = x[sl].contiguous().to(dev)
        N.check(lib.p2l_maxpool3s2_fwd(N.ptr(xd), N.ptr(y.t), b, Hi, Wi, C, N.stream()), 'maxpool3s2_fwd')
        N.check(lib.p2l_maxpool3s2_bwd(N.ptr(xd), N.ptr(gp[sl].contiguous().to(dev)),
                                       N.ptr(gt[sl].contiguous().to(dev)) if gtap_on else None, N.ptr(dx.t), b, Hi, Wi, C,
                                       N.stream()), 'maxpool3s2_bwd')
        return y.cpu(b, Ho, Wo, C), dx.cpu(b, Hi, Wi, C)
    y, dx = run(slice(0, Bn))
    assert _all_equal(run(slice(0, Bn)), (y, dx))
    assert _all_equal([t[0] for t in run(slice(Bn - 1, Bn))], (y[-1], dx[-1]))
    assert torch.equal(y, R.maxpool3s2(x))
    x6, gp6, gt6 = d64(x, gp, gt)
    ref = R.maxpool3s2_bwd(x6, gp6, gt6)
    # an even size leaves the last row / column in no window: gtap (under the mask) and nothing else
    edge = gt * (x > 0).float() if gtap_on else torch.zeros_like(x)
    if Hi % 2 == 0:
        assert torch.equal(dx[:, -1], edge[:, -1])
    if Wi % 2 == 0:
        assert torch.equal(dx[:, :, -1], edge[:, :, -1])
    if not gtap_on:
        assert torch.equal(dx.to(D64), ref)
        return
    den = R.maxpool3s2_bwd(x6, gp6.abs(), gt6.abs())
    # gtap plus up to four windows' gradients, one addition each
    hold('p2l_maxpool3s2_bwd:dx', 'Bn=%d %dx%d C=%d' % (Bn, Hi, Wi, C), dx, ref, den, R.maxpool3s2_bwd(x, gp, gt), 4)


# =====================================================================================================================
# input gradient of the first conv, adjoint of the bilinear upsampling
# =====================================================================================================================
@pytest.mark.parametrize('Bn,H,W,Co,K,S,pad', [(1, 3, 3, 4, 3, 2, 0), (3, 19, 16, 64, 3, 2, 0), (2, 37, 50, 64, 11, 4, 2),
                                               (1, 5, 5, 4, 1, 2, 0)])
@seeded
def test_conv1_dgrad(dev, N, Bn, H, W, Co, K, S, pad):
    """19x16 K3 S2, 37x50 K11 S4 pad 2: (size + 2 pad - K) % S != 0, the border past the last window gets nothing;
    K1 S2: every other row and column lies in no window at all"""
    lib, g = N.lib(), _gen(105, Bn, H, W, Co, K, S)
    Ho, Wo = (H + 2 * pad - K) // S + 1, (W + 2 * pad - K) // S + 1
    gr = randn(g, Bn, Ho, Wo, Co) * _mags(Bn).view(Bn, 1, 1, 1)
    w = 0.05 * randn(g, K * K, 3, Co)

    def run(sl):
        b = sl.stop - sl.start
        d = Out(dev, b * H * W * 16)
        N.check(lib.p2l_conv1_dgrad(N.ptr(gr[sl].contiguous().to(dev)), N.ptr(w.to(dev)), N.ptr(d.t), b, H, W, Co, K, S,
                                    pad, N.stream()), 'conv1_dgrad')
        return d.cpu(b, H, W, 16)
    got = run(slice(0, Bn))
    assert torch.equal(run(slice(0, Bn)), got) and torch.equal(run(slice(Bn - 1, Bn))[0], got[-1])
    assert bool((got[..., 3:].contiguous().view(torch.int32) == 0).all())    # channels 3..15: +0.0
    gr6, w6 = d64(gr, w)
    ref, den = R.conv1_dgrad(gr6, w6, H, W, K, S, pad), R.conv1_dgrad(gr6.abs(), w6.abs(), H, W, K, S, pad)
    cov_y, cov_x = torch.zeros(H + 2 * pad, dtype=torch.bool), torch.zeros(W + 2 * pad, dtype=torch.bool)
    for o in range(Ho):
        cov_y[o * S:o * S + K] = True
    for o in range(Wo):
        cov_x[o * S:o * S + K] = True
    cov = cov_y[pad:pad + H, None] & cov_x[None, pad:pad + W]
    assert (bool(cov.all()) == ((H + 2 * pad - K) % S == 0 and (W + 2 * pad - K) % S == 0 and K >= S))
    assert bool((got[:, ~cov] == 0).all()) and bool((den[:, ~cov] == 0).all())   # pixels no window covers
    # per live tap (ceil(K / S)^2 of them) Co / 4 accumulations in sequence, each of a four-product tree (1 + 2)
    hold('p2l_conv1_dgrad:dimg16', 'Bn=%d %dx%d Co=%d K=%d S=%d pad=%d' % (Bn, H, W, Co, K, S, pad), got[..., :3],
         ref[..., :3], den[..., :3], R.conv1_dgrad(gr, w, H, W, K, S, pad)[..., :3], math.ceil(K / S) ** 2 * Co // 4 + 3)


@pytest.mark.parametrize('Bn', [1, 3])
@pytest.mark.parametrize('H,W,h,w', [(8, 8, 8, 8), (16, 8, 4, 4), (64, 64, 15, 15), (64, 48, 7, 3), (37, 53, 9, 20),
                                     (64, 64, 1, 1), (256, 256, 63, 63)])
@seeded
def test_bilinear_adjoint(dev, N, H, W, h, w, Bn):
    lib, g = N.lib(), _gen(106, H, W, h, w, Bn)
    wsrc = randn(g, Bn, H, W) * _mags(Bn).view(Bn, 1, 1)

    def run(sl):
        b = sl.stop - sl.start
        wt = Out(dev, b * h * w)
        N.check(lib.p2l_bilinear_adjoint(N.ptr(wsrc[sl].contiguous().to(dev)), N.ptr(wt.t), b, H, W, h, w, N.stream()),
                'bilinear_adjoint')
        return wt.cpu(b, h, w)
    got = run(slice(0, Bn))
    assert torch.equal(run(slice(0, Bn)), got) and torch.equal(run(slice(Bn - 1, Bn))[0], got[-1])
    w6 = wsrc.to(D64)
    # The source coordinate fy = (h / H)(py + 0.5) - 0.5 is computed in fp32: three roundings of up to h x 2^-24
    # ABSOLUTE in a weight that is 1/2 on average.  A target pixel collects about 2 H / h + 1 source rows whose
    # weights add up to H / h >= 1, so their errors are up to 3 h (2 H / h + 1) / (H / h) <= 9 h roundings of the
    # sum of the terms, and the same along x (nothing where the ratio is a power of two: the restatement, fp32
    # F.interpolate autograd, rounds its coordinates the same way and then sets the bar).  Then 1 - l and two
    # products, ceil(2 W / w) + 3 additions along the row and ceil(2 H / h) + 3 over the rows.
    k = 9 * (h + w) + 4 + math.ceil(2 * W / w) + 3 + math.ceil(2 * H / h) + 3
    hold('p2l_bilinear_adjoint:wt', 'Bn=%d %dx%d -> %dx%d' % (Bn, H, W, h, w), got, R.bilinear_adjoint(w6, h, w),
         R.bilinear_adjoint(w6.abs(), h, w), R.bilinear_adjoint(wsrc, h, w), k)


# =====================================================================================================================
# refusals: what these entry points reject, they reject on the host, before anything is launched.  (They check
# only what their comments state -- include/p2l.h -- so every pointer handed over here is a real buffer, except the
# NULL that p2l_lpips_tap_pool_bwd documents.)
# =====================================================================================================================
def test_refusals_before_any_launch(dev, N):
    lib, st, i64 = N.lib(), N.stream(), N.i64
    a, b, c, d, e, f = (torch.ones(65536, device=dev) for _ in range(6))
    o1, o2 = Out(dev, 65536), Out(dev, 65536)
    A, B, C_, D_, E, F_, O1, O2 = N.ptr(a), N.ptr(b), N.ptr(c), N.ptr(d), N.ptr(e), N.ptr(f), N.ptr(o1.t), N.ptr(o2.t)
    z = i64(0)
    calls = [
        ('lpips_normalize C=96', lib.p2l_lpips_normalize(A, O1, i64(4), 96, st), EUNSUP),
        ('lpips_normalize C=1024', lib.p2l_lpips_normalize(A, O1, i64(4), 1024, st), EUNSUP),
        ('lpips_tap_fwd C=96', lib.p2l_lpips_tap_fwd(A, B, z, C_, D_, z, O1, 1, 4, 96, st), EUNSUP),
        ('lpips_tap_bwd C=32', lib.p2l_lpips_tap_bwd(A, B, z, C_, D_, z, E, O1, 1, 4, 32, st), EUNSUP),
        ('lpips_tap_pool_bwd C=96', lib.p2l_lpips_tap_pool_bwd(A, B, z, C_, D_, z, E, F_, O1, O2, 1, 2, 16, 96, st), EUNSUP),
        ('lpips_tap_pool_bwd NULL f', lib.p2l_lpips_tap_pool_bwd(None, B, z, C_, D_, z, E, F_, O1, O2, 1, 2, 8, 64, st), EINVAL),
        ('lpips_tap_pool_bwd NULL df', lib.p2l_lpips_tap_pool_bwd(A, B, z, C_, D_, z, E, F_, None, O2, 1, 2, 8, 64, st), EINVAL),
        ('lpips_tap_pool_bwd H odd', lib.p2l_lpips_tap_pool_bwd(A, B, z, C_, D_, z, E, F_, O1, O2, 1, 3, 8, 64, st), EINVAL),
        ('lpips_tap_pool_bwd W % half', lib.p2l_lpips_tap_pool_bwd(A, B, z, C_, D_, z, E, F_, O1, O2, 1, 2, 12, 64, st), EINVAL),
        ('lpips_tap_pool_bwd W % half, C=512', lib.p2l_lpips_tap_pool_bwd(A, B, z, C_, D_, z, E, F_, O1, O2, 1, 2, 3, 512, st), EINVAL),
        ('lpips_tap_pool_bwd Bn<1', lib.p2l_lpips_tap_pool_bwd(A, B, z, C_, D_, z, E, F_, O1, O2, 0, 2, 8, 64, st), EINVAL),
        ('bilinear_adjoint h>H', lib.p2l_bilinear_adjoint(A, O1, 1, 8, 8, 9, 8, st), EINVAL),
        ('bilinear_adjoint w>W', lib.p2l_bilinear_adjoint(A, O1, 1, 8, 8, 8, 9, st), EINVAL),
        ('bilinear_adjoint h<1', lib.p2l_bilinear_adjoint(A, O1, 1, 8, 8, 0, 8, st), EINVAL),
        ('maxpool2_bwd C%4', lib.p2l_maxpool2_bwd(A, 8, B, 8, C_, 8, O1, 8, 1, 4, 4, 6, 0, st), EINVAL),
        ('maxpool2_bwd H odd', lib.p2l_maxpool2_bwd(A, 4, B, 4, C_, 4, O1, 4, 1, 3, 4, 4, 0, st), EINVAL),
        ('maxpool2_bwd W odd', lib.p2l_maxpool2_bwd(A, 4, B, 4, C_, 4, O1, 4, 1, 4, 3, 4, 1, st), EINVAL),
        ('maxpool2_bwd Bn<1', lib.p2l_maxpool2_bwd(A, 4, B, 4, C_, 4, O1, 4, 0, 4, 4, 4, 0, st), EINVAL),
        ('maxpool2_bwd Bn>65535', lib.p2l_maxpool2_bwd(A, 4, B, 4, C_, 4, O1, 4, 65536, 2, 2, 4, 0, st), EINVAL),
        ('maxpool2_bwd_amax C%4', lib.p2l_maxpool2_bwd_amax(A, 8, B, 8, C_, 8, O1, 8, 1, 4, 4, 6, 0, O2, st), EINVAL),
        ('maxpool2_bwd_amax Bn>65535', lib.p2l_maxpool2_bwd_amax(A, 4, B, 4, C_, 4, O1, 4, 65536, 2, 2, 4, 0, O2, st), EINVAL),
        ('maxpool2_bwd_amax_slots C%4', lib.p2l_maxpool2_bwd_amax_slots(4, 4, 6), 0),
        ('maxpool2_bwd_amax_slots H odd', lib.p2l_maxpool2_bwd_amax_slots(3, 4, 4), 0),
        ('maxpool2_bwd_amax_slots W odd', lib.p2l_maxpool2_bwd_amax_slots(4, 3, 4), 0),
        ('maxpool3s2_fwd C%4', lib.p2l_maxpool3s2_fwd(A, O1, 1, 5, 5, 6, st), EINVAL),
        ('maxpool3s2_fwd Hi<3', lib.p2l_maxpool3s2_fwd(A, O1, 1, 2, 5, 4, st), EINVAL),
        ('maxpool3s2_fwd Wi<3', lib.p2l_maxpool3s2_fwd(A, O1, 1, 5, 2, 4, st), EINVAL),
        ('maxpool3s2_bwd C%4', lib.p2l_maxpool3s2_bwd(A, B, C_, O1, 1, 5, 5, 6, st), EINVAL),
        ('maxpool3s2_bwd Hi<3', lib.p2l_maxpool3s2_bwd(A, B, C_, O1, 1, 2, 5, 4, st), EINVAL),
        ('maxpool3s2_bwd Wi<3', lib.p2l_maxpool3s2_bwd(A, B, C_, O1, 1, 5, 2, 4, st), EINVAL),
        ('conv1_dgrad Co%4', lib.p2l_conv1_dgrad(A, B, O1, 1, 8, 8, 6, 3, 2, 0, st), EINVAL),
        ('conv1_dgrad K<1', lib.p2l_conv1_dgrad(A, B, O1, 1, 8, 8, 4, 0, 2, 0, st), EINVAL),
        ('conv1_dgrad S<1', lib.p2l_conv1_dgrad(A, B, O1, 1, 8, 8, 4, 3, 0, 0, st), EINVAL),
    ]
    bad = [(what, rc, want) for what, rc, want in calls if rc != want]
    assert not bad, bad
    assert is_sentinel(o1.cpu()) and is_sentinel(o2.cpu())

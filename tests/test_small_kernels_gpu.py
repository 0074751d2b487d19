"""Every small entry point of include/p2l.h against a float64 reference of its own (tests/_small_refs.py), called
through ctypes at sizes that are not multiples of the launch geometry, at the production sizes, with every flag,
with guard bands around every output and with values on the decision edges.

Exact kernels (copies, masks, clamps, one-rounding updates) are compared bit for bit.  Rounded kernels are held to
    |got - r64| / sum_i |t_i|  <=  bar * 2^-24,      r = sum_i t_i, the t_i from the fp64 reference,
where bar = k, the number of roundings on the longest dependency chain that the header's formula and the documented
summation imply (written next to each call).  The same metric is evaluated for a straightforward fp32 torch-CPU
restatement (the reference functions called with float32 tensors); a derived k above 4 x that figure is tightened to
4 x it.  So that neither maximum is the luck of a handful of elements, every rounded case is drawn with SEEDS
or more independent seeds (up to MAX_SEEDS where an output has one or a few elements, until MIN_ELEMS of them are
behind the maxima): the kernel's figure is its maximum over all of them, the fp32 figure the restatement's maximum
over the same draws (`seeded`); the exact comparisons, guard bands and flags are checked on every draw.
P2L_SMALL_ERR_FILE=<path> records kernel figure, fp32 figure and bar of every case, merged into what the file already
holds (profiles/small_kernels_err.txt)."""
import ctypes as ct
import math

import pytest
import torch

import _small_refs as R
from _pin import D64, SENT, U, N, Out, _gen, _record_file, d64, hold, is_sentinel, randn, seeded  # noqa: F401

pytestmark = pytest.mark.gpu


FLAT = [1, 255, 256, 257, 65537]                 # 65537: a prime above 65 536


# =====================================================================================================================
# StyleGAN2 mapping
# =====================================================================================================================
@pytest.mark.parametrize('D', [1, 63, 64, 65, 512])
@pytest.mark.parametrize('Bn', [1, 3, 4, 5, 18, 22])
@seeded
def test_sg2_pixelnorm_fwd_bwd(dev, N, Bn, D):
    lib, g = N.lib(), _gen(1, Bn, D)
    z, dy = randn(g, Bn, D), randn(g, Bn, D)

    def run(z_, dy_):
        b = z_.shape[0]
        y, dz = Out(dev, b * D), Out(dev, b * D)
        N.check(lib.p2l_sg2_pixelnorm_fwd(N.ptr(z_.to(dev)), N.ptr(y.t), b, D, N.stream()), 'pixelnorm_fwd')
        N.check(lib.p2l_sg2_pixelnorm_bwd(N.ptr(z_.to(dev)), N.ptr(dy_.to(dev)), N.ptr(dz.t), b, D, N.stream()),
                'pixelnorm_bwd')
        return y.cpu(b, D), dz.cpu(b, D)
    y, dz = run(z, dy)
    y2, dz2 = run(z, dy)
    assert torch.equal(y, y2) and torch.equal(dz, dz2)
    for b in {0, Bn - 1}:                                     # a row does not depend on its batch
        yb, dzb = run(z[b:b + 1], dy[b:b + 1])
        assert torch.equal(yb[0], y[b]) and torch.equal(dzb[0], dz[b])
    z6, dy6 = d64(z, dy)
    case = 'Bn=%d D=%d' % (Bn, D)
    seq = math.ceil(D / 64)
    # sum of D squares: 1 (square) + seq adds per lane + 6 (wave tree); / D, + eps: 2; rsqrt halves that and adds its
    # own 2 (1 ulp); one multiply
    k_r = (1 + seq + 6 + 2) / 2 + 2
    ref = R.pixelnorm(z6)
    hold('p2l_sg2_pixelnorm_fwd:y', case, y, ref, ref.abs(), R.pixelnorm(z), k_r + 1)
    # dz = r dy - z r^3 (z.dy)/D: terms r dy_j and z_j r^3 z_i dy_i / D.  dot: 1 + seq + 6; r^3 dot / D: 3 k_r + 4;
    # z * c and the subtraction: 2
    r = torch.rsqrt((z6 * z6).mean(1, keepdim=True) + 1e-8)
    den = (r * dy6).abs() + z6.abs() * r ** 3 * (z6 * dy6).abs().sum(1, keepdim=True) / D
    hold('p2l_sg2_pixelnorm_bwd:dz', case, dz, R.vjp(R.pixelnorm, [z6], dy6), den, R.vjp(R.pixelnorm, [z], dy),
         (1 + seq + 6) + 3 * k_r + 4 + 2)


@pytest.mark.parametrize('Bn,D', [(1, 1), (1, 255), (1, 256), (1, 257), (1, 65537), (18, 512), (22, 512), (3, 65)])
@seeded
def test_sg2_bias_lrelu_fwd_and_lrelu_bwd(dev, N, Bn, D):
    lib, g = N.lib(), _gen(2, Bn, D)
    n = Bn * D
    x, bias, gr = randn(g, Bn, D), randn(g, D), randn(g, Bn, D)
    bias[::3] = 0.0
    x[:, ::6] = 0.0                                          # pre-activation exactly +0 ...
    x[:, 3::6] = -0.0                                        # ... and -0: the negative slope, like torch.where(v > 0)
    mul = 0.01

    def run():
        xo = Out(dev, n, prefill=x)                          # in place
        N.check(lib.p2l_sg2_bias_lrelu_fwd(N.ptr(xo.t), N.ptr(bias.to(dev)), N.f32(mul), Bn, D, N.stream()), 'bl')
        y = xo.cpu(Bn, D)
        go = Out(dev, n, prefill=gr)                         # in place on g
        N.check(lib.p2l_sg2_lrelu_bwd(N.ptr(y.to(dev)), N.ptr(go.t), n, N.stream()), 'lrelu_bwd')
        return y, go.cpu(Bn, D)
    y, gy = run()
    y2, gy2 = run()
    assert torch.equal(y, y2) and torch.equal(gy, gy2)
    x6, b6 = d64(x, bias)
    mul32 = float(torch.tensor(mul, dtype=torch.float32))
    ref = R.bias_lrelu(x6, b6, mul32)
    slope = torch.where(x6 + b6 * mul32 > 0, torch.tensor(R.SQRT2, dtype=D64), torch.tensor(R.SLOPE * R.SQRT2, dtype=D64))
    # x + bias * mul: 2 (or one fma); times the slope constant: 1, the constant's own rounding: 1
    hold('p2l_sg2_bias_lrelu_fwd:x', 'Bn=%d D=%d' % (Bn, D), y, ref, slope * (x6.abs() + (b6 * mul32).abs()),
         R.bias_lrelu(x, bias, mul32), 4)
    # one fp32 multiply by the fp32 constant: bit-exact
    s2 = torch.tensor(1.41421356237, dtype=torch.float32)
    want = gr * torch.where(y > 0, s2, torch.tensor(0.2, dtype=torch.float32) * s2)
    assert torch.equal(gy, want)
    assert (gy.to(D64) - R.lrelu_bwd(y.to(D64), gr.to(D64))).abs().max().item() <= 2 * U * gr.abs().max().item() * 1.5


# =====================================================================================================================
# StyleGAN2 modulation
# =====================================================================================================================
@pytest.mark.parametrize('Cin,Cout', [(512, 512), (64, 32), (32, 3)])
@pytest.mark.parametrize('Bn', [1, 18, 22])
@seeded
def test_sg2_demod_fwd_bwd(dev, N, Bn, Cin, Cout):
    lib, g = N.lib(), _gen(3, Bn, Cin, Cout)
    s = randn(g, Bn, Cin) + 1.0
    Wsq = torch.rand(Cin, Cout, generator=g) / Cin
    dd = randn(g, Bn, Cout)
    pre = randn(g, Bn, Cin)
    d_in = R.demod(s.to(D64), Wsq.to(D64)).float()          # the saved d the backward is handed

    def run(s_, d_, dd_, pre_, acc):
        b = s_.shape[0]
        d, ds = Out(dev, b * Cout), Out(dev, b * Cin, prefill=pre_ if acc else None)
        N.check(lib.p2l_sg2_demod_fwd(N.ptr(s_.to(dev)), N.ptr(Wsq.to(dev)), N.ptr(d.t), b, Cin, Cout, N.stream()), 'demod')
        N.check(lib.p2l_sg2_demod_bwd(N.ptr(s_.to(dev)), N.ptr(Wsq.to(dev)), N.ptr(d_.to(dev)), N.ptr(dd_.to(dev)),
                                      N.ptr(ds.t), b, Cin, Cout, acc, N.stream()), 'demod_bwd')
        return d.cpu(b, Cout), ds.cpu(b, Cin)
    s6, W6, dd6, d6 = d64(s, Wsq, dd, d_in)
    ref_d = R.demod(s6, W6)
    # the gradient w.r.t. s THROUGH the d the kernel is handed: sum_o dd_o * (-d_o^3 / 2) * 2 s_i Wsq_io
    ref_ds = R.vjp(lambda s_: R.demod(s_, W6), [s6], dd6 * (d6 / ref_d) ** 3)
    den_ds = 2 * s6.abs() * ((dd6 * 0.5 * d6 ** 3).abs() @ W6.t())
    for acc in (0, 1):
        d, ds = run(s, d_in, dd, pre, acc)
        d2, ds2 = run(s, d_in, dd, pre, acc)
        assert torch.equal(d, d2) and torch.equal(ds, ds2)
        b = Bn - 1
        db, dsb = run(s[b:b + 1], d_in[b:b + 1], dd[b:b + 1], pre[b:b + 1], acc)
        assert torch.equal(db[0], d[b]) and torch.equal(dsb[0], ds[b])
        case = 'Bn=%d %dx%d acc=%d' % (Bn, Cin, Cout, acc)
        if acc == 0:
            # q: Cin fma in sequence + 1 (s^2) + 1 (eps), halved by the rsqrt; rsqrt: 2
            hold('p2l_sg2_demod_fwd:d', case, d, ref_d, ref_d.abs(), R.demod(s, Wsq), (Cin + 2) / 2 + 2)
        # -0.5 d^3 dd: 4; Cout fma in sequence; 2 s a: 1 (the 2 is exact); accumulate: 1
        f32 = R.vjp(lambda s_: R.demod(s_, Wsq), [s], dd)
        hold('p2l_sg2_demod_bwd:ds', case, ds, ref_ds + (pre.to(D64) if acc else 0), den_ds + (pre.to(D64).abs() if acc else 0),
             f32 + (pre if acc else 0), 4 + Cout + 1 + acc)


@pytest.mark.parametrize('skip_on', [0, 1])
@pytest.mark.parametrize('Bn,H,W,C', [(1, 12, 12, 32), (3, 16, 16, 64), (2, 20, 20, 96), (18, 8, 8, 64), (22, 4, 4, 512)])
@seeded
def test_scale_bwd(dev, N, Bn, H, W, C, skip_on):
    lib, g = N.lib(), _gen(4, Bn, H, W, C)
    P, ld = H * W, C + 32                                     # pitched da / x / dx: 32 gap channels
    nblk = lib.p2l_affine_relu_bwd_nblk(P)
    da, x, s = randn(g, Bn, P, C), randn(g, Bn, P, C), randn(g, Bn, C)
    skip_C = 32
    skip = randn(g, Bn, P, skip_C) if skip_on else None

    def pitched(t):
        o = torch.zeros(t.shape[0], P, ld)
        o[..., :C] = t
        return o.to(dev)

    def run(da_, x_, s_, skip_):
        b = da_.shape[0]
        dx, ds, dts = Out(dev, b * P * ld), Out(dev, b * C), Out(dev, b * C)
        part = Out(dev, 2 * b * nblk * C)
        N.check(lib.p2l_scale_bwd(N.ptr(pitched(da_)), ld, N.ptr(pitched(x_)), ld, N.ptr(s_.to(dev)), C,
                                  N.ptr(skip_.contiguous().to(dev)) if skip_ is not None else None, skip_C, skip_C,
                                  N.ptr(dx.t), ld, N.ptr(ds.t), N.ptr(dts.t), C, N.ptr(part.t), b, H, W, C,
                                  N.stream()), 'scale_bwd')
        dxc = dx.cpu(b, P, ld)
        assert is_sentinel(dxc[..., C:]), 'gap columns of the pitched dx written'
        part.cpu()
        dts.cpu()
        return dxc[..., :C].contiguous(), ds.cpu(b, C)
    dx, ds = run(da, x, s, skip)
    dx2, ds2 = run(da, x, s, skip)
    assert torch.equal(dx, dx2) and torch.equal(ds, ds2)
    b = Bn - 1
    dxb, dsb = run(da[b:b + 1], x[b:b + 1], s[b:b + 1], None if skip is None else skip[b:b + 1])
    assert torch.equal(dxb[0], dx[b]) and torch.equal(dsb[0], ds[b])
    da6, x6, s6, sk6 = d64(da, x, s, skip)
    rdx, rds = R.scale_bwd(da6, x6, s6, sk6, skip_C)
    fdx, fds = R.scale_bwd(da, x, s, skip, skip_C)
    den = (da6 * s6[:, None]).abs()
    if skip_on:
        den[..., :skip_C] += sk6.abs()
    case = 'Bn=%d %dx%d C=%d skip=%d' % (Bn, H, W, C, skip_on)
    hold('p2l_scale_bwd:dx', case, dx, rdx, den, fdx, 2)                   # multiply, add
    # product 1; 16 pixels per thread in sequence; 15 adds over the pixel lanes; finish: ceil(nblk / 64) per chain,
    # 2 to combine the chains, 15 over the segments
    hold('p2l_scale_bwd:ds', case, ds, rds, (da6 * x6).abs().sum(1), fds, 1 + 16 + 15 + math.ceil(nblk / 64) + 2 + 15)


# =====================================================================================================================
# StyleGAN2 styled-conv activation backward (+ deferred second stage)
# =====================================================================================================================
def _act_case(g, Bn, P, C, regime, with_noise):
    """inputs built FORWARDS from the true conv result c (fp64)"""
    c = torch.randn(Bn, P, C, generator=g, dtype=D64)                  # unit variance, d in [0.5, 1.5]: |c d| ~ 1
    d = (0.5 + torch.rand(Bn, C, generator=g)).to(D64)                 # fp32-representable: the kernel's input
    # A: nw = 0.3 (noise term 0.3 sigma), bias 0.1 sigma.  B: nw = 100 and bias 100 sigma, both 100 x the conv term
    nw = float(torch.tensor(100.0 if regime == 'B' else 0.3, dtype=torch.float32))
    noise = torch.randn(Bn, P, generator=g).to(D64) if with_noise else None
    bias = ((100.0 if regime == 'B' else 0.1) * torch.randn(C, generator=g)).to(D64)
    dy = torch.randn(Bn, P, C, generator=g).to(D64)
    y = R.styled_act(c, d, noise, nw, bias).float()                     # y = fp32(lrelu(pre) * sqrt2)
    return c, d, nw, noise, bias, dy, y


def _act_run(dev, N, dy, y, d, noise, nw, bias, want_dn, amax=False):
    lib = N.lib()
    Bn, P, C = dy.shape
    nblk = lib.p2l_sg2_act_bwd_nblk(P)
    assert nblk == (P + 255) // 256
    gd, dd, part = Out(dev, Bn * P * C), Out(dev, Bn * C), Out(dev, Bn * nblk * C)
    dn = Out(dev, Bn * P)
    strips = Out(dev, (C // (32 if C % 64 else 64)) * Bn * P)           # exactly what p2l.h documents
    args = [N.ptr(dy.float().to(dev)), N.ptr(y.to(dev)), N.ptr(d.float().to(dev)),
            N.ptr(noise.float().to(dev)) if noise is not None else None, N.f32(nw), N.ptr(bias.float().to(dev)),
            N.ptr(gd.t), N.ptr(dd.t), N.ptr(dn.t) if want_dn else None, N.ptr(part.t),
            N.ptr(strips.t) if want_dn else None, Bn, P, C]
    if amax:
        am = torch.zeros(Bn, 64, device=dev)
        N.check(lib.p2l_sg2_styled_act_bwd_amax(*(args + [N.ptr(am), N.stream()])), 'styled_act_bwd_amax')
    else:
        N.check(lib.p2l_sg2_styled_act_bwd(*(args + [N.stream()])), 'styled_act_bwd')
    part.cpu()
    strips.cpu()
    dnc = dn.cpu(Bn, P)
    if not want_dn:
        assert is_sentinel(dnc)
    return gd.cpu(Bn, P, C), dd.cpu(Bn, C), dnc if want_dn else None


@pytest.mark.parametrize('regime', ['A', 'B'])
@pytest.mark.parametrize('Bn,HW,C,noise_on,dn_on', [(2, 12, 32, 1, 1), (3, 20, 64, 1, 1), (2, 12, 96, 1, 1),
                                                   (1, 16, 512, 1, 0), (18, 8, 64, 0, 0), (22, 4, 512, 1, 1)])
@seeded
def test_sg2_styled_act_bwd(dev, N, Bn, HW, C, noise_on, dn_on, regime):
    """Regime A: conv term, noise term and bias of comparable size.  Regime B: bias and noise 100 x the conv term,
    where recomputing c = ((y / slope) - bias - nw noise) / d from the rounded y cancels; the bound for dd is the
    one inherent in that recompute, sum_p |g| (|pre| + |nw noise| + |bias|) / |d| -- measured figures in
    profiles/small_kernels_err.txt."""
    g = _gen(5, Bn, HW, C, regime)
    P = HW * HW
    c, d, nw, noise, bias, dy, y = _act_case(g, Bn, P, C, regime, noise_on)
    gd, dd, dn = _act_run(dev, N, dy, y, d, noise, nw, bias, dn_on)
    for amax in (False, True):
        gd2, dd2, dn2 = _act_run(dev, N, dy, y, d, noise, nw, bias, dn_on, amax=amax)
        assert torch.equal(gd, gd2) and torch.equal(dd, dd2) and (dn is None or torch.equal(dn, dn2))
    b = Bn - 1
    gdb, ddb, dnb = _act_run(dev, N, dy[b:b + 1], y[b:b + 1], d[b:b + 1], None if noise is None else noise[b:b + 1],
                             nw, bias, dn_on)
    assert torch.equal(gdb[0], gd[b]) and torch.equal(ddb[0], dd[b]) and (dn is None or torch.equal(dnb[0], dn[b]))
    rgd, rdd, rdn = R.styled_act_bwd(dy, c, d, noise, nw, bias)
    # the fp32 restatement: the header's formula on the saved fp32 y
    y32, dy32, d32, b32 = y, dy.float(), d.float(), bias.float()
    sl = torch.where(y32 > 0, torch.tensor(1.41421356237), torch.tensor(0.2) * torch.tensor(1.41421356237))
    g32 = dy32 * sl
    nz32 = (torch.tensor(nw) * noise.float())[:, :, None] if noise is not None else 0.0
    dd32 = (g32 * ((y32 / sl - b32 - nz32) / d32[:, None])).sum(1)
    case = '%s Bn=%d %dx%d C=%d' % (regime, Bn, HW, HW, C)
    g1 = (rgd / d[:, None])                                             # dy * lrelu'(pre)
    hold('p2l_sg2_styled_act_bwd:gd', case, gd, rgd, rgd.abs(), g32 * d32[:, None], 3)      # slope const, 2 multiplies
    pre = c * d[:, None] + bias + (nw * noise[:, :, None] if noise is not None else 0.0)
    mag = pre.abs() + bias.abs()
    if noise is not None:
        mag = mag + (nw * noise[:, :, None]).abs()
    den = (g1.abs() * mag).sum(1) / d.abs()
    sw = 32 if C % 64 else 64
    nblk = (P + 255) // 256
    # y rounded to fp32: 1; y / slope: 2; - bias, nw * noise, - that, / d: 4; g: 2; g * c: 1; the sum: 256 / PL pixels
    # per thread in sequence, PL - 1 over the pixel lanes (PL = 1024 / strip width), ceil(nblk / 16) + 15 to finish
    PL = 1024 // sw
    hold('p2l_sg2_styled_act_bwd:dd', case, dd, rdd, den, dd32, 10 + 256 // PL + PL - 1 + math.ceil(nblk / 16) + 15)
    if dn_on:
        # g: 2; 3 adds in the thread; log2(strip / 4) shuffles; C / strip strips in sequence; times nw: 1
        hold('p2l_sg2_styled_act_bwd:dnoise', case, dn, rdn, abs(nw) * g1.abs().sum(2), torch.tensor(nw) * g32.sum(2),
             2 + 3 + int(math.log2(sw // 4)) + C // sw + 1)


def test_sg2_styled_act_bwd_zero_takes_the_negative_slope(dev, N):
    """y == +0 / -0: lrelu'(y) is the negative slope, the branch torch.where(v > 0, ...) takes"""
    Bn, P, C = 1, 16, 32
    g = _gen(6)
    y = torch.randn(Bn, P, C, generator=g)
    y[:, ::2, ::3] = 0.0
    y[:, 1::2, 1::3] = -0.0
    dy = torch.randn(Bn, P, C, generator=g)
    d = 0.5 + torch.rand(Bn, C, generator=g)
    gd, _, _ = _act_run(dev, N, dy, y, d, None, 0.0, torch.zeros(C), 0)
    s2 = torch.tensor(1.41421356237)
    want = dy * torch.where(y > 0, s2, torch.tensor(0.2) * s2) * d[:, None]
    assert torch.equal(gd, want)


def test_sg2_rows_defer_begin_flush_cancel(dev, N):
    """the deferred second stage gives the dd of the immediate one, bit for bit; _cancel runs nothing; a full group and
    a change of Bn inside a group flush early"""
    lib = N.lib()
    g = _gen(7)
    layers = [(2, 144, 32), (2, 400, 64), (2, 64, 96)]

    def make(Bn, P, C):
        c, d, nw, noise, bias, dy, y = _act_case(g, Bn, P, C, 'A', True)
        return dict(dy=dy.float().to(dev), y=y.to(dev), d=d.float().to(dev), noise=noise.float().to(dev), nw=nw,
                    bias=bias.float().to(dev), Bn=Bn, P=P, C=C)

    def call(L):
        Bn, P, C = L['Bn'], L['P'], L['C']
        nblk = lib.p2l_sg2_act_bwd_nblk(P)
        gd, dd, part = Out(dev, Bn * P * C), Out(dev, Bn * C), Out(dev, Bn * nblk * C)
        N.check(lib.p2l_sg2_styled_act_bwd(N.ptr(L['dy']), N.ptr(L['y']), N.ptr(L['d']), N.ptr(L['noise']),
                                           N.f32(L['nw']), N.ptr(L['bias']), N.ptr(gd.t), N.ptr(dd.t), None,
                                           N.ptr(part.t), None, Bn, P, C, N.stream()), 'styled_act_bwd')
        return gd, dd, part
    cases = [make(*l) for l in layers]
    now = [call(L)[1].cpu() for L in cases]
    # deferred: nothing in dd before the flush, the same bits after it
    lib.p2l_sg2_rows_defer_begin()
    held = [call(L) for L in cases]
    assert all(is_sentinel(h[1].cpu()) for h in held)
    N.check(lib.p2l_sg2_rows_defer_flush(N.stream()), 'flush')
    for h, want in zip(held, now):
        assert torch.equal(h[1].cpu(), want)
    # cancel: nothing recorded is run, and the next un-deferred call works
    lib.p2l_sg2_rows_defer_begin()
    held = [call(L) for L in cases]
    lib.p2l_sg2_rows_defer_cancel()
    N.check(lib.p2l_sg2_rows_defer_flush(N.stream()), 'flush after cancel')
    assert all(is_sentinel(h[1].cpu()) for h in held)
    assert torch.equal(call(cases[0])[1].cpu(), now[0])
    # more layers than a group holds (20), and a change of Bn inside the group: early flushes, same bits
    other = make(3, 144, 32)
    other_now = call(other)[1].cpu()
    lib.p2l_sg2_rows_defer_begin()
    held = [call(cases[i % 3]) for i in range(23)]
    ho = call(other)
    held2 = [call(cases[i % 3]) for i in range(2)]
    N.check(lib.p2l_sg2_rows_defer_flush(N.stream()), 'flush')
    for i, h in enumerate(held):
        assert torch.equal(h[1].cpu(), now[i % 3])
    assert torch.equal(ho[1].cpu(), other_now)
    for i, h in enumerate(held2):
        assert torch.equal(h[1].cpu(), now[i % 3])


# =====================================================================================================================
# StyleGAN2 image tail
# =====================================================================================================================
@pytest.mark.parametrize('h,w', [(1, 1), (4, 4), (3, 5), (64, 64)])
@pytest.mark.parametrize('Bn', [1, 18])
@seeded
def test_sg2_rgb_up_fwd_bwd(dev, N, Bn, h, w):
    lib, g = N.lib(), _gen(8, Bn, h, w)
    skip, dout, pre = randn(g, Bn, h, w, 16), randn(g, Bn, 2 * h, 2 * w, 16), randn(g, Bn, h, w, 16)

    def run(skip_, dout_, pre_, acc):
        b = skip_.shape[0]
        out, dsk = Out(dev, b * 4 * h * w * 16), Out(dev, b * h * w * 16, prefill=pre_ if acc else None)
        N.check(lib.p2l_sg2_rgb_up_fwd(N.ptr(skip_.to(dev)), N.ptr(out.t), b, h, w, N.stream()), 'rgb_up_fwd')
        N.check(lib.p2l_sg2_rgb_up_bwd(N.ptr(dout_.to(dev)), N.ptr(dsk.t), b, h, w, acc, N.stream()), 'rgb_up_bwd')
        return out.cpu(b, 2 * h, 2 * w, 16), dsk.cpu(b, h, w, 16)
    s6, do6, pre6 = d64(skip, dout, pre)
    ref, den = R.rgb_up(s6), R.rgb_up(s6.abs())
    rds, dds = R.rgb_up_bwd(do6, h, w), R.rgb_up_bwd(do6.abs(), h, w)
    for acc in (0, 1):
        out, dsk = run(skip, dout, pre, acc)
        out2, dsk2 = run(skip, dout, pre, acc)
        assert torch.equal(out, out2) and torch.equal(dsk, dsk2)
        outb, dskb = run(skip[-1:], dout[-1:], pre[-1:], acc)
        assert torch.equal(outb[0], out[-1]) and torch.equal(dskb[0], dsk[-1])
        case = 'Bn=%d %dx%d acc=%d' % (Bn, h, w, acc)
        assert torch.equal(out[..., 4:], torch.zeros_like(out[..., 4:]))
        if acc == 0:
            # weight * value: 1, pair sum: 1, * row weight: 1, sum of the two rows: 1
            hold('p2l_sg2_rgb_up_fwd:out', case, out[..., :4], ref[..., :4], den[..., :4], R.rgb_up(skip)[..., :4], 4)
            assert torch.equal(dsk[..., 4:], torch.zeros_like(dsk[..., 4:]))
            hold('p2l_sg2_rgb_up_bwd:dskip', case, dsk[..., :4], rds[..., :4], dds[..., :4],
                 R.rgb_up_bwd(dout, h, w)[..., :4], 9)           # (1 + 3) per row, (1 + 3) over the rows, and 1
        else:
            assert torch.equal(dsk[..., 4:], pre[..., 4:])       # accumulate leaves channels 4..15
            hold('p2l_sg2_rgb_up_bwd:dskip', case, dsk[..., :4], rds[..., :4] + pre6[..., :4],
                 dds[..., :4] + pre6[..., :4].abs(), R.rgb_up_bwd(dout, h, w)[..., :4] + pre[..., :4], 10)


@pytest.mark.parametrize('P', FLAT + [18 * 64 * 64])
def test_sg2_clamp16_fwd_bwd_add_inplace_broadcast_rows(dev, N, P):
    lib, g = N.lib(), _gen(9, P)
    x = randn(g, P, 16) * 1.5
    edge = torch.tensor([1.0, -1.0, 0.0, -0.0, 1.0000001, -1.0000001, 0.99999994, -0.99999994])
    for i in range(min(P, 3)):                               # exactly at +-1, one ulp either side, +-0: channels 0..2
        x[i, :3] = edge[[i, 3 + i, (6 + i) % 8]]
    dy = randn(g, P, 16)
    y, dx = Out(dev, P * 16), Out(dev, P * 16)
    N.check(lib.p2l_sg2_clamp16_fwd(N.ptr(x.to(dev)), N.ptr(y.t), N.i64(P), N.stream()), 'clamp16_fwd')
    N.check(lib.p2l_sg2_clamp16_bwd(N.ptr(x.to(dev)), N.ptr(dy.to(dev)), N.ptr(dx.t), N.i64(P), N.stream()), 'clamp16_bwd')
    assert torch.equal(y.cpu(P, 16), R.clamp16(x))                       # channels 3..15 written as zero
    assert torch.equal(dx.cpu(P, 16), R.clamp16_bwd(x, dy))              # +-1 pass their gradient (torch.clamp)
    # add_inplace: one rounding, a + b in fp32; n = 16 P floats and n = P
    for n in (P, 16 * P):
        a, b = x.view(-1)[:n].clone(), dy.view(-1)[:n].clone()
        ao = Out(dev, n, prefill=a)
        N.check(lib.p2l_add_inplace(N.ptr(ao.t), N.ptr(b.to(dev)), N.i64(n), N.stream()), 'add_inplace')
        assert torch.equal(ao.cpu(), a + b)
    # broadcast_rows: dst[b] = src for every b
    for Bn in (1, 3, 18):
        src = dy.view(-1)[:P].clone()
        dst = Out(dev, P * Bn)
        N.check(lib.p2l_broadcast_rows(N.ptr(src.to(dev)), N.ptr(dst.t), N.i64(P), Bn, N.stream()), 'broadcast_rows')
        assert torch.equal(dst.cpu(Bn, P), src.repeat(Bn, 1))


# =====================================================================================================================
# BigGAN conditioning
# =====================================================================================================================
@pytest.mark.parametrize('C,raw_ld', [(1, 1), (255, 255), (257, 300), (512, 2 * 4096), (2048, 2 * 19000 // 4 * 4)])
@pytest.mark.parametrize('Bn', [1, 18, 22])
@seeded
def test_cbn_fold_fwd_bwd(dev, N, Bn, C, raw_ld):
    """raw_ld > C: g_raw / b_raw (and their gradients) are slices of the rows of the one big linear"""
    lib, g = N.lib(), _gen(10, Bn, C)
    g_raw, b_raw = 0.3 * randn(g, Bn, C), randn(g, Bn, C)
    mean, rstd = randn(g, C), 0.5 + torch.rand(C, generator=g)
    ds, dt = randn(g, Bn, C), randn(g, Bn, C)

    def run(sl):
        nb = sl.stop - sl.start
        span = (nb - 1) * raw_ld + C

        def rows(t):                                         # [nb, C] at pitch raw_ld
            o = torch.zeros(nb * raw_ld)
            o.view(nb, raw_ld)[:, :C] = t[sl]
            return o[:span].contiguous().to(dev)

        def unrows(o):
            tail = torch.full((nb * raw_ld - span,), SENT, dtype=torch.int32).view(torch.float32)
            full = torch.cat([o, tail]).view(nb, raw_ld)
            assert is_sentinel(full[:, C:]), 'gap columns of the pitched gradient written'
            return full[:, :C].contiguous()
        s, t = Out(dev, nb * C), Out(dev, nb * C)
        dg, db = Out(dev, span), Out(dev, span)
        N.check(lib.p2l_cbn_fold_fwd(N.ptr(rows(g_raw)), N.ptr(rows(b_raw)), N.ptr(mean.to(dev)), N.ptr(rstd.to(dev)),
                                     N.ptr(s.t), N.ptr(t.t), nb, C, raw_ld, N.stream()), 'cbn_fold_fwd')
        N.check(lib.p2l_cbn_fold_bwd(N.ptr(ds[sl].contiguous().to(dev)), N.ptr(dt[sl].contiguous().to(dev)),
                                     N.ptr(mean.to(dev)), N.ptr(rstd.to(dev)), N.ptr(dg.t), N.ptr(db.t), nb, C, raw_ld,
                                     N.stream()), 'cbn_fold_bwd')
        return s.cpu(nb, C), t.cpu(nb, C), unrows(dg.cpu()), unrows(db.cpu())
    s, t, dg, db = run(slice(0, Bn))
    assert all(torch.equal(a, b) for a, b in zip((s, t, dg, db), run(slice(0, Bn))))
    for b in {0, Bn - 1}:                                    # a row does not depend on its batch
        assert all(torch.equal(one[0], full[b]) for one, full in zip(run(slice(b, b + 1)), (s, t, dg, db)))
    g6, b6, m6, r6, ds6, dt6 = d64(g_raw, b_raw, mean, rstd, ds, dt)
    rs, rt = R.cbn_fold(g6, b6, m6, r6)
    fs, ft = R.cbn_fold(g_raw, b_raw, mean, rstd)
    case = 'Bn=%d C=%d ld=%d' % (Bn, C, raw_ld)
    den_s = r6.abs() * (1 + g6.abs())
    hold('p2l_cbn_fold_fwd:s', case, s, rs, den_s, fs, 2)                          # 1 + g, * rstd
    hold('p2l_cbn_fold_fwd:t', case, t, rt, b6.abs() + m6.abs() * den_s, ft, 4)    # s: 2, mean * s, the subtraction
    rdg, rdb = R.cbn_fold_bwd(ds6, dt6, m6, r6)
    fdg, _ = R.cbn_fold_bwd(ds, dt, mean, rstd)
    hold('p2l_cbn_fold_bwd:dg_raw', case, dg, rdg, (ds6.abs() + (dt6 * m6).abs()) * r6.abs(), fdg, 3)
    assert torch.equal(db, dt)


@pytest.mark.parametrize('Bn,nz,nc', [(1, 1, 1), (1, 128, 127), (3, 128, 128), (18, 128, 128), (22, 120, 137), (5, 13001, 113)])
def test_concat2_split2(dev, N, Bn, nz, nc):
    lib, g = N.lib(), _gen(11, Bn, nz, nc)
    z, c, dcond = randn(g, Bn, nz), randn(g, Bn, nc), randn(g, Bn, nz + nc)
    cond, dz, dc = Out(dev, Bn * (nz + nc)), Out(dev, Bn * nz), Out(dev, Bn * nc)
    N.check(lib.p2l_concat2(N.ptr(z.to(dev)), N.ptr(c.to(dev)), N.ptr(cond.t), Bn, nz, nc, N.stream()), 'concat2')
    N.check(lib.p2l_split2(N.ptr(dcond.to(dev)), N.ptr(dz.t), N.ptr(dc.t), Bn, nz, nc, N.stream()), 'split2')
    assert torch.equal(cond.cpu(Bn, nz + nc), torch.cat([z, c], dim=1))
    gz, gc = R.vjp(lambda a, b: torch.cat([a, b], dim=1), [z, c], dcond)
    assert torch.equal(dz.cpu(Bn, nz), gz) and torch.equal(dc.cpu(Bn, nc), gc)


@pytest.mark.parametrize('Bn,K,N_,nlat', [(1, 4, 1, 1), (3, 128, 65, 2), (18, 512, 512, 18), (22, 512, 512, 16), (17, 256, 1028, 3)])
@seeded
def test_linear_fwd_ld_bwd_ld(dev, N, Bn, K, N_, nlat):
    """rows of x / dx are one latent of a [B, n_latent, K] w+ tensor: pitch n_latent * K"""
    lib, g = N.lib(), _gen(12, Bn, K, N_)
    ld, j = nlat * K, nlat // 2
    wp, W, bias = randn(g, Bn, nlat, K), randn(g, K, N_) / math.sqrt(K), randn(g, N_)
    Nb = (N_ + 3) // 4 * 4 if N_ % 4 else N_                 # the backward needs N % 4 == 0
    dy, pre = randn(g, Bn, Nb), randn(g, Bn, nlat, K)
    Wb = randn(g, K, Nb) / math.sqrt(K)
    x = wp[:, j]

    def run(acc, sl=None):
        sl = slice(0, Bn) if sl is None else sl
        nb = sl.stop - sl.start
        wpd = wp[sl].contiguous().to(dev)
        N.alive.append(wpd)
        y = Out(dev, nb * N_)
        N.check(lib.p2l_linear_fwd_ld(ct.c_void_p(wpd.data_ptr() + 4 * j * K), ld, N.ptr(W.to(dev)), N.ptr(bias.to(dev)),
                                      N.ptr(y.t), nb, K, N_, N.stream()), 'linear_fwd_ld')
        dwp = Out(dev, nb * ld, prefill=pre[sl] if acc else None)
        N.check(lib.p2l_linear_bwd_ld(N.ptr(dy[sl].contiguous().to(dev)), N.ptr(Wb.to(dev)),
                                      ct.c_void_p(dwp.t.data_ptr() + 4 * j * K), ld, nb, K, Nb, acc, N.stream()),
                'linear_bwd_ld')
        return y.cpu(nb, N_), dwp.cpu(nb, nlat, K)
    x6, W6, b6, dy6, Wb6, pre6 = d64(x, W, bias, dy, Wb, pre)
    for acc in (0, 1):
        y, dwp = run(acc)
        y2, dwp2 = run(acc)
        assert torch.equal(y, y2) and torch.equal(dwp, dwp2)
        for b in {0, Bn - 1}:                                # a row does not depend on its batch (nor on the 16- / 24-row
            yb, dwpb = run(acc, slice(b, b + 1))             # grouping the launcher picks from Bn)
            assert torch.equal(yb[0], y[b]) and torch.equal(dwpb[0], dwp[b])
        other = torch.ones(nlat, dtype=torch.bool)
        other[j] = False
        if acc:
            assert torch.equal(dwp[:, other], pre[:, other])              # the other latents' rows: untouched
        else:
            assert is_sentinel(dwp[:, other])
        case = 'Bn=%d K=%d N=%d ld=%d acc=%d' % (Bn, K, N_, ld, acc)
        if acc == 0:
            # K / 4 fma in sequence per K-group, 2 to combine the four groups, the bias
            hold('p2l_linear_fwd_ld:y', case, y, R.linear(x6, W6, b6), x6.abs() @ W6.abs() + b6.abs(), R.linear(x, W, bias),
                 K // 4 + 3)
        # per thread ceil(N / 4096) x (1 product + 3 adds), wave tree 6, 16 waves in sequence, accumulate
        hold('p2l_linear_bwd_ld:dx', case, dwp[:, j], R.linear_bwd(dy6, Wb6) + (pre6[:, j] if acc else 0),
             dy6.abs() @ Wb6.abs().t() + (pre6[:, j].abs() if acc else 0), R.linear_bwd(dy, Wb) + (pre[:, j] if acc else 0),
             4 * math.ceil(Nb / 4096) + 6 + 16 + acc)


# =====================================================================================================================
# image layout
# =====================================================================================================================
@pytest.mark.parametrize('Bn,H,W', [(1, 1, 1), (1, 15, 17), (3, 16, 16), (1, 257, 1), (18, 24, 40), (2, 256, 256)])
@seeded
def test_nchw3_nhwc16_tanh_bwd16(dev, N, Bn, H, W):
    lib, g = N.lib(), _gen(13, Bn, H, W)
    src = randn(g, Bn, 3, H, W)
    d16, back = Out(dev, Bn * H * W * 16), Out(dev, Bn * 3 * H * W)
    N.check(lib.p2l_nchw3_to_nhwc16(N.ptr(src.to(dev)), N.ptr(d16.t), Bn, H, W, N.stream()), 'nchw3_to_nhwc16')
    got16 = d16.cpu(Bn, H, W, 16)
    assert torch.equal(got16, R.nchw3_to_nhwc16(src))                    # channels 3..15 WRITTEN as zero (p2l.h)
    assert bool((got16[..., 3:].contiguous().view(torch.int32) == 0).all())
    src16 = randn(g, Bn, H, W, 16)                                       # junk in channels 3..15 must not leak
    N.check(lib.p2l_nhwc16_to_nchw3(N.ptr(src16.to(dev)), N.ptr(back.t), Bn, H, W, N.stream()), 'nhwc16_to_nchw3')
    assert torch.equal(back.cpu(Bn, 3, H, W), R.nhwc16_to_nchw3(src16))
    # tanh backward, in place on the gradient; img in (-1, 1) with +-1 and 0 on the edges
    img = torch.tanh(2 * randn(g, Bn, H, W, 16))
    img.view(-1)[:3] = torch.tensor([1.0, -1.0, 0.0])[:min(3, img.numel())]
    dimg = randn(g, Bn, H, W, 16)
    P = Bn * H * W
    do = Out(dev, P * 16, prefill=dimg)
    N.check(lib.p2l_tanh_bwd16(N.ptr(img.to(dev)), N.ptr(do.t), N.i64(P), N.stream()), 'tanh_bwd16')
    got = do.cpu(Bn, H, W, 16)
    assert torch.equal(got[..., 4:], dimg[..., 4:]) and bool((got[..., 3] == 0).all())
    i6, di6 = d64(img, dimg)
    ref = di6[..., :3] * (1 - i6[..., :3] ** 2)                          # = autograd through tanh (test_small_refs)
    f32 = dimg[..., :3] * (1 - img[..., :3] * img[..., :3])
    hold('p2l_tanh_bwd16:dimg', 'Bn=%d %dx%d' % (Bn, H, W), got[..., :3], ref, di6[..., :3].abs() * (1 + i6[..., :3] ** 2),
         f32, 3)                                                         # o * o, 1 - that, the multiply


@pytest.mark.parametrize('P,C,ld', [(1, 4, 4), (255, 4, 8), (257, 64, 64), (65537, 4, 4), (18 * 64, 256, 320)])
def test_relu_mask(dev, N, P, C, ld):
    lib, g = N.lib(), _gen(14, P, C)
    y, gr = randn(g, P, ld), randn(g, P, ld)
    y[::2, ::3] = 0.0
    y[1::2, 1::3] = -0.0                                                 # zero and minus zero: masked, like v > 0
    dy = Out(dev, P * ld)
    N.check(lib.p2l_relu_mask(N.ptr(y.to(dev)), ld, N.ptr(gr.to(dev)), ld, N.ptr(dy.t), ld, N.i64(P), C, N.stream()),
            'relu_mask')
    got = dy.cpu(P, ld)
    assert is_sentinel(got[:, C:]) if ld > C else True
    assert torch.equal(got[:, :C], R.relu_mask(y[:, :C].contiguous(), gr[:, :C].contiguous()))


# =====================================================================================================================
# losses
# =====================================================================================================================
@pytest.mark.parametrize('mask_on', [0, 1])
@pytest.mark.parametrize('Bn,H,W', [(1, 1, 1), (3, 24, 40), (2, 5, 7), (18, 256, 256), (22, 64, 64), (1, 1024, 1024)])
@seeded
def test_weight_sum_weight_map_l1_loss(dev, N, Bn, H, W, mask_on):
    lib, g = N.lib(), _gen(15, Bn, H, W)
    HW = H * W
    out, target = torch.tanh(randn(g, Bn, 3, H, W)), torch.tanh(randn(g, Bn, 3, H, W))
    out[:, 0, 0, 0] = target[:, 0, 0, 0]                                # a tie: sign(0) = 0
    weight = torch.rand(Bn, 3, H, W, generator=g)
    mask = (torch.rand(Bn, 3, H, W, generator=g) > 0.3).float() if mask_on else None
    img16 = R.nchw3_to_nhwc16(out)
    img16[..., 3:] = 7.0                                                 # junk in the pad channels must not leak
    gscale, pre = randn(g, Bn), randn(g, Bn, H, W, 16)
    nblk = lib.p2l_l1_loss_nblk(H, W)
    assert nblk == (HW + 255) // 256
    mp = N.ptr(mask.to(dev)) if mask_on else None

    def run(sl, acc):
        b = sl.stop - sl.start
        o16, tg, wt = img16[sl].contiguous().to(dev), target[sl].contiguous().to(dev), weight[sl].contiguous().to(dev)
        mk = N.ptr(mask[sl].contiguous().to(dev)) if mask_on else None
        wsum, wmap, loss, part = Out(dev, b), Out(dev, b * HW), Out(dev, b), Out(dev, b * nblk)
        dimg = Out(dev, b * HW * 16, prefill=pre[sl] if acc else None)
        N.check(lib.p2l_weight_sum(N.ptr(wt), mk, N.ptr(wsum.t), b, 3 * HW, N.stream()), 'weight_sum')
        N.check(lib.p2l_weight_map(N.ptr(wt), mk, N.ptr(wmap.t), b, H, W, N.stream()), 'weight_map')
        N.check(lib.p2l_l1_loss_fwd(N.ptr(o16), N.ptr(tg), N.ptr(wt), mk, N.ptr(wsum.t), N.ptr(loss.t), N.ptr(part.t),
                                    b, H, W, N.stream()), 'l1_loss_fwd')
        N.check(lib.p2l_l1_loss_bwd(N.ptr(o16), N.ptr(tg), N.ptr(wt), mk, N.ptr(wsum.t), N.ptr(gscale[sl].contiguous().to(dev)),
                                    N.ptr(dimg.t), b, H, W, acc, N.stream()), 'l1_loss_bwd')
        part.cpu()
        return wsum.cpu(), wmap.cpu(b, H, W), loss.cpu(), dimg.cpu(b, H, W, 16)
    del mp
    o6, t6, w6, m6, gs6, pre6 = d64(img16, target, weight, mask, gscale, pre)
    w_eff = R._w(w6, m6)
    for acc in (0, 1):
        wsum, wmap, loss, dimg = run(slice(0, Bn), acc)
        assert all(torch.equal(a, b) for a, b in zip((wsum, wmap, loss, dimg), run(slice(0, Bn), acc)))
        rb = run(slice(Bn - 1, Bn), acc)
        assert all(torch.equal(a[0], b[Bn - 1]) for a, b in zip(rb, (wsum, wmap, loss, dimg)))
        case = 'Bn=%d %dx%d mask=%d acc=%d' % (Bn, H, W, mask_on, acc)
        ws6 = wsum.to(D64)                                               # l1 takes the wsum it is handed
        if acc == 0:
            # weight * mask: 1; ceil(3HW / 1024) adds per thread, wave tree 6, 16 waves in sequence
            hold('p2l_weight_sum:wsum', case, wsum, R.weight_sum(w6, m6), R.weight_sum(w6, m6), R.weight_sum(weight, mask),
                 1 + math.ceil(3 * HW / 1024) + 6 + 16)
            hold('p2l_weight_map:wsrc', case, wmap, R.weight_map(w6, m6), R.weight_map(w6, m6), R.weight_map(weight, mask),
                 3)                                                      # weight * mask: 1; two adds
            ref = (torch.abs(t6 - R.nhwc16_to_nchw3(o6)) * w_eff).sum((1, 2, 3)) / ws6
            f32 = (torch.abs(target - out) * R._w(weight, mask)).sum((1, 2, 3)) / wsum
            # |t - o|: 1, w * mask: 1, * w: 1, 2 adds; block: 6 + 2; rows: ceil(nblk / 256) + 6 + 2; / wsum: 1
            hold('p2l_l1_loss_fwd:loss', case, loss, ref, ref, f32, 5 + 8 + math.ceil(nblk / 256) + 8 + 1)
            assert torch.equal(dimg[..., 3:], torch.zeros_like(dimg[..., 3:]))
        else:
            assert torch.equal(dimg[..., 4:], pre[..., 4:])              # accumulate: channels 4..15 left alone
        sg = torch.sign(R.nhwc16_to_nchw3(o6) - t6)
        rd = (sg * w_eff * (gs6 / ws6).view(Bn, 1, 1, 1)).permute(0, 2, 3, 1) + (pre6[..., :3] if acc else 0)
        fd = (torch.sign(out - target) * R._w(weight, mask) * (gscale / wsum).view(Bn, 1, 1, 1)).permute(0, 2, 3, 1) \
            + (pre[..., :3] if acc else 0)
        den = (w_eff * (gs6 / ws6).abs().view(Bn, 1, 1, 1)).permute(0, 2, 3, 1) + (pre6[..., :3].abs() if acc else 0)
        # gscale / wsum: 1, w * mask: 1, the product: 1, accumulate: 1
        hold('p2l_l1_loss_bwd:dimg', case, dimg[..., :3], rd, den, fd, 3 + acc)
        assert bool((dimg[:, 0, 0, 0] == (pre[:, 0, 0, 0] if acc else 0)).all())          # the tie: no gradient


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 4097])
@pytest.mark.parametrize('Bn', [1, 18])
@seeded
def test_reduce_rows_vec_scale_div(dev, N, Bn, n):
    """p2l_reduce_rows at every flag; p2l_vec_scale_div, its elementwise sibling, is held in test_vec_scale_div"""
    lib, g = N.lib(), _gen(16, Bn, n)
    part, div, pre = randn(g, Bn, n), 0.5 + torch.rand(Bn, generator=g), randn(g, Bn)
    scale = 0.37
    sc32 = float(torch.tensor(scale, dtype=torch.float32))
    p6, dv6, pre6 = d64(part, div, pre)
    for div_on in (0, 1):
        for acc in (0, 1):
            def run(sl):
                b = sl.stop - sl.start
                out = Out(dev, b, prefill=pre[sl] if acc else None)
                N.check(lib.p2l_reduce_rows(N.ptr(part[sl].contiguous().to(dev)), N.ptr(out.t), b, n, N.f32(scale),
                                            N.ptr(div[sl].contiguous().to(dev)) if div_on else None, acc, N.stream()), 'rr')
                return out.cpu()
            got = run(slice(0, Bn))
            assert torch.equal(got, run(slice(0, Bn))) and torch.equal(run(slice(Bn - 1, Bn))[0], got[Bn - 1])
            ref = R.reduce_rows(p6, sc32, dv6 if div_on else None) + (pre6 if acc else 0)
            den = R.reduce_rows(p6.abs(), sc32, dv6 if div_on else None) + (pre6.abs() if acc else 0)
            f32 = R.reduce_rows(part, sc32, div if div_on else None) + (pre if acc else 0)
            # ceil(n / 256) adds per thread, wave tree 6, 2 over the waves; scale, division, accumulate
            hold('p2l_reduce_rows:out', 'Bn=%d n=%d div=%d acc=%d' % (Bn, n, div_on, acc), got, ref, den, f32,
                 math.ceil(n / 256) + 8 + 1 + div_on + acc)


@pytest.mark.parametrize('n', FLAT)
@seeded
def test_vec_scale_div(dev, N, n):
    lib, g = N.lib(), _gen(18, n)
    scale = 0.37
    sc32 = float(torch.tensor(scale, dtype=torch.float32))
    a = randn(g, n)
    for div_on in (0, 1):
        dv = 0.5 + torch.rand(n, generator=g)
        out = Out(dev, n)
        N.check(lib.p2l_vec_scale_div(N.ptr(a.to(dev)), N.ptr(dv.to(dev)) if div_on else None, N.ptr(out.t), n, N.f32(scale),
                                      N.stream()), 'vec_scale_div')
        got = out.cpu()
        out2 = Out(dev, n)
        N.check(lib.p2l_vec_scale_div(N.ptr(a.to(dev)), N.ptr(dv.to(dev)) if div_on else None, N.ptr(out2.t), n, N.f32(scale),
                                      N.stream()), 'vec_scale_div')
        assert torch.equal(got, out2.cpu())
        ref = R.vec_scale_div(a.to(D64), sc32, dv.to(D64) if div_on else None)
        hold('p2l_vec_scale_div:out', 'n=%d div=%d' % (n, div_on), got, ref, ref.abs(),
             R.vec_scale_div(a, sc32, dv if div_on else None), 1 + div_on)        # the multiply, the division


@pytest.mark.parametrize('n', FLAT)
def test_clamp(dev, N, n):
    lib, g = N.lib(), _gen(19, n)
    p = randn(g, n)
    p[:3] = torch.tensor([0.25, -0.25, -0.0])[:min(3, n)]              # bounds hit exactly
    for lo, hi in ((-0.25, 0.25), (-2.0, 2.0)):
        co = Out(dev, n, prefill=p)                                      # in place
        N.check(lib.p2l_clamp(N.ptr(co.t), N.i64(n), N.f32(lo), N.f32(hi), N.stream()), 'clamp')
        assert torch.equal(co.cpu(), torch.clamp(p, lo, hi))


# =====================================================================================================================
# optimiser
# =====================================================================================================================
@pytest.mark.parametrize('start', [0, 999, 9999])
@pytest.mark.parametrize('n', [1, 257, 18 * 128, 8400000])
def test_adam_step_dev_and_clamp(dev, N, n, start):
    lib, g = N.lib(), _gen(17, n, start)
    lr, b1, b2, eps = 0.05, 0.9, 0.999, 1e-8
    steps = 6 if n < 10 ** 6 else 2
    # |p| < 1 (+ six steps of at most lr): two correct fp32 evaluations of the update may round p to neighbouring
    # floats at every step, ulp(p) <= 1.2e-7 keeps six such steps under the absolute 1e-6; at |p| ~ 4 one ulp is 4.8e-7
    # and the same bound would measure ulp(p), not the arithmetic
    p0 = 0.5 * torch.fmod(randn(g, n), 2.0)
    # a state an Adam history can have reached: |m| <= sqrt(v) (m and v are averages of g and g^2), so that a step
    # moves a parameter by about lr and the absolute 1e-6 of the existing test means what it means there
    m0 = 0.1 * randn(g, n) if start else torch.zeros(n)
    v0 = m0 * m0 + 1e-3 * torch.rand(n, generator=g) if start else torch.zeros(n)
    # gradients inside that history's scale, |g| <= sqrt(v): |m| / sqrt(v) stays <= ~1, the invariant Adam's averages
    # keep.  (The ABI takes the betas as floats: 0.999f is 1.3e-8 above torch's double 0.999, which near step 1000
    # shifts sqrt(1 - beta2^t) by 3.7e-6 and p by lr * 3.7e-6 * |m| / sqrt(v) per step -- 2e-7 at ratio 1, but past
    # the absolute 1e-6 of the existing test once a state is handed in whose ratio is 5 or more.)
    if start:
        grads = [(2 * torch.rand(n, generator=g) - 1) * v0.sqrt() * (10.0 ** -(i % 4)) for i in range(steps)]
    else:
        grads = [randn(g, n) * (10.0 ** -(i % 4)) for i in range(steps)]
    n_counters, extra = 18, 5
    cnt = torch.full((n_counters + extra,), start, dtype=torch.int32, device=dev)
    cnt[n_counters:] = -7
    pd, md, vd = Out(dev, n, prefill=p0), Out(dev, n, prefill=m0), Out(dev, n, prefill=v0)
    ph, mh, vh = Out(dev, n, prefill=p0), Out(dev, n, prefill=m0), Out(dev, n, prefill=v0)
    ref = R.adam_reference(p0, grads, lr, first_step=start + 1, m0=m0, v0=v0)
    for i, gr in enumerate(grads):
        gd = gr.to(dev)
        N.check(lib.p2l_adam_step_dev(N.ptr(pd.t), N.ptr(gd), N.ptr(md.t), N.ptr(vd.t), N.i64(n), N.f32(lr), N.f32(b1),
                                      N.f32(b2), N.f32(eps), ct.c_void_p(cnt.data_ptr()), n_counters, N.stream()), 'adam_dev')
        N.check(lib.p2l_adam_step(N.ptr(ph.t), N.ptr(gd), N.ptr(mh.t), N.ptr(vh.t), N.i64(n), N.f32(lr), N.f32(b1),
                                  N.f32(b2), N.f32(eps), start + i + 1, N.stream()), 'adam')
        c = cnt.cpu()
        assert bool((c[:n_counters] == start + i + 1).all()) and bool((c[n_counters:] == -7).all())
        assert torch.equal(pd.cpu(), ph.cpu()), 'step %d: device-counter form differs from the host-counter form' % (start + i + 1)
        assert (pd.cpu() - ref[i]).abs().max().item() < 1e-6
    assert torch.equal(md.cpu(), mh.cpu()) and torch.equal(vd.cpu(), vh.cpu())
    # clamp, in place; bounds hit exactly
    p = pd.cpu().clone()
    p[:1] = 0.25
    co = Out(dev, n, prefill=p)
    N.check(lib.p2l_clamp(N.ptr(co.t), N.i64(n), N.f32(-0.25), N.f32(0.25), N.stream()), 'clamp')
    assert torch.equal(co.cpu(), torch.clamp(p, -0.25, 0.25))


# =====================================================================================================================
# error codes: the documented constraints are refused on the host, before anything is launched
# =====================================================================================================================
def test_error_codes_before_any_launch(dev, N):
    lib = N.lib()
    EINVAL, EUNSUP = -1, -4
    st = N.stream()
    a, b, c, d = (torch.ones(4096, device=dev) for _ in range(4))
    o1, o2 = Out(dev, 4096), Out(dev, 4096)
    A, B, C_, D_, O1, O2, NUL = N.ptr(a), N.ptr(b), N.ptr(c), N.ptr(d), N.ptr(o1.t), N.ptr(o2.t), None
    f, i64 = N.f32, N.i64
    cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    CNT = ct.c_void_p(cnt.data_ptr())
    calls = [
        ('pixelnorm_fwd Bn<1', lib.p2l_sg2_pixelnorm_fwd(A, O1, 0, 8, st), EINVAL),
        ('pixelnorm_fwd NULL', lib.p2l_sg2_pixelnorm_fwd(NUL, O1, 2, 8, st), EINVAL),
        ('pixelnorm_bwd D<1', lib.p2l_sg2_pixelnorm_bwd(A, B, O1, 2, -1, st), EINVAL),
        ('bias_lrelu NULL bias', lib.p2l_sg2_bias_lrelu_fwd(O1, NUL, f(1), 2, 8, st), EINVAL),
        ('bias_lrelu Bn<1', lib.p2l_sg2_bias_lrelu_fwd(O1, A, f(1), 0, 8, st), EINVAL),
        ('lrelu_bwd n<1', lib.p2l_sg2_lrelu_bwd(A, O1, 0, st), EINVAL),
        ('demod_fwd NULL', lib.p2l_sg2_demod_fwd(A, B, NUL, 2, 8, 8, st), EINVAL),
        ('demod_fwd Bn<1', lib.p2l_sg2_demod_fwd(A, B, O1, 0, 8, 8, st), EINVAL),
        ('demod_bwd Cout<1', lib.p2l_sg2_demod_bwd(A, B, C_, D_, O1, 2, 8, 0, 0, st), EINVAL),
        ('scale_bwd C%32', lib.p2l_scale_bwd(A, 48, B, 48, C_, 48, NUL, 0, 0, O1, 48, O2, O2, 48, O2, 1, 2, 2, 48, st), EINVAL),
        ('scale_bwd Bn<1', lib.p2l_scale_bwd(A, 32, B, 32, C_, 32, NUL, 0, 0, O1, 32, O2, O2, 32, O2, 0, 2, 2, 32, st), EINVAL),
        ('scale_bwd Bn>65535', lib.p2l_scale_bwd(A, 32, B, 32, C_, 32, NUL, 0, 0, O1, 32, O2, O2, 32, O2, 65536, 2, 2, 32, st), EINVAL),
        ('scale_bwd NULL', lib.p2l_scale_bwd(A, 32, B, 32, C_, 32, NUL, 0, 0, NUL, 32, O2, O2, 32, O2, 1, 2, 2, 32, st), EINVAL),
        ('styled_act_bwd C%32', lib.p2l_sg2_styled_act_bwd(A, B, C_, NUL, f(0), D_, O1, O2, NUL, O2, NUL, 1, 4, 48, st), EINVAL),
        ('styled_act_bwd Bn<1', lib.p2l_sg2_styled_act_bwd(A, B, C_, NUL, f(0), D_, O1, O2, NUL, O2, NUL, 0, 4, 32, st), EINVAL),
        ('styled_act_bwd Bn>65535', lib.p2l_sg2_styled_act_bwd(A, B, C_, NUL, f(0), D_, O1, O2, NUL, O2, NUL, 65536, 4, 32, st), EINVAL),
        ('styled_act_bwd dnoise without strips', lib.p2l_sg2_styled_act_bwd(A, B, C_, NUL, f(0), D_, O1, O2, O2, O2, NUL, 1, 4, 32, st), EINVAL),
        ('styled_act_bwd_amax NULL', lib.p2l_sg2_styled_act_bwd_amax(A, B, C_, NUL, f(0), D_, O1, NUL, NUL, O2, NUL, 1, 4, 32, NUL, st), EINVAL),
        ('rgb_up_fwd h<1', lib.p2l_sg2_rgb_up_fwd(A, O1, 1, 0, 4, st), EINVAL),
        ('rgb_up_bwd NULL', lib.p2l_sg2_rgb_up_bwd(A, NUL, 1, 2, 2, 0, st), EINVAL),
        ('clamp16_fwd P<1', lib.p2l_sg2_clamp16_fwd(A, O1, i64(0), st), EINVAL),
        ('clamp16_bwd NULL', lib.p2l_sg2_clamp16_bwd(A, NUL, O1, i64(4), st), EINVAL),
        ('broadcast_rows Bn<1', lib.p2l_broadcast_rows(A, O1, i64(4), 0, st), EINVAL),
        ('add_inplace n<1', lib.p2l_add_inplace(O1, A, i64(-1), st), EINVAL),
        ('cbn_fold_fwd raw_ld<C', lib.p2l_cbn_fold_fwd(A, B, C_, D_, O1, O2, 2, 8, 4, st), EINVAL),
        ('cbn_fold_fwd NULL', lib.p2l_cbn_fold_fwd(A, B, NUL, D_, O1, O2, 2, 8, 8, st), EINVAL),
        ('cbn_fold_bwd Bn<1', lib.p2l_cbn_fold_bwd(A, B, C_, D_, O1, O2, 0, 8, 8, st), EINVAL),
        ('concat2 Bn<1', lib.p2l_concat2(A, B, O1, 0, 4, 4, st), EINVAL),
        ('split2 NULL', lib.p2l_split2(A, O1, NUL, 2, 4, 4, st), EINVAL),
        ('linear_fwd_ld K%4', lib.p2l_linear_fwd_ld(A, 6, B, NUL, O1, 2, 6, 8, st), EINVAL),
        ('linear_fwd_ld x_ld<K', lib.p2l_linear_fwd_ld(A, 4, B, NUL, O1, 2, 8, 8, st), EINVAL),
        ('linear_fwd_ld Bn<1', lib.p2l_linear_fwd_ld(A, 8, B, NUL, O1, 0, 8, 8, st), EINVAL),
        ('linear_bwd_ld N%4', lib.p2l_linear_bwd_ld(A, B, O1, 8, 2, 8, 6, 0, st), EINVAL),
        ('linear_bwd_ld NULL', lib.p2l_linear_bwd_ld(A, NUL, O1, 8, 2, 8, 8, 0, st), EINVAL),
        ('nchw3_to_nhwc16 H<1', lib.p2l_nchw3_to_nhwc16(A, O1, 1, 0, 4, st), EINVAL),
        ('nhwc16_to_nchw3 NULL', lib.p2l_nhwc16_to_nchw3(NUL, O1, 1, 4, 4, st), EINVAL),
        ('tanh_bwd16 P<1', lib.p2l_tanh_bwd16(A, O1, i64(0), st), EINVAL),
        ('relu_mask C%4', lib.p2l_relu_mask(A, 8, B, 8, O1, 8, i64(4), 6, st), EINVAL),
        ('relu_mask ld%4', lib.p2l_relu_mask(A, 6, B, 8, O1, 8, i64(4), 4, st), EINVAL),
        ('weight_sum Bn<1', lib.p2l_weight_sum(A, NUL, O1, 0, 12, st), EINVAL),
        ('weight_map Bn>65535', lib.p2l_weight_map(A, NUL, O1, 65536, 1, 1, st), EINVAL),
        ('l1_loss_fwd NULL wsum', lib.p2l_l1_loss_fwd(A, B, C_, NUL, NUL, O1, O2, 1, 2, 2, st), EINVAL),
        ('l1_loss_fwd Bn>65535', lib.p2l_l1_loss_fwd(A, B, C_, NUL, D_, O1, O2, 65536, 1, 1, st), EINVAL),
        ('l1_loss_bwd W<1', lib.p2l_l1_loss_bwd(A, B, C_, NUL, D_, D_, O1, 1, 2, 0, 0, st), EINVAL),
        ('reduce_rows n<0', lib.p2l_reduce_rows(A, O1, 2, -1, f(1), NUL, 0, st), EINVAL),
        ('reduce_rows Bn<1', lib.p2l_reduce_rows(A, O1, 0, 4, f(1), NUL, 0, st), EINVAL),
        ('vec_scale_div n<1', lib.p2l_vec_scale_div(A, NUL, O1, 0, f(1), st), EINVAL),
        ('adam_step_dev NULL counters', lib.p2l_adam_step_dev(O1, A, O2, O2, i64(4), f(.1), f(.9), f(.999), f(1e-8), NUL, 1, st), EINVAL),
        ('adam_step_dev n_counters<1', lib.p2l_adam_step_dev(O1, A, O2, O2, i64(4), f(.1), f(.9), f(.999), f(1e-8), CNT, 0, st), EINVAL),
        ('adam_step_dev n<1', lib.p2l_adam_step_dev(O1, A, O2, O2, i64(0), f(.1), f(.9), f(.999), f(1e-8), CNT, 1, st), EINVAL),
        ('clamp n<1', lib.p2l_clamp(O1, i64(0), f(-1), f(1), st), EINVAL),
        ('maxpool2_bwd H odd', lib.p2l_maxpool2_bwd(A, 4, B, 4, NUL, 4, O1, 4, 1, 3, 4, 4, 0, st), EINVAL),
        ('maxpool2_bwd W odd', lib.p2l_maxpool2_bwd(A, 4, B, 4, NUL, 4, O1, 4, 1, 4, 3, 4, 0, st), EINVAL),
        ('maxpool2_bwd_amax H odd', lib.p2l_maxpool2_bwd_amax(A, 4, B, 4, NUL, 4, O1, 4, 1, 3, 4, 4, 0, NUL, st), EINVAL),
        ('softmax_fwd cols', lib.p2l_softmax_fwd(A, O1, i64(4), 300, st), EUNSUP),
        ('softmax_bwd cols', lib.p2l_softmax_bwd(A, B, O1, i64(4), 300, st), EUNSUP),
        ('lpips_normalize C', lib.p2l_lpips_normalize(A, O1, i64(4), 96, st), EUNSUP),
    ]
    bad = [(what, rc, want) for what, rc, want in calls if rc != want]
    assert not bad, bad
    assert is_sentinel(o1.cpu()) and is_sentinel(o2.cpu()) and bool((cnt.cpu() == 0).all())
    # the empty sum is a valid reduce_rows: out = 0
    N.check(lib.p2l_reduce_rows(A, O1, 2, 0, f(1), NUL, 0, st), 'reduce_rows n=0')
    assert o1.cpu()[:2].tolist() == [0.0, 0.0]

"""The glue kernels that are neither "small" nor convs -- the batched GEMM and its split-K form, the row softmax, the
ReLU-affine backward with its two-stage reduction, the fused affine warp and the StyleGAN2 FIR blur -- against the
float64 references of tests/_small_refs.py, through ctypes, with the harness, the metric and the bars of
tests/test_small_kernels_gpu.py (tests/_pin.py):

    p2l_gemm, p2l_gemm_ws, p2l_softmax_fwd / _bwd, p2l_affine_relu_bwd, p2l_arb_finish, p2l_arb_defer_*,
    p2l_affine_grid_sample(_bwd), p2l_sg2_blur_fwd(_amax), p2l_sg2_blur_bwd(_amax).

Rounded outputs are held to |got - r64| / sum|terms| <= min(k, 4 x fp32 restatement) x 2^-24, k counted from the
kernel's arithmetic next to each `hold`; whatever the contract calls exact (a masked element, a sample outside the
image, a row's bits in another batch, the documented order of a reduction) is compared bit for bit.  Every output sits
between guard bands, every pitch is above its row with junk (inputs) or sentinels (outputs) in the gap, every image of
a batch has a magnitude of its own.  P2L_GLUE_ERR_FILE=<path> records the figures (profiles/glue_kernels_err.txt)."""
import ctypes as C
import math

import pytest
import torch

import _small_refs as R
from _small_refs import _cancellation_case
from _pin import D64, G, N, SENT, Out, _gen, _record_file, d64, draw, hold, is_sentinel, randn, seeded  # noqa: F401

pytestmark = pytest.mark.gpu
EINVAL, EWS, EUNSUP = -1, -3, -4
U = R.U


def _mags(Bn, lo=-2.0, hi=2.0):
    """one magnitude per image, 1e-2 .. 1e2"""
    return 10.0 ** torch.linspace(lo, hi, Bn) if Bn > 1 else torch.tensor([3.0])


def _pitched(t, ld, dev=None, junk=7.0):
    """[..., C] -> the same rows at pitch ld, junk in the gap columns"""
    o = torch.full(t.shape[:-1] + (ld,), junk)
    o[..., :t.shape[-1]] = t
    return o if dev is None else o.to(dev)


def _sent(*shape):
    return torch.full(shape, SENT, dtype=torch.int32).view(torch.float32)


def _chain32(terms, dim):
    """fp32 sum along `dim` as ONE sequential chain (the class of order of a kernel's per-thread accumulator)"""
    acc = torch.zeros_like(terms.select(dim, 0))
    for i in range(terms.shape[dim]):
        acc = acc + terms.select(dim, i)
    return acc


# =====================================================================================================================
# GEMM
# =====================================================================================================================
def _gemm_desc(N, batch, M, Nn, K, lda, ldb, ldc, sa, sb, sc, akm, bkm, alpha, acc):
    d = N.P2LGemm()
    d.batch, d.M, d.N, d.K = batch, M, Nn, K
    d.lda, d.ldb, d.ldc = lda, ldb, ldc
    d.stride_a, d.stride_b, d.stride_c = sa, sb, sc
    d.a_kmajor, d.b_kmajor, d.alpha, d.accumulate = int(akm), int(bkm), alpha, int(acc)
    return d


class _GemmCase(object):
    """operands of one product at pitches above the row and batch strides above the matrix, on the host"""

    def __init__(self, g, batch, M, Nn, K, akm, bkm, shared_b):
        self.dims = (batch, M, Nn, K, akm, bkm)
        mag = _mags(batch)
        self.a = randn(g, batch, M, K) * mag.view(batch, 1, 1)                   # dense [batch, M, K]
        nb = 1 if shared_b else batch
        self.b = randn(g, nb, Nn, K) * (1.0 if shared_b else mag.flip(0).view(batch, 1, 1))
        self.c0 = randn(g, batch, M, Nn) * mag.view(batch, 1, 1) * math.sqrt(K)
        self.shared_b = shared_b
        self.lda, self.ldb, self.ldc = (M + 8 if akm else K + 4), (Nn + 12 if bkm else K + 8), Nn + 4
        self.A = _pitched(self.a.transpose(1, 2).contiguous() if akm else self.a, self.lda)
        self.B = _pitched(self.b.transpose(1, 2).contiguous() if bkm else self.b, self.ldb, junk=-3.0)
        self.sa = self.A.shape[1] * self.lda + 16
        self.sb = 0 if shared_b else self.B.shape[1] * self.ldb + 32
        self.sc = M * self.ldc + 32

    def _strided(self, T, stride):
        o = torch.full((T.shape[0], max(stride, T.shape[1] * T.shape[2])), 11.0)
        o[:, :T.shape[1] * T.shape[2]] = T.flatten(1)
        return o

    def run(self, dev, N, alpha, acc, ws=None, sl=None):
        """-> C [batch, M, N] of the images sl.  ws: None = p2l_gemm; else p2l_gemm_ws with a workspace `ws` bytes short
        of p2l_gemm_ws_bytes (0: the full one; more than that: none at all, a NULL pointer)"""
        lib = N.lib()
        batch, M, Nn, K, akm, bkm = self.dims
        sl = slice(0, batch) if sl is None else sl
        nb = sl.stop - sl.start
        Ad = self._strided(self.A[sl], self.sa).to(dev)
        Bd = self._strided(self.B if self.shared_b else self.B[sl], self.sb).to(dev)
        pre = _sent(nb, self.sc)
        if acc:
            rows = pre[:, :M * self.ldc].view(nb, M, self.ldc)
            rows[..., :Nn] = self.c0[sl]
        out = Out(dev, nb * self.sc, prefill=pre)
        d = _gemm_desc(N, nb, M, Nn, K, self.lda, self.ldb, self.ldc, self.sa, self.sb, self.sc, akm, bkm, alpha, acc)
        if ws is None:
            N.check(lib.p2l_gemm(C.byref(d), N.ptr(Ad), N.ptr(Bd), N.ptr(out.t), N.stream()), 'gemm')
        else:
            need = lib.p2l_gemm_ws_bytes(C.byref(d))
            give = max(need - ws, 0)
            buf = Out(dev, max(give // 4, 1))
            N.check(lib.p2l_gemm_ws(C.byref(d), N.ptr(Ad), N.ptr(Bd), N.ptr(out.t), N.ptr(buf.t) if give else None,
                                    C.c_size_t(give), N.stream()), 'gemm_ws')
            buf.cpu()
        got = out.cpu(nb, self.sc)
        assert is_sentinel(got[:, M * self.ldc:]), 'padding between the images of C written'
        rows = got[:, :M * self.ldc].view(nb, M, self.ldc)
        assert is_sentinel(rows[..., Nn:]), 'gap columns of C written'
        return rows[..., :Nn].contiguous()

    def refs(self, alpha, acc, kper):
        """fp64 reference on the pitched operands, sum|terms|, the fp32 restatement in the kernel's class of order"""
        batch, M, Nn, K, akm, bkm = self.dims
        A6, B6, c6 = d64(self.A, self.B, _pitched(self.c0, self.ldc))
        ref = R.gemm(A6, B6, M, Nn, K, akm, bkm, alpha, c6 if acc else None)
        den = R.gemm(A6.abs(), B6.abs(), M, Nn, K, akm, bkm, abs(alpha), c6.abs() if acc else None)
        # one accumulator per output walks k upwards; per K slice, the slices added in index order, alpha, + C
        bt = self.b.transpose(1, 2)                                              # [nb, K, N]
        total = None
        for k0 in range(0, K, kper):
            part = _chain32(self.a[:, :, k0:k0 + kper, None] * bt[:, None, k0:k0 + kper, :], 2)
            total = part if total is None else total + part
        r32 = total * torch.tensor(alpha, dtype=torch.float32)
        return ref, den, r32 + self.c0 if acc else r32


# alpha x accumulate, B per image or one B for the batch (stride_b = 0)
GEMM_FORMS = [(1.0, 0, False), (-0.37, 1, True), (1.0, 1, False), (-0.37, 0, True)]


@pytest.mark.parametrize('M,Nn,K', [(128, 32, 16), (128, 64, 48), (256, 96, 80)])
@pytest.mark.parametrize('akm,bkm', [(0, 0), (0, 1), (1, 0), (1, 1)])
@seeded
def test_gemm(dev, N, akm, bkm, M, Nn, K):
    """one chunk with 32-wide tiles, an odd chunk count with 64-wide tiles, three 32-wide N tiles"""
    batch = 3
    for alpha, acc, shared in GEMM_FORMS:
        g = _gen(201, akm, bkm, M, Nn, K, alpha, acc)
        cs = _GemmCase(g, batch, M, Nn, K, akm, bkm, shared)
        got = cs.run(dev, N, alpha, acc)
        assert torch.equal(cs.run(dev, N, alpha, acc), got)
        assert torch.equal(cs.run(dev, N, alpha, acc, sl=slice(batch - 1, batch))[0], got[-1])
        assert torch.equal(cs.run(dev, N, alpha, acc, ws=0), got)               # ws_bytes == 0: never split
        ref, den, r32 = cs.refs(alpha, acc, K)
        # per k a product and an addition (the matrix pipe is not known to fuse them), alpha, + C
        hold('p2l_gemm:C', '%dx%dx%d akm=%d bkm=%d alpha=%g acc=%d' % (M, Nn, K, akm, bkm, alpha, acc), got, ref, den,
             r32, 2 * K + 2)


def _split_plan(M, Nn, K):
    """the header's formula: slices asked for, depth of a slice, slices launched"""
    tiles = (M // 128) * (Nn // (64 if Nn % 64 == 0 else 32))
    s = min(8, K // 256, -(-512 // (4 * tiles))) if K >= 1024 and 4 * tiles < 192 else 1
    kper = -(-(-(-K // s)) // 16) * 16
    return s, kper, -(-K // kper)


def test_split_plan_has_a_ragged_case():
    plans = {K: _split_plan(128, 32, K) for K in (1024, 1040, 2064)}
    assert plans[1024] == (4, 256, 4) and 1024 % 256 == 0                         # even slices
    assert plans[1040] == (4, 272, 4) and plans[2064] == (8, 272, 8)              # a short last slice: 224, 160
    assert any(K % p[1] for K, p in plans.items())


@pytest.mark.parametrize('K', [1024, 1040, 2064])
@pytest.mark.parametrize('akm,bkm', [(0, 0), (0, 1), (1, 0), (1, 1)])
@seeded
def test_gemm_splitk(dev, N, akm, bkm, K):
    lib, batch, M, Nn = N.lib(), 3, 128, 32
    s, kper, nsl = _split_plan(M, Nn, K)
    for alpha, acc, shared in GEMM_FORMS[:2]:
        g = _gen(202, akm, bkm, K, alpha, acc)
        cs = _GemmCase(g, batch, M, Nn, K, akm, bkm, shared)
        for nb in (batch, 1):
            d = _gemm_desc(N, nb, M, Nn, K, cs.lda, cs.ldb, cs.ldc, cs.sa, cs.sb, cs.sc, akm, bkm, alpha, acc)
            assert lib.p2l_gemm_ws_bytes(C.byref(d)) == s * nb * M * Nn * 4
        got = cs.run(dev, N, alpha, acc, ws=0)
        assert torch.equal(cs.run(dev, N, alpha, acc, ws=0), got)
        # the slice count does not depend on the batch: an image alone has the bits it has among three
        for b in range(batch):
            assert torch.equal(cs.run(dev, N, alpha, acc, ws=0, sl=slice(b, b + 1))[0], got[b]), b
        plain = cs.run(dev, N, alpha, acc)
        assert torch.equal(cs.run(dev, N, alpha, acc, ws=1 << 40), plain)          # no workspace
        assert torch.equal(cs.run(dev, N, alpha, acc, ws=4), plain)                # one float short
        ref, den, r32 = cs.refs(alpha, acc, kper)
        case = '128x32x%d akm=%d bkm=%d alpha=%g acc=%d' % (K, akm, bkm, alpha, acc)
        # the deepest slice's chain, the slices in order, alpha, + C
        hold('p2l_gemm_ws:C', case, got, ref, den, r32, 2 * kper + (nsl - 1) + 2)
        hold('p2l_gemm:C', case, plain, ref, den, cs.refs(alpha, acc, K)[2], 2 * K + 2)


# =====================================================================================================================
# softmax
# =====================================================================================================================
SM_KINDS = 8
SM_BASE = 64      # different rows of a case; more rows repeat them
# row kind -> the largest max - x of its entries that are not exact zeros
SM_SPREAD = {'ordinary': 8.0, 'dominant': 68.0}


def _softmax_case(g, rows, cols):
    """S [rows, cols] and the kind of every row, (r + 3 draw) % 8: 0, 1 ordinary (spread <= 8); 2 all entries equal;
    3 one entry + 60 over the rest; 4 shifted by +80 (even r) / -80; 5 shifted by 1e4; 6 the maximum three times;
    7 one entry + 120 over the rest: the others are below the smallest fp32 subnormal and must be exact zeros"""
    S = (torch.rand(rows, cols, generator=g) - 0.5) * 8.0
    kind = (torch.arange(rows) + 3 * draw()) % SM_KINDS
    hot = torch.randint(cols, (rows,), generator=g)
    ar = torch.arange(rows)
    S[kind == 2] = S[kind == 2][:, :1]
    S[ar[kind == 3], hot[kind == 3]] = 4.0 + 60.0
    S[kind == 4] += torch.where(ar[kind == 4] % 2 == 0, 80.0, -80.0)[:, None]
    S[kind == 5] += 1e4
    for r in ar[kind == 6].tolist():
        S[r, torch.randperm(cols, generator=g)[:3]] = S[r].max()
    S[ar[kind == 7], hot[kind == 7]] = 4.0 + 120.0
    return S, kind


def _softmax_run(dev, N, S):
    rows, cols = S.shape
    P = Out(dev, rows * cols)
    N.check(N.lib().p2l_softmax_fwd(N.ptr(S.contiguous().to(dev)), N.ptr(P.t), rows, cols, N.stream()), 'softmax_fwd')
    return P.cpu(rows, cols)


def _softmax_bwd_run(dev, N, P, dP):
    rows, cols = P.shape
    dS = Out(dev, rows * cols)
    N.check(N.lib().p2l_softmax_bwd(N.ptr(P.contiguous().to(dev)), N.ptr(dP.contiguous().to(dev)), N.ptr(dS.t), rows,
                                    cols, N.stream()), 'softmax_bwd')
    return dS.cpu(rows, cols)


@pytest.mark.parametrize('rows', [1, 3, 4, 5, 4097])
@pytest.mark.parametrize('cols', [256, 512, 1024, 2048])
@seeded
def test_softmax_fwd_bwd(dev, N, cols, rows):
    g = _gen(203, cols, rows)
    full = rows
    rows = min(rows, SM_BASE)
    S, kind = _softmax_case(g, rows, cols)
    vpl = cols // 256
    reps = -(-full // rows)
    tiled = lambda t: t.repeat(reps, 1)[:full]
    P = _softmax_run(dev, N, tiled(S))
    assert torch.equal(_softmax_run(dev, N, tiled(S)), P)
    # 4097 rows are 64 different ones over and over (the kinds have period 8): the bits of a row do not depend on
    # its index, and the references are computed for the 64
    assert torch.equal(P, tiled(P[:rows]))
    P = P[:rows].contiguous()
    # a row's bits do not depend on how many rows there are, nor on the wave and the block it falls into
    assert torch.equal(_softmax_run(dev, N, S[-1:])[0], P[-1])
    if rows > 1:
        assert torch.equal(_softmax_run(dev, N, S[1:]), P[1:])
    S6 = S.to(D64)
    ref = R.softmax_rows(S6)
    r32 = R.softmax_rows(S)
    dead = ref < 2.0 ** -150                       # fp64 rounds to below the smallest subnormal: exactly zero
    assert bool((P[dead] == 0).all()) and bool((P[~dead] > 0).all())
    assert bool(dead[kind == 7].any()) or not bool((kind == 7).any())
    assert bool((ref[~dead] >= 2.0 ** -126).all()), 'a probability in the subnormal range: no relative bar holds there'
    ref = den = torch.where(dead, torch.zeros_like(ref), ref)
    case = 'rows=%d cols=%d' % (full, cols)
    for name, spread in sorted(SM_SPREAD.items()):
        sel = (kind == 3) if name == 'dominant' else (kind != 3)
        if not bool(sel.any()):
            continue
        # x - m: one rounding of a number up to `spread`, i.e. `spread` roundings of e; expf 1 ulp = 2.  The sum:
        # the same again on every term, the float4's tree (2), the lane's chain (vpl), 6 shuffles.  1 / sum: 2.  The
        # product: 1.
        k = 2 * (spread + 2) + (2 + vpl + 6) + 2 + 1
        hold('p2l_softmax_fwd:P', case + ' ' + name, P[sel], ref[sel], den[sel], r32[sel], k)
        assert bool(((P[sel].to(D64).sum(1) - 1).abs() <= k * U).all()), 'a row does not add up to 1 within its bar'
    # backward from the SAVED (fp32) probabilities
    dP = randn(g, rows, cols) * (10.0 ** ((torch.arange(rows) % 5).float() - 2.0))[:, None]
    dS = _softmax_bwd_run(dev, N, tiled(P), tiled(dP))
    assert torch.equal(_softmax_bwd_run(dev, N, tiled(P), tiled(dP)), dS)
    assert torch.equal(dS, tiled(dS[:rows]))
    dS = dS[:rows].contiguous()
    assert torch.equal(_softmax_bwd_run(dev, N, P[-1:], dP[-1:])[0], dS[-1])
    if rows > 1:
        assert torch.equal(_softmax_bwd_run(dev, N, P[1:], dP[1:]), dS[1:])
    P6, dP6 = d64(P, dP)
    den = P6.abs() * (dP6.abs() + (P6 * dP6).abs().sum(1, keepdim=True))
    # the dot product: a product, the float4's tree (2), the lane's chain (vpl), 6 shuffles; dP - dot; the product
    hold('p2l_softmax_bwd:dS', case, dS, R.softmax_rows_bwd(P6, dP6), den, R.softmax_rows_bwd(P, dP), 1 + 2 + vpl + 6 + 2)


# =====================================================================================================================
# ReLU-affine backward
# =====================================================================================================================
ARB_SKIPS = ['none', 'same', 'half', 'zero', 'ups']


def _arb_case(g, Bn, H, W, Cc, kind):
    """da, x [Bn, P, C], s, t [Bn, C], skip.  In image draw % Bn: x s + t == +0 at (pixel 0, channel 1) and == -0 at
    (pixel P - 1, channel 2); channels 3 and C - 1 are masked off in every pixel"""
    P = H * W
    mag = _mags(Bn, -1.0, 1.0)
    x = randn(g, Bn, P, Cc) * mag.view(Bn, 1, 1)
    da = randn(g, Bn, P, Cc) * mag.flip(0).view(Bn, 1, 1)
    s = (0.5 + torch.rand(Bn, Cc, generator=g)) * torch.where(torch.rand(Bn, Cc, generator=g) < 0.3, -1.0, 1.0)
    t = 0.3 * randn(g, Bn, Cc) * mag.view(Bn, 1)
    b0 = draw() % Bn
    s[b0, 1], t[b0, 1], x[b0, 0, 1] = 0.5, -1.0, 2.0               # 2 * 0.5 - 1 = +0
    s[b0, 2], t[b0, 2], x[b0, P - 1, 2] = -1.0, -0.0, 0.0          # 0 * -1 + -0 = -0
    for c in (3, Cc - 1):
        s[b0, c], t[b0, c] = 1.0, -1e6 * float(mag[b0])
    skip, skip_C, ups = None, 0, 0
    if kind in ('same', 'half', 'zero'):
        skip, skip_C = randn(g, Bn, P, Cc) * mag.view(Bn, 1, 1), {'same': Cc, 'half': Cc // 2, 'zero': 0}[kind]
    elif kind == 'ups':
        skip, skip_C, ups = randn(g, Bn, 2 * H, 2 * W, Cc) * mag.view(Bn, 1, 1, 1), Cc // 2, 1
    return da, x, s, t, skip, skip_C, ups, b0


def _arb_run(dev, N, da, x, s, t, skip, skip_C, ups, H, W):
    """every pitch above C: junk in the gaps of the inputs, sentinels in those of dx, ds and dt"""
    lib = N.lib()
    Bn, P, Cc = x.shape
    nblk = lib.p2l_affine_relu_bwd_nblk(P)
    assert nblk == -(-P // 256)
    da_ld, x_ld, dx_ld, sk_ld, stb, dsb = Cc + 4, Cc + 8, Cc + 12, Cc + 4, Cc + 4, Cc + 8
    dx, ds, dt = Out(dev, Bn * P * dx_ld), Out(dev, Bn * dsb), Out(dev, Bn * dsb)
    part = Out(dev, 2 * Bn * nblk * Cc)
    N.check(lib.p2l_affine_relu_bwd(
        N.ptr(_pitched(da, da_ld, dev)), da_ld, N.ptr(_pitched(x, x_ld, dev)), x_ld, N.ptr(_pitched(s, stb, dev)),
        N.ptr(_pitched(t, stb, dev)), stb, N.ptr(_pitched(skip, sk_ld, dev)) if skip is not None else None, sk_ld,
        skip_C, ups, N.ptr(dx.t), dx_ld, N.ptr(ds.t), N.ptr(dt.t), dsb, N.ptr(part.t), Bn, H, W, Cc, N.stream()),
        'affine_relu_bwd')
    part.cpu()
    out = []
    for o, shape in ((dx, (Bn, P, dx_ld)), (ds, (Bn, dsb)), (dt, (Bn, dsb))):
        v = o.cpu(*shape)
        assert is_sentinel(v[..., Cc:]), 'gap columns written'
        out.append(v[..., :Cc].contiguous())
    return out


@pytest.mark.parametrize('Bn', [1, 3])
@pytest.mark.parametrize('H,W', [(1, 1), (3, 5), (16, 16), (17, 16)])
@pytest.mark.parametrize('Cc', [32, 64, 96, 128])
@seeded
def test_affine_relu_bwd(dev, N, Cc, H, W, Bn):
    """P = 1, 15, 256, 272: below, at and across the 256-pixel slab; C = 32, 96: the upper half of the last 64-channel
    strip idles"""
    P = H * W
    nblk = -(-P // 256)
    for kind in ARB_SKIPS:
        g = _gen(204, Cc, H, W, Bn, kind)
        da, x, s, t, skip, skip_C, ups, b0 = _arb_case(g, Bn, H, W, Cc, kind)
        dx, ds, dt = got = _arb_run(dev, N, da, x, s, t, skip, skip_C, ups, H, W)
        again = _arb_run(dev, N, da, x, s, t, skip, skip_C, ups, H, W)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        sl = slice(Bn - 1, Bn)
        alone = _arb_run(dev, N, da[sl], x[sl], s[sl], t[sl], None if skip is None else skip[sl], skip_C, ups, H, W)
        assert all(torch.equal(a[0], b[-1]) for a, b in zip(alone, got))
        da6, x6, s6, t6, skip6 = d64(da, x, s, t, skip)
        rdx, rds, rdt = R.affine_relu_bwd(da6, x6, s6, t6, skip6, skip_C, ups, H, W)
        f32 = R.affine_relu_bwd(da, x, s, t, skip, skip_C, ups, H, W)
        g6 = da6 * (R.affine_relu_fwd(x6, s6, t6) > 0).to(D64)
        sk6 = R.skip_term(skip6.abs(), skip_C, ups, Bn, H, W, Cc) if skip is not None else torch.zeros_like(x6)
        # the skip term in fp32 as the kernel adds it: the children (c0 + c1) + (c2 + c3), row-major (p2l.h)
        skv = torch.zeros_like(x)
        if ups:
            kids = skip.view(Bn, H, 2, W, 2, Cc)
            kids = (kids[:, :, 0, :, 0] + kids[:, :, 0, :, 1]) + (kids[:, :, 1, :, 0] + kids[:, :, 1, :, 1])
            skv[:, :, :skip_C] = kids.reshape(Bn, P, Cc)[:, :, :skip_C]
        elif skip is not None:
            skv[:, :, :skip_C] = skip[:, :, :skip_C]
        # the two zeros: masked off, dx is the skip exactly, nothing reaches ds / dt; the dead channels: exactly 0
        for p, c in ((0, 1), (P - 1, 2)):
            assert float(g6[b0, p, c]) == 0.0
            assert float(dx[b0, p, c]) == float(skv[b0, p, c]), (kind, p, c)
        for c in (3, Cc - 1):
            assert float(ds[b0, c]) == 0.0 and float(dt[b0, c]) == 0.0
            assert torch.equal(dx[b0, :, c], skv[b0, :, c])
        case = 'Bn=%d %dx%d C=%d skip=%s' % (Bn, H, W, Cc, kind)
        # g * s, and: + skip (1), or the children's tree (2) and + (1)
        hold('p2l_affine_relu_bwd:dx', case, dx, rdx, (g6 * s6[:, None]).abs() + sk6, f32[0],
             1 + {'none': 0, 'ups': 3}.get(kind, 1))
        # a product and an addition per pixel of a thread's chain (16), the block's 16 pixel lanes in sequence (15), the
        # finish: the rows of a chain (nblk / 64, at least one), the chains' tree (2), the 16 segments in sequence (15)
        k_sum = 16 + 15 + max(1, -(-nblk // 64)) + 2 + 15
        gm = (da * (R.affine_relu_fwd(x6, s6, t6) > 0).float())
        hold('p2l_affine_relu_bwd:ds', case, ds, rds, (g6 * x6).abs().sum(1), _chain32(gm * x, 1), 1 + k_sum)
        hold('p2l_affine_relu_bwd:dt', case, dt, rdt, g6.abs().sum(1), _chain32(gm, 1), k_sum)


ARB_NBLK = [1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 130]


_finish_order32 = R.arb_finish_order32            # (shared with the 1x1 convs' ds / dt restatement)


def _finish_case(g, Bn, nblk, Cc):
    mag = _mags(Bn, -1.0, 1.0)
    return randn(g, 2, Bn, nblk, Cc) * mag.view(1, Bn, 1, 1) * (10.0 ** (torch.arange(nblk) % 4).float()).view(1, 1, nblk, 1)


class _Finish(object):
    """one p2l_arb_finish call: its buffers, and the check of what it left"""

    def __init__(self, dev, N, part, bstride=None):
        _, self.Bn, self.nblk, self.Cc = part.shape
        self.part, self.N = part, N
        self.bs = self.Cc + 4 if bstride is None else bstride
        self.pd = part.contiguous().to(dev)
        self.ds, self.dt = Out(dev, self.Bn * self.bs), Out(dev, self.Bn * self.bs)

    def call(self):
        N = self.N
        return N.lib().p2l_arb_finish(N.ptr(self.pd), N.ptr(self.ds.t), N.ptr(self.dt.t), self.Bn, self.nblk, self.Cc,
                                      self.bs, N.stream())

    def results(self):
        out = []
        for o in (self.ds, self.dt):
            v = o.cpu(self.Bn, self.bs)
            assert is_sentinel(v[:, self.Cc:]), 'gap of ds / dt written'
            out.append(v[:, :self.Cc].contiguous())
        return out

    def untouched(self):
        return is_sentinel(self.ds.cpu()) and is_sentinel(self.dt.cpu())

    def check(self):
        ds, dt = self.results()
        assert torch.equal(ds, _finish_order32(self.part[0])), 'ds: not the documented order'
        assert torch.equal(dt, _finish_order32(self.part[1])), 'dt: not the documented order'
        return ds, dt


@pytest.mark.parametrize('Cc', [32, 96, 128])
@pytest.mark.parametrize('nblk', ARB_NBLK)
def test_arb_finish_order(dev, N, nblk, Cc):
    """every side of the 16-segment x 4-chain loop and of its tail, bit for bit"""
    for Bn in (1, 3):
        f = _Finish(dev, N, _finish_case(_gen(205, nblk, Cc, Bn), Bn, nblk, Cc))
        N.check(f.call(), 'arb_finish')
        f.check()


def test_arb_finish_deferred(dev, N):
    lib = N.lib()
    mk = lambda i, Bn, nblk, Cc: _Finish(dev, N, _finish_case(_gen(206, i, Bn, nblk, Cc), Bn, nblk, Cc))
    try:
        # three layers of different C and nblk: recorded and flushed == called directly
        layers = [(2, 17, 96), (2, 130, 32), (2, 1, 128)]
        direct = [mk(i, *l) for i, l in enumerate(layers)]
        for f in direct:
            N.check(f.call(), 'arb_finish')
        want = [f.check() for f in direct]
        lib.p2l_arb_defer_begin()
        rec = [mk(i, *l) for i, l in enumerate(layers)]
        for f in rec:
            N.check(f.call(), 'arb_finish (recorded)')
        torch.cuda.synchronize()
        assert all(f.untouched() for f in rec), 'a recorded finish ran before the flush'
        N.check(lib.p2l_arb_defer_flush(N.stream()), 'arb_defer_flush')
        for f, (ds, dt) in zip(rec, want):
            got = f.results()
            assert torch.equal(got[0], ds) and torch.equal(got[1], dt)
        # 57 records: the 57th flushes the 56 before it (ARB_GROUP_MAX), the flush the last one
        lib.p2l_arb_defer_begin()
        rec = [mk(100 + i, 1, 1 + i % 5, 32 + 32 * (i % 3)) for i in range(57)]
        for f in rec:
            N.check(f.call(), 'arb_finish (recorded)')
        N.check(lib.p2l_arb_defer_flush(N.stream()), 'arb_defer_flush')
        for f in rec:
            f.check()
        # a change of Bn between two records flushes what was recorded
        lib.p2l_arb_defer_begin()
        rec = [mk(200, 2, 5, 64), mk(201, 2, 3, 32), mk(202, 1, 4, 64), mk(203, 3, 2, 96)]
        for f in rec:
            N.check(f.call(), 'arb_finish (recorded)')
        N.check(lib.p2l_arb_defer_flush(N.stream()), 'arb_defer_flush')
        for f in rec:
            f.check()
        # _cancel drops what was recorded: nothing runs, then or at a later flush
        lib.p2l_arb_defer_begin()
        rec = [mk(300, 2, 5, 64), mk(301, 2, 3, 32)]
        for f in rec:
            N.check(f.call(), 'arb_finish (recorded)')
        lib.p2l_arb_defer_cancel()
        N.check(lib.p2l_arb_defer_flush(N.stream()), 'arb_defer_flush (empty)')
        torch.cuda.synchronize()
        assert all(f.untouched() for f in rec)
        N.check(rec[0].call(), 'arb_finish')                                    # ... and the direct form is back
        rec[0].check()
    finally:
        lib.p2l_arb_defer_cancel()


# ---- the backward takes the forward's decision -------------------------------------------------------------------
@pytest.mark.parametrize('taps,wfmt', [(1, 0), (1, 3), (9, 0), (9, 1), (9, 2)])
def test_backward_mask_is_the_forwards_decision(dev, N, taps, wfmt):
    """{dx != 0} of p2l_affine_relu_bwd (da = 1, s != 0) == {a > 0}, a = what the conv's PRO_AFFINE_RELU prologue
    produced, read through an identity weight; the default form of every weight format (no workspace: no fp16 x 2)"""
    lib = N.lib()
    Bn, H, Cc = 2, 16, 64
    P = H * H
    k = 3 if taps == 9 else 1
    w = torch.zeros(Cc, Cc, k, k)
    w[torch.arange(Cc), torch.arange(Cc), k // 2, k // 2] = 1.0
    wp = N.pack_conv_weight(w.to(dev), taps, Cc, Cc, False, wfmt)
    d = N.P2LConv()
    d.B, d.H, d.W, d.Cin, d.Cout, d.taps = Bn, H, H, Cc, Cc, taps
    d.x_ld, d.pro, d.pro_bstride, d.alpha = Cc, N.PRO_AFFINE_RELU, Cc, 1.0
    d.n_store = d.y_ld = d.yp_ld = Cc
    d.splitk, d.wfmt, d.form, d.w_floats = 1, wfmt, N.FORM_AUTO, wp.numel()
    for seed in range(5):
        x, s, t, once, twice, A, B = _cancellation_case(seed, Bn, P, Cc)
        xd, sd, td = x.to(dev), s.to(dev), t.to(dev)
        y = Out(dev, Bn * P * Cc)
        N.check(lib.p2l_conv_fwd(C.byref(d), N.ptr(xd), N.ptr(wp), None, N.ptr(sd), N.ptr(td), None, None, N.ptr(y.t),
                                 None, None, C.c_size_t(0), N.stream()), 'conv_fwd')
        fwd = y.cpu(Bn, P, Cc) > 0
        dx, ds, dt = Out(dev, Bn * P * Cc), Out(dev, Bn * Cc), Out(dev, Bn * Cc)
        part = Out(dev, 2 * Bn * Cc)
        N.check(lib.p2l_affine_relu_bwd(N.ptr(torch.ones(Bn, P, Cc, device=dev)), Cc, N.ptr(xd), Cc, N.ptr(sd), N.ptr(td),
                                        Cc, None, 0, 0, 0, N.ptr(dx.t), Cc, N.ptr(ds.t), N.ptr(dt.t), Cc, N.ptr(part.t),
                                        Bn, H, H, Cc, N.stream()), 'affine_relu_bwd')
        bwd = dx.cpu(Bn, P, Cc) != 0
        print('taps=%d wfmt=%d seed=%d: forward == fma %s, == unfused %s; backward == fma %s, == unfused %s' % (
            taps, wfmt, seed, torch.equal(fwd, once), torch.equal(fwd, twice), torch.equal(bwd, once),
            torch.equal(bwd, twice)))
        diff = fwd != bwd
        assert not bool(diff.any()), ('forward and backward decide differently', int(diff.sum()), int((diff & A).sum()),
                                      int((diff & B).sum()))
        assert torch.equal(dt.cpu(Bn, Cc), fwd.float().sum(1))                  # dt counts the live pixels (da = 1)


# =====================================================================================================================
# affine warp
# =====================================================================================================================
KC = 9            # roundings of a sampling coordinate: /, -, two products, two sums, + 1, * W, - 1


def _coord_bound(theta6, H, W):
    """[Bn] each: absolute error bounds (in units of 2^-24) of the fp32 ix and iy.  g0 = (2 x + 1) / W - 1 carries 3
    roundings of a number <= 2; g = th0 g0x + th1 g0y + th2 three more of at most T = |th0| + |th1| + |th2| each and
    T times g0's; g + 1 one of T + 1; times W one of (T + 1) W; - 1 one of (T + 1) W + 1; the half is exact:
    W (4.5 T + 1.5) + 0.5"""
    Tx, Ty = theta6[:, 0:3].abs().sum(1), theta6[:, 3:6].abs().sum(1)
    return W * (4.5 * Tx + 1.5) + 0.5, H * (4.5 * Ty + 1.5) + 0.5


def _near_integer(th6, H, W):
    """-> [Bn, H, W] samples whose fp64 ix or iy lies within the coordinate bound of an integer, and the bounds"""
    Bn = th6.shape[0]
    bx, by = _coord_bound(th6, H, W)
    ix, iy = R.warp_coords(th6, H, W)
    near = ((ix - ix.round()).abs() <= (bx * U).view(Bn, 1, 1)) | ((iy - iy.round()).abs() <= (by * U).view(Bn, 1, 1))
    return near, bx, by


def _warp_run(dev, N, src, theta, dout, want=(1, 1), sl=None):
    """-> dst, dsrc, dtheta (None where not asked for)"""
    lib = N.lib()
    sl = slice(0, src.shape[0]) if sl is None else sl
    src, theta, dout = src[sl].contiguous(), theta[sl].contiguous(), dout[sl].contiguous()
    Bn, Cc, H, W = src.shape
    sd, td, dd = src.to(dev), theta.to(dev), dout.to(dev)
    dst, dsrc, dth = Out(dev, src.numel()), Out(dev, src.numel()), Out(dev, Bn * 6)
    nbytes = lib.p2l_affine_grid_sample_bwd_ws_bytes(Bn, H, W)
    assert nbytes == Bn * -(-(H * W) // 256) * 6 * 4
    ws = Out(dev, nbytes // 4)
    N.check(lib.p2l_affine_grid_sample(N.ptr(sd), N.ptr(td), N.ptr(dst.t), Bn, Cc, H, W, N.stream()), 'affine_grid_sample')
    N.check(lib.p2l_affine_grid_sample_bwd(N.ptr(sd), N.ptr(td), N.ptr(dd), N.ptr(dsrc.t) if want[0] else None,
                                           N.ptr(dth.t) if want[1] else None, Bn, Cc, H, W, N.ptr(ws.t),
                                           C.c_size_t(nbytes), N.stream()), 'affine_grid_sample_bwd')
    ws.cpu()
    a, b, c = dst.cpu(Bn, Cc, H, W), dsrc.cpu(Bn, Cc, H, W), dth.cpu(Bn, 6)
    assert want[0] or is_sentinel(b)
    assert want[1] or is_sentinel(c)
    return a, (b if want[0] else None), (c if want[1] else None)


def _dtheta_terms(src, theta, dout):
    """[Bn, 6, H*W], in the dtype of src: what one output pixel adds to d theta -- d L / d (ix, iy) summed over the
    channels, chained through i = ((g + 1) size - 1) / 2 and g = theta (g0x, g0y, 1)"""
    Bn, Cc, H, W = src.shape
    dt = src.dtype
    ix, iy = R.warp_coords(theta.to(dt), H, W)
    wx1, wy1 = (ix - ix.floor())[:, None], (iy - iy.floor())[:, None]
    v00, v01, v10, v11 = [v for v, _ in R.warp_corners(src, theta)]
    gix = (dout.to(dt) * ((v01 - v00) * (1 - wy1) + (v11 - v10) * wy1)).sum(1) * (0.5 * W)
    giy = (dout.to(dt) * ((v10 - v00) * (1 - wx1) + (v11 - v01) * wx1)).sum(1) * (0.5 * H)
    gx0 = ((2 * torch.arange(W, dtype=dt) + 1) / W - 1)[None, None, :]
    gy0 = ((2 * torch.arange(H, dtype=dt) + 1) / H - 1)[None, :, None]
    return torch.stack([gix * gx0, gix * gy0, gix, giy * gx0, giy * gy0, giy], dim=1).flatten(2)


def _warp_hold(dev, N, case, src, theta, dout, exact):
    """run, the bit-level statements, and the three outputs against fp64.  exact: the coordinates and the weights are
    exact in fp32 (no coordinate term, no exclusion).  Otherwise the coordinate bound enters the denominators (times
    the corner sum, counted as KC roundings), samples whose fp64 coordinate lies within that bound of an integer are
    left out of the forward comparison -- the floor may differ there -- and carry no gradient in the backward.
    -> the share of samples left out"""
    Bn, Cc, H, W = src.shape
    src6, th6 = d64(src, theta)
    near, bx, by = _near_integer(th6, H, W)
    ix, iy = R.warp_coords(th6, H, W)
    if exact:
        near = torch.zeros(Bn, H, W, dtype=torch.bool)
    else:
        dout = dout * (~near)[:, None].float()
    share = float(near.float().mean(dim=(1, 2)).max())
    got = _warp_run(dev, N, src, theta, dout)
    again = _warp_run(dev, N, src, theta, dout)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    alone = _warp_run(dev, N, src, theta, dout, sl=slice(Bn - 1, Bn))
    assert all(torch.equal(a[0], b[-1]) for a, b in zip(alone, got))
    assert torch.equal(_warp_run(dev, N, src, theta, dout, want=(1, 0))[1], got[1])
    assert torch.equal(_warp_run(dev, N, src, theta, dout, want=(0, 1))[2], got[2])
    dst, dsrc, dth = got
    dout6 = dout.to(D64)
    corners = R.warp_corners(src6, th6)
    cden = 0.0 if exact else ((bx + by) / KC).view(Bn, 1, 1, 1)
    kc = 0 if exact else KC
    keep = (~near)[:, None].expand(Bn, Cc, H, W)
    # forward: the weight's product, four products, three additions (the first adds to zero)
    ref = R.affine_warp(src6, th6)
    den = sum((v * w).abs() for v, w in corners) + cden * sum(v.abs() for v, _ in corners)
    hold('p2l_affine_grid_sample:dst', case, dst[keep], ref[keep], den[keep], R.affine_warp(src, theta)[keep], 8 + kc)
    outside = sum(v.abs() for v, _ in R.warp_corners(torch.ones_like(src6), th6)) == 0
    assert bool((dst[outside & keep] == 0).all())                               # all four corners outside: exactly 0
    # d src: every contributor of a source pixel a weight's product, a product and an addition
    rsrc, rth = R.affine_warp_bwd(src6, th6, dout6)
    f32 = R.affine_warp_bwd(src, theta, dout)
    ones = torch.ones_like(src6)
    touch = lambda gr: R.vjp(lambda s_: sum(v for v, _ in R.warp_corners(s_, th6)), [ones], gr)
    ncon = int(touch((~near)[:, None].expand_as(src6).to(D64)).max().item())
    den = R.affine_warp_bwd(src6, th6, dout6.abs())[0] + cden * touch(dout6.abs())
    hold('p2l_affine_grid_sample_bwd:dsrc', case, dsrc, rsrc, den, f32[0], 3 * max(ncon, 1) + kc)
    # d theta: per channel two differences, two products, a sum, the product with g, the addition (C of them); times
    # W / 2; times g0 (3 roundings of its own); 6 shuffles, the waves' tree (2), the blocks in sequence
    wx1, wy1 = (ix - ix.floor())[:, None], (iy - iy.floor())[:, None]
    v00, v01, v10, v11 = [v.abs() for v, _ in corners]
    ga = dout6.abs()
    # (d / d ix holds the weights along y, so it carries iy's bound, and the other way round)
    cy, cx = (0.0, 0.0) if exact else ((by / KC).view(Bn, 1, 1, 1), (bx / KC).view(Bn, 1, 1, 1))
    vsum = v00 + v01 + v10 + v11
    gix = (ga * ((v01 + v00) * (1 - wy1) + (v11 + v10) * wy1 + cy * vsum)).sum(1) * (0.5 * W)
    giy = (ga * ((v10 + v00) * (1 - wx1) + (v11 + v01) * wx1 + cx * vsum)).sum(1) * (0.5 * H)
    gx0 = ((2 * torch.arange(W, dtype=D64) + 1) / W - 1).abs()[None, None, :]
    gy0 = ((2 * torch.arange(H, dtype=D64) + 1) / H - 1).abs()[None, :, None]
    den = torch.stack([(gix * gx0).sum((1, 2)), (gix * gy0).sum((1, 2)), gix.sum((1, 2)),
                       (giy * gx0).sum((1, 2)), (giy * gy0).sum((1, 2)), giy.sum((1, 2))], dim=1)
    nblk = -(-(H * W) // 256)
    # (the fp32 restatement: the same per-pixel terms added in one chain -- 18 numbers a draw are too few to hold a
    #  tree against another tree; the terms themselves are the reference's: their fp64 sum is the vjp)
    t64 = _dtheta_terms(src6, th6, dout6).sum(2)
    assert bool(((t64 - rth).abs() <= 1e-10 * den + 1e-300).all())
    hold('p2l_affine_grid_sample_bwd:dtheta', case, dth, rth, den, _chain32(_dtheta_terms(src, theta, dout), 2),
         7 * Cc + 1 + 4 + 6 + 2 + nblk + kc)
    return share


def _exact_thetas(H, W):
    """entries are multiples of 2^-6 (H, W powers of two <= 32): ix, iy and the weights are exact in fp32"""
    px, py = 2.0 / W, 2.0 / H                                # one pixel in normalised coordinates
    I = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    sh = lambda dx, dy: [1.0, 0.0, dx * px, 0.0, 1.0, dy * py]
    return [
        ('identity', I), ('shift +1 px', sh(1, 0)), ('shift -2 px', sh(-2, -1)), ('shift +3 rows', sh(0, 3)),
        ('half pixel', sh(0.5, 0.5)), ('half pixel back', sh(-0.5, -0.5)),     # x0 = -1 at one end, x1 = W at the other
        ('1.5 px', sh(1.5, -1.5)), ('past the image', [1.0, 0.0, 4.0, 0.0, 1.0, 0.0]),
        ('past the image, rows', [1.0, 0.0, 0.0, 0.0, 1.0, -4.0]),
        ('flip x', [-1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), ('flip y', [1.0, 0.0, 0.0, 0.0, -1.0, 0.0]),
        ('flip both', [-1.0, 0.0, 0.0, 0.0, -1.0, 0.0]), ('rot 90', [0.0, 1.0, 0.0, -1.0, 0.0, 0.0]),
        ('scale 1/4', [0.25, 0.0, 0.0, 0.0, 0.25, 0.0]), ('scale 4', [4.0, 0.0, 0.0, 0.0, 4.0, 0.0]),
        ('shear', [1.0, 0.5, 0.0, 0.0, 1.0, 0.0]), ('zero matrix', [0.0, 0.0, 0.25, 0.0, 0.0, -0.25]),
        ('rank 1', [1.0, 1.0, 0.0, 1.0, 1.0, 0.0]),
    ]


@pytest.mark.parametrize('H,W', [(8, 8), (16, 32)])
@pytest.mark.parametrize('Cc', [1, 3])
@seeded
def test_affine_warp_exact_coordinates(dev, N, Cc, H, W):
    g = _gen(207, Cc, H, W)
    named = _exact_thetas(H, W)
    mag = _mags(3, -1.0, 1.0)
    for i in range(0, len(named), 3):
        grp = named[i:i + 3]
        theta = torch.tensor([t for _, t in grp])
        assert bool(((theta * 64) == (theta * 64).round()).all())
        src = randn(g, 3, Cc, H, W) * mag.view(3, 1, 1, 1)
        dout = randn(g, 3, Cc, H, W) * mag.flip(0).view(3, 1, 1, 1)
        case = 'C=%d %dx%d %s' % (Cc, H, W, ' / '.join(n for n, _ in grp))
        _warp_hold(dev, N, case, src, theta, dout, exact=True)
        if 'identity' in case:
            assert torch.equal(_warp_run(dev, N, src, theta, dout)[0][0], src[0])
    # |det| just below and just above the 1e-12 under which the gather visits the whole image: 2^-40, 2^-39 (the
    # samples of such a map all sit next to one point; their coordinates are rounded: the general bound)
    theta = torch.tensor([[2.0 ** -20, 0, 0.1, 0, 2.0 ** -20, -0.1], [2.0 ** -20, 0, 0.1, 0, 2.0 ** -19, -0.1],
                          [0.0, 2.0 ** -20, 0.0, -2.0 ** -19, 0.0, 0.0]])
    src, dout = randn(g, 3, Cc, H, W), randn(g, 3, Cc, H, W)
    assert _warp_hold(dev, N, 'C=%d %dx%d |det| = 2^-40, 2^-39' % (Cc, H, W), src, theta, dout, exact=False) == 0.0


def _general_thetas(g):
    from pix2latent_amd.transform.spatial_transform import SpatialTransform
    th = torch.eye(2, 3).view(1, 6) + 0.35 * randn(g, 2, 6)
    scale = 0.5 + 1.5 * torch.rand(1, generator=g)
    st = SpatialTransform._theta(scale, (torch.rand(1, 2, generator=g) - 0.5)).view(1, 6)
    return torch.cat([th, st], dim=0)


WARP_GENERAL = [(1, 24, 40), (3, 24, 40), (1, 37, 53), (3, 37, 53)]
WARP_CAP = 0.01


@pytest.mark.parametrize('Cc,H,W', WARP_GENERAL)
@seeded
def test_affine_warp_general(dev, N, Cc, H, W):
    """two or more 256-pixel blocks with a ragged last one; every image a theta of its own"""
    g = _gen(208, Cc, H, W)
    theta = _general_thetas(g)
    mag = _mags(3, -1.0, 1.0)
    src = randn(g, 3, Cc, H, W) * mag.view(3, 1, 1, 1)
    dout = randn(g, 3, Cc, H, W) * mag.flip(0).view(3, 1, 1, 1)
    share = _warp_hold(dev, N, 'C=%d %dx%d' % (Cc, H, W), src, theta, dout, exact=False)
    print('warp general C=%d %dx%d draw %d: %.4f %% of the samples left out' % (Cc, H, W, draw(), 100 * share))
    assert share < WARP_CAP


# =====================================================================================================================
# FIR blur of the up-convs
# =====================================================================================================================
def _blur_case(g, Bn, H, W, Cc):
    """the frame u [Bn, H+2, W+2, C] (last row and column zero), d [Bn, C], noise [Bn, H*W], bias [C].  In image
    draw % Bn channel 0 of u is zero and bias[0] = 0: without noise the pre-activation is +0; channel 1 likewise with
    bias -0 and a negative d: with nw = 0 and a negative noise it is -0"""
    mag = _mags(Bn, -1.0, 1.0)
    u = randn(g, Bn, H + 2, W + 2, Cc) * mag.view(Bn, 1, 1, 1)
    u[:, H + 1] = 0.0
    u[:, :, W + 1] = 0.0
    d = 0.5 + torch.rand(Bn, Cc, generator=g)
    noise = randn(g, Bn, H * W)
    bias = 0.3 * randn(g, Cc)
    b0 = draw() % Bn
    u[b0, :, :, 0:2] = 0.0
    bias[0], bias[1] = 0.0, -0.0
    d[b0, 1] = -d[b0, 1]
    return u, d, noise, bias, b0


def _blur_fwd_run(dev, N, u, d, noise, nw, bias, amax=None, next_s=None):
    lib = N.lib()
    Bn, UH, UW, Cc = u.shape
    H, W = UH - 2, UW - 2
    y = Out(dev, Bn * H * W * Cc)
    args = [N.ptr(u.contiguous().to(dev)), N.ptr(d.contiguous().to(dev)),
            N.ptr(noise.contiguous().to(dev)) if noise is not None else None, nw, N.ptr(bias.to(dev)), N.ptr(y.t), Bn, H, W,
            Cc]
    if amax is None:
        N.check(lib.p2l_sg2_blur_fwd(*(args + [N.stream()])), 'blur_fwd')
        return y.cpu(Bn, H, W, Cc)
    am = Out(dev, Bn * 64, prefill=torch.zeros(Bn * 64))
    N.check(lib.p2l_sg2_blur_fwd_amax(*(args + [N.ptr(next_s.contiguous().to(dev)) if next_s is not None else None,
                                               N.ptr(am.t) if amax else None, N.stream()])), 'blur_fwd_amax')
    got, amc = y.cpu(Bn, H, W, Cc), am.cpu(Bn, 64)
    if amax:
        seen = got * next_s.view(Bn, 1, 1, Cc) if next_s is not None else got
        assert torch.equal(amc.amax(dim=1), seen.abs().amax(dim=(1, 2, 3))), 'per-image maxima'
    else:
        assert bool((amc == 0).all())
    return got


def _blur_bwd_run(dev, N, gr, amax=None):
    lib = N.lib()
    Bn, H, W, Cc = gr.shape
    du = Out(dev, Bn * (H + 2) * (W + 2) * Cc)
    gd = gr.contiguous().to(dev)
    if amax is None:
        N.check(lib.p2l_sg2_blur_bwd(N.ptr(gd), N.ptr(du.t), Bn, H, W, Cc, N.stream()), 'blur_bwd')
        return du.cpu(Bn, H + 2, W + 2, Cc)
    am = Out(dev, Bn * 64, prefill=torch.zeros(Bn * 64))
    N.check(lib.p2l_sg2_blur_bwd_amax(N.ptr(gd), N.ptr(du.t), Bn, H, W, Cc, N.ptr(am.t) if amax else None, N.stream()),
            'blur_bwd_amax')
    got, amc = du.cpu(Bn, H + 2, W + 2, Cc), am.cpu(Bn, 64)
    if amax:
        assert torch.equal(amc.amax(dim=1), got.abs().amax(dim=(1, 2, 3))), 'per-image maxima'
    else:
        assert bool((amc == 0).all())
    return got


# a row sum: four products and three additions (the first adds to zero); the column sum: the same again
K_FIR = 14


@pytest.mark.parametrize('Bn', [1, 3, 5])
@pytest.mark.parametrize('Cc', [4, 12, 32, 64])
@pytest.mark.parametrize('H,W', [(4, 4), (4, 8), (8, 4), (8, 12), (16, 4)])
@seeded
def test_sg2_blur_fwd_bwd(dev, N, H, W, Cc, Bn):
    """H != W; (H / 4)(W / 4)(C / 4) items per image from 1 up: waves straddle images; UH = H + 2 is never a multiple
    of 4: every case cuts the last patch of the transpose"""
    g = _gen(209, H, W, Cc, Bn)
    u, d, noise, bias, b0 = _blur_case(g, Bn, H, W, Cc)
    next_s = randn(g, Bn, Cc) * 3.0
    u6, d6, noise6, bias6 = d64(u, d, noise, bias)
    case = 'Bn=%d %dx%d C=%d' % (Bn, H, W, Cc)
    for tag, nz, nw in (('noise', noise, 0.3), ('no noise', None, 0.3), ('nw=0', noise, 0.0)):
        y = _blur_fwd_run(dev, N, u, d, nz, nw, bias)
        for amax, ns in ((0, None), (1, None), (1, next_s)):                    # the _amax forms: the same bits
            assert torch.equal(_blur_fwd_run(dev, N, u, d, nz, nw, bias, amax, ns), y), (tag, amax)
        sl = slice(Bn - 1, Bn)
        assert torch.equal(_blur_fwd_run(dev, N, u[sl], d[sl], None if nz is None else nz[sl], nw, bias)[0], y[-1])
        if nw == 0.0 or nz is None:
            assert bool((y[b0, :, :, 0:2] == 0).all()), 'a pre-activation of +-0 must give 0'
        nz6 = None if nz is None else noise6
        ref = R.sg2_blur_fwd(u6, d6, nz6, nw, bias6)
        pre_den = R.blur4(u6.abs()) * d6.abs()[:, None, None, :] + bias6.abs()
        if nz is not None:
            pre_den = pre_den + abs(nw) * noise6.abs().view(Bn, H, W, 1)
        # the FIR, * d, + bias, nw * noise and its addition, sqrt2 (a rounded constant, for the negative slope a
        # rounded product of two) and the product with it
        k = K_FIR + 1 + 1 + 2 + 3
        # where the pre-activation is within its own rounding bound of zero fp32 may take the other slope
        slope = torch.where((ref > 0) | (ref.abs() <= R.SLOPE * R.SQRT2 * k * U * pre_den), R.SQRT2, R.SLOPE * R.SQRT2)
        hold('p2l_sg2_blur_fwd:y', case + ' ' + tag, y, ref, pre_den * slope,
             R.sg2_blur_fwd(u, d, nz, nw, bias), k)
    gr = randn(g, Bn, H, W, Cc) * _mags(Bn, -1.0, 1.0).view(Bn, 1, 1, 1)
    du = _blur_bwd_run(dev, N, gr)
    for amax in (0, 1):
        assert torch.equal(_blur_bwd_run(dev, N, gr, amax), du)
    assert torch.equal(_blur_bwd_run(dev, N, gr[-1:])[0], du[-1])
    # the whole frame is written, row H + 1 and column W + 1 from the last real row and column
    assert not bool((du.view(torch.int32) == SENT).any())
    assert bool((du[:, H + 1, 1:] != 0).all()) and bool((du[:, 1:, W + 1] != 0).all())
    gr6 = gr.to(D64)
    hold('p2l_sg2_blur_bwd:du', case, du, R.sg2_blur_bwd(gr6, H, W), R.sg2_blur_bwd(gr6.abs(), H, W),
         R.sg2_blur_bwd(gr, H, W), K_FIR)


# =====================================================================================================================
# refusals: rejected on the host, before anything is launched
# =====================================================================================================================
def test_refusals_before_any_launch(dev, N):
    lib, st = N.lib(), N.stream()
    a, b, c, d, e = (torch.ones(1 << 17, device=dev) for _ in range(5))
    o1, o2, o3 = Out(dev, 1 << 17), Out(dev, 1 << 17), Out(dev, 1 << 17)
    A, B, C_, D_, E = N.ptr(a), N.ptr(b), N.ptr(c), N.ptr(d), N.ptr(e)
    O1, O2, O3 = N.ptr(o1.t), N.ptr(o2.t), N.ptr(o3.t)
    sz = C.c_size_t

    def gemm(ws=False, A_=A, B_=B, C__=O1, **kw):
        f = dict(batch=1, M=128, Nn=32, K=16, lda=16, ldb=16, ldc=32, sa=0, sb=0, sc=0, akm=0, bkm=0, alpha=1.0, acc=0)
        f.update(kw)
        gd = _gemm_desc(N, **f)
        if ws:
            return lib.p2l_gemm_ws(C.byref(gd), A_, B_, C__, O2, sz(1 << 19), st)
        return lib.p2l_gemm(C.byref(gd), A_, B_, C__, st)

    def arb(da=A, x=B, s=C_, t=D_, skip=None, dx=O1, ds=O2, dt=O3, part=E, da_ld=32, x_ld=32, stb=32, sk_ld=32, skip_C=0,
            dx_ld=32, dsb=32, Bn=1, H=2, W=2, Cc=32):
        return lib.p2l_affine_relu_bwd(da, da_ld, x, x_ld, s, t, stb, skip, sk_ld, skip_C, 0, dx, dx_ld, ds, dt, dsb, part,
                                       Bn, H, W, Cc, st)

    def blur_f(u=A, d_=B, bias=C_, y=O1, Bn=1, H=4, W=4, Cc=4, amax=False):
        if amax:
            return lib.p2l_sg2_blur_fwd_amax(u, d_, D_, 0.3, bias, y, Bn, H, W, Cc, None, O2, st)
        return lib.p2l_sg2_blur_fwd(u, d_, D_, 0.3, bias, y, Bn, H, W, Cc, st)

    def blur_b(g_=A, du=O1, Bn=1, H=4, W=4, Cc=4, amax=False):
        if amax:
            return lib.p2l_sg2_blur_bwd_amax(g_, du, Bn, H, W, Cc, O2, st)
        return lib.p2l_sg2_blur_bwd(g_, du, Bn, H, W, Cc, st)

    def warp_b(src=A, th=B, dout=C_, dsrc=O1, dth=O2, Bn=1, Cc=1, H=8, W=8, ws=O3, nbytes=1 << 19):
        return lib.p2l_affine_grid_sample_bwd(src, th, dout, dsrc, dth, Bn, Cc, H, W, ws, sz(nbytes), st)

    calls = [
        ('gemm NULL d', lib.p2l_gemm(None, A, B, O1, st), EINVAL),
        ('gemm NULL A', gemm(A_=None), EINVAL), ('gemm NULL B', gemm(B_=None), EINVAL),
        ('gemm NULL C', gemm(C__=None), EINVAL), ('gemm_ws NULL C', gemm(ws=True, C__=None), EINVAL),
        ('gemm K=0', gemm(K=0), EINVAL), ('gemm_ws K=0', gemm(ws=True, K=0), EINVAL), ('gemm K<0', gemm(K=-16), EINVAL),
        ('gemm M=0', gemm(M=0), EINVAL), ('gemm N=0', gemm(Nn=0), EINVAL), ('gemm M%128', gemm(M=64), EINVAL),
        ('gemm N%32', gemm(Nn=48, ldc=48), EINVAL), ('gemm K%16', gemm(K=24, lda=24, ldb=24), EINVAL),
        ('gemm batch=0', gemm(batch=0), EINVAL), ('gemm batch>65535', gemm(batch=65536), EINVAL),
        ('gemm ldc<N', gemm(ldc=28), EINVAL), ('gemm_ws ldc<N', gemm(ws=True, ldc=28), EINVAL),
        ('gemm lda<K', gemm(K=32, lda=16, ldb=32), EINVAL), ('gemm ldb<K', gemm(K=32, lda=32, ldb=16), EINVAL),
        ('gemm lda<M (K-major)', gemm(akm=1, lda=64), EINVAL), ('gemm ldb<N (K-major)', gemm(bkm=1, ldb=16), EINVAL),
        ('gemm lda%4', gemm(lda=18), EINVAL), ('gemm ldb%4', gemm(ldb=18), EINVAL),
        ('gemm stride<0', gemm(sa=-4), EINVAL),
        ('softmax_fwd NULL S', lib.p2l_softmax_fwd(None, O1, 4, 256, st), EINVAL),
        ('softmax_fwd NULL P', lib.p2l_softmax_fwd(A, None, 4, 256, st), EINVAL),
        ('softmax_fwd rows=0', lib.p2l_softmax_fwd(A, O1, 0, 256, st), EINVAL),
        ('softmax_fwd rows<0', lib.p2l_softmax_fwd(A, O1, -4, 256, st), EINVAL),
        ('softmax_fwd rows: grid', lib.p2l_softmax_fwd(A, O1, 1 << 34, 256, st), EINVAL),
        ('softmax_fwd cols=128', lib.p2l_softmax_fwd(A, O1, 4, 128, st), EUNSUP),
        ('softmax_fwd cols=768', lib.p2l_softmax_fwd(A, O1, 4, 768, st), EUNSUP),
        ('softmax_fwd cols=4096', lib.p2l_softmax_fwd(A, O1, 4, 4096, st), EUNSUP),
        ('softmax_fwd cols=0', lib.p2l_softmax_fwd(A, O1, 4, 0, st), EUNSUP),
        ('softmax_bwd NULL P', lib.p2l_softmax_bwd(None, B, O1, 4, 256, st), EINVAL),
        ('softmax_bwd NULL dP', lib.p2l_softmax_bwd(A, None, O1, 4, 256, st), EINVAL),
        ('softmax_bwd NULL dS', lib.p2l_softmax_bwd(A, B, None, 4, 256, st), EINVAL),
        ('softmax_bwd rows=0', lib.p2l_softmax_bwd(A, B, O1, 0, 256, st), EINVAL),
        ('softmax_bwd cols=768', lib.p2l_softmax_bwd(A, B, O1, 4, 768, st), EUNSUP),
        ('arb NULL da', arb(da=None), EINVAL), ('arb NULL x', arb(x=None), EINVAL), ('arb NULL s', arb(s=None), EINVAL),
        ('arb NULL t', arb(t=None), EINVAL), ('arb NULL dx', arb(dx=None), EINVAL), ('arb NULL ds', arb(ds=None), EINVAL),
        ('arb NULL dt', arb(dt=None), EINVAL), ('arb NULL partial', arb(part=None), EINVAL),
        ('arb Bn=0', arb(Bn=0), EINVAL), ('arb Bn>65535', arb(Bn=65536), EINVAL), ('arb H=0', arb(H=0), EINVAL),
        ('arb W=0', arb(W=0), EINVAL), ('arb C=0', arb(Cc=0), EINVAL), ('arb C=16', arb(Cc=16), EINVAL),
        ('arb C=48', arb(Cc=48, da_ld=48, x_ld=48, dx_ld=48, stb=48, dsb=48), EINVAL),
        ('arb da_ld<C', arb(da_ld=28), EINVAL), ('arb x_ld<C', arb(x_ld=28), EINVAL), ('arb dx_ld<C', arb(dx_ld=28), EINVAL),
        ('arb da_ld%4', arb(da_ld=34), EINVAL), ('arb x_ld%4', arb(x_ld=34), EINVAL), ('arb dx_ld%4', arb(dx_ld=34), EINVAL),
        ('arb st_bstride<C', arb(stb=28), EINVAL), ('arb st_bstride%4', arb(stb=34), EINVAL),
        ('arb dsdt_bstride<C', arb(dsb=28), EINVAL), ('arb dsdt_bstride%4', arb(dsb=34), EINVAL),
        ('arb skip_C<0', arb(skip=A, skip_C=-4), EINVAL), ('arb skip_C>C', arb(skip=A, skip_C=36, sk_ld=36), EINVAL),
        ('arb skip_C%4', arb(skip=A, skip_C=6), EINVAL), ('arb skip_ld%4', arb(skip=A, skip_C=4, sk_ld=34), EINVAL),
        ('arb skip_ld<skip_C', arb(skip=A, skip_C=32, sk_ld=28), EINVAL),
        ('arb_finish NULL partial', lib.p2l_arb_finish(None, O1, O2, 1, 1, 32, 32, st), EINVAL),
        ('arb_finish NULL ds', lib.p2l_arb_finish(A, None, O2, 1, 1, 32, 32, st), EINVAL),
        ('arb_finish NULL dt', lib.p2l_arb_finish(A, O1, None, 1, 1, 32, 32, st), EINVAL),
        ('arb_finish Bn=0', lib.p2l_arb_finish(A, O1, O2, 0, 1, 32, 32, st), EINVAL),
        ('arb_finish Bn>65535', lib.p2l_arb_finish(A, O1, O2, 65536, 1, 32, 32, st), EINVAL),
        ('arb_finish nblk=0', lib.p2l_arb_finish(A, O1, O2, 1, 0, 32, 32, st), EINVAL),
        ('arb_finish C=16', lib.p2l_arb_finish(A, O1, O2, 1, 1, 16, 32, st), EINVAL),
        ('arb_finish bstride<C', lib.p2l_arb_finish(A, O1, O2, 1, 1, 64, 32, st), EINVAL),
        ('arb_finish bstride%4', lib.p2l_arb_finish(A, O1, O2, 1, 1, 32, 34, st), EINVAL),
        ('warp NULL src', lib.p2l_affine_grid_sample(None, B, O1, 1, 1, 8, 8, st), EINVAL),
        ('warp NULL theta', lib.p2l_affine_grid_sample(A, None, O1, 1, 1, 8, 8, st), EINVAL),
        ('warp NULL dst', lib.p2l_affine_grid_sample(A, B, None, 1, 1, 8, 8, st), EINVAL),
        ('warp Bn=0', lib.p2l_affine_grid_sample(A, B, O1, 0, 1, 8, 8, st), EINVAL),
        ('warp C=0', lib.p2l_affine_grid_sample(A, B, O1, 1, 0, 8, 8, st), EINVAL),
        ('warp H=0', lib.p2l_affine_grid_sample(A, B, O1, 1, 1, 0, 8, st), EINVAL),
        ('warp W<0', lib.p2l_affine_grid_sample(A, B, O1, 1, 1, 8, -8, st), EINVAL),
        ('warp_bwd NULL theta', warp_b(th=None), EINVAL), ('warp_bwd NULL dout', warp_b(dout=None), EINVAL),
        ('warp_bwd no output', warp_b(dsrc=None, dth=None), EINVAL), ('warp_bwd dtheta, NULL src', warp_b(src=None), EINVAL),
        ('warp_bwd Bn=0', warp_b(Bn=0), EINVAL), ('warp_bwd C=0', warp_b(Cc=0), EINVAL), ('warp_bwd H=0', warp_b(H=0), EINVAL),
        ('warp_bwd W=0', warp_b(W=0), EINVAL), ('warp_bwd dtheta, Bn>65535', warp_b(Bn=65536, nbytes=1 << 30), EINVAL),
        ('warp_bwd NULL workspace', warp_b(ws=None), EWS), ('warp_bwd short workspace', warp_b(nbytes=20), EWS),
        ('blur_fwd NULL u', blur_f(u=None), EINVAL), ('blur_fwd NULL d', blur_f(d_=None), EINVAL),
        ('blur_fwd NULL bias', blur_f(bias=None), EINVAL), ('blur_fwd NULL y', blur_f(y=None), EINVAL),
        ('blur_fwd_amax NULL y', blur_f(y=None, amax=True), EINVAL),
        ('blur_fwd Bn=0', blur_f(Bn=0), EINVAL), ('blur_fwd H=0', blur_f(H=0), EINVAL), ('blur_fwd W=0', blur_f(W=0), EINVAL),
        ('blur_fwd C=0', blur_f(Cc=0), EINVAL), ('blur_fwd H%4', blur_f(H=6), EINVAL), ('blur_fwd W%4', blur_f(W=6), EINVAL),
        ('blur_fwd C%4', blur_f(Cc=6), EINVAL), ('blur_fwd_amax W%4', blur_f(W=6, amax=True), EINVAL),
        ('blur_bwd NULL g', blur_b(g_=None), EINVAL), ('blur_bwd NULL du', blur_b(du=None), EINVAL),
        ('blur_bwd_amax NULL du', blur_b(du=None, amax=True), EINVAL),
        ('blur_bwd Bn=0', blur_b(Bn=0), EINVAL), ('blur_bwd H=0', blur_b(H=0), EINVAL), ('blur_bwd W<0', blur_b(W=-4), EINVAL),
        ('blur_bwd C=0', blur_b(Cc=0), EINVAL), ('blur_bwd C%4', blur_b(Cc=6), EINVAL),
        ('blur_bwd_amax C%4', blur_b(Cc=6, amax=True), EINVAL),
    ]
    bad = [(what, rc, want) for what, rc, want in calls if rc != want]
    assert not bad, bad
    assert is_sentinel(o1.cpu()) and is_sentinel(o2.cpu()) and is_sentinel(o3.cpu())

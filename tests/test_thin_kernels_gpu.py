"""The thin 3x3 routes (taps = 9, ups = 0, P2L_WFMT_BF16X3T: three real channels on one side, the image ends of both
pipelines) -- TI: conv_thinin_kernel (16 (3 real) -> Cout, the 27 tap-channel products as one K dimension), TO:
conv_thinout_kernel (Cin -> 32 (3 real), a pointwise product onto 27 columns and a nine-tap gather; csrc/p2l_thin.hip),
B: the generic bf16 x 3 kernel on the first image of the same buffer -- under P2L_FORM_NO_THIN, for a shape thin_shape
does not take, and wherever the ARGUMENTS of a launch keep it off the thin kernels (thin_takes: oscale / noise; on a
thin-output shape a residual, a mask, a pool, y == NULL, a fused backward) -- and F (P2L_WFMT_F32), recorded next to
each: forward and fused input gradient, against the float64 references of tests/_small_refs.py, through ctypes, with
the harness, the metric and the bars of tests/test_small_kernels_gpu.py (tests/_pin.py):

    p2l_conv_fwd, p2l_conv_fwd_ex, p2l_conv_dgrad_arb, p2l_pack_conv_weight_bf3t, p2l_pack_conv_weight_bf3,
    p2l_pack_conv_weight, p2l_packed_weight_floats, p2l_conv_amax_slots, p2l_conv_suggest_splitk,
    p2l_conv_workspace_bytes, p2l_conv_arb_nblk.

Every launch proves its route under the launch profiler: one 3x3 launch, six products per fp32 product, and for TI /
TO the family THIN with 2 B H W 32 Cout / 2 B H W 1.5 Cin 32 executed products (launch_thin), for B the family OTHER
with the direct count; a case the dispatch moves elsewhere fails.  Rounded outputs are held to |got - r64| / den_d <=
min(k, 4 x the route's fp32 restatement) x 2^-24 with den_d = sum_taps,k |a| |w| through the epilogue and k counted in
_small_refs.thin_k (B: direct_k); every TI / TO case runs on B as well, held, and on F, recorded.  No element is left
out of a comparison.  What the contract calls exact is compared bit for bit.  Every output sits between guard bands,
every pitch but the products' y_ld = n_store is above its row with junk (inputs) or sentinels (outputs) in the gap.
P2L_THIN_ERR_FILE=<path> records the figures (profiles/thin_kernels_err.txt).  The cases, their inputs and k live in
tests/_small_refs.py; tests/test_small_refs.py holds them to "the restatement is within k / 4" on the host."""
import ctypes as C

import pytest
import torch

import _small_refs as R
from _pin import (D64, G, N, SENT, Out, _gen, _record_file, hold, hold_k, is_sentinel, note, randn,  # noqa: F401
                  seeded)

pytestmark = pytest.mark.gpu
EINVAL = -1
FAM_OTHER, FAM_THIN = 0, 4


def _pitched(t, ld, dev, junk=7.0):
    """[..., C] -> the same rows at pitch ld on the device, junk in the gap columns"""
    o = torch.full(t.shape[:-1] + (ld,), junk)
    n = min(ld, t.shape[-1])
    o[..., :n] = t[..., :n]
    return o.to(dev)


class _Got(object):
    pass


def _profiled(N, fn):
    """fn() under the launch profiler -> its return code and the totals of the launches it made"""
    lib = N.lib()
    N.check(lib.p2l_prof_begin(64), 'p2l_prof_begin')
    lib.p2l_prof_step(0, 1)
    rc = fn()
    torch.cuda.synchronize()
    T = N.prof_end()
    ratio = T.mfma_flops[0] / T.exec_flops[0] if T.count[0] else 0.0
    return rc, ratio, T.exec_flops[0], (T.count[0], T.count[1]), list(T.fam_count)


def _on_route(got, c, route, what=''):
    """one 3x3 launch; six (F: sixteen) products per fp32 product; TI / TO: the family THIN and the executed products
    launch_thin reports (ProfSlot::took(P2L_PROF_FAM_THIN, 0, ..)); B / F: the family OTHER and the direct count"""
    px = 2.0 * got.B * c['H'] * c['W']
    want = {'TI': px * 32.0 * c['Cout'], 'TO': px * 1.5 * c['Cin'] * 32.0}.get(route, px * c['Cin'] * c['Cout'] * 9)
    fam = FAM_THIN if route in ('TI', 'TO') else FAM_OTHER
    assert got.rc == 0, (what, got.rc)
    assert got.count == (1, 0), (what, got.count)
    assert abs(got.ratio - (16.0 if route == 'F' else 6.0)) < 1e-6, (what, route, got.ratio)
    assert got.fam[fam] == 1 and sum(got.fam) == 1, '%s: expected route %s, got families %s' % (what, route, got.fam)
    assert abs(got.exec_flops - want) <= 1e-9 * want, (what, route, got.exec_flops, want)


def _thin_mode(c):
    return 0 if c['Cout'] == 32 and c['Cin'] > 16 else 1 if c['Cin'] == 16 and c['Cout'] > 32 else -1


def _weights(dev, N, i, c, wfmt, flip=False):
    """the packed buffer of the case's weight in format wfmt, from the real channels alone; flip: through the
    transpose_flip copy, from the OIHW tensor of the forward conv whose input gradient the launch applies.  A shape
    neither thin mode admits has no thin image to pack (the packer refuses it): its P2L_WFMT_BF16X3T buffer is the
    bf16 x 3 image, which the format puts first, in a buffer of the format's size"""
    lib = N.lib()
    cache = i.setdefault('_packed', {})
    key = (id(i['w']), wfmt, flip)
    if key not in cache:
        src = R.thin_weight(c, i, flip).to(dev)
        if wfmt == R.WFMT_BF16X3T and _thin_mode(c) < 0:
            dst = torch.zeros(lib.p2l_packed_weight_floats(9, c['Cout'], c['Cin'], wfmt), device=dev)
            N.check(lib.p2l_pack_conv_weight_bf3(N.ptr(src), src.shape[0], src.shape[1], 9, c['Cout'], c['Cin'],
                                                 int(flip), N.ptr(dst), N.stream()), 'p2l_pack_conv_weight_bf3')
        else:
            dst = N.pack_conv_weight(src, 9, c['Cout'], c['Cin'], flip, wfmt)
        cache[key] = (i['w'], dst)
    return cache[key][1]


def _desc(N, c, wfmt, form, B):
    d = N.P2LConv()
    d.B, d.H, d.W, d.Cin, d.Cout, d.taps, d.ups = B, c['H'], c['W'], c['Cin'], c['Cout'], 9, 0
    d.x_ld, d.alpha, d.splitk = c['Cin'] + c.get('x_gap', 4), c['alpha'], 1
    d.wfmt, d.form = wfmt, form
    return d


def _fwd(dev, N, c, i, route=None, sl=None, want_amax=False, next_st=None, tamper=None, flip=False, amax_anyway=False):
    """one forward launch of case c on inputs i (images sl) on `route` (default: the case's) -> _Got: rc, y [B, H, W,
    n_store], yp, the profiler's figures, the maxima slots.  Everything the launch may write is an Out; the gap
    columns are checked here."""
    lib = N.lib()
    route = route or c['route']
    sl = slice(0, c['B']) if sl is None else sl
    B, H, W, Cin, Cout, ns = sl.stop - sl.start, c['H'], c['W'], c['Cin'], c['Cout'], c['n_store']
    wfmt, form = R.thin_form(c, route)
    wp = _weights(dev, N, i, c, wfmt, flip)
    d = _desc(N, c, wfmt, form, B)
    d.pro, d.act, d.pool = c['pro'], c['act'], c['pool']
    d.y_ld, d.yp_ld = ns + c['y_gap'], ns + 4
    d.n_store, d.res_ups, d.w_floats = ns, int(c['res'] == 'ups'), wp.numel()
    xd = _pitched(i['x'][sl], d.x_ld, dev)
    sd = td = resd = maskd = None
    if c['pro'] != R.PRO_NONE:
        d.pro_bstride = Cin + 4 if c['pro_b'] else 0
        rows = sl if c['pro_b'] else slice(0, 1)
        sd, td = _pitched(i['s'][rows], Cin + 4, dev, -5.0), _pitched(i['t'][rows], Cin + 4, dev, 9.0)
    if c['res']:
        d.res_ld = ns + 8 if c['res'] == 'same' else Cout + 32
        resd = _pitched(i['res'][sl], d.res_ld, dev, 3.0)
    if c['mask']:
        d.mask_ld = ns + 12
        maskd = _pitched(i['mask'][sl], d.mask_ld, dev, 1.0)
    y = Out(dev, B * H * W * (ns + c['y_gap'])) if c['want_y'] else None
    yp = Out(dev, B * (H // 2) * (W // 2) * (ns + 4)) if c['pool'] != R.POOL_NONE else None
    biasd = i['bias'].to(dev) if c['bias'] else None
    ex = None
    if c['oscale'] or c['noise'] or want_amax:
        ex = N.P2LConvExtra()
        if c['oscale']:
            ex.oscale, ex.oscale_bstride = N.ptr(_pitched(i['oscale'][sl], Cout + 4, dev, 2.0)).value, Cout + 4
        if c['noise']:
            ex.noise, ex.noise_w = N.ptr(i['noise'][sl].contiguous().to(dev)).value, i['noise_w']
    y_ld = d.y_ld
    if tamper is not None:
        tamper(d)
    slots = lib.p2l_conv_amax_slots(C.byref(d)) if want_amax else 0
    am = amp = None
    if want_amax and (slots > 0 or amax_anyway):
        am = Out(dev, B * max(slots, 4))
        ex.amax.out = N.ptr(am.t).value
        if yp is not None:
            amp = Out(dev, B * max(slots, 4))
            ex.amax.outp = N.ptr(amp.t).value
        if next_st is not None:
            ex.amax.next_s, ex.amax.next_t = N.ptr(next_st[0].to(dev)).value, N.ptr(next_st[1].to(dev)).value
            ex.amax.next_bstride = next_st[0].shape[1]
    got = _Got()
    got.ws_bytes, got.suggest = lib.p2l_conv_workspace_bytes(C.byref(d)), lib.p2l_conv_suggest_splitk(C.byref(d))

    def call():
        args = (N.ptr(xd), N.ptr(wp), N.ptr(biasd), N.ptr(sd), N.ptr(td), N.ptr(resd), N.ptr(maskd),
                N.ptr(y.t) if y else None, N.ptr(yp.t) if yp else None, None, C.c_size_t(0), N.stream())
        if ex is None:
            return lib.p2l_conv_fwd(C.byref(d), *args)
        return lib.p2l_conv_fwd_ex(C.byref(d), C.byref(ex), *args)
    got.B = B
    got.rc, got.ratio, got.exec_flops, got.count, got.fam = _profiled(N, call)
    got.ex, got.slots, got.outs = ex is not None, slots, [o for o in (y, yp, am, amp) if o is not None]
    got.y = got.yp = got.amax = got.amaxp = None
    if y is not None:
        full = y.cpu(B, H, W, y_ld)
        assert got.rc != 0 or is_sentinel(full[..., ns:]), 'gap columns of y written'
        got.y = full[..., :ns].contiguous()
    if yp is not None:
        full = yp.cpu(B, H // 2, W // 2, ns + 4)
        assert got.rc != 0 or is_sentinel(full[..., ns:]), 'gap columns of yp written'
        got.yp = full[..., :ns].contiguous()
    if am is not None:
        got.amax = am.cpu(B, -1)
    if amp is not None:
        got.amaxp = amp.cpu(B, -1)
    return got


def _untouched(got):
    return all(is_sentinel(o.cpu()) for o in got.outs)


def _entry(got):
    return 'p2l_conv_fwd_ex' if got.ex else 'p2l_conv_fwd'


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, names, what=''):
    for name in names:
        u, v = getattr(a, name), getattr(b, name)
        assert (u is None) == (v is None), (what, name)
        if u is not None:
            assert torch.equal(_bits(u), _bits(v)), (what, name, int((u != v).sum()))


def _held(got, c, i, route, cid):
    r64, r32 = R.thin_refs(c, i, route)
    for name in ('y', 'yp'):
        if getattr(got, name) is not None:
            hold('%s:%s' % (_entry(got), name), cid, getattr(got, name), r64[name],
                 r64['den' if name == 'y' else 'denp'], r32[name], R.thin_k(c, route, pooled=name == 'yp'))
    return r64


# =====================================================================================================================
# forward: every route, every epilogue
# =====================================================================================================================
@pytest.mark.parametrize('case', R.THIN_FWD_CASES, ids=R.thin_id)
@seeded
def test_forward(dev, N, case):
    cid = R.thin_id(case)
    i = R.thin_inputs(_gen('thin', cid), case)
    got = _fwd(dev, N, case, i)
    _on_route(got, case, case['route'], cid)
    assert R.thin_kind(case) < 0 or (got.ws_bytes == 0 and got.suggest == 1)
    r64 = _held(got, case, i, case['route'], cid)
    if case['route'] != 'B':
        # the same inputs on the generic kernel, from the same buffer (P2L_FORM_NO_THIN): held under direct_k
        twin = _fwd(dev, N, case, i, route='B')
        _on_route(twin, case, 'B', cid + ' on B')
        _held(twin, case, i, 'B', cid + ' on B')
    f = _fwd(dev, N, case, i, route='F')
    _on_route(f, case, 'F', cid + ' on F')
    for name in ('y', 'yp'):
        if getattr(f, name) is not None:
            note('%s:%s' % (_entry(f), name), cid + ' on F', getattr(f, name), r64[name],
                 r64['den' if name == 'y' else 'denp'])
    # exact: a repeated launch; a masked element is +0; yp is the pool of the y this launch stored
    _same_bits(_fwd(dev, N, case, i), got, ('y', 'yp'), cid)
    if case['mask'] and got.y is not None:
        dead = ~(i['mask'][..., :case['n_store']] > 0)
        assert bool(dead.any()) and bool((_bits(got.y)[dead] == 0).all())
    if got.y is not None and got.yp is not None:
        v0, v1, v2, v3 = R.quads(got.y)
        want = torch.maximum(torch.maximum(v0, v1), torch.maximum(v2, v3)) if case['pool'] == R.POOL_MAX \
            else (v0 + v1) + (v2 + v3)
        assert torch.equal(got.yp, want)


TO_CASES = [c for c in R.THIN_FWD_CASES if c['route'] == 'TO']


@pytest.mark.parametrize('case', TO_CASES, ids=R.thin_id)
def test_thin_output_stores_act_of_bias_behind_its_three_channels(dev, N, case):
    """channels 3 .. n_store - 1 of what a thin-output launch stores are act(bias[c]) at every pixel -- the same bits
    everywhere; the fp32 value itself where the activation is none, ReLU or the leaky ReLU (one fp32 product with the
    kernel's constant 1.41421356237f or 0.2f * 1.41421356237f); under tanh the bits the generic kernel stores for the
    same channel (both hand the bias itself to the same tanhf), within the 5 ulp OpenCL allows tanh of the fp64 value
    -- and +0 bits with a zero or absent bias; the generic kernel stores the same from the same buffer"""
    ns = case['n_store']
    i = R.thin_inputs(_gen('to-pad', R.thin_id(case)), case)
    for bias in ('case', 'zero'):
        ii = dict(i)
        if bias == 'zero' and case['bias']:
            ii['bias'] = torch.zeros(case['Cout'])
        firsts = {}
        for route in ('TO', 'B'):
            got = _fwd(dev, N, case, ii, route=route)
            _on_route(got, case, route)
            pad = got.y[..., 3:ns]
            assert pad.shape[-1] == ns - 3
            first = pad[0, 0, 0]
            assert torch.equal(_bits(pad), _bits(first.expand_as(pad))), (route, bias)
            if not case['bias'] or bias == 'zero':
                assert bool((_bits(pad) == 0).all()), (route, bias)
            elif case['act'] == R.ACT_TANH:
                firsts[route] = first
                want = torch.tanh(ii['bias'][3:ns].double())
                ulp = 2.0 ** (torch.floor(torch.log2(want.abs())) - 23)
                assert bool(((first.double() - want).abs() <= 5 * ulp).all()), (route, bias)
            else:
                bv = ii['bias'][3:ns]
                a = torch.tensor(1.41421356237, dtype=torch.float32)
                want = {R.ACT_NONE: bv, R.ACT_RELU: torch.relu(bv),
                        R.ACT_LRELU_SQRT2: bv * torch.where(bv > 0, a, torch.tensor(0.2, dtype=torch.float32) * a)}[case['act']]
                assert torch.equal(_bits(first), _bits(want)), (route, bias)
        if firsts:
            assert torch.equal(_bits(firsts['TO']), _bits(firsts['B'])), bias


# =====================================================================================================================
# exact inputs: tap, channel and pixel placement bit for bit
# =====================================================================================================================
ONEHOT = [R._tsh('TI', 'i8x16'), R._tsh('TI', 'i16x32'), R._tsh('TI', 'i24x16'), R._tsh('TI', 'i8x48'),
          R._tsh('TO', 'o8x16', n_store=4), R._tsh('TO', 'o16x32', n_store=16, y_gap=0), R._tsh('TO', 'o24x16', n_store=4),
          R._tsh('TO', 'o8x48', n_store=32), R._tsh('B', 'i16x32'), R._tsh('B', 'o16x32', n_store=16),
          R._tsh('B', 'n12x20'), R._tsh('B', 'n32from16', n_store=16)]


@pytest.mark.parametrize('flip', [False, True], ids=['forward', 'transpose_flip'])
@pytest.mark.parametrize('tap', range(9))
def test_one_hot_inputs_are_exact(dev, N, tap, flip):
    """single power-of-two pixels at the corners, the edges, both sides of every block seam, wave boundary and quad
    boundary and the first and last pixel of the second image, single power-of-two weights on one tap: every route
    gives the fp64 result bit for bit -- also through the transpose_flip copy of the packer"""
    for c in ONEHOT:
        if flip and _thin_mode(c) < 0:
            continue
        i = R.thin_onehot(c, tap, tap % 2)
        got = _fwd(dev, N, c, i, flip=flip)
        _on_route(got, c, c['route'], R.thin_id(c))
        want = R.conv3x3(i['x'].double(), i['w'].double(), den_w=False)['y'][..., :c['n_store']]
        assert int((want != 0).sum()) >= 3
        assert torch.equal(got.y.double(), want), (R.thin_id(c), int((got.y.double() != want).sum()))


def test_all_zero_inputs_give_exactly_zero(dev, N):
    for c in (R._tsh('TI', 'i16x32'), R._tsh('TO', 'o16x32', n_store=16), R._tsh('B', 'o24x16', n_store=16),
              R._tsh('B', 'i8x48')):
        i = R.thin_inputs(_gen('zero', R.thin_id(c)), c)
        i['x'] = torch.zeros_like(i['x'])
        got = _fwd(dev, N, c, i)
        _on_route(got, c, c['route'])
        assert bool((_bits(got.y) == 0).all()), R.thin_id(c)


# =====================================================================================================================
# bit-exact contracts
# =====================================================================================================================
ALONE = [c for c in R.THIN_FWD_CASES if c['B'] > 1 and R.thin_kind(c) >= 0 and
         (c['route'] != 'B' or R.thin_falls_back(c))]


@pytest.mark.parametrize('case', ALONE, ids=R.thin_id)
def test_an_image_alone_has_the_bits_it_has_in_any_batch(dev, N, case):
    """on TI, on TO and on the launch-side fallback; every image of the batch, at magnitudes 3e14 apart"""
    i = R.thin_inputs(_gen('alone', R.thin_id(case)), case)
    whole = _fwd(dev, N, case, i)
    _on_route(whole, case, case['route'])
    for b in range(case['B']):
        one = _fwd(dev, N, case, i, sl=slice(b, b + 1))
        _on_route(one, case, case['route'])
        for name in ('y', 'yp'):
            if getattr(whole, name) is not None:
                assert torch.equal(_bits(getattr(one, name)[0]), _bits(getattr(whole, name)[b])), (name, b)


def _set(**kw):
    def tamper(d, *_):
        for k, v in kw.items():
            setattr(d, k, v)
    return tamper


SLICED = [R._tsh('TI', 'i16x32', **R.EPI[1]), R._tsh('TI', 'i24x16', pro=R.PRO_AFFINE, pro_b=0, bias=True, act=R.ACT_RELU),
          R._tsh('TO', 'o16x32', n_store=16, y_gap=0, pro=R.PRO_AFFINE_RELU, pro_b=0, bias=True, act=R.ACT_TANH),
          R._tsh('TO', 'o24x16', n_store=16, y_gap=0), R._tsh('B', 'o8x16', n_store=16, res='same', bias=True),
          R._tsh('B', 'i8x48', noise=True, bias=True)]


@pytest.mark.parametrize('case', SLICED, ids=R.thin_id)
def test_a_slice_request_changes_nothing(dev, N, case):
    """a thin shape never takes K slices, on its own kernels or on the generic one it falls back to: d.splitk = 4 gives
    the bits of splitk = 1, p2l_conv_workspace_bytes asks for nothing and p2l_conv_suggest_splitk is 1"""
    assert R.thin_kind(case) >= 0 and (case['route'] != 'B' or R.thin_falls_back(case))
    i = R.thin_inputs(_gen('splitk', R.thin_id(case)), case)
    one = _fwd(dev, N, case, i)
    four = _fwd(dev, N, case, i, tamper=_set(splitk=4))
    for got in (one, four):
        _on_route(got, case, case['route'])
        assert got.ws_bytes == 0 and got.suggest == 1
    _same_bits(one, four, ('y', 'yp'))


# =====================================================================================================================
# maxima
# =====================================================================================================================
AMAX_CASES = [R._tsh('TI', 'i16x32', pro=R.PRO_AFFINE, pro_b=0, bias=True, act=R.ACT_RELU),    # the first VGG conv
              R._tsh('TI', 'i24x16', act=R.ACT_RELU, pool=R.POOL_MAX), R._tsh('TI', 'i8x48', n_store=36, bias=True),
              R._tsh('TI', 'i8x16', alpha=0.5, act=R.ACT_TANH)]


@pytest.mark.parametrize('nxt', [False, True], ids=['plain', 'next-affine'])
@pytest.mark.parametrize('case', AMAX_CASES, ids=R.thin_id)
def test_the_maxima_slots_hold_the_maximum_of_what_was_stored(dev, N, case, nxt):
    """thin input: p2l_conv_amax_slots(d) = blocks per image x 4 (one per wave); the per-image maximum over them ==
    max |y| of the y the launch stored (outp: of yp), with next_s / next_t == max |fma(y, s, t)|, bit for bit; every
    slot is written and non-negative; the buffers are exactly that long, between guard bands"""
    g = _gen('amax', R.thin_id(case))
    i = R.thin_inputs(g, case)
    B, ns = case['B'], case['n_store']
    st = (0.5 + torch.rand(B, ns, generator=g), randn(g, B, ns) * R.mags(B).view(B, 1)) if nxt else None
    got = _fwd(dev, N, case, i, want_amax=True, next_st=st)
    _on_route(got, case, 'TI')
    assert got.slots == (case['H'] // 8) * (case['W'] // 16) * 4 and got.amax.shape == (B, got.slots)
    assert bool((_bits(got.amax) != SENT).all()) and bool((got.amax >= 0).all())
    assert torch.equal(got.amax.amax(dim=1), R.producer_amax(got.y, *st) if nxt else R.producer_amax(got.y))
    if got.amaxp is not None:
        assert bool((_bits(got.amaxp) != SENT).all())
        assert torch.equal(got.amaxp.amax(dim=1), R.producer_amax(got.yp))
    # a slot is its wave's: rows 2 w, 2 w + 1 of block (ty, tx), at tile * 4 + w
    if not nxt:
        blocks = got.y.abs().reshape(B, case['H'] // 8, 4, 2, case['W'] // 16, 16, ns).amax(dim=(3, 5, 6))
        assert torch.equal(got.amax.view(B, case['H'] // 8, case['W'] // 16, 4), blocks.permute(0, 1, 3, 2))


def test_thin_output_and_fallback_launches_record_no_maxima(dev, N):
    """p2l_conv_amax_slots is 0 for a thin-output shape: its launch ignores the fields.  For a thin-input shape the
    query -- a function of the descriptor -- promises blocks x 4 slots; with oscale or noise the launch runs the
    generic kernel, whose tiles are others, and records none (conv_prepare): every slot still holds what it held.
    Pinned as what the launcher does today and the header now says, not as what is wanted: a reader of such slots
    would take stale maxima (no plan launches this combination; DESIGN lists it as open)"""
    c = R._tsh('TO', 'o16x32', n_store=16, bias=True)
    got = _fwd(dev, N, c, R.thin_inputs(_gen('amax-to'), c), want_amax=True, amax_anyway=True)
    _on_route(got, c, 'TO')
    assert got.slots == 0 and is_sentinel(got.amax)
    for kw in (dict(oscale=True), dict(noise=True)):
        c = R._tsh('B', 'i16x32', bias=True, **kw)
        got = _fwd(dev, N, c, R.thin_inputs(_gen('amax-fb'), c), want_amax=True)
        _on_route(got, c, 'B')
        assert got.slots == 2 * 2 * 4 and is_sentinel(got.amax)


# =====================================================================================================================
# fused input gradient
# =====================================================================================================================
def _arb(dev, N, c, i, route=None, tamper=None):
    """one p2l_conv_dgrad_arb launch of case c -> _Got: rc, dx, ds, dt and the profiler's figures; the weight goes
    through the transpose_flip pack, from the OIHW tensor of the forward conv whose input gradient the launch applies"""
    lib = N.lib()
    route = route or c['route']
    B, H, W, Cin, Cout = c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    Ho, Wo = (H // 2, W // 2) if c['pool_sum'] else (H, W)
    wfmt = 0 if route == 'F' else R.WFMT_BF16X3T
    form = R.FORM_NO_THIN if route == 'B' and _thin_mode(c) == 1 else 0        # (a thin-output shape: by the arb alone)
    wp = _weights(dev, N, i, c, wfmt, True)
    d = _desc(N, dict(c, alpha=1.0), wfmt, form, B)
    d.y_ld, d.yp_ld, d.n_store, d.w_floats = Cout + 4, Cout + 4, Cout, wp.numel()
    d.pool = R.POOL_SUM if c['pool_sum'] else R.POOL_NONE
    a = N.P2LArb()
    a.x, a.x_ld = N.ptr(_pitched(i['ax'], Cout + 8, dev)).value, Cout + 8
    a.s = N.ptr(_pitched(i['as'], Cout + 4, dev, -5.0)).value
    a.t = N.ptr(_pitched(i['at'], Cout + 4, dev, 9.0)).value
    a.st_bstride, a.nomask = Cout + 4, int(c['nomask'])
    if c['skip']:
        a.skip, a.skip_ld = N.ptr(_pitched(i['skip'], Cout + 12, dev, 3.0)).value, Cout + 12
        a.skip_C, a.skip_ups = Cout // 2, int(c['skip'] == 'ups')
    ds, dt = Out(dev, B * (Cout + 4)), Out(dev, B * (Cout + 4))
    a.ds, a.dt, a.dsdt_bstride = N.ptr(ds.t).value, N.ptr(dt.t).value, Cout + 4
    if tamper is not None:
        tamper(d, a)
    nblk = lib.p2l_conv_arb_nblk(C.byref(d))
    assert nblk == (H // 8) * (W // 16)
    part = Out(dev, 2 * B * nblk * Cout)
    a.partial = N.ptr(part.t).value
    am, slots = None, lib.p2l_conv_amax_slots(C.byref(d))
    amp = None
    if c['amax_out']:
        assert slots > 0
        am = Out(dev, B * slots)
        a.amax.out = N.ptr(am.t).value
        if c['pool_sum']:                          # (dx is the pooled output: its maxima go to outp)
            amp = Out(dev, B * slots)
            a.amax.outp = N.ptr(amp.t).value
    dx = Out(dev, B * Ho * Wo * (Cout + 4))
    xd = _pitched(i['x'], d.x_ld, dev)
    assert lib.p2l_conv_workspace_bytes(C.byref(d)) == 0

    def call():
        return lib.p2l_conv_dgrad_arb(C.byref(d), C.byref(a), N.ptr(xd), N.ptr(wp), N.ptr(dx.t), N.stream())
    got = _Got()
    got.B, got.slots = B, slots
    got.rc, got.ratio, got.exec_flops, got.count, got.fam = _profiled(N, call)
    got.outs = [dx, ds, dt, part]
    part.cpu()
    full = dx.cpu(B, Ho, Wo, Cout + 4)
    got.dx = full[..., :Cout].contiguous()
    rows = [o.cpu(B, Cout + 4) for o in (ds, dt)]
    if got.rc == 0:
        assert is_sentinel(full[..., Cout:]) and all(is_sentinel(r[:, Cout:]) for r in rows), 'gap columns written'
    got.ds, got.dt = rows[0][:, :Cout].contiguous(), rows[1][:, :Cout].contiguous()
    got.amax = am.cpu(B, -1) if am is not None else None
    got.amaxp = amp.cpu(B, -1) if amp is not None else None
    return got


def _arb_held(got, pos, c, i, ip, route, cid):
    cr = dict(c, route=route)
    kfn = lambda cc, r=None, pooled=False: R.thin_k(cc, route, pooled)
    r64, r32 = R.thin_arb_refs(cr, i)
    kdx, kds, kdt = R.arb_k(cr, kfn)
    hold('p2l_conv_dgrad_arb:dx', cid, got.dx, r64['dx'], r64['den_dx'], r32['dx'], kdx)
    # ds, dt: on these signed operands inside the a-priori bound; held to their bar on the positive ones
    for name, bound in zip(('ds', 'dt'), R.arb_bound(cr, r64, i['ax'], kfn)):
        err = (getattr(got, name).to(D64) - r64[name]).abs()
        assert bool((err <= bound * R.U).all()), (cid, name)
    p64, p32 = R.thin_arb_refs(cr, ip)
    for name, k in (('ds', kds), ('dt', kdt)):
        hold('p2l_conv_dgrad_arb:%s' % name, cid, getattr(pos, name), p64[name], p64['den_' + name], p32[name], k)
    return r64


@pytest.mark.parametrize('case', R.THIN_ARB_CASES, ids=R.thin_arb_id)
@seeded
def test_dgrad_fused_affine_relu_bwd(dev, N, case):
    cid = R.thin_arb_id(case)
    i = R.thin_arb_inputs(_gen('tarb', cid), case)
    ip = R.arb_positive(i)
    got, pos = _arb(dev, N, case, i), _arb(dev, N, case, ip)
    for g_ in (got, pos):
        _on_route(g_, case, case['route'], cid)
    r64 = _arb_held(got, pos, case, i, ip, case['route'], cid)
    if case['route'] == 'TI':
        twin, tpos = _arb(dev, N, case, i, route='B'), _arb(dev, N, case, ip, route='B')
        for g_ in (twin, tpos):
            _on_route(g_, case, 'B', cid + ' on B')
        _arb_held(twin, tpos, case, i, ip, 'B', cid + ' on B')
    f = _arb(dev, N, case, i, route='F')
    _on_route(f, case, 'F', cid + ' on F')
    note('p2l_conv_dgrad_arb:dx', cid + ' on F', f.dx, r64['dx'], r64['den_dx'])
    _same_bits(_arb(dev, N, case, i), got, ('dx', 'ds', 'dt'), cid)
    if not case['nomask']:
        # the dead unit: channel 5 has no live pixel -- g = 0 there, ds = dt = +0
        assert bool((r64['g'][..., 5] == 0).all())
        assert bool((got.ds[:, 5] == 0).all()) and bool((got.dt[:, 5] == 0).all())
        if not case['skip']:
            dead = r64['g'] == 0                                           # (no shortcut: dx = g s, +-0 where masked)
            assert bool((got.dx[dead] == 0).all())
    if case['route'] == 'TI':
        assert got.slots == (case['H'] // 8) * (case['W'] // 16) * 4
    if got.amax is not None:
        # every slot is written; under pool_sum dx is the pooled output and its maxima are outp's
        assert bool((_bits(got.amax) != SENT).all()) and bool((got.amax >= 0).all())
        where = got.amaxp if case['pool_sum'] else got.amax
        assert bool((_bits(where) != SENT).all()) and bool((where >= 0).all())
        assert torch.equal(where.amax(dim=1), got.dx.abs().amax(dim=(1, 2, 3)))


# =====================================================================================================================
# arguments
# =====================================================================================================================
_TI = R._tsh('TI', 'i16x32', pro=R.PRO_AFFINE, pro_b=1, bias=True, act=R.ACT_RELU, pool=R.POOL_MAX, mask=True, res='same')
_TO = R._tsh('TO', 'o16x32', n_store=16, pro=R.PRO_AFFINE_RELU, pro_b=1, bias=True, act=R.ACT_TANH)
FWD_ARGS = [
    ('w_floats-of-bf3-TI', _TI, 'w_floats'), ('w_floats-of-bf3-TO', _TO, 'w_floats'),
    ('x_ld-unaligned-TI', _TI, _set(x_ld=22)), ('x_ld-unaligned-TO', _TO, _set(x_ld=54)),
    ('x_ld-short-TO', _TO, _set(x_ld=44)),
    ('n_store-unaligned-TI', _TI, _set(n_store=34)), ('n_store-unaligned-TO', _TO, _set(n_store=14)),
    ('n_store-above-Cout-TO', _TO, _set(n_store=36, y_ld=40)),
    ('y_ld-short-TI', _TI, _set(y_ld=60)), ('y_ld-short-TO', _TO, _set(y_ld=12)), ('y_ld-unaligned-TO', _TO, _set(y_ld=18)),
    ('yp_ld-short-TI', _TI, _set(yp_ld=60)), ('res_ld-short-TI', _TI, _set(res_ld=60)),
    ('mask_ld-short-TI', _TI, _set(mask_ld=60)),
    ('pro_bstride-short-TI', _TI, _set(pro_bstride=12)), ('pro_bstride-short-TO', _TO, _set(pro_bstride=44)),
    ('pro_bstride-unaligned-TO', _TO, _set(pro_bstride=50)),
]


@pytest.mark.parametrize('what,case,tamper', FWD_ARGS, ids=[a[0] for a in FWD_ARGS])
def test_forward_arguments_are_refused_before_the_launch(dev, N, what, case, tamper):
    """P2L_EINVAL, nothing is launched, every output still holds sentinels; the same launch without the fault is a
    good one on the thin kernel"""
    lib = N.lib()
    i = R.thin_inputs(_gen('targs', what), case)
    if tamper == 'w_floats':                   # the size of a P2L_WFMT_BF16X3 buffer: packed for something else
        tamper = _set(w_floats=lib.p2l_packed_weight_floats(9, case['Cout'], case['Cin'], R.WFMT_BF16X3))
    got = _fwd(dev, N, case, i, tamper=tamper)
    assert got.rc == EINVAL, (what, got.rc)
    assert got.count == (0, 0) and _untouched(got)
    ok = _fwd(dev, N, case, i)
    _on_route(ok, case, case['route'], what)


def test_the_packer_refuses_what_no_thin_mode_takes(dev, N):
    """p2l_pack_conv_weight_bf3t: more than three real channels on the thin side, and padded shapes neither mode
    admits -> P2L_EINVAL, and nothing of the thin image is written; three real channels pack"""
    lib = N.lib()
    g = _gen('pack')
    for O, I, n_pad, k_pad, flip, want in ((64, 4, 64, 16, 0, EINVAL), (4, 32, 32, 32, 0, EINVAL),
                                           (4, 64, 64, 16, 1, EINVAL), (32, 4, 32, 32, 1, EINVAL),
                                           (3, 3, 32, 16, 0, EINVAL), (64, 32, 64, 32, 0, EINVAL),
                                           (3, 16, 32, 16, 0, EINVAL), (64, 3, 64, 16, 0, 0), (3, 32, 32, 32, 0, 0),
                                           (3, 64, 64, 16, 1, 0), (32, 3, 32, 32, 1, 0)):
        src = randn(g, O, I, 3, 3).to(dev)
        n = lib.p2l_packed_weight_floats(9, n_pad, k_pad, R.WFMT_BF16X3T)
        head = lib.p2l_packed_weight_floats(9, n_pad, k_pad, R.WFMT_BF16X3)
        dst = Out(dev, n)
        rc = lib.p2l_pack_conv_weight_bf3t(N.ptr(src), O, I, n_pad, k_pad, flip, N.ptr(dst.t), N.stream())
        assert rc == want, (O, I, n_pad, k_pad, flip, rc)
        tail = dst.cpu()[head:]
        assert tail.numel() == (n_pad + k_pad) * 48
        written = (k_pad if n_pad == 32 and k_pad > 16 else n_pad) * 48        # [K_pad / 16 | 2 N_pad / 32] groups x 768
        assert is_sentinel(tail) if want else (bool((_bits(tail[:written]) != SENT).all()) and is_sentinel(tail[written:]))

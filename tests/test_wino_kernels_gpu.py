"""The Winograd F(2x2, 3x3) routes of a taps = 9, ups = 0, P2L_WFMT_BF16X3W launch (csrc/p2l_wino.hip) -- W8:
wino_conv_kernel (8x16-pixel blocks, bf16 x 3), forced with P2L_FORM_WINO_8X16 and by the dispatch's own choice where
H % 16 != 0; W16: wino16s_conv_kernel (16x16, bf16 x 3: P2L_FORM_WINO_BF3); H: the same kernel in fp16 x 2, both block
shapes, maxima from the pass in front, handed over, handed over with in_applied; HS: its K-sliced small-grid form with
conv_splitk_finish4 -- forward and fused input gradient, against the float64 references of tests/_small_refs.py,
through ctypes, with the harness, the metric and the bars of tests/test_small_kernels_gpu.py (tests/_pin.py):

    p2l_conv_fwd, p2l_conv_fwd_ex, p2l_conv_dgrad_arb, p2l_conv_dgrad_arb_ws, p2l_pack_conv_weight_bf3w,
    p2l_pack_conv_weight_bf3, p2l_packed_weight_floats, p2l_conv_amax_slots, p2l_wino_split_factor,
    p2l_conv_suggest_splitk.

Every case proves its route under the launch profiler: one 3x3 launch, 6 or 3 MFMA products per fp32 product, the
family P2L_PROF_FAM_WINO_H2 for H and HS, and exec_flops = 16 / 36 of the padded direct count ("16 products per 2x2
quad"), which is what tells W8 and W16 from the direct bf16 x 3 kernel; a case the dispatch moves elsewhere fails.
(The profiler does not tell W8 from W16 nor the two blocks of H: the form bits do, and the contract that they give the
same bits is tested here.)  Rounded outputs are held to |got - r64| / den_w <= min(k, 4 x the route's fp32
restatement) x 2^-24 with den_w = |A^T| (|U| (.) |B^T| |a| |B|) |A| (H, HS: plus wino_h2_floor) and k counted in
_small_refs.wino_k; the figure against the direct denominator den_d = sum |a| |w| is recorded next to it, and so is
the figure of the same inputs on the exact-fp32 direct kernel (P2L_WFMT_F32), which is held to its own counted k.
What the contract calls exact is compared bit for bit; so are one-hot power-of-two inputs, tap by tap.  Every output
sits between guard bands, every pitch is above its row with junk (inputs) or sentinels (outputs) in the gap.
P2L_WINO_ERR_FILE=<path> records the figures (profiles/wino_kernels_err.txt).  The cases, their inputs and k live in
tests/_small_refs.py; tests/test_small_refs.py holds them to "the restatement is within k / 4" on the host."""
import ctypes as C

import pytest
import torch

import _small_refs as R
from _pin import (D64, G, N, SENT, Out, _gen, _record_file, hold, hold_k, is_sentinel, note, randn,  # noqa: F401
                  seeded)
from _small_refs import _cancellation_case

pytestmark = pytest.mark.gpu
EINVAL, EWS = -1, -3
FAM_OTHER, FAM_WINO_H2, FAM_DIRECT_H2 = 0, 1, 2
PRODUCTS = {'W8': 6.0, 'W16': 6.0, 'H': 3.0, 'HS': 3.0, 'F': 16.0}


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
    """one 3x3 launch, the route's products per fp32 product, its family, and the Winograd count of executed
    products: 16 per 2x2 quad and (cin, cout) pair where the direct kernels make 36"""
    direct = 2.0 * got.B * c['H'] * c['W'] * c['Cin'] * c['Cout'] * 9
    assert got.rc == 0, (what, got.rc)
    assert got.count == (1, 0), (what, got.count)
    assert abs(got.ratio - PRODUCTS[route]) < 1e-6, '%s: expected route %s, got %g products' % (what, route, got.ratio)
    fam = FAM_WINO_H2 if route in ('H', 'HS') else FAM_OTHER
    assert got.fam[fam] == 1 and sum(got.fam) == 1, (what, got.fam)
    want = direct if route == 'F' else direct * 16.0 / 36.0
    assert abs(got.exec_flops - want) <= 1e-9 * want, (what, route, got.exec_flops, want)


def _weights(dev, N, i, c, route, flip=False):
    """the packed buffer of the case's weight for the route's format; flip: through the transpose_flip copy, from the
    OIHW tensor of the forward conv whose input gradient the launch applies"""
    wfmt = 0 if route == 'F' else R.WFMT_BF16X3W
    cache = i.setdefault('_packed', {})
    key = (id(i['w']), wfmt, flip)                 # (a copy of i with another weight shares the dict, not the entry)
    if key not in cache:
        src = i['w'].permute(1, 0, 2, 3).flip(2, 3).contiguous() if flip else i['w']
        cache[key] = (i['w'], N.pack_conv_weight(src.to(dev), 9, c['Cout'], c['Cin'], flip, wfmt))
    return cache[key][1]


def _desc(N, c, route, B):
    d = N.P2LConv()
    d.B, d.H, d.W, d.Cin, d.Cout, d.taps, d.ups = B, c['H'], c['W'], c['Cin'], c['Cout'], 9, 0
    d.x_ld, d.alpha = c['Cin'] + 4, c['alpha']
    d.wfmt = 0 if route == 'F' else R.WFMT_BF16X3W
    d.form = 0 if route == 'F' else R.wino_form(c, route)
    d.splitk = c['splitk'] if route == 'HS' else 1
    return d


def _fwd(dev, N, c, i, route=None, sl=None, handed='case', want_amax=False, next_st=None, tamper=None, ws_short=0,
         flip=False, ex_tamper=None):
    """one forward launch of case c on inputs i (images sl) on `route` (default: the case's) -> _Got: rc, y [B, H, W,
    n_store], yp, the profiler's figures, the maxima slots.  Everything the launch may write is an Out; the gap
    columns are checked here."""
    lib = N.lib()
    route = route or c['route']
    sl = slice(0, c['B']) if sl is None else sl
    B, H, W, Cin, Cout, ns = sl.stop - sl.start, c['H'], c['W'], c['Cin'], c['Cout'], c['n_store']
    wp = _weights(dev, N, i, c, route, flip)
    d = _desc(N, c, route, B)
    d.pro, d.act, d.pool = c['pro'], c['act'], c['pool']
    d.y_ld = d.yp_ld = ns + 4
    d.n_store, d.res_ups, d.w_floats = ns, int(c['res'] == 'ups'), wp.numel()
    xd = _pitched(i['x'][sl], Cin + 4, dev)
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
    y = Out(dev, B * H * W * (ns + 4)) if c['want_y'] else None
    yp = Out(dev, B * (H // 2) * (W // 2) * (ns + 4)) if c['pool'] != R.POOL_NONE else None
    biasd = i['bias'].to(dev) if c['bias'] else None
    h2 = route in ('H', 'HS')
    hand = (R.pw_amax(c, i)[0] if c['amax'] and h2 else None) if isinstance(handed, str) else handed
    ex = None
    if c['oscale'] or c['noise'] or hand is not None or want_amax:
        ex = N.P2LConvExtra()
        if c['oscale']:
            ex.oscale, ex.oscale_bstride = N.ptr(_pitched(i['oscale'][sl], Cout + 4, dev, 2.0)).value, Cout + 4
        if c['noise']:
            ex.noise, ex.noise_w = N.ptr(i['noise'][sl].contiguous().to(dev)).value, i['noise_w']
        if hand is not None:                      # three partial maxima per image, the maximum in the middle one
            part = (hand[sl].view(B, 1) * torch.tensor([0.5, 1.0, 0.25])).contiguous()
            ex.amax.in_, ex.amax.in_n = N.ptr(part.to(dev)).value, 3
            ex.amax.in_applied = int(c['amax'] == 'applied' and isinstance(handed, str))
    if tamper is not None:
        tamper(d)
    slots = lib.p2l_conv_amax_slots(C.byref(d)) if want_amax else 0
    am = amp = None
    if want_amax and slots > 0:
        am = Out(dev, B * slots)
        ex.amax.out = N.ptr(am.t).value
        if yp is not None:
            amp = Out(dev, B * slots)
            ex.amax.outp = N.ptr(amp.t).value
        if next_st is not None:
            ex.amax.next_s, ex.amax.next_t = N.ptr(next_st[0].to(dev)).value, N.ptr(next_st[1].to(dev)).value
            ex.amax.next_bstride = next_st[0].shape[1]
    if ex_tamper is not None:
        ex_tamper(ex)
    need = lib.p2l_conv_workspace_bytes(C.byref(d))
    assert (need > 0) == h2, (route, need)        # (only the fp16 x 2 routes ask for one)
    ws = Out(dev, max((need - ws_short) // 4, 1)) if need else None
    wsp, wsb = (N.ptr(ws.t), C.c_size_t(ws.n * 4)) if ws is not None else (None, C.c_size_t(0))

    def call():
        args = (N.ptr(xd), N.ptr(wp), N.ptr(biasd), N.ptr(sd), N.ptr(td), N.ptr(resd), N.ptr(maskd),
                N.ptr(y.t) if y else None, N.ptr(yp.t) if yp else None, wsp, wsb, N.stream())
        if ex is None:
            return lib.p2l_conv_fwd(C.byref(d), *args)
        return lib.p2l_conv_fwd_ex(C.byref(d), C.byref(ex), *args)
    got = _Got()
    got.B = B
    got.rc, got.ratio, got.exec_flops, got.count, got.fam = _profiled(N, call)
    got.ex, got.slots, got.outs = ex is not None, slots, [o for o in (y, yp, am, amp) if o is not None]
    got.y = got.yp = got.amax = got.amaxp = None
    if ws is not None:
        ws.cpu()                                                        # (its guard bands)
    if y is not None:
        full = y.cpu(B, H, W, ns + 4)
        assert got.rc != 0 or is_sentinel(full[..., ns:]), 'gap columns of y written'
        got.y = full[..., :ns].contiguous()
    if yp is not None:
        full = yp.cpu(B, H // 2, W // 2, ns + 4)
        assert got.rc != 0 or is_sentinel(full[..., ns:]), 'gap columns of yp written'
        got.yp = full[..., :ns].contiguous()
    if am is not None:
        got.amax = am.cpu(B, slots)
    if amp is not None:
        got.amaxp = amp.cpu(B, slots)
    return got


def _untouched(got):
    return all(is_sentinel(o.cpu()) for o in got.outs)


def _entry(got):
    return 'p2l_conv_fwd_ex' if got.ex else 'p2l_conv_fwd'


def _same_bits(a, b, names, what=''):
    for name in names:
        u, v = getattr(a, name), getattr(b, name)
        assert (u is None) == (v is None), (what, name)
        if u is not None:
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), (what, name, int((u != v).sum()))


# =====================================================================================================================
# forward: every route, every epilogue
# =====================================================================================================================
@pytest.mark.parametrize('case', R.WINO_FWD_CASES, ids=R.wino_id)
@seeded
def test_forward(dev, N, case):
    cid = R.wino_id(case)
    i = R.wino_inputs(_gen('wino', cid), case)
    got = _fwd(dev, N, case, i)
    _on_route(got, case, case['route'], cid)
    r64, r32 = R.wino_refs(case, i)
    for name in ('y', 'yp'):
        if getattr(got, name) is not None:
            den = 'den' if name == 'y' else 'denp'
            hold('%s:%s' % (_entry(got), name), cid, getattr(got, name), r64[name], r64[den], r32[name],
                 R.wino_k(case, pooled=name == 'yp'))
            # "agrees to fp32 rounding": the same error on the direct kernels' denominator, recorded
            note('%s:%s / den_d' % (_entry(got), name), cid, getattr(got, name), r64[name], r64[den + '_d'])
    # the same inputs on the exact-fp32 direct kernel, held to its own counted k on its own denominator
    twin = _fwd(dev, N, case, i, route='F')
    _on_route(twin, case, 'F', cid + ' on F')
    f64, _ = R.wino_refs(case, i, 'F')
    for name in ('y', 'yp'):
        if getattr(twin, name) is not None:
            hold_k('%s:%s / den_d' % (_entry(twin), name), cid + ' on F', getattr(twin, name), f64[name],
                   f64['den_d' if name == 'y' else 'denp_d'], R.wino_k(case, 'F', name == 'yp'))
    # exact: a repeated launch; a masked element is +0; yp is the pool of the y this launch stored
    _same_bits(_fwd(dev, N, case, i), got, ('y', 'yp'), cid)
    if case['mask'] and got.y is not None:
        dead = ~(i['mask'][..., :case['n_store']] > 0)
        assert bool(dead.any()) and bool((got.y.view(torch.int32)[dead] == 0).all())
    if got.y is not None and got.yp is not None:
        v0, v1, v2, v3 = R.quads(got.y)
        want = torch.maximum(torch.maximum(v0, v1), torch.maximum(v2, v3)) if case['pool'] == R.POOL_MAX \
            else (v0 + v1) + (v2 + v3)
        assert torch.equal(got.yp, want)
    if case['route'] in ('H', 'HS') and case['B'] >= 3 and not (case['bias'] or case['res'] or case['noise']) \
            and got.y is not None and case['pro'] == R.PRO_NONE:
        assert bool((got.y[1] == 0).all())                              # the all-zero image


def test_slice_counts_of_the_small_grid_shapes(dev, N):
    """16^2 256 -> 512 runs in 2 slices, 32 x 16 512 -> 256 in 4: p2l_wino_split_factor and, for any batch,
    p2l_conv_suggest_splitk"""
    lib = N.lib()
    for name, sk in (('hs2', 2), ('hs4', 4)):
        c = R._wsh('HS', name, splitk=sk)
        assert lib.p2l_wino_split_factor(c['H'], c['W'], c['Cin'], c['Cout']) == sk
        for B in (1, 18):
            d = _desc(N, c, 'HS', B)
            d.y_ld = d.n_store = c['Cout']
            assert lib.p2l_conv_suggest_splitk(C.byref(d)) == sk, (name, B)
    for name in ('16x16', '16x32', '32x16', '32x32', '24x16', '8x16'):
        c = R._wsh('W16', name)
        assert lib.p2l_wino_split_factor(c['H'], c['W'], c['Cin'], c['Cout']) == 1, name


# =====================================================================================================================
# exact inputs: tap, channel and frequency placement bit for bit
# =====================================================================================================================
@pytest.mark.parametrize('flip', [False, True], ids=['forward', 'transpose_flip'])
@pytest.mark.parametrize('tap', range(9))
def test_one_hot_inputs_are_exact(dev, N, tap, flip):
    """single power-of-two pixels at corners, edges, block seams and the interior, single power-of-two weights on one
    tap: every route gives the fp64 result bit for bit -- also through the transpose_flip copy of the packer"""
    for route, kw in (('W8', {}), ('W16', {}), ('H', dict(blk=8)), ('H', dict(blk=16))):
        c = R._wsh(route, '16x32', **kw)
        for seed in range(2):
            i = R.wino_onehot(c, tap, seed)
            got = _fwd(dev, N, c, i, flip=flip)
            _on_route(got, c, route)
            want = R.conv3x3(i['x'].double(), i['w'].double())['y']
            assert int((want != 0).sum()) >= 3
            assert torch.equal(got.y.double(), want), (route, kw, seed, int((got.y.double() != want).sum()))


def test_all_zero_inputs_give_exactly_zero(dev, N):
    for route, name, kw in (('W8', '16x16', {}), ('W16', '16x16', {}), ('H', '16x16', {}), ('HS', 'hs2', dict(splitk=2))):
        c = R._wsh(route, name, **kw)
        i = dict(x=torch.zeros(c['B'], c['H'], c['W'], c['Cin']), w=randn(_gen('zero', route), c['Cout'], c['Cin'], 3, 3))
        got = _fwd(dev, N, c, i)
        _on_route(got, c, route)
        assert bool((got.y.view(torch.int32) == 0).all()), route


@pytest.mark.parametrize('N_pad,K_pad,flip', [(64, 16, 0), (128, 48, 0), (64, 48, 1)])
def test_packed_buffer_is_what_the_header_says(dev, N, N_pad, K_pad, flip):
    """the leading image of a _bf3w buffer is the _bf3 buffer, the fp16 x 2 Winograd image ends in the bits of max |w|
    and three zero words, and p2l_packed_weight_floats is the sum of the documented pieces: 9 N K 3 / 2 (bf16 x 3) +
    16 frequencies x 6 B (Winograd, three pieces) + 16 x 4 B + 4 (Winograd, two pieces + tail) + 9 x 4 B + 4 (the
    direct fp16 x 2 image + tail)"""
    lib = N.lib()
    O, I = (K_pad, N_pad) if flip else (N_pad, K_pad)
    w = randn(_gen('packw', N_pad, K_pad), O, I, 3, 3) / 5
    wd = w.to(dev)
    nk = N_pad * K_pad
    n = lib.p2l_packed_weight_floats(9, N_pad, K_pad, R.WFMT_BF16X3W)
    assert n == nk * 27 // 2 + nk * 24 + (nk * 16 + 4) + (nk * 9 + 4)
    n3 = lib.p2l_packed_weight_floats(9, N_pad, K_pad, 1)
    assert n3 == nk * 27 // 2
    full, lead = Out(dev, n), Out(dev, n3)
    N.check(lib.p2l_pack_conv_weight_bf3w(N.ptr(wd), O, I, 9, N_pad, K_pad, flip, N.ptr(full.t), N.stream()), 'bf3w')
    N.check(lib.p2l_pack_conv_weight_bf3(N.ptr(wd), O, I, 9, N_pad, K_pad, flip, N.ptr(lead.t), N.stream()), 'bf3')
    words = full.cpu().view(torch.int32)
    assert torch.equal(words[:n3], lead.cpu().view(torch.int32))
    wmax = w.abs().max().view(torch.int32).item()
    end = n3 + nk * 24 + nk * 16 + 4                                         # (the tail of the Winograd fp16 x 2 image)
    assert words[end - 4:end].tolist() == [wmax, 0, 0, 0]


# =====================================================================================================================
# bit-exact contracts
# =====================================================================================================================
W16_CASES = [c for c in R.WINO_FWD_CASES if c['route'] == 'W16']
H_CASES = [c for c in R.WINO_FWD_CASES if c['route'] == 'H']


@pytest.mark.parametrize('case', W16_CASES, ids=R.wino_id)
def test_the_8x16_and_16x16_kernels_agree_bit_for_bit(dev, N, case):
    i = R.wino_inputs(_gen('w8w16', R.wino_id(case)), case)
    a, b = _fwd(dev, N, case, i, route='W8'), _fwd(dev, N, case, i, route='W16')
    _on_route(a, case, 'W8')
    _on_route(b, case, 'W16')
    _same_bits(a, b, ('y', 'yp'))


@pytest.mark.parametrize('case', H_CASES, ids=R.wino_id)
def test_the_two_blocks_of_the_fp16_kernel_agree_bit_for_bit(dev, N, case):
    """y, yp and every maxima slot"""
    i = R.wino_inputs(_gen('blocks', R.wino_id(case)), case)
    a, b = [_fwd(dev, N, dict(case, blk=blk), i, want_amax=True) for blk in (8, 16)]
    for got in (a, b):
        _on_route(got, case, 'H')
    assert a.slots == b.slots == (case['H'] // 16) * (case['W'] // 16) * (case['Cout'] // 64) * 8
    _same_bits(a, b, ('y', 'yp', 'amax', 'amaxp'))


ALONE = [R._wsh('W8', '16x32', **R.EPI[0]), R._wsh('W8', '24x16', own=True, **R.EPI[3]),
         R._wsh('W16', '16x32', **R.EPI[1]), R._wsh('H', '16x32', blk=8, **R.EPI[2]),
         R._wsh('H', '16x32', blk=16, amax='raw', **R.EPI[3]), R._wsh('HS', 'hs2', splitk=2, **R.EPI[0]),
         R._wc('HS', (16, 16), 3, 256, 512, splitk=2, amax='applied', pro=R.PRO_AFFINE_RELU, pool=R.POOL_SUM)]


@pytest.mark.parametrize('case', ALONE, ids=R.wino_id)
def test_an_image_alone_has_the_bits_it_has_in_any_batch(dev, N, case):
    i = R.wino_inputs(_gen('alone', R.wino_id(case)), case)
    whole = _fwd(dev, N, case, i)
    _on_route(whole, case, case['route'])
    for b in sorted(set([0, case['B'] // 2, case['B'] - 1])):
        one = _fwd(dev, N, case, i, sl=slice(b, b + 1))
        _on_route(one, case, case['route'])
        for name in ('y', 'yp'):
            if getattr(whole, name) is not None:
                assert torch.equal(getattr(one, name)[0].view(torch.int32), getattr(whole, name)[b].view(torch.int32)), \
                    (name, b)


@pytest.mark.parametrize('case', [R._wsh('H', '16x32', blk=8, bias=True), R._wsh('H', '32x32', blk=16, act=R.ACT_RELU),
                                  R._wsh('HS', 'hs2', splitk=2, bias=True)], ids=R.wino_id)
def test_handed_true_maxima_equal_the_pass_in_front(dev, N, case):
    """a consumer without a prologue: the same bits with handed-over maxima as with its own max-|x| pass"""
    i = R.wino_inputs(_gen('handed', R.wino_id(case)), case)
    own = _fwd(dev, N, case, i)
    handed = _fwd(dev, N, case, i, handed=i['x'].abs().amax(dim=(1, 2, 3)))
    for got in (own, handed):
        _on_route(got, case, case['route'])
    _same_bits(own, handed, ('y', 'yp'))


AMAX_CASES = [R._wsh('W16', '16x32', act=R.ACT_RELU, pool=R.POOL_MAX), R._wsh('W16', '32x32', bias=True, n_store=36),
              R._wsh('H', '16x32', blk=8, bias=True, pool=R.POOL_SUM), R._wsh('H', '32x16', blk=16, act=R.ACT_TANH),
              R._wsh('HS', 'hs2', splitk=2, bias=True, pool=R.POOL_MAX), R._wsh('HS', 'hs4', splitk=4, n_store=100)]


@pytest.mark.parametrize('nxt', [False, True], ids=['plain', 'next-affine'])
@pytest.mark.parametrize('case', AMAX_CASES, ids=R.wino_id)
def test_the_maxima_slots_hold_the_maximum_of_what_was_stored(dev, N, case, nxt):
    """the per-image maximum over the p2l_conv_amax_slots(d) slots == max |y| of the y the launch stored (outp: of
    yp); with next_s / next_t == max |fma(y, s, t)|.  The slot buffers are exactly that long, between guard bands:
    no slot beyond the promised ones is written"""
    g = _gen('amax', R.wino_id(case))
    i = R.wino_inputs(g, case)
    B, ns = case['B'], case['n_store']
    st = (0.5 + torch.rand(B, ns, generator=g), randn(g, B, ns) * R.mags(B).view(B, 1)) if nxt else None
    got = _fwd(dev, N, case, i, want_amax=True, next_st=st)
    _on_route(got, case, case['route'])
    if case['route'] == 'HS':
        assert got.slots == (case['H'] // 2) * (case['W'] // 2) * (ns // 4) // 64
    else:
        assert got.slots == (case['H'] // 16) * (case['W'] // 16) * (case['Cout'] // 64) * 8
    assert bool((got.amax.view(torch.int32) != SENT).all()) and bool((got.amax >= 0).all())
    if nxt:
        assert torch.equal(got.amax.amax(dim=1), R.producer_amax(got.y, *st))
    else:
        assert torch.equal(got.amax.amax(dim=1), R.producer_amax(got.y))
    if got.amaxp is not None:
        assert bool((got.amaxp.view(torch.int32) != SENT).all())
        assert torch.equal(got.amaxp.amax(dim=1), R.producer_amax(got.yp))


def test_the_8x16_kernel_promises_and_writes_no_maxima(dev, N):
    """the header: the 8x16 Winograd kernel writes none -- p2l_conv_amax_slots is 0 and the fields are ignored"""
    for case in (R._wsh('W8', '16x16', bias=True), R._wsh('W8', '24x16', own=True)):
        got = _fwd(dev, N, case, R.wino_inputs(_gen('w8amax'), case), want_amax=True)
        _on_route(got, case, 'W8')
        assert got.slots == 0 and got.amax is None


@pytest.mark.parametrize('pro', [R.PRO_NONE, R.PRO_AFFINE], ids=['plain', 'prologue-applied'])
@pytest.mark.parametrize('blk', [8, 16])
def test_the_scales_leave_the_transform_its_factor_four(dev, N, blk, pro):
    """every image's maximum is nextafter(2^e, 0), in the +, -, -, + pattern that drives B^T d B to 4 max; once with a
    prologue (s = 1, t = 0 on that channel, maxima handed over with in_applied), where the factor 1.001 carries the
    maximum over the binade: finite and within the bar"""
    case = R._wsh('H', '16x16', blk=blk, pro=pro, amax='applied' if pro else None)

    @seeded
    def body():
        i = R.wino_inputs(_gen('headroom', blk, pro), case)
        for b in range(case['B']):
            if pro:
                i['s'][b, 3], i['t'][b, 3] = 1.0, 0.0
            a, _ = R.pw_prologue(i['x'], pro, i.get('s'), i.get('t'))
            e = torch.ceil(torch.log2(a[b].abs().max())) + 1
            m = (2.0 ** e).float().nextafter(torch.tensor(0.0))
            i['x'][b, 5, 5, 3], i['x'][b, 5, 7, 3], i['x'][b, 7, 5, 3], i['x'][b, 7, 7, 3] = m, -m, -m, m
        true = R.pw_prologue(i['x'], pro, i.get('s'), i.get('t'))[0].abs().amax(dim=(1, 2, 3))
        crossed = R.pw_amax(case, i)[1].double().log2().floor() > true.double().log2().floor()
        assert bool(crossed.all()) == bool(pro) and bool(crossed.any()) == bool(pro)
        got = _fwd(dev, N, case, i)
        _on_route(got, case, 'H')
        assert bool(torch.isfinite(got.y).all())
        r64, r32 = R.wino_refs(case, i)
        hold('%s:y' % _entry(got), 'headroom-' + R.wino_id(case), got.y, r64['y'], r64['den'], r32['y'], R.wino_k(case))
    body()


# =====================================================================================================================
# fused input gradient
# =====================================================================================================================
def _arb(dev, N, c, i, route=None, tamper=None, ax=None, a_s=None, a_t=None):
    """one p2l_conv_dgrad_arb(_ws) launch of case c -> _Got: rc, dx, ds, dt and the profiler's figures"""
    lib = N.lib()
    route = route or c['route']
    B, H, W, Cin, Cout = c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    Ho, Wo = (H // 2, W // 2) if c['pool_sum'] else (H, W)
    wp = _weights(dev, N, i, c, route)
    d = _desc(N, c, route, B)
    d.alpha, d.y_ld, d.yp_ld, d.n_store, d.w_floats = 1.0, Cout + 4, Cout + 4, Cout, wp.numel()
    d.pool = R.POOL_SUM if c['pool_sum'] else R.POOL_NONE
    a = N.P2LArb()
    ax = i['ax'] if ax is None else ax
    a.x, a.x_ld = N.ptr(_pitched(ax, Cout + 8, dev)).value, Cout + 8
    a.s = N.ptr(_pitched(i['as'] if a_s is None else a_s, Cout + 4, dev, -5.0)).value
    a.t = N.ptr(_pitched(i['at'] if a_t is None else a_t, Cout + 4, dev, 9.0)).value
    a.st_bstride, a.nomask = Cout + 4, int(c['nomask'])
    if c['skip']:
        a.skip, a.skip_ld = N.ptr(_pitched(i['skip'], Cout + 12, dev, 3.0)).value, Cout + 12
        a.skip_C, a.skip_ups = Cout // 2, int(c['skip'] == 'ups')
    ds, dt = Out(dev, B * (Cout + 4)), Out(dev, B * (Cout + 4))
    a.ds, a.dt, a.dsdt_bstride = N.ptr(ds.t).value, N.ptr(dt.t).value, Cout + 4
    if tamper is not None:
        tamper(d, a)
    nblk = max(lib.p2l_conv_arb_nblk_ws(C.byref(d)), lib.p2l_conv_arb_nblk(C.byref(d)), 1)
    part = Out(dev, 2 * B * nblk * Cout)
    a.partial = N.ptr(part.t).value
    if c['amax'] and route in ('H', 'HS'):
        hand = (R.pw_amax(c, i)[0].view(B, 1) * torch.tensor([0.5, 1.0, 0.25])).contiguous()
        a.amax.in_, a.amax.in_n = N.ptr(hand.to(dev)).value, 3
    dx = Out(dev, B * Ho * Wo * (Cout + 4))
    xd = _pitched(i['x'], Cin + 4, dev)
    need = lib.p2l_conv_workspace_bytes(C.byref(d))
    assert (need > 0) == (route in ('H', 'HS')), (route, need)
    ws = Out(dev, need // 4) if need else None

    def call():
        if ws is None:
            return lib.p2l_conv_dgrad_arb(C.byref(d), C.byref(a), N.ptr(xd), N.ptr(wp), N.ptr(dx.t), N.stream())
        return lib.p2l_conv_dgrad_arb_ws(C.byref(d), C.byref(a), N.ptr(xd), N.ptr(wp), N.ptr(dx.t), N.ptr(ws.t),
                                         C.c_size_t(ws.n * 4), N.stream())
    got = _Got()
    got.B = B
    got.rc, got.ratio, got.exec_flops, got.count, got.fam = _profiled(N, call)
    got.entry = 'p2l_conv_dgrad_arb' if ws is None else 'p2l_conv_dgrad_arb_ws'
    got.outs = [dx, ds, dt, part]
    if ws is not None:
        ws.cpu()
    part.cpu()
    full = dx.cpu(B, Ho, Wo, Cout + 4)
    got.dx = full[..., :Cout].contiguous()
    rows = [o.cpu(B, Cout + 4) for o in (ds, dt)]
    if got.rc == 0:
        assert is_sentinel(full[..., Cout:]) and all(is_sentinel(r[:, Cout:]) for r in rows), 'gap columns written'
    got.ds, got.dt = rows[0][:, :Cout].contiguous(), rows[1][:, :Cout].contiguous()
    return got


@pytest.mark.parametrize('case', R.WINO_ARB_CASES, ids=R.wino_arb_id)
@seeded
def test_dgrad_fused_affine_relu_bwd(dev, N, case):
    cid = R.wino_arb_id(case)
    i = R.wino_arb_inputs(_gen('warb', cid), case)
    got = _arb(dev, N, case, i)
    _on_route(got, case, case['route'], cid)
    r64, r32 = R.wino_arb_refs(case, i)
    kdx, kds, kdt = R.arb_k(case, R.wino_k)
    hold('%s:dx' % got.entry, cid, got.dx, r64['dx'], r64['den_dx'], r32['dx'], kdx)
    note('%s:dx / den_d' % got.entry, cid, got.dx, r64['dx'], r64['den_dx_d'])
    # ds, dt: on these signed operands inside the a-priori bound; held to their bar on the positive ones
    for name, bound in zip(('ds', 'dt'), R.arb_bound(case, r64, i['ax'], R.wino_k)):
        err = (getattr(got, name).to(D64) - r64[name]).abs()
        print('%s %s: %.3f of the a-priori bound' % (cid, name, float((err / (bound * R.U).clamp_min(1e-300)).max())))
        assert bool((err <= bound * R.U).all()), name
    ip = R.arb_positive(i)
    pos = _arb(dev, N, case, ip)
    _on_route(pos, case, case['route'], cid)
    p64, p32 = R.wino_arb_refs(case, ip)
    for name, k in (('ds', kds), ('dt', kdt)):
        hold('%s:%s' % (got.entry, name), cid, getattr(pos, name), p64[name], p64['den_' + name], p32[name], k)
    _same_bits(_arb(dev, N, case, i), got, ('dx', 'ds', 'dt'), cid)
    if case['route'] == 'W16':                                         # W8 = W16: dx, ds, dt
        _same_bits(_arb(dev, N, case, i, route='W8'), got, ('dx', 'ds', 'dt'), cid + ' W8')
    if case['route'] == 'H':                                           # ... and the other block of the fp16 x 2 kernel
        _same_bits(_arb(dev, N, dict(case, blk=24 - case['blk']), i), got, ('dx', 'ds', 'dt'), cid + ' other block')
    if not case['nomask'] and not case['skip']:
        dead = r64['g'] == 0                                               # (no shortcut: dx = g s, +0 where masked)
        assert bool((got.dx[dead] == 0).all())


MASK_ROUTES = [('W8', 64, 64, {}), ('W16', 64, 64, {}), ('H', 64, 64, dict(blk=8)), ('H', 64, 64, dict(blk=16)),
               ('HS', 256, 512, dict(splitk=2))]


@pytest.mark.parametrize('route,Cin,Cc,kw', MASK_ROUTES, ids=lambda v: str(v))
def test_fused_backward_mask_is_the_forwards_decision(dev, N, route, Cin, Cc, kw):
    """{g != 0} of the fused dgrad epilogue (HS: of conv_splitk_finish4) -- read off dt with da = 1 through a weight
    that is the identity on its centre tap, and off dx -- == {a > 0} of the forward's PRO_AFFINE_RELU prologue in the
    exact-fp32 direct kernel (the Winograd transforms do not carry a 2^-120 next to a 1, so the decision cannot be read
    through them), on inputs where x s + t rounded once and
    rounded twice decide differently (_cancellation_case)"""
    Bn, H = 2, 16
    P = H * H
    nk = min(Cin, Cc)
    wf = torch.zeros(Cc, Cc, 3, 3)
    wf[:, :, 1, 1] = torch.eye(Cc)
    wa = torch.zeros(Cc, Cin, 3, 3)
    wa[:nk, :nk, 1, 1] = torch.eye(nk)
    fc = R._wc('W8', (H, H), Bn, Cc, Cc, pro=R.PRO_AFFINE_RELU)
    ac = R._wac(route, (H, H), Bn, Cin, Cc, **kw)
    for seed in range(3):
        x, s, t, once, twice, A, B = _cancellation_case(seed, Bn, P, Cc)
        fwd = _fwd(dev, N, fc, dict(x=x.view(Bn, H, H, Cc), w=wf, s=s, t=t), route='F')
        _on_route(fwd, fc, 'F')
        live = fwd.y.view(Bn, P, Cc) > 0
        i = dict(x=torch.ones(Bn, H, H, Cin), w=wa, ax=x.view(Bn, H, H, Cc), **{'as': s, 'at': t})
        got = _arb(dev, N, ac, i)
        _on_route(got, ac, route)
        bwd = got.dx.view(Bn, P, Cc) != 0
        diff = (live != bwd)[..., :nk]
        assert not bool(diff.any()), ('forward and backward decide differently', int(diff.sum()),
                                      int((diff & A[..., :nk]).sum()), int((diff & B[..., :nk]).sum()))
        assert torch.equal(got.dt[:, :nk], live.float().sum(1)[:, :nk])        # dt counts the live pixels (da = 1)
        assert bool((got.dx[..., nk:] == 0).all())


# =====================================================================================================================
# arguments
# =====================================================================================================================
@pytest.mark.parametrize('what', ['workspace', 'w_floats', 'next_bstride', 'next_bstride-sliced'])
def test_arguments_are_refused_before_the_launch(dev, N, what):
    """an HS launch whose workspace is one float short of its slices returns P2L_EWS, a w_floats below the format's size
    P2L_EINVAL, and so does a maxima producer whose reader's affine is pitched below the row it is read at
    (P2LAmax.next_bstride in 1 .. n_store - 1): nothing is launched, every output still holds sentinels"""
    lib = N.lib()
    c = R._wsh('HS', 'hs2', splitk=2, bias=True, pool=R.POOL_MAX)
    if what == 'next_bstride':
        c = R._wsh('W16', '16x32', bias=True)
    i = R.wino_inputs(_gen('wargs', what), c)
    if what.startswith('next_bstride'):
        g = _gen('wargs-st', what)
        st = (0.5 + torch.rand(c['B'], c['n_store'], generator=g), randn(g, c['B'], c['n_store']))
        got = _fwd(dev, N, c, i, want_amax=True, next_st=st,
                   ex_tamper=lambda ex: setattr(ex.amax, 'next_bstride', c['n_store'] - 4))
        want = EINVAL
    elif what == 'workspace':
        # (the slices' share, splitk B H W Cout floats, is what the launch cannot do without: see the next test)
        got, want = _fwd(dev, N, c, i, ws_short=c['B'] * 64 * 4 + 4, want_amax=True), EWS
    else:
        n = lib.p2l_packed_weight_floats(9, c['Cout'], c['Cin'], R.WFMT_BF16X3W)

        def tamper(d):
            d.w_floats = n - 1
        got, want = _fwd(dev, N, c, i, tamper=tamper, want_amax=True), EINVAL
    assert got.rc == want, (what, got.rc)
    assert got.count == (0, 0) and _untouched(got)
    ok = _fwd(dev, N, c, i, want_amax=True)                                  # ... and the launch itself is a good one
    _on_route(ok, c, c['route'])


def test_without_the_maxima_share_of_the_workspace_the_slices_run_in_bf16x3(dev, N):
    """the header: the fp16 x 2 form needs 256 B of workspace per image, "without it ... the launch keeps the bf16 x 3
    arithmetic" -- a K-sliced launch whose workspace is one float short of p2l_conv_workspace_bytes still holds its
    slices and runs the same Winograd kernel with six products, inside the workspace it was given (guard bands); its
    result is held to the counted k of that arithmetic"""
    c = R._wsh('HS', 'hs2', splitk=2, bias=True)
    i = R.wino_inputs(_gen('wsfall'), c)
    got = _fwd(dev, N, c, i, ws_short=4)
    want = 2.0 * c['B'] * c['H'] * c['W'] * c['Cin'] * c['Cout'] * 4
    assert got.rc == 0 and got.count == (1, 0) and abs(got.ratio - 6.0) < 1e-6
    assert got.fam[FAM_OTHER] == 1 and sum(got.fam) == 1 and abs(got.exec_flops - want) <= 1e-9 * want
    r64, _ = R.wino_refs(c, i, 'W16')                     # (den_w without the fp16 x 2 floor)
    k = R.wino_k(c, 'WS')                                  # (the bf16 x 3 arithmetic in two slices)
    err = (got.y.double() - r64['y']).abs() / r64['den'] / R.U
    print('sliced bf16 x 3: %.3f x 2^-24 (k = %d)' % (float(err.max()), k))
    assert float(err.max()) <= k


@seeded
def test_another_slice_count_runs_the_direct_kernel(dev, N):
    """the header: a small-grid layer takes the Winograd form IF splitk is exactly p2l_wino_split_factor -- with 4
    where the factor is 2 the launch is the direct fp16 x 2 kernel's (family, 3 products, the direct count), and its
    result is held to that kernel's counted k on den_d + h2_floor over the nine taps"""
    c = R._wsh('HS', 'hs2', splitk=4, bias=True)
    i = R.wino_inputs(_gen('othersk'), c)
    got = _fwd(dev, N, c, i)
    direct = 2.0 * c['B'] * c['H'] * c['W'] * c['Cin'] * c['Cout'] * 9
    assert got.rc == 0 and got.count == (1, 0) and abs(got.ratio - 3.0) < 1e-6
    assert got.fam[FAM_DIRECT_H2] == 1 and sum(got.fam) == 1 and abs(got.exec_flops - direct) <= 1e-9 * direct
    r64, _ = R.wino_refs(c, i, 'F')
    hold_k('p2l_conv_fwd:y / den_d', 'direct-h2-' + R.wino_id(c), got.y, r64['y'],
           r64['den_d'] + R.direct_h2_floor(i['x'], i['w']), R.direct_k(c, 'H'))

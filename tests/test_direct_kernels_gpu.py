"""The direct stride-1 3x3 routes (taps = 9, ups 0 / 1) -- F: conv_mfma_kernel<9, .., BF3 = false> (P2L_WFMT_F32,
csrc/p2l_conv.hip); B: the same kernel in bf16 x 3 (P2L_WFMT_BF16X3; P2L_WFMT_BF16X3W kept on it with
P2L_FORM_NO_WINO | P2L_FORM_WINO_BF3; every ups = 1 launch); H: the chunked fp16 x 2 kernel conv_h2_kernel<9, ..>
(csrc/p2l_h2.hip), maxima from the pass in front, handed over, handed over with in_applied; R: the register-resident
conv_h2r_kernel (csrc/p2l_h2r.hip), its pipelined epilogues 1 / 2 / 3 and, under P2L_FORM_H2R_SEQ_EPI, the shared
item; and the two split-K finish kernels behind F, B and H -- forward and fused input gradient, against the float64
references of tests/_small_refs.py, through ctypes, with the harness, the metric and the bars of
tests/test_small_kernels_gpu.py (tests/_pin.py):

    p2l_conv_fwd, p2l_conv_fwd_ex, p2l_conv_dgrad_arb, p2l_conv_dgrad_arb_ws, p2l_pack_conv_weight,
    p2l_pack_conv_weight_bf3, p2l_pack_conv_weight_bf3w, p2l_conv_amax_slots, p2l_conv_suggest_splitk,
    p2l_conv_workspace_bytes, p2l_conv_arb_nblk, p2l_conv_arb_nblk_ws, p2l_conv_epilogue_class.

Every case proves its route under the launch profiler: one 3x3 launch, the direct count of executed products, 16 / 6 /
3 MFMA products per fp32 product and the family (OTHER, DIRECT_H2, DIRECT_H2R); a case the dispatch moves elsewhere
fails.  Rounded outputs are held to |got - r64| / den_d <= min(k, 4 x the route's fp32 restatement) x 2^-24 with den_d
= sum_taps,k |a| |w| through the epilogue (H, R: plus direct_h2_floor) and k counted in _small_refs.direct_k; each B /
H / R case records the figure of the same inputs on route F next to its own.  What the contract calls exact is
compared bit for bit; so are one-hot power-of-two inputs, tap by tap.  Every output sits between guard bands, every
pitch is above its row with junk (inputs) or sentinels (outputs) in the gap.  P2L_DIRECT_ERR_FILE=<path> records the
figures (profiles/direct_kernels_err.txt).  The cases, their inputs and k live in tests/_small_refs.py;
tests/test_small_refs.py holds them to "the restatement is within k / 4" on the host."""
import ctypes as C

import pytest
import torch

import _small_refs as R
from _pin import (D64, G, N, SENT, Out, _gen, _record_file, hold, hold_k, is_sentinel, note, randn,  # noqa: F401
                  seeded)
from _small_refs import _cancellation_case

pytestmark = pytest.mark.gpu
EINVAL, EWS, EUNSUP = -1, -3, -4
FAM = {'F': 0, 'B': 0, 'H': 2, 'R': 6}
PRODUCTS = {'F': 16.0, 'B': 6.0, 'H': 3.0, 'R': 3.0}


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
    """one 3x3 launch, the route's products per fp32 product, its family, the direct count of executed products"""
    want = 2.0 * got.B * c['H'] * c['W'] * c['Cin'] * c['Cout'] * 9
    assert got.rc == 0, (what, got.rc)
    assert got.count == (1, 0), (what, got.count)
    assert abs(got.ratio - PRODUCTS[route]) < 1e-6, '%s: expected route %s, got %g products' % (what, route, got.ratio)
    assert got.fam[FAM[route]] == 1 and sum(got.fam) == 1, (what, route, got.fam)
    assert abs(got.exec_flops - want) <= 1e-9 * want, (what, route, got.exec_flops, want)


def _weights(dev, N, i, c, route, flip=False):
    """the packed buffer of the case's weight for the route's format; flip: through the transpose_flip copy, from the
    OIHW tensor of the forward conv whose input gradient the launch applies"""
    wfmt = R.direct_form(c, route)[0]
    cache = i.setdefault('_packed', {})
    key = (id(i['w']), wfmt, flip)                 # (a copy of i with another weight shares the dict, not the entry)
    if key not in cache:
        src = i['w'].permute(1, 0, 2, 3).flip(2, 3).contiguous() if flip else i['w']
        cache[key] = (i['w'], N.pack_conv_weight(src.to(dev), 9, c['Cout'], c['Cin'], flip, wfmt))
    return cache[key][1]


def _desc(N, c, route, B):
    d = N.P2LConv()
    d.B, d.H, d.W, d.Cin, d.Cout, d.taps, d.ups = B, c['H'], c['W'], c['Cin'], c['Cout'], 9, c['ups']
    d.x_ld, d.alpha, d.splitk = c['Cin'] + 4, c['alpha'], c['splitk']
    d.wfmt, d.form = R.direct_form(c, route)
    return d


def _scalar_finish(d, has_yp, has_mask, has_res):
    """a pitch field of an ABSENT operand that is no multiple of four: the launch's finish is the scalar kernel"""
    if not has_yp:
        d.yp_ld = 1
    elif not has_mask:
        d.mask_ld = 1
    else:
        assert not has_res
        d.res_ld = 1


def _fwd(dev, N, c, i, route=None, sl=None, handed='case', want_amax=False, next_st=None, tamper=None, ws_short=0,
         flip=False, finish=None, no_ws=False):
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
    if (finish or c['finish']) == 'scalar':
        _scalar_finish(d, c['pool'] != R.POOL_NONE, c['mask'], c['res'])
    y = Out(dev, B * H * W * (ns + 4)) if c['want_y'] else None
    yp = Out(dev, B * (H // 2) * (W // 2) * (ns + 4)) if c['pool'] != R.POOL_NONE else None
    biasd = i['bias'].to(dev) if c['bias'] else None
    h2 = route in 'HR'
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
    need = lib.p2l_conv_workspace_bytes(C.byref(d))
    assert tamper is not None or (need > 0) == (h2 or d.splitk > 1), (route, need)
    ws = Out(dev, max((need - ws_short) // 4, 1)) if need and not no_ws else None
    wsp, wsb = (N.ptr(ws.t), C.c_size_t(ws.n * 4)) if ws is not None else (None, C.c_size_t(0))

    def call():
        args = (N.ptr(xd), N.ptr(wp), N.ptr(biasd), N.ptr(sd), N.ptr(td), N.ptr(resd), N.ptr(maskd),
                N.ptr(y.t) if y else None, N.ptr(yp.t) if yp else None, wsp, wsb, N.stream())
        if ex is None:
            return lib.p2l_conv_fwd(C.byref(d), *args)
        return lib.p2l_conv_fwd_ex(C.byref(d), C.byref(ex), *args)
    got = _Got()
    got.B = B
    got.ec = lib.p2l_conv_epilogue_class(C.byref(d), C.byref(ex) if ex is not None else None, None, N.ptr(biasd),
                                         N.ptr(resd), N.ptr(maskd), N.ptr(y.t) if y else None,
                                         N.ptr(yp.t) if yp else None, wsp, wsb)
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
@pytest.mark.parametrize('case', R.DIRECT_FWD_CASES, ids=R.direct_id)
@seeded
def test_forward(dev, N, case):
    cid = R.direct_id(case)
    i = R.direct_inputs(_gen('direct', cid), case)
    got = _fwd(dev, N, case, i)
    _on_route(got, case, case['route'], cid)
    print('%s: epilogue class %d' % (cid, got.ec))
    r64, r32 = R.direct_refs(case, i)
    for name in ('y', 'yp'):
        if getattr(got, name) is not None:
            hold('%s:%s' % (_entry(got), name), cid, getattr(got, name), r64[name],
                 r64['den' if name == 'y' else 'denp'], r32[name], R.direct_k(case, pooled=name == 'yp'))
    if case['route'] != 'F':
        # the same inputs on the exact-fp32 kernel, on the plain direct denominator: recorded next to the case
        twin = _fwd(dev, N, case, i, route='F')
        _on_route(twin, case, 'F', cid + ' on F')
        f64 = R.direct_refs(case, i, 'F', restate=False)[0] if case['route'] in 'HR' else r64
        for name in ('y', 'yp'):
            if getattr(twin, name) is not None:
                note('%s:%s' % (_entry(twin), name), cid + ' on F', getattr(twin, name), f64[name],
                     f64['den' if name == 'y' else 'denp'])
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
    if case['route'] in 'HR' and case['B'] >= 3 and not (case['bias'] or case['res'] or case['noise']) \
            and got.y is not None and case['pro'] == R.PRO_NONE:
        assert bool((got.y[1] == 0).all())                              # the all-zero image


def test_slice_counts_and_channel_tiles_of_the_shapes(dev, N):
    """p2l_conv_suggest_splitk gives 8 / 4 / 4 slices for the k8 / k4 / k4s shapes whatever the batch; the maxima
    slots tell the channel tile: 64 x 64 16 -> 64 runs 64-channel tiles alone and 32-channel ones in the batch of
    ten (choose_bn's grid rule), Cout = 96 32-channel ones, Cout = 128 on a small grid 64-channel ones"""
    lib = N.lib()
    for name, sk in (('k8', 8), ('k4', 4), ('k4s', 4)):
        c = R._dsh('F', name)
        for route in 'FBH':
            for B in (1, 18):
                d = _desc(N, c, route, B)
                d.y_ld = d.n_store = c['Cout']
                assert lib.p2l_conv_suggest_splitk(C.byref(d)) == sk, (name, route, B)
    for name, B, tiles, bn in (('64x64', 1, 32, 64), ('64x64', 10, 32, 32), ('32x4', 2, 1, 32), ('8x16', 1, 1, 64)):
        c = R._dsh('F', name)
        d = _desc(N, c, 'F', B)
        d.y_ld = d.n_store = c['Cout']
        assert lib.p2l_conv_amax_slots(C.byref(d)) == tiles * (c['Cout'] // bn) * 4, (name, B)


# =====================================================================================================================
# exact inputs: tap, channel and pixel placement bit for bit
# =====================================================================================================================
ONEHOT = [R._dsh('F', '4x4'), R._dsh('F', '12x20'), R._dsh('B', '6x6'), R._dsh('B', '24x16', wfmt='bf3w'),
          R._dsh('H', '8x8'), R._dsh('H', '12x20'), R._dsh('H', '16x32'), R._dsh('R', '16x32'),
          R._dsh('R', '16x32', seq=True), R._dsh('F', '16x16', ups=1), R._dsh('B', '8x8', ups=1, wfmt='bf3w'),
          R._dsh('H', 'k3', splitk=3), R._dsh('B', 'k4s', splitk=4)]


@pytest.mark.parametrize('flip', [False, True], ids=['forward', 'transpose_flip'])
@pytest.mark.parametrize('tap', range(9))
def test_one_hot_inputs_are_exact(dev, N, tap, flip):
    """single power-of-two pixels at corners, edges, both sides of every tile seam, the last row / column of a partial
    tile and the first pixel of the second image of a multi-image tile, single power-of-two weights on one tap: every
    route gives the fp64 result bit for bit -- also through the transpose_flip copy of the packer, with ups = 1 and
    in K slices"""
    for c in ONEHOT:
        i = R.direct_onehot(c, tap, tap % 2)
        got = _fwd(dev, N, c, i, flip=flip)
        _on_route(got, c, c['route'], R.direct_id(c))
        want = R.conv3x3(i['x'].double(), i['w'].double(), ups=bool(c['ups']), den_w=False)['y']
        assert int((want != 0).sum()) >= 3
        assert torch.equal(got.y.double(), want), (R.direct_id(c), int((got.y.double() != want).sum()))


def test_all_zero_inputs_give_exactly_zero(dev, N):
    for c in (R._dsh('F', '8x8'), R._dsh('B', '12x20'), R._dsh('H', '4x4'), R._dsh('H', 'k3', splitk=3),
              R._dsh('R', '16x32'), R._dsh('B', '8x8', ups=1, wfmt='bf3w')):
        h, w = (c['H'] // 2, c['W'] // 2) if c['ups'] else (c['H'], c['W'])
        i = dict(x=torch.zeros(c['B'], h, w, c['Cin']), w=randn(_gen('zero', c['route']), c['Cout'], c['Cin'], 3, 3))
        got = _fwd(dev, N, c, i)
        _on_route(got, c, c['route'])
        assert bool((got.y.view(torch.int32) == 0).all()), R.direct_id(c)


# =====================================================================================================================
# bit-exact contracts
# =====================================================================================================================
R_CASES = [c for c in R.DIRECT_FWD_CASES if c['route'] == 'R']


@pytest.mark.parametrize('case', R_CASES, ids=R.direct_id)
def test_the_register_resident_kernel_is_the_chunked_one_bit_for_bit(dev, N, case):
    """R = H (P2L_FORM_NO_H2R): y, yp and every maxima slot; each pipelined epilogue (EPI 1 / 2 / 3) = the shared
    item (P2L_FORM_H2R_SEQ_EPI)"""
    i = R.direct_inputs(_gen('r-is-h', R.direct_id(case)), case)
    r = _fwd(dev, N, case, i, want_amax=True)
    h = _fwd(dev, N, case, i, route='H', want_amax=True)
    _on_route(r, case, 'R')
    _on_route(h, case, 'H')
    assert r.slots == h.slots == (case['H'] // 8) * (case['W'] // 16) * 4
    _same_bits(r, h, ('y', 'yp', 'amax', 'amaxp'), 'R vs H')
    if not case['seq']:
        s = _fwd(dev, N, dict(case, seq=True), i, want_amax=True)
        _on_route(s, case, 'R')
        _same_bits(r, s, ('y', 'yp', 'amax', 'amaxp'), 'pipelined vs shared item')


ALONE = [R._dsh('F', '4x4', **R.EPI[0]), R._dsh('B', '8x8', wfmt='bf3w', **R.EPI[1]), R._dsh('H', '4x4', **R.EPI[2]),
         R._dsh('H', '8x8', amax='raw', **R.EPI[1]), R._dsh('F', '64x64', bias=True), R._dsh('B', '64x64', bias=True),
         R._dsh('H', '64x64', bias=True), R._dsh('R', '16x32', **R.EPI[3]), R._dsh('R', '16x32', seq=True, **R.EPI[0]),
         R._dsh('F', 'k4s', splitk=4, **R.EPI[0]), R._dsh('B', 'k8', splitk=8, **R.EPI[3]),
         R._dsh('H', 'k8', splitk=8, amax='applied', pro=R.PRO_AFFINE_RELU, pool=R.POOL_SUM),
         R._dsh('B', '8x8', ups=1, wfmt='bf3w', **R.EPI[0]), R._dsh('H', '12x20', act=R.ACT_TANH)]


@pytest.mark.parametrize('case', ALONE, ids=R.direct_id)
def test_an_image_alone_has_the_bits_it_has_in_any_batch(dev, N, case):
    """... with the same splitk: in the multi-image tiles of the 4x4 / 8x8 layers, and at 64 x 64 16 -> 64, where the
    batch of ten runs 32-channel tiles and the image alone 64-channel ones"""
    i = R.direct_inputs(_gen('alone', R.direct_id(case)), case)
    whole = _fwd(dev, N, case, i)
    _on_route(whole, case, case['route'])
    for b in sorted(set([0, case['B'] // 2, case['B'] - 1])):
        one = _fwd(dev, N, case, i, sl=slice(b, b + 1))
        _on_route(one, case, case['route'])
        for name in ('y', 'yp'):
            if getattr(whole, name) is not None:
                assert torch.equal(getattr(one, name)[0].view(torch.int32), getattr(whole, name)[b].view(torch.int32)), \
                    (name, b)


@pytest.mark.parametrize('case', [c for c in R.DIRECT_FWD_CASES if c['finish'] == 'scalar'] +
                         [R._dsh('F', 'k3', splitk=3, res='ups', mask=True, act=R.ACT_TANH, n_store=36),
                          R._dsh('H', 'k4', splitk=4, act=R.ACT_RELU, pool=R.POOL_MAX)], ids=R.direct_id)
def test_the_two_finish_kernels_agree_bit_for_bit(dev, N, case):
    i = R.direct_inputs(_gen('finish', R.direct_id(case)), case)
    v4, sc = _fwd(dev, N, case, i, finish='v4'), _fwd(dev, N, case, i, finish='scalar')
    for got in (v4, sc):
        _on_route(got, case, case['route'])
    _same_bits(v4, sc, ('y', 'yp'))


@pytest.mark.parametrize('case', [R._dsh('H', '8x8', bias=True), R._dsh('H', '12x20', act=R.ACT_RELU),
                                  R._dsh('H', 'k8', splitk=8, bias=True), R._dsh('R', '16x32', bias=True)],
                         ids=R.direct_id)
def test_handed_true_maxima_equal_the_pass_in_front(dev, N, case):
    """a consumer without a prologue: the same bits with handed-over maxima as with its own max-|x| pass"""
    i = R.direct_inputs(_gen('handed', R.direct_id(case)), case)
    own = _fwd(dev, N, case, i)
    handed = _fwd(dev, N, case, i, handed=i['x'].abs().amax(dim=(1, 2, 3)))
    for got in (own, handed):
        _on_route(got, case, case['route'])
    _same_bits(own, handed, ('y', 'yp'))


AMAX_CASES = [R._dsh('B', '16x16', act=R.ACT_RELU, pool=R.POOL_MAX), R._dsh('B', '32x4', bias=True, n_store=36),
              R._dsh('H', '24x16', bias=True, pool=R.POOL_SUM), R._dsh('H', '8x16', act=R.ACT_TANH),
              R._dsh('R', '16x32', act=R.ACT_RELU, pool=R.POOL_MAX), R._dsh('R', '16x32', seq=True, alpha=0.5),
              R._dsh('F', 'k4', splitk=4, bias=True, pool=R.POOL_MAX), R._dsh('H', 'k8', splitk=8, n_store=32)]


@pytest.mark.parametrize('nxt', [False, True], ids=['plain', 'next-affine'])
@pytest.mark.parametrize('case', AMAX_CASES, ids=R.direct_id)
def test_the_maxima_slots_hold_the_maximum_of_what_was_stored(dev, N, case, nxt):
    """the per-image maximum over the p2l_conv_amax_slots(d) slots == max |y| of the y the launch stored (outp: of
    yp); with next_s / next_t == max |fma(y, s, t)|.  The slot buffers are exactly that long, between guard bands:
    no slot beyond the promised ones is written"""
    g = _gen('amax', R.direct_id(case))
    i = R.direct_inputs(g, case)
    B, ns = case['B'], case['n_store']
    st = (0.5 + torch.rand(B, ns, generator=g), randn(g, B, ns) * R.mags(B).view(B, 1)) if nxt else None
    got = _fwd(dev, N, case, i, want_amax=True, next_st=st)
    _on_route(got, case, case['route'])
    TW, TH, TB = R.direct_tile(case['H'], case['W'])
    if case['splitk'] > 1:
        assert got.slots == (case['H'] // 2) * (case['W'] // 2) * (ns // 4) // 64
    else:
        assert TB == 1
        bn = 64 if case['Cout'] % 64 == 0 else 32
        assert got.slots == (case['H'] // TH) * (case['W'] // TW) * (1 if case['route'] == 'R' else case['Cout'] // bn) * 4
    assert bool((got.amax.view(torch.int32) != SENT).all()) and bool((got.amax >= 0).all())
    if nxt:
        assert torch.equal(got.amax.amax(dim=1), R.producer_amax(got.y, *st))
    else:
        assert torch.equal(got.amax.amax(dim=1), R.producer_amax(got.y))
    if got.amaxp is not None:
        assert bool((got.amaxp.view(torch.int32) != SENT).all())
        assert torch.equal(got.amaxp.amax(dim=1), R.producer_amax(got.yp))


# =====================================================================================================================
# fused input gradient
# =====================================================================================================================
def _arb(dev, N, c, i, route=None, tamper=None, flip=True):
    """one p2l_conv_dgrad_arb(_ws) launch of case c -> _Got: rc, dx, ds, dt, the profiler's figures and the
    epilogue class; flip: the weight goes through the transpose_flip pack, from the OIHW tensor of the forward conv
    whose input gradient the launch applies"""
    lib = N.lib()
    route = route or c['route']
    B, H, W, Cin, Cout = c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    Ho, Wo = (H // 2, W // 2) if c['pool_sum'] else (H, W)
    wp = _weights(dev, N, i, c, route, flip)
    d = _desc(N, c, route, B)
    d.alpha, d.y_ld, d.yp_ld, d.n_store, d.w_floats = 1.0, Cout + 4, Cout + 4, Cout, wp.numel()
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
    nblk = max(lib.p2l_conv_arb_nblk_ws(C.byref(d)), lib.p2l_conv_arb_nblk(C.byref(d)), 1)
    part = Out(dev, 2 * B * nblk * Cout)
    a.partial = N.ptr(part.t).value
    if c['amax'] and route in 'HR':
        hand = (R.pw_amax(c, i)[0].view(B, 1) * torch.tensor([0.5, 1.0, 0.25])).contiguous()
        a.amax.in_, a.amax.in_n = N.ptr(hand.to(dev)).value, 3
    am = None
    if c['amax_out']:                              # the maxima of dx, in exactly p2l_conv_amax_slots slots
        got_slots = lib.p2l_conv_amax_slots(C.byref(d))
        assert got_slots > 0
        am = Out(dev, B * got_slots)
        a.amax.out = N.ptr(am.t).value
    dx = Out(dev, B * Ho * Wo * (Cout + 4))
    xd = _pitched(i['x'], Cin + 4, dev)
    need = lib.p2l_conv_workspace_bytes(C.byref(d))
    assert (need > 0) == (route in 'HR' or d.splitk > 1), (route, need)
    ws = Out(dev, need // 4) if need else None
    wsp, wsb = (N.ptr(ws.t), C.c_size_t(ws.n * 4)) if ws is not None else (None, C.c_size_t(0))

    def call():
        if ws is None:
            return lib.p2l_conv_dgrad_arb(C.byref(d), C.byref(a), N.ptr(xd), N.ptr(wp), N.ptr(dx.t), N.stream())
        return lib.p2l_conv_dgrad_arb_ws(C.byref(d), C.byref(a), N.ptr(xd), N.ptr(wp), N.ptr(dx.t), wsp, wsb, N.stream())
    got = _Got()
    got.B = B
    got.ec = lib.p2l_conv_epilogue_class(C.byref(d), None, C.byref(a), None, None, None, N.ptr(dx.t), None, wsp, wsb)
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
    got.amax = am.cpu(B, -1) if am is not None else None
    return got


_ARB_CLASSES = {}


@pytest.mark.parametrize('case', R.DIRECT_ARB_CASES, ids=R.direct_arb_id)
@seeded
def test_dgrad_fused_affine_relu_bwd(dev, N, case):
    cid = R.direct_arb_id(case)
    i = R.direct_arb_inputs(_gen('darb', cid), case)
    got = _arb(dev, N, case, i)
    _on_route(got, case, case['route'], cid)
    _ARB_CLASSES[cid] = (case['route'], case['splitk'], got.ec)
    print('%s: epilogue class %d' % (cid, got.ec))
    r64, r32 = R.direct_arb_refs(case, i)
    kdx, kds, kdt = R.arb_k(case, R.direct_k)
    hold('%s:dx' % got.entry, cid, got.dx, r64['dx'], r64['den_dx'], r32['dx'], kdx)
    # ds, dt: on these signed operands inside the a-priori bound; held to their bar on the positive ones
    for name, bound in zip(('ds', 'dt'), R.arb_bound(case, r64, i['ax'], R.direct_k)):
        err = (getattr(got, name).to(D64) - r64[name]).abs()
        print('%s %s: %.3f of the a-priori bound' % (cid, name, float((err / (bound * R.U).clamp_min(1e-300)).max())))
        assert bool((err <= bound * R.U).all()), name
    ip = R.arb_positive(i)
    pos = _arb(dev, N, case, ip)
    _on_route(pos, case, case['route'], cid)
    p64, p32 = R.direct_arb_refs(case, ip)
    for name, k in (('ds', kds), ('dt', kdt)):
        hold('%s:%s' % (got.entry, name), cid, getattr(pos, name), p64[name], p64['den_' + name], p32[name], k)
    _same_bits(_arb(dev, N, case, i), got, ('dx', 'ds', 'dt'), cid)
    if case['route'] == 'R':                                           # R = H: dx, ds, dt
        _same_bits(_arb(dev, N, case, i, route='H'), got, ('dx', 'ds', 'dt'), cid + ' on H')
    if not case['nomask'] and not case['skip']:
        dead = r64['g'] == 0                                               # (no shortcut: dx = g s, +0 where masked)
        assert bool((got.dx[dead] == 0).all())
    if got.amax is not None and not case['pool_sum']:
        assert bool((got.amax.view(torch.int32) != SENT).all())
        assert torch.equal(got.amax.amax(dim=1), got.dx.abs().amax(dim=(1, 2, 3)))


def test_both_kinds_of_epilogue_ran_under_the_fp64_bar(dev, N):
    """of the unsplit H gradient cases at least one runs an epilogue compiled for its class (epi_item_ct<EC>:
    p2l_conv_epilogue_class != 0) and at least one the shared item: test_dgrad_fused_affine_relu_bwd pins both
    against fp64, not only against each other.  The class is a function of the descriptor: asked here once more, so
    that the test stands on its own"""
    classes = {}
    for case in R.DIRECT_ARB_CASES:
        if case['route'] != 'H' or case['splitk'] > 1:
            continue
        cid = R.direct_arb_id(case)
        got = _arb(dev, N, case, R.direct_arb_inputs(_gen('darb-class', cid), case))
        _on_route(got, case, 'H', cid)
        classes[cid] = got.ec
        assert _ARB_CLASSES.get(cid, ('H', 1, got.ec))[2] == got.ec          # (what the pinned launch reported)
    assert any(ec != 0 for ec in classes.values()) and any(ec == 0 for ec in classes.values()), classes


MASK_ROUTES = [('F', 64, dict()), ('B', 64, dict()), ('B', 64, dict(wfmt='bf3w')), ('H', 64, dict()),
               ('R', 64, dict(seq=True)), ('F', 128, dict(splitk=4)), ('H', 128, dict(splitk=4)),
               ('H', 128, dict(splitk=4, finish='scalar'))]


@pytest.mark.parametrize('route,Cin,kw', MASK_ROUTES, ids=lambda v: str(v))
def test_fused_backward_mask_is_the_forwards_decision(dev, N, route, Cin, kw):
    """{g != 0} of the fused dgrad epilogue (sliced: of the finish kernel) -- read off dt with da = 1 through a weight
    that is the identity on its centre tap, and off dx -- == {a > 0} of the forward's PRO_AFFINE_RELU prologue read
    through route F, on inputs where x s + t rounded once and rounded twice decide differently (_cancellation_case)"""
    Bn, H, Cc = 2, 16, 64
    P = H * H
    wf = torch.zeros(Cc, Cc, 3, 3)
    wf[:, :, 1, 1] = torch.eye(Cc)
    wa = torch.zeros(Cc, Cin, 3, 3)
    wa[:, :Cc, 1, 1] = torch.eye(Cc)
    fc = R._dc('F', (H, H), Bn, Cc, Cc, pro=R.PRO_AFFINE_RELU)
    ac = R._dac(route, (H, 2 * H if route == 'R' else H), Bn, Cin, Cc, **kw)
    for seed in range(3):
        x, s, t, once, twice, A, B = _cancellation_case(seed, Bn, P, Cc)
        fwd = _fwd(dev, N, fc, dict(x=x.view(Bn, H, H, Cc), w=wf, s=s, t=t))
        _on_route(fwd, fc, 'F')
        live = (fwd.y > 0).view(Bn, H, H, Cc)
        ax = x.view(Bn, H, H, Cc)
        if route == 'R':                                                # (whole 8x16 tiles: the image twice, side by side)
            ax, live = torch.cat([ax, ax], dim=2), torch.cat([live, live], dim=2)
        live = live.reshape(Bn, -1, Cc)
        i = dict(x=torch.ones(Bn, ac['H'], ac['W'], Cin), w=wa, ax=ax.contiguous(), **{'as': s, 'at': t})
        tamper = (lambda d, a: setattr(d, 'mask_ld', 1)) if kw.get('finish') == 'scalar' else None
        got = _arb(dev, N, ac, i, flip=False, tamper=tamper)
        _on_route(got, ac, route)
        diff = live != (got.dx.view(Bn, -1, Cc) != 0)
        assert not bool(diff.any()), ('forward and backward decide differently', int(diff.sum()))
        assert torch.equal(got.dt, live.float().sum(1))                    # dt counts the live pixels (da = 1)


# =====================================================================================================================
# arguments
# =====================================================================================================================
def _set(**kw):
    def tamper(d, *_):
        for k, v in kw.items():
            setattr(d, k, v)
    return tamper


FWD_ARGS = [
    # partial tiles with a pool / K slices
    ('partial-pool', R._dsh('F', '12x20', act=R.ACT_RELU, pool=R.POOL_MAX), {}, None, EUNSUP),
    ('partial-pool-multi-image', R._dsh('H', '6x6', pool=R.POOL_SUM), {}, None, EUNSUP),
    ('partial-splitk', R._dc('B', (12, 20), 2, 128, 64, splitk=4), {}, None, EUNSUP),
    ('partial-splitk-multi-image', R._dc('H', (6, 6), 3, 128, 64, splitk=4), {}, None, EUNSUP),
    # the workspace one float short of the slices
    ('workspace-F', R._dsh('F', 'k4', splitk=4, bias=True), dict(ws_short=4), None, EWS),
    ('workspace-H', R._dsh('H', 'k8', splitk=8, bias=True), dict(ws_short=3 * 64 * 4 + 4), None, EWS),
    # maxima slots asked of an h2r-shaped layer without workspace
    ('h2r-slots-no-workspace', R._dsh('R', '16x32', bias=True), dict(no_ws=True, want_amax=True), None, EWS),
    # odd H / W, and every pitch check on a 3x3 descriptor
    ('odd-H', R._dsh('F', '8x8', bias=True), {}, _set(H=7), EINVAL),
    ('odd-W', R._dsh('H', '8x8', bias=True), {}, _set(W=7), EINVAL),
    ('x_ld-short', R._dsh('B', '8x8', bias=True), {}, _set(x_ld=44), EINVAL),
    ('x_ld-unaligned', R._dsh('H', '8x8', bias=True), {}, _set(x_ld=50), EINVAL),
    ('y_ld-short', R._dsh('R', '16x32', bias=True), {}, _set(y_ld=60), EINVAL),
    ('y_ld-unaligned', R._dsh('F', '8x8', bias=True), {}, _set(y_ld=66), EINVAL),
    ('yp_ld-short', R._dsh('H', '16x16', pool=R.POOL_MAX), {}, _set(yp_ld=60), EINVAL),
    ('res_ld-short', R._dsh('B', '8x8', res='same'), {}, _set(res_ld=60), EINVAL),
    ('mask_ld-short', R._dsh('H', '8x8', mask=True), {}, _set(mask_ld=60), EINVAL),
    ('pro_bstride-short', R._dsh('F', '8x8', pro=R.PRO_AFFINE), {}, _set(pro_bstride=44), EINVAL),
    ('n_store-unaligned', R._dsh('B', '8x8', bias=True), {}, _set(n_store=34), EINVAL),
    # w_floats too short for the format
    ('w_floats-F', R._dsh('F', '8x8', bias=True), {}, _set(w_floats=9 * 64 * 48 - 1), EINVAL),
    ('w_floats-bf3', R._dsh('B', '8x8', bias=True), {}, _set(w_floats=9 * 64 * 48 * 3 // 2 - 1), EINVAL),
    ('w_floats-bf3w', R._dsh('H', '8x8', bias=True), {}, 'w_floats', EINVAL),
]


@pytest.mark.parametrize('what,case,kw,tamper,want', FWD_ARGS, ids=[a[0] for a in FWD_ARGS])
def test_forward_arguments_are_refused_before_the_launch(dev, N, what, case, kw, tamper, want):
    """nothing is launched, every output still holds sentinels; the same launch without the fault is a good one"""
    lib = N.lib()
    i = R.direct_inputs(_gen('dargs', what), case)
    if tamper == 'w_floats':
        n = lib.p2l_packed_weight_floats(9, case['Cout'], case['Cin'], R.WFMT_BF16X3W)
        tamper = _set(w_floats=n - 1)
    got = _fwd(dev, N, case, i, tamper=tamper, **kw)
    assert got.rc == want, (what, got.rc)
    assert got.count == (0, 0) and _untouched(got)
    if not what.startswith('partial'):
        ok = _fwd(dev, N, case, i, **{k: v for k, v in kw.items() if k == 'want_amax'})
        _on_route(ok, case, case['route'], what)


ARB_ARGS = [
    ('partial', R._dac('F', (12, 20), 2, 32, 64), EUNSUP),
    ('partial-multi-image-sliced', R._dac('H', (6, 6), 3, 128, 64, splitk=4), EUNSUP),
    ('multi-image-unsplit-F', R._dac('F', (8, 8), 3, 32, 64), EUNSUP),
    ('multi-image-unsplit-B', R._dac('B', (4, 4), 5, 32, 64, wfmt='bf3w'), EUNSUP),
    ('multi-image-unsplit-H', R._dac('H', (8, 8), 3, 32, 64), EUNSUP),
]


@pytest.mark.parametrize('what,case,want', ARB_ARGS, ids=[a[0] for a in ARB_ARGS])
def test_fused_backward_arguments_are_refused_before_the_launch(dev, N, what, case, want):
    got = _arb(dev, N, case, R.direct_arb_inputs(_gen('dargs-arb', what), case))
    assert got.rc == want, (what, got.rc)
    assert got.count == (0, 0) and _untouched(got)


@seeded
def test_without_the_maxima_share_of_the_workspace_the_launch_keeps_bf16x3(dev, N):
    """the header: the fp16 x 2 form needs 256 B of workspace per image, without it the launch keeps the bf16 x 3
    arithmetic -- unsplit without any workspace, and in K slices with a workspace one float short of
    p2l_conv_workspace_bytes (it still holds the slices): six products on the direct kernel, inside the workspace it
    was given, held as route B"""
    for case, kw in ((R._dsh('H', '8x8', bias=True), dict(no_ws=True)),
                     (R._dsh('H', 'k8', splitk=8, bias=True), dict(ws_short=4))):
        cid = R.direct_id(case) + ' kept on bf16 x 3'
        i = R.direct_inputs(_gen('wsfall', cid), case)
        got = _fwd(dev, N, case, i, **kw)
        want = 2.0 * case['B'] * case['H'] * case['W'] * case['Cin'] * case['Cout'] * 9
        assert got.rc == 0 and got.count == (1, 0) and abs(got.ratio - 6.0) < 1e-6
        assert got.fam[0] == 1 and sum(got.fam) == 1 and abs(got.exec_flops - want) <= 1e-9 * want
        r64, r32 = R.direct_refs(case, i, 'B')
        hold('p2l_conv_fwd:y', cid, got.y, r64['y'], r64['den'], r32['y'], R.direct_k(case, 'B'))

"""The 1x1 convolution, every route of conv_launch_impl for taps = 1 -- A: conv_mfma_kernel<1, ..> on the exact-fp32
MFMA (KC 32 / 16, 64- and 32-channel tiles, multi-image and partial tiles, K slices and both finish kernels), B:
pw_bf3_kernel (bf16 x 3), C: pw_h2_kernel (fp16 x 2 on handed-over maxima), D: pw_h2_kernel<.., SM> (small grids, K
slices, maxima from the pass in front or handed over) -- forward and fused input gradient, against the float64
references of tests/_small_refs.py, through ctypes, with the harness, the metric and the bars of
tests/test_small_kernels_gpu.py (tests/_pin.py):

    p2l_conv_fwd, p2l_conv_fwd_ex, p2l_conv_dgrad_arb, p2l_conv_dgrad_arb_ws, p2l_pack_conv_weight (taps 1),
    p2l_pack_conv_weight_pw, p2l_conv_amax_slots, p2l_conv_suggest_splitk.

Every case proves its arithmetic and kernel family: it runs under the launch profiler and asserts the 16-bit MFMA
products per fp32 product (16 / 6 / 3) and the family of the launch; a case that lands on another one fails.  (The
profiler does not tell route C from D -- same products, same family: the shape does, pw_shape against the small
grids -- nor the sub-forms of route A: KC, the channel tile and the images per tile follow from the shape alone.)  Rounded outputs are held
to |got - r64| / den <= min(k, 4 x the route's fp32 restatement) x 2^-24 with den = sum |terms| (routes C and D: plus
the absolute floor of the fp16 x 2 contract, _small_refs.h2_floor) and k counted in _small_refs.pw_k / arb_k; the
inputs of routes B, C and D also run on route A and that figure is recorded next to theirs.  What the contract calls
exact is compared bit for bit.  Every output sits between guard bands, every pitch is above its row with junk (inputs)
or sentinels (outputs) in the gap.  P2L_PW_ERR_FILE=<path> records the figures (profiles/pw_kernels_err.txt).
The cases, their inputs and k live in tests/_small_refs.py; tests/test_small_refs.py holds them to "the restatement
is within k / 4" on the host."""
import ctypes as C

import pytest
import torch

import _small_refs as R
from _pin import D64, G, N, SENT, Out, _gen, _record_file, d64, draw, hold, is_sentinel, randn, seeded  # noqa: F401
from _small_refs import _cancellation_case

pytestmark = pytest.mark.gpu
EINVAL, EWS, EUNSUP = -1, -3, -4
FAM_OTHER, FAM_PW = 0, 5
RATIO = {'A': 16.0, 'B': 6.0, 'C': 3.0, 'D': 3.0}


def _pitched(t, ld, dev, junk=7.0):
    """[..., C] -> the same rows at pitch ld on the device, junk in the gap columns"""
    o = torch.full(t.shape[:-1] + (ld,), junk)
    n = min(ld, t.shape[-1])
    o[..., :n] = t[..., :n]
    return o.to(dev)


class _Got(object):
    pass


def _profiled(N, fn):
    """fn() under the launch profiler -> its return code, MFMA products per fp32 product and launches per family of
    the 1x1 launches it made"""
    lib = N.lib()
    N.check(lib.p2l_prof_begin(64), 'p2l_prof_begin')
    lib.p2l_prof_step(0, 1)
    rc = fn()
    torch.cuda.synchronize()
    T = N.prof_end()
    ratio = T.mfma_flops[1] / T.exec_flops[1] if T.count[1] else 0.0
    return rc, ratio, (T.count[0], T.count[1]), list(T.fam_count)


def _on_route(got, route, what=''):
    assert got.rc == 0, (what, got.rc)
    assert got.count == (0, 1), (what, got.count)
    assert abs(got.ratio - RATIO[route]) < 1e-6, '%s: expected route %s, got %g products' % (what, route, got.ratio)
    fam = FAM_OTHER if route == 'A' else FAM_PW
    assert got.fam[fam] == 1 and sum(got.fam) == 1, (what, got.fam)


def _weights(dev, N, w, wfmt):
    Cout, Cin = w.shape
    return N.pack_conv_weight(w.reshape(Cout, Cin, 1, 1).to(dev), 1, Cout, Cin, False, wfmt)


def _scalar_finish(d, has_yp, has_mask, has_res):
    """a pitch field of an ABSENT operand that is no multiple of four: the launch's finish is the scalar kernel"""
    if not has_yp:
        d.yp_ld = 1
    elif not has_mask:
        d.mask_ld = 1
    else:
        assert not has_res
        d.res_ld = 1


def _fwd(dev, N, c, i, form=None, sl=None, splitk=None, finish=None, handed='case', want_amax=False, next_st=None,
         tamper=None, ex_tamper=None, ws_short=0):
    """one forward launch of case c on inputs i (images sl) -> _Got: rc, y [B, H, W, n_store], yp, the profiler's
    figures, the maxima slots.  Everything the launch may write is an Out; the gap columns are checked here."""
    lib = N.lib()
    sl = slice(0, c['B']) if sl is None else sl
    B, H, W, Cin, Cout, ns = sl.stop - sl.start, c['H'], c['W'], c['Cin'], c['Cout'], c['n_store']
    wp = _weights(dev, N, i['w'], c['wfmt'])
    d = N.P2LConv()
    d.B, d.H, d.W, d.Cin, d.Cout, d.taps, d.ups = B, H, W, Cin, Cout, 1, 0
    d.x_ld, d.pro, d.alpha, d.act, d.pool = Cin + 4, c['pro'], c['alpha'], c['act'], c['pool']
    d.y_ld = d.yp_ld = ns + 4
    d.n_store, d.res_ups = ns, int(c['res'] == 'ups')
    d.splitk = c['splitk'] if splitk is None else splitk
    d.wfmt, d.form, d.w_floats = c['wfmt'], c['form'] if form is None else form, wp.numel()
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
    if (c['finish'] if finish is None else finish) == 'scalar':
        _scalar_finish(d, c['pool'] != R.POOL_NONE, c['mask'], c['res'])
    y = Out(dev, B * H * W * (ns + 4)) if c['want_y'] else None
    yp = Out(dev, B * (H // 2) * (W // 2) * (ns + 4)) if c['pool'] != R.POOL_NONE else None
    biasd = i['bias'].to(dev) if c['bias'] else None
    hand = (R.pw_amax(c, i)[0] if c['amax'] else None) if isinstance(handed, str) else handed
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
    if ex_tamper is not None:
        ex_tamper(ex)
    slots = lib.p2l_conv_amax_slots(C.byref(d)) if want_amax else 0
    am = amp = None
    if want_amax:
        assert slots > 0
        am = Out(dev, B * slots)
        ex.amax.out = N.ptr(am.t).value
        if yp is not None:
            amp = Out(dev, B * slots)
            ex.amax.outp = N.ptr(amp.t).value
        if next_st is not None:
            ex.amax.next_s, ex.amax.next_t = N.ptr(next_st[0].to(dev)).value, N.ptr(next_st[1].to(dev)).value
            ex.amax.next_bstride = next_st[0].shape[1]
    need = lib.p2l_conv_workspace_bytes(C.byref(d))
    ws = Out(dev, max((need - ws_short) // 4, 1)) if c['ws'] and need else None
    wsp, wsb = (N.ptr(ws.t), C.c_size_t(ws.n * 4)) if ws is not None else (None, C.c_size_t(0))

    def call():
        args = (N.ptr(xd), N.ptr(wp), N.ptr(biasd), N.ptr(sd), N.ptr(td), N.ptr(resd), N.ptr(maskd),
                N.ptr(y.t) if y else None, N.ptr(yp.t) if yp else None, wsp, wsb, N.stream())
        if ex is None:
            return lib.p2l_conv_fwd(C.byref(d), *args)
        return lib.p2l_conv_fwd_ex(C.byref(d), C.byref(ex), *args)
    got = _Got()
    got.rc, got.ratio, got.count, got.fam = _profiled(N, call)
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


# =====================================================================================================================
# forward: every route, every epilogue
# =====================================================================================================================
@pytest.mark.parametrize('case', R.PW_FWD_CASES, ids=R.pw_id)
@seeded
def test_forward(dev, N, case):
    cid = R.pw_id(case)
    i = R.pw_inputs(_gen('pw', cid), case)
    got = _fwd(dev, N, case, i)
    _on_route(got, case['route'], cid)
    r64, r32 = R.pw_refs(case, i)
    for name, den in (('y', 'den'), ('yp', 'denp')):
        if getattr(got, name) is not None:
            hold('%s:%s' % (_entry(got), name), cid, getattr(got, name), r64[name], r64[den], r32[name],
                 R.pw_k(case, pooled=name == 'yp'))
    if case['route'] != 'A':
        # the same inputs on the exact-fp32 kernel: "fp32-equivalent" can be read off the record file
        twin = _fwd(dev, N, case, i, form=R.FORM_NO_PW, handed=None)
        _on_route(twin, 'A', cid + ' on A')
        a64, a32 = R.pw_refs(case, i, 'A')
        for name, den in (('y', 'den'), ('yp', 'denp')):
            if getattr(twin, name) is not None:
                hold('%s:%s' % (_entry(twin), name), cid + ' on A', getattr(twin, name), a64[name], a64[den],
                     a32[name], R.pw_k(case, 'A', name == 'yp'))
    # exact: a repeated launch; a masked element is +0; yp is the pool of the y this launch stored
    again = _fwd(dev, N, case, i)
    for name in ('y', 'yp'):
        if getattr(got, name) is not None:
            assert torch.equal(getattr(again, name).view(torch.int32), getattr(got, name).view(torch.int32)), name
    if case['mask'] and got.y is not None:
        dead = ~(i['mask'][..., :case['n_store']] > 0)
        assert bool(dead.any()) and bool((got.y.view(torch.int32)[dead] == 0).all())
    if got.y is not None and got.yp is not None:
        v0, v1, v2, v3 = R.quads(got.y)
        want = torch.maximum(torch.maximum(v0, v1), torch.maximum(v2, v3)) if case['pool'] == R.POOL_MAX \
            else (v0 + v1) + (v2 + v3)
        assert torch.equal(got.yp, want)
    if case['route'] in 'CD' and case['B'] >= 3 and not (case['bias'] or case['res'] or case['noise']) \
            and got.y is not None and case['pro'] == R.PRO_NONE:
        assert bool((got.y[1] == 0).all())                              # the all-zero image


# =====================================================================================================================
# bit-exact contracts
# =====================================================================================================================
ALONE = [c for c in R.PW_FWD_CASES if c['B'] >= 3 and c['finish'] == 'v4' and not c['form'] & R.FORM_WINO_BF3
         and R.pw_id(c) in ('A-9x4x4-32to32-alpha0.5-biasTrue-ressame', 'A-3x8x8-48to64-pro1-resups',
                            'A-3x16x16-160to64-act1-pool1', 'A-9x64x64-64to64',
                            'B-3x8x128-192to128-pro1-resups', 'B-3x24x48-192to64-act1-pool1',
                            'C-3x32x32-64to64-alpha0.5-amaxtrue-biasTrue-ressame',
                            'C-3x8x128-192to128-amaxraw-pro1-resups', 'C-3x24x48-192to64-amaxapplied-maskTrue-pro2',
                            'D-9x4x4-32to64-alpha0.5-biasTrue-ressame', 'D-5x8x8-96to128-amaxraw-pro1-resups-splitk3',
                            'D-3x8x16-160to64-maskTrue-pro2-splitk2', 'D-3x8x8-160to64-act3-biasTrue-noiseTrue-oscaleTrue')]


def test_the_alone_list_names_cases_of_every_route():
    assert sorted(set(c['route'] for c in ALONE)) == ['A', 'B', 'C', 'D'] and len(ALONE) == 13


@pytest.mark.parametrize('case', ALONE, ids=R.pw_id)
def test_an_image_alone_has_the_bits_it_has_in_any_batch(dev, N, case):
    """with the slice count p2l_conv_suggest_splitk gives for the layer, an image launched alone (B = 1) has the bits
    it has at its position of the batch -- first, middle and last image, all four routes"""
    lib = N.lib()
    i = R.pw_inputs(_gen('alone', R.pw_id(case)), case)
    d = N.P2LConv()
    d.B, d.H, d.W, d.Cin, d.Cout, d.taps = case['B'], case['H'], case['W'], case['Cin'], case['Cout'], 1
    d.x_ld, d.n_store, d.y_ld, d.yp_ld, d.wfmt, d.form = case['Cin'] + 4, case['n_store'], case['n_store'] + 4, \
        case['n_store'] + 4, case['wfmt'], case['form']
    sk = lib.p2l_conv_suggest_splitk(C.byref(d))
    d.B = 1
    assert lib.p2l_conv_suggest_splitk(C.byref(d)) == sk                # a function of the layer, not of the batch
    c = dict(case, splitk=sk, ws=case['ws'] or sk > 1)
    whole = _fwd(dev, N, c, i)
    _on_route(whole, case['route'])
    for b in sorted(set([0, case['B'] // 2, case['B'] - 1])):
        one = _fwd(dev, N, c, i, sl=slice(b, b + 1))
        _on_route(one, case['route'])
        for name in ('y', 'yp'):
            if getattr(whole, name) is not None:
                assert torch.equal(getattr(one, name)[0].view(torch.int32), getattr(whole, name)[b].view(torch.int32)), \
                    (name, b, sk)


@pytest.mark.parametrize('splitk', [1, 3])
def test_small_grid_handed_true_maxima_equal_its_own_pass(dev, N, splitk):
    c = R._pwc('D', (8, 8), 5, 96, 64, splitk=splitk, bias=True)
    i = R.pw_inputs(_gen('handed', splitk), c)
    own = _fwd(dev, N, c, i)
    handed = _fwd(dev, N, c, i, handed=i['x'].abs().amax(dim=(1, 2, 3)))
    _on_route(own, 'D')
    _on_route(handed, 'D')
    assert torch.equal(own.y.view(torch.int32), handed.y.view(torch.int32))


FINISH_PAIRS = [R._pwc('A', (8, 8), 3, 160, 64, splitk=3, ws=True, **R.EPI[0]),
                R._pwc('A', (16, 16), 3, 160, 64, splitk=8, ws=True, **R.EPI[3]),
                R._pwc('A', (8, 8), 9, 160, 32, splitk=2, ws=True, res='ups', act=R.ACT_TANH, n_store=20),
                R._pwc('D', (8, 8), 3, 160, 64, splitk=8, **R.EPI[0]),
                R._pwc('D', (16, 16), 1, 96, 128, splitk=3, pro=R.PRO_AFFINE_RELU, mask=True)]


@pytest.mark.parametrize('case', FINISH_PAIRS, ids=R.pw_id)
def test_the_two_finish_kernels_agree_bit_for_bit(dev, N, case):
    i = R.pw_inputs(_gen('finish', R.pw_id(case)), case)
    v4, sc = _fwd(dev, N, case, i, finish='v4'), _fwd(dev, N, case, i, finish='scalar')
    for got in (v4, sc):
        _on_route(got, case['route'])
    for name in ('y', 'yp'):
        if getattr(v4, name) is not None:
            assert torch.equal(getattr(v4, name).view(torch.int32), getattr(sc, name).view(torch.int32)), name


AMAX_CASES = [R._pwc('A', (16, 16), 3, 96, 64, act=R.ACT_RELU, pool=R.POOL_MAX),                # one image per tile
              R._pwc('A', (8, 8), 3, 160, 64, splitk=3, ws=True, bias=True),                     # 16-byte finish
              R._pwc('A', (8, 8), 3, 160, 64, splitk=3, ws=True, bias=True, finish='scalar'),    # scalar finish
              R._pwc('B', (32, 32), 3, 64, 128, bias=True, pool=R.POOL_SUM),
              R._pwc('C', (32, 32), 3, 64, 64, amax='true', act=R.ACT_TANH),
              R._pwc('D', (16, 16), 3, 96, 64, bias=True),
              R._pwc('D', (8, 8), 3, 160, 64, splitk=3, bias=True)]


@pytest.mark.parametrize('nxt', [False, True], ids=['plain', 'next-affine'])
@pytest.mark.parametrize('case', AMAX_CASES, ids=R.pw_id)
def test_the_maxima_slots_hold_the_maximum_of_what_was_stored(dev, N, case, nxt):
    """the per-image maximum over the p2l_conv_amax_slots(d) slots == max |y| of the y the launch stored (outp: of
    yp); with next_s / next_t == max |y s + t|"""
    g = _gen('amax', R.pw_id(case))
    i = R.pw_inputs(g, case)
    B, ns = case['B'], case['n_store']
    st = None
    if nxt:
        st = (0.5 + torch.rand(B, ns, generator=g), randn(g, B, ns) * R.mags(B).view(B, 1))
    got = _fwd(dev, N, case, i, want_amax=True, next_st=st)
    _on_route(got, case['route'])
    assert not is_sentinel(got.amax) and bool((got.amax >= 0).all())
    if nxt:
        # (one rounding: the epilogue's t * s + t' is a fused multiply-add)
        once = R.fma(got.y, st[0][:, None, None], st[1][:, None, None]).abs().amax(dim=(1, 2, 3))
        assert torch.equal(got.amax.amax(dim=1), once)
    else:
        assert torch.equal(got.amax.amax(dim=1), got.y.abs().amax(dim=(1, 2, 3)))
    if got.amaxp is not None:
        assert torch.equal(got.amaxp.amax(dim=1), got.yp.abs().amax(dim=(1, 2, 3)))


# =====================================================================================================================
# fused input gradient
# =====================================================================================================================
def _arb(dev, N, c, i, finish='v4', tamper=None, splitk=None, ax=None, a_s=None, a_t=None):
    """one p2l_conv_dgrad_arb(_ws) launch of case c -> _Got: rc, dx, ds, dt and the profiler's figures"""
    lib = N.lib()
    B, H, W, Cin, Cout = c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    Ho, Wo = (H // 2, W // 2) if c['pool_sum'] else (H, W)
    wp = _weights(dev, N, i['w'], c['wfmt'])
    d = N.P2LConv()
    d.B, d.H, d.W, d.Cin, d.Cout, d.taps, d.ups = B, H, W, Cin, Cout, 1, 0
    d.x_ld, d.alpha, d.y_ld, d.yp_ld, d.n_store = Cin + 4, 1.0, Cout + 4, Cout + 4, Cout
    d.pool = R.POOL_SUM if c['pool_sum'] else R.POOL_NONE
    d.splitk = c['splitk'] if splitk is None else splitk
    d.wfmt, d.form, d.w_floats = c['wfmt'], 0, wp.numel()
    if finish == 'scalar':
        d.mask_ld = 1
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
    if c['amax']:
        hand = (R.pw_amax(c, i)[0].view(B, 1) * torch.tensor([0.5, 1.0, 0.25])).contiguous()
        a.amax.in_, a.amax.in_n = N.ptr(hand.to(dev)).value, 3
    dx = Out(dev, B * Ho * Wo * (Cout + 4))
    xd = _pitched(i['x'], Cin + 4, dev)
    need = lib.p2l_conv_workspace_bytes(C.byref(d))
    ws = Out(dev, max(need // 4, 1)) if c['ws'] and need else None

    def call():
        if ws is None:
            return lib.p2l_conv_dgrad_arb(C.byref(d), C.byref(a), N.ptr(xd), N.ptr(wp), N.ptr(dx.t), N.stream())
        return lib.p2l_conv_dgrad_arb_ws(C.byref(d), C.byref(a), N.ptr(xd), N.ptr(wp), N.ptr(dx.t), N.ptr(ws.t),
                                         C.c_size_t(ws.n * 4), N.stream())
    got = _Got()
    got.rc, got.ratio, got.count, got.fam = _profiled(N, call)
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


@pytest.mark.parametrize('case', R.PW_ARB_CASES, ids=R.arb_id)
@seeded
def test_dgrad_fused_affine_relu_bwd(dev, N, case):
    cid = R.arb_id(case)
    i = R.arb_inputs(_gen('arb', cid), case)
    got = _arb(dev, N, case, i)
    _on_route(got, case['route'], cid)
    r64, r32 = R.arb_refs(case, i)
    kdx, kds, kdt = R.arb_k(case)
    hold('%s:dx' % got.entry, cid, got.dx, r64['dx'], r64['den_dx'], r32['dx'], kdx)
    # ds, dt: on these signed operands inside the a-priori bound; held to their bar on the positive ones
    for name, bound in zip(('ds', 'dt'), R.arb_bound(case, r64, i['ax'])):
        err = (getattr(got, name).to(D64) - r64[name]).abs()
        print('%s %s: %.3f of the a-priori bound' % (cid, name, float((err / (bound * R.U).clamp_min(1e-300)).max())))
        assert bool((err <= bound * R.U).all()), name
    ip = R.arb_positive(i)
    pos = _arb(dev, N, case, ip)
    _on_route(pos, case['route'], cid)
    p64, p32 = R.arb_refs(case, ip)
    for name, k in (('ds', kds), ('dt', kdt)):
        hold('%s:%s' % (got.entry, name), cid, getattr(pos, name), p64[name], p64['den_' + name], p32[name], k)
    again = _arb(dev, N, case, i)
    for name in ('dx', 'ds', 'dt'):
        assert torch.equal(getattr(again, name).view(torch.int32), getattr(got, name).view(torch.int32)), name
    if not case['nomask'] and not case['skip']:
        dead = r64['g'] == 0                                               # (no shortcut: dx = g s, +0 where masked)
        assert bool((got.dx[dead] == 0).all())


MASK_ROUTES = [('A', 16, 1, 'v4'), ('B', 32, 1, 'v4'), ('D', 16, 1, 'v4'), ('A', 16, 2, 'v4'), ('A', 16, 2, 'scalar'),
               ('D', 16, 2, 'v4'), ('D', 16, 2, 'scalar')]


@pytest.mark.parametrize('route,H,splitk,finish', MASK_ROUTES, ids=lambda v: str(v))
def test_fused_backward_mask_is_the_forwards_decision(dev, N, route, H, splitk, finish):
    """{g != 0} of the fused dgrad epilogue and of either finish kernel -- read off dt with da = 1 through an identity
    weight, and off dx -- == {a > 0} of the forward's PRO_AFFINE_RELU prologue, read through the exact-fp32 kernel, on
    inputs where x s + t rounded once and rounded twice decide differently (_cancellation_case)"""
    Bn, Cc = 2, 64
    P = H * H
    eye = torch.eye(Cc)
    fc = R._pwc('A', (H, H), Bn, Cc, Cc, pro=R.PRO_AFFINE_RELU)
    ac = R._arbc(route, (H, H), Bn, Cc, Cc, splitk=splitk, ws=route == 'D' or splitk > 1, amax=None)
    for seed in range(5):
        x, s, t, once, twice, A, B = _cancellation_case(seed, Bn, P, Cc)
        fwd = _fwd(dev, N, fc, dict(x=x.view(Bn, H, H, Cc), w=eye, s=s, t=t))
        _on_route(fwd, 'A')
        live = fwd.y.view(Bn, P, Cc) > 0
        i = dict(x=torch.ones(Bn, H, H, Cc), w=eye, ax=x.view(Bn, H, H, Cc), **{'as': s, 'at': t})
        got = _arb(dev, N, ac, i, finish=finish)
        _on_route(got, route)
        bwd = got.dx.view(Bn, P, Cc) != 0
        print('%s splitk=%d %s seed=%d: forward == fma %s, == unfused %s; backward == fma %s, == unfused %s' % (
            route, splitk, finish, seed, torch.equal(live, once), torch.equal(live, twice), torch.equal(bwd, once),
            torch.equal(bwd, twice)))
        diff = live != bwd
        assert not bool(diff.any()), ('forward and backward decide differently', int(diff.sum()),
                                      int((diff & A).sum()), int((diff & B).sum()))
        assert torch.equal(got.dt, live.float().sum(1))                          # dt counts the live pixels (da = 1)


# =====================================================================================================================
# packers
# =====================================================================================================================
@pytest.mark.parametrize('flip', [0, 1])
@pytest.mark.parametrize('O,I,pad', [(40, 24, (64, 32)), (64, 48, (64, 48)), (96, 160, (96, 160))])
def test_packers_bit_for_bit(dev, N, O, I, pad, flip):
    """p2l_pack_conv_weight (taps 1) and p2l_pack_conv_weight_pw == the host packers written from the header: every
    word, the +0 padding, the tail; the buffer is exactly p2l_packed_weight_floats long, between guard bands"""
    lib = N.lib()
    N_pad, K_pad = (pad[0], pad[1]) if not flip else (-(-I // 32) * 32, -(-O // 16) * 16)
    for zero in (False, True):
        w = torch.zeros(O, I) if zero else randn(_gen('pack', O, I, flip), O, I) / 7
        m = w.t().contiguous() if flip else w                                     # the [N, K] matrix the launch applies
        wd = w.reshape(O, I, 1, 1).to(dev)
        n = lib.p2l_packed_weight_floats(1, N_pad, K_pad, 3)
        assert n == N_pad * K_pad * 7 // 2 + 4
        buf = Out(dev, n)
        N.check(lib.p2l_pack_conv_weight_pw(N.ptr(wd), O, I, N_pad, K_pad, flip, N.ptr(buf.t), N.stream()), 'pack_pw')
        got, want = buf.cpu().view(torch.int32), R.pack_pw(m, N_pad, K_pad)
        tot = N_pad * K_pad
        for name, lo, hi in (('fp32', 0, tot), ('bf16 x 3', tot, tot * 5 // 2), ('fp16 x 2', tot * 5 // 2, n - 4),
                             ('tail', n - 4, n)):
            assert torch.equal(got[lo:hi], want[lo:hi]), (name, int((got[lo:hi] != want[lo:hi]).sum()))
        assert got[n - 4:n - 3].view(torch.float32).item() == w.abs().max().item()
        assert lib.p2l_packed_weight_floats(1, N_pad, K_pad, 0) == tot
        b32 = Out(dev, tot)
        N.check(lib.p2l_pack_conv_weight(N.ptr(wd), O, I, 1, N_pad, K_pad, flip, N.ptr(b32.t), N.stream()), 'pack')
        assert torch.equal(b32.cpu().view(torch.int32), R.pack_f32(m, N_pad, K_pad).view(torch.int32))


# =====================================================================================================================
# arguments: refused before anything is launched, every output still sentinels
# =====================================================================================================================
def _set(**kw):
    def f(d, *rest):
        for k, v in kw.items():
            setattr(d, k, v)
    return f


ARG_BASE = R._pwc('A', (8, 8), 3, 160, 64, splitk=3, ws=True, bias=True, res='same', pro=R.PRO_AFFINE)


@pytest.mark.parametrize('what', ['w_floats', 'y_ld', 'yp_ld', 'res_ld', 'mask_ld', 'pro_bstride', 'workspace',
                                  'oscale_bstride', 'scalar-finish-oscale', 'scalar-finish-lrelu',
                                  'scalar-finish-oscale-small-grid'])
def test_forward_arguments_are_refused_before_the_launch(dev, N, what):
    lib = N.lib()
    c, kw, want = dict(ARG_BASE), {}, EINVAL
    if what == 'w_floats':
        kw['tamper'] = _set(w_floats=lib.p2l_packed_weight_floats(1, 64, 160, 0) - 1)
    elif what == 'y_ld':
        kw['tamper'] = _set(y_ld=60)
    elif what == 'yp_ld':
        c.update(pool=R.POOL_MAX)
        kw['tamper'] = _set(yp_ld=60)
    elif what == 'res_ld':
        kw['tamper'] = _set(res_ld=60)
    elif what == 'mask_ld':
        c.update(mask=True)
        kw['tamper'] = _set(mask_ld=32)
    elif what == 'pro_bstride':
        kw['tamper'] = _set(pro_bstride=156)
    elif what == 'workspace':
        kw['ws_short'], want = 4, EWS
    elif what == 'oscale_bstride':
        c.update(oscale=True)
        kw['ex_tamper'] = lambda ex: setattr(ex, 'oscale_bstride', 32)
    elif what == 'scalar-finish-oscale':
        c.update(oscale=True, noise=True, finish='scalar')
        want = EUNSUP
    elif what == 'scalar-finish-oscale-small-grid':
        c = R._pwc('D', (8, 8), 3, 160, 64, splitk=3, finish='scalar', **R.EPI[6])
        want = EUNSUP
    elif what == 'scalar-finish-lrelu':
        c.update(act=R.ACT_LRELU_SQRT2, finish='scalar')
        want = EUNSUP
    i = R.pw_inputs(_gen('args', what), c)
    got = _fwd(dev, N, c, i, **kw)
    assert got.rc == want, (what, got.rc)
    assert got.count == (0, 0) and _untouched(got)
    ok = _fwd(dev, N, dict(c, finish='v4'), i)                                  # ... and the launch itself is a good one
    assert ok.rc == 0


@pytest.mark.parametrize('what', ['multi-image-tile', 'x_ld', 'st_bstride', 'skip_ld', 'skip_C', 'dx_ld', 'ds-null',
                                  'dt-null', 'dsdt_bstride', 'dsdt_bstride-odd', 'split-x_ld-odd', 'split-skip_ld-odd'])
def test_dgrad_arguments_are_refused_before_the_launch(dev, N, what):
    c, want, tamper = R._arbc('A', (8, 16), 2, 96, 64, skip='same'), EINVAL, None
    if what == 'multi-image-tile':
        c, want = R._arbc('A', (8, 8), 3, 96, 64), EUNSUP                        # two images per tile, no K slices
    elif what == 'x_ld':
        def tamper(d, a):
            a.x_ld = 60
    elif what == 'st_bstride':
        def tamper(d, a):
            a.st_bstride = 32
    elif what == 'skip_ld':
        def tamper(d, a):
            a.skip_ld = 28
    elif what == 'skip_C':
        def tamper(d, a):
            a.skip_C = 68
    elif what == 'dx_ld':
        def tamper(d, a):
            d.y_ld = 60
    elif what == 'ds-null':
        def tamper(d, a):
            a.ds = None
    elif what == 'dt-null':
        def tamper(d, a):
            a.dt = None
    elif what == 'dsdt_bstride':
        def tamper(d, a):
            a.dsdt_bstride = 60
    elif what == 'dsdt_bstride-odd':
        def tamper(d, a):
            a.dsdt_bstride = 66
    elif what.startswith('split-'):                                             # K slices, the 16-byte finish kernel
        c = R._arbc('A', (8, 8), 3, 160, 64, splitk=3, ws=True, skip='same')

        def tamper(d, a):
            setattr(a, what[6:-4], 70)
    got = _arb(dev, N, c, R.arb_inputs(_gen('arbargs', what), c), tamper=tamper)
    assert got.rc == want, (what, got.rc)
    assert got.count == (0, 0) and _untouched(got)

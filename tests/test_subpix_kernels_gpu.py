"""The sub-pixel 3x3 routes (taps = 9, ups 2 / 3, ext 0 / 1) -- F: conv_mfma_kernel<4, .., BF3 = false> (P2L_WFMT_F32,
csrc/p2l_conv.hip); B: the same kernel in bf16 x 3 (P2L_WFMT_BF16X3; P2L_WFMT_BF16X3W kept on it with P2L_FORM_WINO_BF3
or by withholding the 256 B per image of workspace); H: conv_h2_kernel<4, ..> (fp16 x 2, csrc/p2l_h2.hip), maxima from
the pass in front, handed over, handed over with in_applied, with and without the skipped taps of ext = 1; P:
conv_h2_kernel<8, ..>, two output phases per block (P2L_FORM_SP_PAIR, or by the launcher's own rule); and the two
split-K finish kernels behind H for ups = 3, ext = 1 -- forward, input gradient and fused input gradient, against the
float64 references of tests/_small_refs.py, through ctypes, with the harness, the metric and the bars of
tests/test_small_kernels_gpu.py (tests/_pin.py):

    p2l_conv_fwd, p2l_conv_fwd_ex, p2l_conv_dgrad_arb, p2l_conv_dgrad_arb_ws, p2l_pack_conv_weight_subpix,
    p2l_pack_conv_weight_subpix_bf3, p2l_pack_conv_weight_subpix_h2, p2l_packed_subpix_weight_floats,
    p2l_conv_amax_slots, p2l_conv_suggest_splitk, p2l_conv_workspace_bytes, p2l_conv_arb_nblk, p2l_conv_arb_nblk_ws.

Every case proves its route under the launch profiler: one 3x3 launch, 2 B H W Cin Cout 4 executed products on the
high-resolution dims of the descriptor, 16 / 6 / 3 MFMA products per fp32 product and the family (OTHER, SUBPIX_H2); a
case the dispatch moves elsewhere fails.  (The profiler cannot tell P from H: both are SUBPIX_H2 at three products.  P
cases state the condition under which the launcher pairs the phases; that the two are the same bits is tested at
every forward case.)  Rounded outputs are held to |got - r64| / den <= min(k, 4 x the route's fp32 restatement) x 2^-24
with den = sum |a| |w| over the ORIGINAL 3x3 taps that reach the output, through the epilogue (H, P: plus
subpix_h2_floor) and k counted in _small_refs.subpix_k; each B / H / P case records the figure of the same inputs on
route F next to its own.  What the contract calls exact is compared bit for bit; so are one-hot power-of-two inputs,
original tap by original tap.  Every output sits between guard bands, every pitch is above its row with junk (inputs)
or sentinels (outputs) in the gap.  P2L_SUBPIX_ERR_FILE=<path> records the figures (profiles/subpix_kernels_err.txt).
The cases, their inputs and k live in tests/_small_refs.py; tests/test_small_refs.py holds them to "the restatement
is within k / 4" on the host."""
import ctypes as C

import pytest
import torch

import _small_refs as R
from _pin import (D64, G, N, SENT, Out, _gen, _record_file, hold, hold_k, is_sentinel, note, randn,  # noqa: F401
                  seeded)

pytestmark = pytest.mark.gpu
EINVAL, EWS, EUNSUP = -1, -3, -4
FAM = {'F': 0, 'B': 0, 'H': 3, 'P': 3}
PRODUCTS = {'F': 16.0, 'B': 6.0, 'H': 3.0, 'P': 3.0}


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
    """one 3x3 launch, the route's products per fp32 product, its family, four phase-taps per high-resolution pixel"""
    want = 2.0 * got.B * c['H'] * c['W'] * c['Cin'] * c['Cout'] * 4
    assert got.rc == 0, (what, got.rc)
    assert got.count == (1, 0), (what, got.count)
    assert abs(got.ratio - PRODUCTS[route]) < 1e-6, '%s: expected route %s, got %g products' % (what, route, got.ratio)
    assert got.fam[FAM[route]] == 1 and sum(got.fam) == 1, (what, route, got.fam)
    assert abs(got.exec_flops - want) <= 1e-9 * want, (what, route, got.exec_flops, want)


def _weights(dev, N, i, c, route):
    """the packed sub-pixel buffer of the case's forward weight for the route's format: mode = ext, and through
    transpose_flip for the input gradient"""
    wfmt = R.subpix_form(c, route)[0]
    cache = i.setdefault('_packed', {})
    key = (id(i['w']), wfmt, c['ups'], c['ext'])
    if key not in cache:
        cache[key] = (i['w'], N.pack_conv_weight(i['w'].to(dev), 9, c['Cout'], c['Cin'], c['ups'] == 3, wfmt,
                                                 subpix_mode=c['ext']))
    return cache[key][1]


def _desc(N, c, route, B):
    d = N.P2LConv()
    d.B, d.H, d.W, d.Cin, d.Cout, d.taps, d.ups, d.ext = B, c['H'], c['W'], c['Cin'], c['Cout'], 9, c['ups'], c['ext']
    d.x_ld, d.alpha, d.splitk = c['Cin'] + 4, c['alpha'], c['splitk']
    d.wfmt, d.form, _ = R.subpix_form(c, route)
    return d


def _out_hw(c):
    """rows and columns of the buffer the launch writes"""
    if c['ups'] == 3:
        return c['H'] // 2, c['W'] // 2
    return c['H'] + 2 * c['ext'], c['W'] + 2 * c['ext']


def _fwd(dev, N, c, i, route=None, sl=None, handed='case', want_amax=False, next_st=None, tamper=None, ws_short=0,
         finish=None, no_ws=False, slot_ptrs=False):
    """one p2l_conv_fwd(_ex) launch of case c (ups 2 or 3) on inputs i (images sl) on `route` (default: the case's)
    -> _Got: rc, y [B, rows, cols, n_store], the profiler's figures, the maxima slots.  Everything the launch may
    write is an Out; the gap columns are checked here.  slot_ptrs: a maxima buffer is handed over even where
    p2l_conv_amax_slots answers 0 (it must stay untouched)"""
    lib = N.lib()
    route = route or c['route']
    sl = slice(0, c['B']) if sl is None else sl
    B, Cin, Cout, ns = sl.stop - sl.start, c['Cin'], c['Cout'], c['n_store']
    oh, ow = _out_hw(c)
    wp = _weights(dev, N, i, c, route)
    d = _desc(N, c, route, B)
    d.pro, d.act, d.pool = c['pro'], c['act'], R.POOL_NONE
    d.y_ld = d.yp_ld = ns + 4
    d.n_store, d.w_floats = ns, wp.numel()
    xd = _pitched(i['x'][sl], Cin + 4, dev)
    sd = td = resd = maskd = None
    if c['pro'] != R.PRO_NONE:
        d.pro_bstride = Cin + 4 if c['pro_b'] else 0
        rows = sl if c['pro_b'] else slice(0, 1)
        sd, td = _pitched(i['s'][rows], Cin + 4, dev, -5.0), _pitched(i['t'][rows], Cin + 4, dev, 9.0)
    if c['res']:
        d.res_ld = ns + 8
        resd = _pitched(i['res'][sl], d.res_ld, dev, 3.0)
    if c['mask']:
        d.mask_ld = ns + 12
        maskd = _pitched(i['mask'][sl], d.mask_ld, dev, 1.0)
    if (finish or c['finish']) == 'scalar':
        d.yp_ld = 1                    # a pitch of the ABSENT pooled output that is no multiple of four
    y = Out(dev, B * oh * ow * (ns + 4))
    biasd = i['bias'].to(dev) if c['bias'] else None
    h2 = route in 'HP'
    hand = (R.pw_amax(c, i)[0] if c['amax'] and h2 else None) if isinstance(handed, str) else handed
    ex = None
    if c['oscale'] or c['noise'] or hand is not None or want_amax or slot_ptrs:
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
    slots = lib.p2l_conv_amax_slots(C.byref(d)) if (want_amax or slot_ptrs) else 0
    am = None
    if (want_amax and slots > 0) or slot_ptrs:
        am = Out(dev, B * slots + 16)                 # (16 floats no launch was promised, behind the slots)
        ex.amax.out = N.ptr(am.t).value
        if next_st is not None:
            ex.amax.next_s, ex.amax.next_t = N.ptr(next_st[0].to(dev)).value, N.ptr(next_st[1].to(dev)).value
            ex.amax.next_bstride = next_st[0].shape[1]
    need = lib.p2l_conv_workspace_bytes(C.byref(d))
    assert tamper is not None or (need > 0) == (d.wfmt == R.WFMT_BF16X3W and not d.form & R.FORM_WINO_BF3 or d.splitk > 1), \
        (route, need)
    use_ws = R.subpix_form(c, route)[2] and not no_ws
    ws = Out(dev, max((need - ws_short) // 4, 1)) if need and use_ws else None
    wsp, wsb = (N.ptr(ws.t), C.c_size_t(ws.n * 4)) if ws is not None else (None, C.c_size_t(0))

    def call():
        args = (N.ptr(xd), N.ptr(wp), N.ptr(biasd), N.ptr(sd), N.ptr(td), N.ptr(resd), N.ptr(maskd),
                N.ptr(y.t), None, wsp, wsb, N.stream())
        if ex is None:
            return lib.p2l_conv_fwd(C.byref(d), *args)
        return lib.p2l_conv_fwd_ex(C.byref(d), C.byref(ex), *args)
    got = _Got()
    got.B = B
    got.rc, got.ratio, got.exec_flops, got.count, got.fam = _profiled(N, call)
    got.ex, got.slots, got.outs = ex is not None, slots, [o for o in (y, am) if o is not None]
    got.amax = None
    if ws is not None:
        ws.cpu()                                                        # (its guard bands)
    full = y.cpu(B, oh, ow, ns + 4)
    assert got.rc != 0 or is_sentinel(full[..., ns:]), 'gap columns of y written'
    got.y = full[..., :ns].contiguous()
    if am is not None:
        flat = am.cpu()
        got.amax, got.amax_tail = flat[:B * slots].view(B, slots), flat[B * slots:]
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


def _pinned(dev, N, case, i, cid, tag):
    """the launch of a forward-style case (ups 2 or 3) held to its bar, its twin on route F recorded, and the forms
    that must agree with it bit for bit: a repeated launch; H = P (P2L_FORM_NO_SP_PAIR against P2L_FORM_SP_PAIR) at
    every ups = 2 case of either; the skipped taps of ext = 1 against P2L_FORM_NO_SP_SKIP; the two finish kernels"""
    got = _fwd(dev, N, case, i)
    _on_route(got, case, case['route'], cid)
    r64, r32 = R.subpix_refs(case, i)
    hold('%s:y' % _entry(got), cid, got.y, r64['y'], r64['den'], r32['y'], R.subpix_k(case))
    if case['route'] != 'F':
        one = dict(case, splitk=1)                                  # (route F never takes K slices)
        twin = _fwd(dev, N, one, i, route='F')
        _on_route(twin, case, 'F', cid + ' on F')
        f64 = R.subpix_refs(one, i, 'F', restate=False)[0] if case['route'] in 'HP' else r64
        note('%s:y' % _entry(twin), cid + ' on F', twin.y, f64['y'], f64['den'])
    _same_bits(_fwd(dev, N, case, i), got, ('y',), cid + ' repeated')
    if case['route'] in 'HP':
        if case['ups'] == 2:
            other = 'P' if case['route'] == 'H' else 'H'
            alt = _fwd(dev, N, dict(case, pair='form'), i, route=other)
            _on_route(alt, case, other, cid + ' on ' + other)
            _same_bits(alt, got, ('y',), cid + ': P vs H')
        if case['ext']:
            alt = _fwd(dev, N, dict(case, skip=not case['skip']), i)
            _on_route(alt, case, case['route'], cid + ' other skip form')
            _same_bits(alt, got, ('y',), cid + ': skipped taps vs P2L_FORM_NO_SP_SKIP')
    if len(R.subpix_slices(case)) > 1:
        alt = _fwd(dev, N, case, i, finish='scalar' if case['finish'] == 'v4' else 'v4')
        _on_route(alt, case, case['route'], cid + ' other finish')
        _same_bits(alt, got, ('y',), cid + ': the two finish kernels')
    return got, r64


# =====================================================================================================================
# forward (ups = 2): every route, both geometries, every epilogue term of the mode
# =====================================================================================================================
@pytest.mark.parametrize('case', R.SUBPIX_FWD_CASES, ids=R.subpix_id)
@seeded
def test_forward(dev, N, case):
    cid = R.subpix_id(case)
    i = R.subpix_inputs(_gen('subpix', cid), case)
    got, r64 = _pinned(dev, N, case, i, cid, 'fwd')
    if case['ext'] and not (case['bias'] or case['noise']):
        # row and column H+1 of the frame: written, and +0 (sentinels before the launch)
        H, W = case['H'], case['W']
        bits = got.y.view(torch.int32)
        assert bool((bits[:, H + 1] == 0).all()) and bool((bits[:, :, W + 1] == 0).all())
    if case['route'] in 'HP' and case['B'] >= 3 and case['pro'] == R.PRO_NONE and not (case['bias'] or case['noise']):
        assert bool((got.y[1] == 0).all())                              # the all-zero image


def test_the_frame_of_a_transposed_conv(dev, N):
    """ups = 2, ext = 1 on the plan's launch (PRO_AFFINE per image, t = 0) on every route at the 5x5, 9x9, 17x17 and
    9x17 grids: over sentinels, row and column H+1 of every image are written +0, rows / columns 0 .. H are all
    written, the gap columns and the guard bands keep their sentinels (_fwd, Out.cpu)"""
    for name in ('8x8', '16x16', '32x32', '16x32'):
        for route in 'FBHP':
            c = R._ssh(route, 2, 1, name, pro=R.PRO_AFFINE, t0=True)
            i = R.subpix_inputs(_gen('frame', name), c)
            got = _fwd(dev, N, c, i)
            _on_route(got, c, route, R.subpix_id(c))
            bits = got.y.view(torch.int32)
            assert bool((bits[:, c['H'] + 1] == 0).all()) and bool((bits[:, :, c['W'] + 1] == 0).all()), (name, route)
            assert not bool((bits == SENT).any()), (name, route)
            want = R.subpix_refs(c, i, restate=False)[0]['y']
            assert bool(((want != 0) == (got.y != 0))[:, :c['H'] + 1, :c['W'] + 1].all()), (name, route)


# =====================================================================================================================
# input gradient (ups = 3): plain, residual and mask, activations, K slices through both finish kernels
# =====================================================================================================================
@pytest.mark.parametrize('case', R.SUBPIX_BWD_CASES, ids=R.subpix_id)
@seeded
def test_gradient(dev, N, case):
    cid = R.subpix_id(case)
    i = R.subpix_inputs(_gen('subpix', cid), case)
    got, r64 = _pinned(dev, N, case, i, cid, 'bwd')
    if case['mask']:
        dead = ~(i['mask'][..., :case['n_store']] > 0)
        assert bool(dead.any()) and bool((got.y.view(torch.int32)[dead] == 0).all())
    if case['route'] == 'H' and case['B'] >= 3 and not case['res']:
        assert bool((got.y[1] == 0).all())                              # the all-zero image


def test_slice_counts_and_channel_tiles_of_the_shapes(dev, N):
    """p2l_conv_suggest_splitk of a ups = 3, ext = 1 fp16 x 2 launch: Cin 128 at 16x16 -> 4 slices, Cin 256 at 16x16 ->
    8, Cin 256 at 32x32 -> 4, Cin 64 -> none, for B = 1, 3, 9 alike and equal to the host restatement of
    subpix_bwd_split; never on F, B, on ext = 0 or on ups = 2.  The maxima slots tell the tile: ups = 2 promises four
    phases' worth, 32-channel tiles below n64 = 256 and 64-channel ones at the bn64 shape; ups = 3 unsliced one
    phase's; a partial ext = 1 forward, a multi-image tile and a sliced gradient none"""
    lib = N.lib()
    for (H, Cin, Cout), sk in (((16, 128, 64), 4), ((16, 256, 32), 8), ((32, 256, 32), 4), ((16, 64, 64), 1)):
        assert R.subpix_bwd_split(H, H, Cin, Cout) == sk
        for B in (1, 3, 9):
            for route, ups, ext, want in (('H', 3, 1, sk), ('F', 3, 1, 1), ('B', 3, 1, 1), ('H', 3, 0, 1), ('H', 2, 1, 1),
                                          ('P', 2, 0, 1)):
                c = R._sc(route, ups, ext, (H, H), B, Cin, Cout)
                d = _desc(N, c, route, B)
                d.y_ld = d.n_store = Cout
                assert lib.p2l_conv_suggest_splitk(C.byref(d)) == want, (H, Cin, route, ups, ext, B)
    for c, want in ((R._ssh('F', 2, 0, '16x32'), 1 * 1 * 4 * 4), (R._ssh('H', 2, 0, '32x32'), 2 * 2 * 4 * 4),
                    (R._ssh('P', 2, 0, 'bn64'), 1 * 4 * 4 * 4), (R._ssh('H', 2, 0, '16x64'), 2 * 3 * 4 * 4),
                    (R._ssh('H', 3, 0, '16x32'), 1 * 1 * 4), (R._ssh('B', 3, 1, '32x32'), 2 * 2 * 4),
                    (R._ssh('H', 3, 0, 'bn64g'), 1 * 4 * 4),
                    (R._ssh('H', 2, 1, '16x32'), 0), (R._ssh('H', 2, 0, '8x8'), 0), (R._ssh('H', 3, 1, 's4', splitk=4), 0)):
        d = _desc(N, c, c['route'], c['B'])
        d.y_ld = d.n_store = c['Cout']
        assert lib.p2l_conv_amax_slots(C.byref(d)) == want, R.subpix_id(c)


# =====================================================================================================================
# exact inputs: the four tap tables and the phase / plane addressing, element by element
# =====================================================================================================================
ONEHOT = [R._ssh('F', 2, 0, '32x32'), R._ssh('B', 2, 0, '16x64'), R._ssh('H', 2, 0, '8x8'), R._ssh('P', 2, 0, '32x32'),
          R._ssh('H', 2, 0, '4x4'), R._ssh('F', 2, 1, '8x8'), R._ssh('B', 2, 1, '16x16', wfmt='bf3w'), R._ssh('H', 2, 1, '32x32'),
          R._ssh('P', 2, 1, '16x32'), R._ssh('P', 2, 1, '8x8'), R._ssh('H', 2, 1, '4x4', skip=False),
          R._ssh('F', 3, 0, '32x32'), R._ssh('B', 3, 0, '8x8'), R._ssh('H', 3, 0, '16x64'), R._ssh('H', 3, 0, '4x4'),
          R._ssh('F', 3, 1, '16x16'), R._ssh('B', 3, 1, '32x32', wfmt='nows'), R._ssh('H', 3, 1, '32x32'), R._ssh('H', 3, 1, '8x8b9'),
          R._ssh('H', 3, 1, 's4', splitk=4), R._ssh('H', 3, 1, 's8', splitk=8, finish='scalar'),
          R._ssh('H', 3, 1, 's4w', splitk=4, skip=False),
          R._ssh('H', 3, 1, '16x64'), R._ssh('B', 3, 1, '16x64')]


@pytest.mark.parametrize('tap', range(9))
def test_one_hot_inputs_are_exact(dev, N, tap):
    """single power-of-two pixels at the corners, both sides of every tile seam, the last grid row / column of an ext =
    1 forward, row H of an ext = 1 frame and the first pixel of the second image of a multi-image tile; a single
    power-of-two weight on ONE original tap: every route gives the fp64 result of the definition (subpix_map) bit for
    bit, forward and gradient (through transpose_flip), in both modes and in K slices"""
    for c in ONEHOT:
        i = R.subpix_onehot(c, tap, tap % 2)
        got = _fwd(dev, N, c, i)
        _on_route(got, c, c['route'], R.subpix_id(c))
        want = R.subpix_map(i['x'].double(), i['w'].double(), c['ups'], c['ext'])
        assert int((want != 0).sum()) >= 3, R.subpix_id(c)
        assert torch.equal(got.y.double(), want), (R.subpix_id(c), tap, int((got.y.double() != want).sum()))


def test_all_zero_inputs_give_exactly_zero(dev, N):
    for c in (R._ssh('F', 2, 0, '16x32'), R._ssh('B', 2, 1, '8x8'), R._ssh('H', 2, 1, '16x16'), R._ssh('P', 2, 0, '8x8'),
              R._ssh('H', 3, 0, '16x32'), R._ssh('H', 3, 1, 's4', splitk=4)):
        i = R.subpix_inputs(_gen('zero', R.subpix_id(c)), c)
        i['x'] = torch.zeros_like(i['x'])
        got = _fwd(dev, N, c, i)
        _on_route(got, c, c['route'])
        assert bool((got.y.view(torch.int32) == 0).all()), R.subpix_id(c)


# =====================================================================================================================
# bit-exact contracts
# =====================================================================================================================
ALONE = [R._ssh('F', 2, 0, '8x8', bias=True), R._ssh('B', 2, 1, '8x8', pro=R.PRO_AFFINE), R._ssh('H', 2, 0, '8x8b9', bias=True),
         R._ssh('H', 2, 1, '8x8', pro=R.PRO_AFFINE), R._ssh('P', 2, 1, '8x8b9', pro=R.PRO_AFFINE_RELU),
         R._ssh('P', 2, 0, '16x16', amax='raw', pro=R.PRO_AFFINE_RELU), R._ssh('H', 2, 1, '4x4', bias=True),
         R._ssh('P', 2, 1, 'bn64e', pair='own', pro=R.PRO_AFFINE, t0=True),
         R._ssh('F', 3, 0, '8x8', act=R.ACT_TANH), R._ssh('B', 3, 1, '8x8b9', wfmt='bf3w'), R._ssh('H', 3, 0, '16x16', res='same'),
         R._ssh('H', 3, 1, '8x8b9', act=R.ACT_RELU), R._ssh('H', 3, 1, 's4', splitk=4, res='same', mask=True),
         R._ssh('H', 3, 1, '4x4')]


@pytest.mark.parametrize('neighbour', ['drawn', 'zero', 'huge'])
@pytest.mark.parametrize('case', ALONE, ids=R.subpix_id)
def test_an_image_alone_has_the_bits_it_has_in_any_batch(dev, N, case, neighbour):
    """... with the same splitk, on every route: in the multi-image (and, ext = 1 forward, partial) tiles of the 4x4,
    5x5 and 8x8 grids, where images share a staged patch and a tile of accumulators -- also when every other image of
    the batch is all zero or 1e14 times larger (fp16 x 2: each image is un-scaled by its own power of two).  At the
    bn64e shape the batch of eight runs 64-channel tiles with the phases paired (TAPS = 8) and the image alone, n64 =
    32, 32-channel tiles with one phase per block: the comparison is P at BN = 64 against H at BN = 32"""
    i = R.subpix_inputs(_gen('alone', R.subpix_id(case)), case)
    B = case['B']
    mid = B // 2
    if not bool(i['x'][mid].any()):                  # (the all-zero image of the fp16 x 2 draws)
        i['x'] = i['x'].clone()
        i['x'][mid] = i['x'][0] * 1e3
    if neighbour != 'drawn':
        f = torch.full((B,), 0.0 if neighbour == 'zero' else 1e14)
        f[mid] = 1.0
        i['x'] = i['x'] / i['x'].abs().amax(dim=(1, 2, 3)).clamp_min(1e-30).view(B, 1, 1, 1)
        i = dict(i, x=i['x'] * f.view(B, 1, 1, 1))
    whole = _fwd(dev, N, case, i)
    _on_route(whole, case, case['route'])
    for b in sorted(set([0, mid, B - 1])) if neighbour == 'drawn' else [mid]:
        one = _fwd(dev, N, case, i, sl=slice(b, b + 1))
        _on_route(one, case, case['route'])
        assert torch.equal(one.y[0].view(torch.int32), whole.y[b].view(torch.int32)), (neighbour, b)
    assert bool((whole.y[mid] != 0).any())


@pytest.mark.parametrize('case', [R._ssh('H', 2, 0, '16x32', bias=True), R._ssh('P', 2, 1, '16x16', bias=True),
                                  R._ssh('H', 2, 1, '8x8', act=R.ACT_RELU), R._ssh('H', 3, 0, '32x32'),
                                  R._ssh('H', 3, 1, '8x8b9', act=R.ACT_TANH), R._ssh('H', 3, 1, 's8', splitk=8)],
                         ids=R.subpix_id)
def test_handed_true_maxima_equal_the_pass_in_front(dev, N, case):
    """a consumer without a prologue: the same bits with handed-over maxima as with its own max-|x| pass (ups = 3: over
    the high-resolution frame)"""
    i = R.subpix_inputs(_gen('handed', R.subpix_id(case)), case)
    own = _fwd(dev, N, case, i)
    handed = _fwd(dev, N, case, i, handed=i['x'].abs().amax(dim=(1, 2, 3)))
    for got in (own, handed):
        _on_route(got, case, case['route'])
    _same_bits(own, handed, ('y',))


AMAX_CASES = [R._ssh('F', 2, 0, '16x32', bias=True), R._ssh('B', 2, 0, '32x32', act=R.ACT_RELU, n_store=48),
              R._ssh('H', 2, 0, '16x64', bias=True), R._ssh('P', 2, 0, '32x32', pro=R.PRO_AFFINE_RELU),
              R._ssh('P', 2, 0, 'bn64', bias=True), R._ssh('F', 3, 0, '16x32'), R._ssh('B', 3, 1, '32x32', act=R.ACT_TANH),
              R._ssh('H', 3, 1, '16x32', res='same'), R._ssh('H', 3, 0, '16x64', n_store=48)]


@pytest.mark.parametrize('nxt', [False, True], ids=['plain', 'next-affine'])
@pytest.mark.parametrize('case', AMAX_CASES, ids=R.subpix_id)
def test_the_maxima_slots_hold_the_maximum_of_what_was_stored(dev, N, case, nxt):
    """every slot p2l_conv_amax_slots(d) promises is written -- ups = 2, ext = 0: four phases' worth, ups = 3 unsliced:
    one -- and the per-image maximum over them == max |y| of the y the launch stored; with next_s / next_t == max
    |fma(y, s, t)|.  The slot buffers sit between guard bands: no slot beyond the promised ones is written"""
    g = _gen('amax', R.subpix_id(case))
    i = R.subpix_inputs(g, case)
    B, ns = case['B'], case['n_store']
    st = (0.5 + torch.rand(B, ns, generator=g), randn(g, B, ns) * R.mags(B).view(B, 1)) if nxt else None
    got = _fwd(dev, N, case, i, want_amax=True, next_st=st)
    _on_route(got, case, case['route'])
    (gh, gw), (TW, TH, TB) = R.subpix_grid(case)
    assert TB == 1 and gh % TH == 0 and gw % TW == 0
    bn = 64 if case is AMAX_CASES[4] else 32
    assert got.slots == (gh // TH) * (gw // TW) * (case['Cout'] // bn) * (4 if case['ups'] == 2 else 1) * 4
    slots = got.amax
    assert bool((slots.view(torch.int32) != SENT).all()) and bool((slots >= 0).all())
    assert is_sentinel(got.amax_tail)
    assert torch.equal(slots.amax(dim=1), R.producer_amax(got.y, *st) if nxt else R.producer_amax(got.y))


@pytest.mark.parametrize('case', [R._ssh('H', 2, 1, '16x32'), R._ssh('P', 2, 1, '8x8'), R._ssh('F', 2, 0, '8x8'),
                                  R._ssh('H', 3, 1, 's4', splitk=4), R._ssh('B', 3, 0, '8x8')], ids=R.subpix_id)
def test_no_slot_is_written_where_none_is_promised(dev, N, case):
    """a partial ext = 1 forward, a multi-image tile, a sliced gradient: p2l_conv_amax_slots answers 0 and a launch that
    is handed slot pointers all the same writes none"""
    i = R.subpix_inputs(_gen('noslots', R.subpix_id(case)), case)
    got = _fwd(dev, N, case, i, slot_ptrs=True)
    _on_route(got, case, case['route'])
    assert got.slots == 0 and is_sentinel(got.amax_tail)
    _same_bits(_fwd(dev, N, case, i), got, ('y',))


# =====================================================================================================================
# fused input gradient
# =====================================================================================================================
def _arb(dev, N, c, i, route=None, tamper=None, no_ws=False):
    """one p2l_conv_dgrad_arb(_ws) launch of a ups = 3 case -> _Got: rc, dx, ds, dt, the profiler's figures"""
    lib = N.lib()
    route = route or c['route']
    B, H, W, Cin, Cout = c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    Ho, Wo = H // 2, W // 2
    wp = _weights(dev, N, i, c, route)
    d = _desc(N, c, route, B)
    d.alpha, d.y_ld, d.yp_ld, d.n_store, d.w_floats = 1.0, Cout + 4, Cout + 4, Cout, wp.numel()
    if c['finish'] == 'scalar':
        d.mask_ld = 1
    a = N.P2LArb()
    a.x, a.x_ld = N.ptr(_pitched(i['ax'], Cout + 8, dev)).value, Cout + 8
    a.s = N.ptr(_pitched(i['as'], Cout + 4, dev, -5.0)).value
    a.t = N.ptr(_pitched(i['at'], Cout + 4, dev, 9.0)).value
    a.st_bstride, a.nomask = Cout + 4, int(c['nomask'])
    if c['skip_g']:
        a.skip, a.skip_ld = N.ptr(_pitched(i['skip'], Cout + 12, dev, 3.0)).value, Cout + 12
        a.skip_C, a.skip_ups = Cout // 2, int(c['skip_g'] == 'ups')
    ds, dt = Out(dev, B * (Cout + 4)), Out(dev, B * (Cout + 4))
    a.ds, a.dt, a.dsdt_bstride = N.ptr(ds.t).value, N.ptr(dt.t).value, Cout + 4
    if tamper is not None:
        tamper(d, a)
    nblk = max(lib.p2l_conv_arb_nblk_ws(C.byref(d)), lib.p2l_conv_arb_nblk(C.byref(d)), 1)
    part = Out(dev, 2 * B * nblk * Cout)
    a.partial = N.ptr(part.t).value
    if c['amax'] and route in 'HP':
        hand = (R.pw_amax(c, i)[0].view(B, 1) * torch.tensor([0.5, 1.0, 0.25])).contiguous()
        a.amax.in_, a.amax.in_n = N.ptr(hand.to(dev)).value, 3
    am = None
    if c['amax_out']:
        got_slots = lib.p2l_conv_amax_slots(C.byref(d))
        assert got_slots > 0
        am = Out(dev, B * got_slots)
        a.amax.out = N.ptr(am.t).value
    dx = Out(dev, B * Ho * Wo * (Cout + 4))
    xd = _pitched(i['x'], Cin + 4, dev)
    need = lib.p2l_conv_workspace_bytes(C.byref(d))
    use_ws = R.subpix_form(c, route)[2] and not no_ws
    ws = Out(dev, need // 4) if need and use_ws else None
    wsp, wsb = (N.ptr(ws.t), C.c_size_t(ws.n * 4)) if ws is not None else (None, C.c_size_t(0))

    def call():
        if ws is None and not no_ws:
            return lib.p2l_conv_dgrad_arb(C.byref(d), C.byref(a), N.ptr(xd), N.ptr(wp), N.ptr(dx.t), N.stream())
        return lib.p2l_conv_dgrad_arb_ws(C.byref(d), C.byref(a), N.ptr(xd), N.ptr(wp), N.ptr(dx.t), wsp, wsb, N.stream())
    got = _Got()
    got.B, got.nblk = B, nblk
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


@pytest.mark.parametrize('case', R.SUBPIX_ARB_CASES, ids=R.subpix_arb_id)
@seeded
def test_dgrad_fused_affine_relu_bwd(dev, N, case):
    """p2l_conv_dgrad_arb(_ws) on the sub-pixel gradient: arb_epilogue on the LOW-resolution result; a sliced launch
    sizes its partials by p2l_conv_arb_nblk_ws (one per quad of the low-resolution grid) and may span images"""
    cid = R.subpix_arb_id(case)
    i = R.subpix_arb_inputs(_gen('sarb', cid), case)
    got = _arb(dev, N, case, i)
    _on_route(got, case, case['route'], cid)
    if len(R.subpix_slices(case)) > 1:
        assert got.nblk == (case['H'] // 4) * (case['W'] // 4)
    r64, r32 = R.subpix_arb_refs(case, i)
    kdx, kds, kdt = R.subpix_arb_k(case)
    hold('%s:dx' % got.entry, cid, got.dx, r64['dx'], r64['den_dx'], r32['dx'], kdx)
    for name, bound in zip(('ds', 'dt'), R.subpix_arb_bound(case, r64, i['ax'])):
        err = (getattr(got, name).to(D64) - r64[name]).abs()
        print('%s %s: %.3f of the a-priori bound' % (cid, name, float((err / (bound * R.U).clamp_min(1e-300)).max())))
        assert bool((err <= bound * R.U).all()), name
    ip = R.arb_positive(i)
    pos = _arb(dev, N, case, ip)
    _on_route(pos, case, case['route'], cid)
    p64, p32 = R.subpix_arb_refs(case, ip)
    for name, k in (('ds', kds), ('dt', kdt)):
        hold('%s:%s' % (got.entry, name), cid, getattr(pos, name), p64[name], p64['den_' + name], p32[name], k)
    _same_bits(_arb(dev, N, case, i), got, ('dx', 'ds', 'dt'), cid)
    if case['ext'] and case['route'] == 'H':
        _same_bits(_arb(dev, N, dict(case, skip=False), i), got, ('dx', 'ds', 'dt'), cid + ' P2L_FORM_NO_SP_SKIP')
    if len(R.subpix_slices(case)) > 1:
        other = _arb(dev, N, dict(case, finish='scalar' if case['finish'] == 'v4' else 'v4'), i)
        _on_route(other, case, case['route'], cid)
        # dx bit for bit; ds and dt of each finish kernel are held to the bar on their own (the scalar kernel's
        # `sgx += g * xv` and the 16-byte one's are contracted differently: a few last bits apart)
        _same_bits(other, got, ('dx',), cid + ': the two finish kernels')
    if not case['nomask'] and not case['skip_g']:
        assert bool((got.dx[r64['g'] == 0] == 0).all())
    if got.amax is not None:
        assert bool((got.amax.view(torch.int32) != SENT).all())
        assert torch.equal(got.amax.amax(dim=1), got.dx.abs().amax(dim=(1, 2, 3)))


# =====================================================================================================================
# arguments
# =====================================================================================================================
def _set(**kw):
    def tamper(d, *_):
        for k, v in kw.items():
            setattr(d, k, v)
    return tamper


FWD_ARGS = [
    ('ups2-residual', R._ssh('F', 2, 0, '16x32', res='same'), {}, None, EUNSUP),
    ('ups2-mask', R._ssh('H', 2, 1, '16x16', mask=True), {}, None, EUNSUP),
    ('ups2-pool', R._ssh('B', 2, 0, '16x32'), {}, _set(pool=R.POOL_SUM), EINVAL),          # (no yp: refused earlier)
    ('ups2-splitk', R._ssh('H', 2, 0, '32x32', splitk=2), {}, None, EUNSUP),
    ('ups2-ext-splitk', R._ssh('P', 2, 1, '32x32', splitk=2), {}, None, EUNSUP),
    ('ups3-ext0-splitk', R._ssh('H', 3, 0, '32x32', splitk=2), {}, None, EUNSUP),
    ('ups3-ext1-splitk-on-F', R._ssh('F', 3, 1, 's4', splitk=4), {}, None, EUNSUP),
    ('sliced-without-the-fp16x2-workspace', R._ssh('H', 3, 1, 's4', splitk=4), dict(no_ws=True), None, EWS),
    ('sliced-short-workspace', R._ssh('H', 3, 1, 's8', splitk=8), dict(ws_short=4), None, EWS),
    ('bf3-buffer-on-a-bf3w-launch', R._ssh('B', 2, 0, '16x32'), {}, _set(wfmt=R.WFMT_BF16X3W), EINVAL),
    ('bf3-buffer-on-a-bf3w-gradient', R._ssh('B', 3, 1, '16x32'), {}, _set(wfmt=R.WFMT_BF16X3W), EINVAL),
]


@pytest.mark.parametrize('what,case,kw,tamper,want', FWD_ARGS, ids=[a[0] for a in FWD_ARGS])
def test_arguments_are_refused_before_the_launch(dev, N, what, case, kw, tamper, want):
    """nothing is launched, every output still holds sentinels"""
    i = R.subpix_inputs(_gen('sargs', what), dict(case, res=None, mask=False) if case['ups'] == 2 else case)
    if case['ups'] == 2 and case['res']:
        i['res'] = torch.zeros(case['B'], case['H'], case['W'], case['Cout'])
    if case['ups'] == 2 and case['mask']:
        i['mask'] = torch.ones(case['B'], case['H'] + 2, case['W'] + 2, case['Cout'])
    got = _fwd(dev, N, case, i, tamper=tamper, **kw)
    assert got.rc == want, (what, got.rc)
    assert got.count == (0, 0) and _untouched(got)


def test_a_pool_on_a_sub_pixel_launch_is_unsupported(dev, N):
    """pool != NONE with a pooled output present: P2L_EUNSUP from the sub-pixel branch itself"""
    lib = N.lib()
    for c in (R._ssh('F', 2, 0, '16x32'), R._ssh('H', 3, 1, '16x32')):
        i = R.subpix_inputs(_gen('spool', R.subpix_id(c)), c)
        d = _desc(N, c, c['route'], c['B'])
        wp = _weights(dev, N, i, c, c['route'])
        d.pool, d.y_ld, d.yp_ld, d.n_store, d.w_floats = R.POOL_MAX, c['Cout'], c['Cout'], c['Cout'], wp.numel()
        oh, ow = _out_hw(c)
        y, yp = Out(dev, c['B'] * oh * ow * c['Cout']), Out(dev, c['B'] * oh * ow * c['Cout'])
        need = lib.p2l_conv_workspace_bytes(C.byref(d))
        ws = Out(dev, max(need // 4, 1))
        rc, _, _, count, _ = _profiled(N, lambda: lib.p2l_conv_fwd(
            C.byref(d), N.ptr(_pitched(i['x'], c['Cin'] + 4, dev)), N.ptr(wp), None, None, None, None, None, N.ptr(y.t),
            N.ptr(yp.t), N.ptr(ws.t), C.c_size_t(ws.n * 4), N.stream()))
        assert rc == EUNSUP and count == (0, 0)
        assert is_sentinel(y.cpu()) and is_sentinel(yp.cpu())


ARB_ARGS = [
    ('unsliced-multi-image-tile-F', R._sac('F', 0, (8, 8), 3, 32, 64), EUNSUP),
    ('unsliced-multi-image-tile-H', R._sac('H', 1, (16, 16), 2, 32, 64), EUNSUP),
    ('partial-grid', R._sac('B', 0, (24, 40), 2, 32, 64), EUNSUP),
    ('partial-grid-H', R._sac('H', 1, (24, 40), 2, 32, 64), EUNSUP),
    ('sliced-without-workspace', R._sac('H', 1, (16, 16), 3, 128, 64, splitk=4), EWS),
]


@pytest.mark.parametrize('what,case,want', ARB_ARGS, ids=[a[0] for a in ARB_ARGS])
def test_fused_backward_arguments_are_refused_before_the_launch(dev, N, what, case, want):
    no_ws = what == 'sliced-without-workspace'
    got = _arb(dev, N, case, R.subpix_arb_inputs(_gen('sargs-arb', what), case), no_ws=no_ws)
    assert got.rc == want, (what, got.rc)
    assert got.count == (0, 0) and _untouched(got)


@seeded
def test_without_the_maxima_share_of_the_workspace_the_launch_keeps_bf16x3(dev, N):
    """the header: the fp16 x 2 form needs 256 B of workspace per image, without it an unsliced P2L_WFMT_BF16X3W launch
    keeps the bf16 x 3 arithmetic: six products on conv_mfma_kernel<4, ..>, held as route B -- in all four modes"""
    for ups, ext, name in ((2, 0, '16x32'), (2, 1, '8x8'), (3, 0, '8x8'), (3, 1, '32x32')):
        case = R._ssh('B', ups, ext, name, wfmt='nows', bias=True)
        cid = R.subpix_id(case)
        i = R.subpix_inputs(_gen('wsfall', cid), case)
        got = _fwd(dev, N, case, i)
        _on_route(got, case, 'B', cid)
        r64, r32 = R.subpix_refs(case, i)
        hold('p2l_conv_fwd:y', cid + ' kept on bf16 x 3', got.y, r64['y'], r64['den'], r32['y'], R.subpix_k(case))

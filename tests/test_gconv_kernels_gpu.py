"""The generic gather conv -- gconv_mfma_kernel behind p2l_gconv_fwd (csrc/p2l_alex.hip): every conv of the AlexNet
and SqueezeNet LPIPS plans and, through transpose_flip packings, their input gradients -- and the two pack functions
that feed it, against the float64 references of tests/_small_refs.py, through ctypes, with the harness, the metric and
the bars of tests/test_small_kernels_gpu.py (tests/_pin.py):

    p2l_gconv_fwd, p2l_pack_gconv_weight, p2l_pack_conv_weight (taps 25, 121).

Outputs are held to |got - r64| / den <= min(k, 4 x the fp32 restatement) x 2^-24 with den = sum over taps and
channels of (|pro_s| |x| + |pro_t|) |w| + |bias| + |res| and k counted in _small_refs.gconv_k; the input-gradient
forms against the float64 vjp of the forward conv they differentiate.  A masked element is +0 bit for bit; one-hot
inputs are compared bit for bit, tap by tap and channel by channel, for every (KH, KW, stride, pad) of the cases; a
repeated launch gives the same bits.  Every output sits between guard bands; every input has a pitch above its row
with junk in the gap, every output a pitch above n_store with sentinels in the gap (but for the cases whose point is
y_ld == n_store, and the residual / mask of the gradient forms at pitch n_store).  P2L_GCONV_ERR_FILE=<path> records
the figures (profiles/gconv_kernels_err.txt).  The cases, their inputs and k live in tests/_small_refs.py;
tests/test_small_refs.py holds them to "the restatement is within k / 4" on the host."""
import ctypes as C

import pytest
import torch

import _small_refs as R
from _pin import D64, G, N, SENT, Out, _gen, _record_file, hold, is_sentinel, randn, seeded  # noqa: F401

pytestmark = pytest.mark.gpu
EINVAL, EUNSUP = -1, -4
ENTRY = 'p2l_gconv_fwd:y'


def _pitched(t, ld, dev, junk=7.0):
    """[..., C] -> the same rows at pitch ld on the device, junk in the gap columns"""
    o = torch.full(t.shape[:-1] + (ld,), junk)
    o[..., :t.shape[-1]] = t
    return o.to(dev)


class _Got(object):
    pass


def _packed(dev, N, c, i):
    """the case's weight through p2l_pack_gconv_weight: O x I real channels into Cout x Cin; dgrad: the forward
    conv's OIHW tensor through transpose_flip"""
    src = i['wf'] if c['dgrad'] else i['w']
    return N.pack_gconv_weight(src.to(dev), c['KH'] * c['KW'], c['Cout'], c['Cin'], c['dgrad'])


def _launch(dev, N, c, i, out=None, tamper=None, null=(), null_d=False):
    """one p2l_gconv_fwd launch of case c on inputs i -> _Got: rc, y [B, Ho, Wo, n_store], the whole rows `full` [M,
    y_ld] and the Out they sit in (`out`: an Out of M * y_ld floats that another launch wrote to already; the launch
    writes at column c['col'])"""
    lib = N.lib()
    B, Hi, Wi, Cin, Cout, ns, y_ld = c['B'], c['Hi'], c['Wi'], c['Cin'], c['Cout'], c['n_store'], c['y_ld']
    Ho, Wo = R.gconv_out(c)
    M = B * Ho * Wo
    d = N.P2LGConv()
    d.B, d.Hi, d.Wi, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad = B, Hi, Wi, Cin, Cout, c['KH'], c['KW'], c['stride'], c['pad']
    d.y_ld, d.n_store, d.relu = y_ld, (ns if ns < Cout else 0), int(c['relu'])
    if c['x_off']:                                  # the second half of rows of 2 Cin floats, junk in the first
        xt = torch.full((B, Hi, Wi, 2 * Cin), -3.0)
        xt[..., Cin:] = i['x']
        xt = xt.to(dev)
        N.alive.append(xt)
        d.x_ld, xp = 2 * Cin, C.c_void_p(xt.data_ptr() + 4 * Cin)
    else:
        d.x_ld = Cin + 4
        xp = N.ptr(_pitched(i['x'], Cin + 4, dev))
    resd = maskd = None
    if c['res']:
        d.res_ld = ns if c['aux_tight'] else ns + 8
        resd = _pitched(i['res'], d.res_ld, dev, 3.0)
    if c['mask']:
        d.mask_ld = ns if c['aux_tight'] else ns + 12
        maskd = _pitched(i['mask'], d.mask_ld, dev, 1.0)
    wp = _packed(dev, N, c, i)
    sd = i['pro_s'].to(dev) if c['pro'] else None
    td = i['pro_t'].to(dev) if c['pro'] else None
    biasd = i['bias'].to(dev) if c['bias'] else None
    y = out or Out(dev, M * y_ld)
    if tamper is not None:
        tamper(d)
    ptrs = dict(x=xp, w=N.ptr(wp), bias=N.ptr(biasd), pro_s=N.ptr(sd), pro_t=N.ptr(td), res=N.ptr(resd),
                mask=N.ptr(maskd), y=C.c_void_p(y.t.data_ptr() + 4 * c['col']))
    for name in null:
        ptrs[name] = None
    got = _Got()
    got.rc = lib.p2l_gconv_fwd(None if null_d else C.byref(d), ptrs['x'], ptrs['w'], ptrs['bias'], ptrs['pro_s'],
                               ptrs['pro_t'], ptrs['res'], ptrs['mask'], ptrs['y'], N.stream())
    got.out = y
    got.full = y.cpu(M, y_ld)
    got.y = got.full[:, c['col']:c['col'] + ns].reshape(B, Ho, Wo, ns).contiguous()
    return got


def _judge(c, i, got, refs=None, gaps=True):
    """the launch was good; nothing outside its n_store columns was written (gaps = False: the caller looks); hold y; a
    masked element is +0"""
    ns = c['n_store']
    assert got.rc == 0, (R.gconv_id(c), got.rc)
    gap = torch.ones(c['y_ld'], dtype=torch.bool)
    gap[c['col']:c['col'] + ns] = False
    if gaps:
        assert is_sentinel(got.full[:, gap]), 'columns outside n_store written'
    assert not bool((got.y.view(torch.int32) == SENT).any()), 'stored columns left unwritten'
    r64, r32 = refs or R.gconv_refs(c, i)
    hold(ENTRY, R.gconv_id(c), got.y, r64['y'], r64['den'], r32['y'], R.gconv_k(c))
    if c['mask']:
        dead = ~(i['mask'] > 0)
        assert bool(dead.any()) and bool((got.y.view(torch.int32)[dead] == 0).all()), 'a masked element is not +0'
    assert bool((got.y.view(torch.int32)[r64['den'] == 0] == 0).all()), 'not +0 where every term is zero'
    return r64, r32


# =====================================================================================================================
# every form of the launch the plans make, and the descriptor shapes around them
# =====================================================================================================================
@pytest.mark.parametrize('case', R.GCONV_CASES, ids=R.gconv_id)
@seeded
def test_forward(dev, N, case):
    i = R.gconv_inputs(_gen('gconv', R.gconv_id(case)), case)
    got = _launch(dev, N, case, i)
    r64, _ = _judge(case, i, got)
    again = _launch(dev, N, case, i)
    assert torch.equal(again.full.view(torch.int32), got.full.view(torch.int32)), 'a repeated launch differs'
    if case['pad'] >= max(case['KH'], case['KW']):
        # the border sees padding alone: the epilogue of an exact 0, whatever pro_t holds
        assert case['pro'] and case['bias'] and not case['res'] and bool((i['pro_t'][:case['I']] != 0).all())
        border = torch.ones(got.y.shape[1:3], dtype=torch.bool)
        border[1:-1, 1:-1] = False
        want = i['bias'][:case['n_store']].expand_as(got.y)
        assert torch.equal(got.y[:, border].view(torch.int32), want[:, border].contiguous().view(torch.int32))


@seeded
def test_the_expand_pair_writes_the_halves_of_one_tensor(dev, N):
    """a fire's 1x1 and 3x3 expand convs write columns 0..63 and 64..127 of one tensor of pitch 128: each launch
    leaves the other half untouched, in either order; the pair is the concatenated tensor"""
    e1, e3 = R.GCONV_PAIR
    g = _gen('gconv', 'expand-pair')
    i1 = R.gconv_inputs(g, e1)
    i3 = dict(R.gconv_inputs(g, e3), x=i1['x'])                         # both read the squeeze output
    M = e1['B'] * R.gconv_out(e1)[0] * R.gconv_out(e1)[1]
    refs = {}
    for order in ((e1, i1), (e3, i3)), ((e3, i3), (e1, i1)):
        out = Out(dev, M * 128)
        (ca, ia), (cb, ib) = order
        first = _launch(dev, N, ca, ia, out=out)
        other = slice(cb['col'], cb['col'] + 64)
        assert first.rc == 0 and is_sentinel(first.full[:, other]), 'the first launch wrote the other half'
        kept = first.full[:, ca['col']:ca['col'] + 64].clone()
        second = _launch(dev, N, cb, ib, out=out)
        assert second.rc == 0
        assert torch.equal(second.full[:, ca['col']:ca['col'] + 64].view(torch.int32), kept.view(torch.int32)), \
            'the second launch wrote the first half'
        assert not bool((second.full.view(torch.int32) == SENT).any())
        if not refs:
            for c, i, got in ((ca, ia, first), (cb, ib, second)):
                refs[c['name']] = _judge(c, i, got, gaps=False)
            whole = second.full.view(e1['B'], *R.gconv_out(e1), 128)
            cat = lambda k, j: torch.cat([refs[e1['name']][j][k], refs[e3['name']][j][k]], dim=-1)
            # one k for the tensor, the 1x1 half's: the 3x3 half's denominator carries the ratio of the two counts
            k1, k3 = R.gconv_k(e1), R.gconv_k(e3)
            den = torch.cat([refs[e1['name']][0]['den'], refs[e3['name']][0]['den'] * (float(k3) / k1)], dim=-1)
            hold(ENTRY, 'expand-pair-concatenated', whole, cat('y', 0), den, cat('y', 1), k1)
        else:
            assert torch.equal(second.full.view(torch.int32), keep_bits), 'the order of the pair changes bits'
        keep_bits = second.full.view(torch.int32).clone()


# =====================================================================================================================
# geometry, bit for bit
# =====================================================================================================================
@pytest.mark.parametrize('geom', R.gconv_geometries(), ids=lambda g: '%dx%ds%dp%d' % g)
def test_one_hot_inputs_are_exact(dev, N, geom):
    """a single power-of-two x element at a corner, an edge and an interior pixel of every stride residue; weights
    with a value of their own per (tap, channel, output): every output is one exact product and names the tap and
    the channel that reached it -- compared with float64 exactly"""
    KH, KW, s, p = geom
    c = R._gc('onehot', (KH, KW), s, p, (max(KH, 7) + 2 * s, max(KW, 6) + 2 * s + 1), 2, 16, 64)
    hit = 0
    for n, spot in enumerate(R.gconv_spots(c)):
        i = R.gconv_onehot(c, spot, n)
        got = _launch(dev, N, c, i)
        assert got.rc == 0 and is_sentinel(got.full[:, 64:])
        want = R.gconv(i['x'].double(), i['w'].double(), s, p)['y']
        hit += int((want != 0).sum())
        assert torch.equal(got.y.double(), want), (geom, spot, int((got.y.double() != want).sum()))
        assert not bool(torch.signbit(got.y[want == 0]).any())
    assert hit >= 64


def test_all_zero_inputs_give_exactly_zero(dev, N):
    for c in R.GCONV_CASES[:1] + R.GCONV_CASES[3:4] + R.GCONV_CASES[-1:]:
        i = R.gconv_inputs(_gen('gconv-zero', R.gconv_id(c)), c)
        i = dict(i, x=torch.zeros_like(i['x']))
        for k in ('pro_t', 'bias', 'res'):
            if k in i:
                i[k] = torch.zeros_like(i[k])
        got = _launch(dev, N, c, i)
        assert got.rc == 0 and bool((got.y.view(torch.int32) == 0).all()), R.gconv_id(c)


# =====================================================================================================================
# arguments
# =====================================================================================================================
def _set(**kw):
    def tamper(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return tamper


# 3x3 pad 1 on 5x7, 32 -> 64 with 48 stored, prologue, residual and mask: every operand a refusal can concern is there
ARG_CASE = R._gc('args', 3, 1, 1, (5, 7), 2, 32, 64, O=48, pro=True, bias=True, res=True, mask=True, relu=True)
ARGS = [
    ('null-d', dict(null_d=True), EINVAL), ('null-x', dict(null=('x',)), EINVAL), ('null-w', dict(null=('w',)), EINVAL),
    ('null-y', dict(null=('y',)), EINVAL),
    ('Cin-not-16', dict(tamper=_set(Cin=24, x_ld=24)), EINVAL), ('Cout-not-64', dict(tamper=_set(Cout=96)), EINVAL),
    ('x_ld-unaligned', dict(tamper=_set(x_ld=38)), EINVAL), ('x_ld-short', dict(tamper=_set(x_ld=28)), EINVAL),
    ('KH-0', dict(tamper=_set(KH=0)), EINVAL), ('KW-0', dict(tamper=_set(KW=0)), EINVAL),
    ('stride-0', dict(tamper=_set(stride=0)), EINVAL), ('B-0', dict(tamper=_set(B=0)), EINVAL),
    ('pad-negative', dict(tamper=_set(pad=-1)), EINVAL),
    ('Ho-0', dict(tamper=_set(KH=8)), EINVAL), ('Wo-0', dict(tamper=_set(KW=10)), EINVAL),
    ('pro_s-alone', dict(null=('pro_t',)), EINVAL), ('pro_t-alone', dict(null=('pro_s',)), EINVAL),
    # 2^31 / (5 * 7 * 64) = 958698.06: the first B whose output reaches 2^31 elements (nothing is launched: the
    # buffers are the small ones)
    ('output-2^31', dict(tamper=_set(B=958699)), EUNSUP),
    ('output-2^31-by-y_ld', dict(tamper=_set(B=479350, y_ld=128)), EUNSUP),
    # n_store, the pitches that go with it, Hi / Wi
    ('n_store-negative', dict(tamper=_set(n_store=-4)), EINVAL),
    ('n_store-above-Cout', dict(tamper=_set(n_store=68, y_ld=72, res_ld=72, mask_ld=72)), EINVAL),
    ('y_ld-below-n_store', dict(tamper=_set(y_ld=44)), EINVAL),
    ('y_ld-below-Cout-with-n_store-0', dict(tamper=_set(n_store=0, y_ld=52, res_ld=64, mask_ld=64)), EINVAL),
    ('res_ld-below-n_store', dict(tamper=_set(res_ld=44)), EINVAL),
    ('mask_ld-below-n_store', dict(tamper=_set(mask_ld=47)), EINVAL),
    ('Hi-0', dict(tamper=_set(Hi=0, pad=2)), EINVAL), ('Wi-0', dict(tamper=_set(Wi=0, pad=2)), EINVAL),
    ('Hi-negative', dict(tamper=_set(Hi=-1, pad=3)), EINVAL),
]


@pytest.mark.parametrize('what,kw,want', ARGS, ids=[a[0] for a in ARGS])
def test_arguments_are_refused_before_the_launch(dev, N, what, kw, want):
    """the return code, and every output float still the sentinel"""
    i = R.gconv_inputs(_gen('gconv-args', 'args'), ARG_CASE)
    got = _launch(dev, N, ARG_CASE, i, **kw)
    assert got.rc == want, (what, got.rc)
    assert is_sentinel(got.full), what


@seeded
def test_the_argument_case_is_a_good_launch(dev, N):
    """... and so are the pitches exactly at their bounds: y_ld == res_ld == mask_ld == n_store"""
    i = R.gconv_inputs(_gen('gconv-args', 'args'), ARG_CASE)
    refs = _judge(ARG_CASE, i, _launch(dev, N, ARG_CASE, i))
    tight = dict(ARG_CASE, tight=True, aux_tight=True, y_ld=ARG_CASE['n_store'], name='args-tight')
    _judge(tight, i, _launch(dev, N, tight, i), refs)


def test_a_residual_or_mask_pitch_without_its_operand_is_not_looked_at(dev, N):
    c = R._gc('no-aux', 3, 1, 1, (5, 7), 2, 16, 64, bias=True)
    i = R.gconv_inputs(_gen('gconv-args', 'no-aux'), c)
    got = _launch(dev, N, c, i, tamper=_set(res_ld=0, mask_ld=0))
    assert got.rc == 0 and torch.equal(got.full.view(torch.int32), _launch(dev, N, c, i).full.view(torch.int32))


# =====================================================================================================================
# the pack functions
# =====================================================================================================================
PACKS = [('gconv', taps_hw, O, I, N_pad, K_pad) for taps_hw in ((1, 1), (2, 3), (3, 3), (5, 5), (11, 11))
         for O, I, N_pad, K_pad in ((16, 3, 64, 16), (64, 48, 64, 48), (35, 20, 96, 32))] + \
        [('conv', taps_hw, O, I, N_pad, K_pad) for taps_hw in ((5, 5), (11, 11))
         for O, I, N_pad, K_pad in ((16, 3, 64, 16), (35, 20, 96, 32))]


def _pack_fn(N, which):
    lib = N.lib()
    return lib.p2l_pack_gconv_weight if which == 'gconv' else lib.p2l_pack_conv_weight


@pytest.mark.parametrize('flip', [0, 1], ids=['forward', 'transpose_flip'])
@pytest.mark.parametrize('which,taps_hw,O,I,N_pad,K_pad', PACKS, ids=lambda v: str(v).replace(' ', ''))
def test_packs_are_the_written_out_layout_bit_for_bit(dev, N, which, taps_hw, O, I, N_pad, K_pad, flip):
    """[tap][K_pad / 16][N_pad][16] between guard bands, the fill exact zeros; transpose_flip: N = I, K = O"""
    KH, KW = taps_hw
    if flip:
        O, I = I, O                                                      # (the pads bound I and O the other way round)
    w = randn(_gen('gconv-pack', which, taps_hw, O, I, flip), O, I, KH, KW)
    w.view(-1)[3] = -0.0
    dst = Out(dev, KH * KW * N_pad * K_pad)
    rc = _pack_fn(N, which)(N.ptr(w.to(dev)), O, I, KH * KW, N_pad, K_pad, flip, N.ptr(dst.t), N.stream())
    assert rc == 0
    want = R.gconv_pack(w, N_pad, K_pad, bool(flip))
    got = dst.cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), int((got != want).sum())
    assert int((want == 0).sum()) >= KH * KW * (N_pad * K_pad - O * I)


PACK_ARGS = [('null-src', dict(src=None)), ('null-dst', dict(dst=None)), ('taps-0', dict(taps=0)),
             ('taps-negative', dict(taps=-9)), ('K_pad-not-16', dict(K_pad=24)), ('N_pad-not-32', dict(N_pad=48)),
             ('N_pad-below-O', dict(N_pad=32)), ('K_pad-below-I', dict(K_pad=16)),
             ('N_pad-below-I-flipped', dict(O=16, I=40, N_pad=32, K_pad=64, flip=1)),
             ('K_pad-below-O-flipped', dict(O=40, I=16, N_pad=64, K_pad=32, flip=1))]


@pytest.mark.parametrize('which', ['gconv', 'conv'])
@pytest.mark.parametrize('what,kw', PACK_ARGS, ids=[a[0] for a in PACK_ARGS])
def test_pack_arguments_are_refused_with_the_destination_untouched(dev, N, what, kw, which):
    a = dict(O=40, I=20, taps=25, N_pad=64, K_pad=32, flip=0)
    a.update({k: v for k, v in kw.items() if k not in ('src', 'dst')})
    w = randn(_gen('gconv-pack-args'), a['O'], a['I'], 5, 5).to(dev)
    dst = Out(dev, 25 * 64 * 32)
    rc = _pack_fn(N, which)(None if 'src' in kw else N.ptr(w), a['O'], a['I'], a['taps'], a['N_pad'], a['K_pad'],
                            a['flip'], None if 'dst' in kw else N.ptr(dst.t), N.stream())
    assert rc == EINVAL, (what, rc)
    assert is_sentinel(dst.cpu()), what

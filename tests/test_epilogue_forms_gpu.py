"""The epilogues compiled for a launch's class (csrc/p2l_conv_k.h epi_item_ct) against the shared run-time item
(P2L_FORM_GENERIC_EPI) on the same launch: every buffer the launch writes -- y, yp, both maxima slot arrays, the
activation backward's partial sums, dx, ds, dt -- bit for bit, for every (kernel family, class) pair that ships
(tests/_epilogue_cases.py).  p2l_conv_epilogue_class != 0 for the default launch says the compiled form ran.

Inputs are signed; one pre-activation is exactly zero (forward: an all-zero output channel without bias; backward:
x = 0 under t = 0; mask: one element 0) and one channel has a negative scale (the reader's affine of the maxima, the
s of the activation backward), so the mask and maxima-with-affine decisions are taken both ways."""
import ctypes as C
import zlib

import pytest
import torch

import _epilogue_cases as E
from _pin import N, Out, is_sentinel  # noqa: F401

pytestmark = pytest.mark.gpu


def _inputs(c):
    g = torch.Generator().manual_seed(zlib.crc32(E.case_id(c).encode()))
    B, H, W, Cin, Cout, k = c['B'], c['H'], c['W'], c['Cin'], c['Cout'], 3 if c['taps'] == 9 else 1
    Ho, Wo = E.out_hw(c)
    rn = lambda *s: torch.randn(*s, generator=g)
    i = dict(x=rn(B, H, W, Cin), w=rn(Cout, Cin, k, k) / (Cin * k * k) ** 0.5)
    if c['bias']:
        i['bias'] = rn(Cout)
        i['bias'][0] = 0.0
        i['w'][0] = 0.0                                     # channel 0: pre-activation exactly 0
    if c['pro']:
        i['ps'], i['pt'] = rn(B, Cin), rn(B, Cin)
    if c['res'] == 'same':
        i['res'] = rn(B, H, W, Cout)
    elif c['res'] == 'ups':
        i['res'] = rn(B, H // 2, W // 2, Cout + 32)        # res_ld > channels
    if c['mask']:
        i['mask'] = rn(B, H, W, Cout)
        i['mask'][0, 0, 0, 0] = 0.0
    if c['next_affine']:
        i['ns'], i['nt'] = 0.5 + torch.rand(B, Cout, generator=g), rn(B, Cout)
        i['ns'][:, 1] *= -1.0
    if c['arb']:
        i['ax'], i['as'], i['at'] = rn(B, Ho, Wo, Cout), 0.5 + torch.rand(B, Cout, generator=g), rn(B, Cout)
        i['as'][:, 1] *= -1.0
        i['ax'][0, 0, 0, 0] = 0.0
        i['at'][:, 0] = 0.0
        if c['skip'] == 'same':
            i['skip'] = rn(B, Ho, Wo, Cout)
        elif c['skip'] == 'ups':
            i['skip'] = rn(B, 2 * Ho, 2 * Wo, Cout)        # the 2x2 children of every output pixel
    return i


def _launch(dev, N, c, i, form):
    """one launch of case c -> (rc, class, {name: bits of every buffer it may write})"""
    lib = N.lib()
    d = E.descriptor(N, c, form=form)
    B, Cout = c['B'], c['Cout']
    Ho, Wo = E.out_hw(c)
    if c['ups'] == 3:
        wp = N.pack_conv_weight(i['w'].to(dev), 9, Cout, c['Cin'], True, E.WFMT_BF16X3W, subpix_mode=0)
    else:
        wp = N.pack_conv_weight(i['w'].to(dev), c['taps'], Cout, c['Cin'], False, E.wfmt_of(c))
    d.w_floats = wp.numel()
    t = {k: v.to(dev) for k, v in i.items() if k != 'w'}
    need = lib.p2l_conv_workspace_bytes(C.byref(d))
    ws = Out(dev, max(need // 4, 1))
    wsp, wsb = (N.ptr(ws.t), need) if need else (None, 0)
    slots = lib.p2l_conv_amax_slots(C.byref(d))
    outs = dict(y=Out(dev, B * Ho * Wo * Cout))
    am = N.P2LAmax()
    if slots > 0:
        outs['amax'] = Out(dev, B * slots)
        am.out = N.ptr(outs['amax'].t).value
    if c['pool'] == E.POOL_MAX:
        outs['yp'] = Out(dev, B * (Ho // 2) * (Wo // 2) * Cout)
        if slots > 0:
            outs['amaxp'] = Out(dev, B * slots)
            am.outp = N.ptr(outs['amaxp'].t).value
    if c['handed']:                                          # the true maxima of the raw input, one per image
        hand = i['x'].abs().amax(dim=(1, 2, 3)).view(B, 1).contiguous().to(dev)
        am.in_, am.in_n = N.ptr(hand).value, 1
    if c['next_affine']:
        am.next_s, am.next_t, am.next_bstride = N.ptr(t['ns']).value, N.ptr(t['nt']).value, Cout
    yp = N.ptr(outs['yp'].t) if 'yp' in outs else None
    if c['arb']:
        a = N.P2LArb()
        a.x, a.x_ld = N.ptr(t['ax']).value, Cout
        a.s, a.t, a.st_bstride = N.ptr(t['as']).value, N.ptr(t['at']).value, Cout
        if c['skip']:
            a.skip, a.skip_ld, a.skip_C, a.skip_ups = N.ptr(t['skip']).value, Cout, Cout // 2, int(c['skip'] == 'ups')
        outs['ds'], outs['dt'] = Out(dev, B * Cout), Out(dev, B * Cout)
        a.ds, a.dt, a.dsdt_bstride = N.ptr(outs['ds'].t).value, N.ptr(outs['dt'].t).value, Cout
        nblk = max(lib.p2l_conv_arb_nblk_ws(C.byref(d)), lib.p2l_conv_arb_nblk(C.byref(d)), 1)
        outs['partial'] = Out(dev, 2 * B * nblk * Cout)
        a.partial = N.ptr(outs['partial'].t).value
        a.amax = am
        ec = lib.p2l_conv_epilogue_class(C.byref(d), None, C.byref(a), None, None, None, N.ptr(outs['y'].t), None, wsp,
                                         C.c_size_t(wsb))
        rc = lib.p2l_conv_dgrad_arb_ws(C.byref(d), C.byref(a), N.ptr(t['x']), N.ptr(wp), N.ptr(outs['y'].t), wsp,
                                       C.c_size_t(wsb), N.stream())
    else:
        ex = N.P2LConvExtra()
        ex.amax = am
        ops = (N.ptr(t.get('bias')), N.ptr(t.get('res')), N.ptr(t.get('mask')), N.ptr(outs['y'].t), yp)
        ec = lib.p2l_conv_epilogue_class(C.byref(d), C.byref(ex), None, *ops, wsp, C.c_size_t(wsb))
        rc = lib.p2l_conv_fwd_ex(C.byref(d), C.byref(ex), N.ptr(t['x']), N.ptr(wp), ops[0], N.ptr(t.get('ps')),
                                 N.ptr(t.get('pt')), ops[1], ops[2], ops[3], ops[4], wsp, C.c_size_t(wsb), N.stream())
    torch.cuda.synchronize()
    ws.cpu()                                                 # (its guard bands)
    return rc, ec, {k: o.cpu().view(torch.int32) for k, o in outs.items()}


def _same_bits(c, dev, N, want_class):
    i = _inputs(c)
    rc, ec, got = _launch(dev, N, c, i, c['form'])
    assert rc == 0 and ec == want_class, (rc, ec)
    rc_g, ec_g, ref = _launch(dev, N, c, i, c['form'] | E.FORM_GENERIC_EPI)
    assert rc_g == 0 and ec_g == E.GENERIC, (rc_g, ec_g)
    assert sorted(got) == sorted(ref)
    for name in sorted(got):
        assert not is_sentinel(ref[name]), '%s: the launch wrote nothing' % name
        diff = got[name] != ref[name]
        assert not bool(diff.any()), '%s: %d of %d words differ' % (name, int(diff.sum()), diff.numel())
    return got


@pytest.mark.parametrize('c', E.CASES, ids=E.case_id)
def test_compiled_epilogue_has_the_bits_of_the_shared_item(dev, N, c):
    got = _same_bits(c, dev, N, c['ec'])
    assert 'amax' in got                                     # every class records the maxima of what it stores
    assert ('yp' in got and 'amaxp' in got) == (c['ec'] == E.BIAS_RELU_POOL)
    y = got['y'].view(torch.float32).view(c['B'], *E.out_hw(c), c['Cout'])
    if c['bias'] and not c['res']:
        z = y[..., 0]                                        # the zero pre-activation: + 0 (ReLU) / the bias, 0
        assert bool((z == 0).all())
    if c['mask']:
        assert y.view(torch.int32)[0, 0, 0, 0].item() == 0   # mask == 0 is not > 0: +0


@pytest.mark.parametrize('c', E.FALLBACK, ids=E.case_id)
def test_a_partial_grid_stays_on_the_shared_item(dev, N, c):
    _same_bits(c, dev, N, E.GENERIC)

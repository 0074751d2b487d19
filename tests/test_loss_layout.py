"""The three projection-loss plans (vgg, alex, squeeze) share one host-side shell (csrc/p2l_loss_shell.h).
Host checks, no GPU: every workspace / cache offset equals what the plans laid out BEFORE the shell existed
(tests/golden/loss_layout.json, written by tools/make_loss_layout_golden.py from that build), and the argument
checks of prepare / fwd / bwd come in the same order with the same codes."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWS = -1, -3
NETS = ('vgg', 'alex', 'squeeze')
# the shapes the golden file was asked for: four every net takes, 32^2 (vgg only), and the refused ones
SHAPES = {'vgg': ['1x64x64', '3x64x64', '5x256x256', '2x128x256', '3x32x32', '2x100x100'],
          'alex': ['1x64x64', '3x64x64', '5x256x256', '2x128x256', '3x32x32', '2x34x34'],
          'squeeze': ['1x64x64', '3x64x64', '5x256x256', '2x128x256', '3x32x32', '2x100x100']}
REFUSED = {'vgg': (2, 100, 100), 'alex': (2, 34, 34), 'squeeze': (2, 100, 100)}


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(ROOT, 'pix2latent_amd', 'libp2l_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from pix2latent_amd import _native as N
    return N.lib()


@pytest.fixture(scope='module')
def gold():
    with open(os.path.join(ROOT, 'tests', 'golden', 'loss_layout.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('net', NETS)
def test_layout_equals_the_recorded_one(lib, gold, net):
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_loss_layout_golden',
                                                  os.path.join(ROOT, 'tools', 'make_loss_layout_golden.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)                      # (the calls that wrote the file, so both read alike)
    record = tool.record
    for key in SHAPES[net]:
        B, H, W = (int(v) for v in key.split('x'))
        assert record(lib, net, B, H, W) == gold[net][key], (net, key)
    # the recorded values themselves: refused shapes give 0 bytes, alex and squeeze refuse 32^2 (cache included)
    assert gold[net]['%dx%dx%d' % REFUSED[net]]['ws_bytes'] == 0
    if net != 'vgg':
        assert gold[net]['3x32x32']['ws_bytes'] == 0 and gold[net]['3x32x32']['cache_floats'] == 0
    assert gold[net]['3x64x64']['ws_bytes'] > 0


def _entries(lib, net):
    from pix2latent_amd import _native as N
    pre = {'vgg': 'p2l_projloss', 'alex': 'p2l_alexloss', 'squeeze': 'p2l_sqzloss'}[net]
    cache = N.P2LLossCache7() if net == 'squeeze' else N.P2LLossCache()
    return [getattr(lib, pre + s) for s in ('_ws_bytes', '_prepare', '_fwd', '_bwd')], cache


@pytest.mark.parametrize('net', NETS)
def test_guards_come_in_the_same_order_with_the_same_codes(lib, net):
    """fake non-null device pointers; no case launches anything.  Even a call that got PAST the guards would
    not: it carries no weight, so the L1 kernels' own host check refuses fwd and the L1-only bwd (P2L_EINVAL,
    never P2L_EWS), and without a network descriptor prepare has nothing to do (P2L_OK)."""
    from pix2latent_amd import _native as N
    (f_ws, f_prepare, f_fwd, f_bwd), cache = _entries(lib, net)
    fake, null, beta = C.c_void_p(4096), C.c_void_p(0), C.c_float(1.0)
    B, H, W = 3, 64, 64
    nbytes = f_ws(B, H, W)
    assert nbytes > 0

    def prepare(shape=(B, H, W), ws=fake, n=nbytes, c=C.byref(cache), target=fake):
        return f_prepare(None, target, None, None, *shape, c, ws, C.c_size_t(n), None)

    def fwd(shape=(B, H, W), ws=fake, n=nbytes, c=C.byref(cache), img16=fake, loss=fake):
        return f_fwd(None, img16, fake, None, None, c, beta, 0, *shape, ws, C.c_size_t(n), loss, None, None, None)

    def bwd(shape=(B, H, W), ws=fake, n=nbytes, c=C.byref(cache), img16=fake, gloss=fake, dimg16=fake, v=None):
        return f_bwd(v, img16, fake, None, None, c, beta, 0, gloss, *shape, ws, C.c_size_t(n), dimg16, None)

    def smallest_accepted(**kw):
        lo, hi = 0, nbytes                             # refused, let through
        assert bwd(n=lo, **kw) == EWS and bwd(n=hi, **kw) == EINVAL
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if bwd(n=mid, **kw) == EWS else (lo, mid)
        return hi

    # the bytes the plan itself asks for.  alex, squeeze: what *_ws_bytes says.  vgg: *_ws_bytes has no
    # descriptor and answers for the weight format with the largest layout; a call without one runs as fp32
    total = smallest_accepted()
    if net == 'vgg':
        per_fmt = []
        for fmt in (N.WFMT_F32, N.WFMT_BF16X3W, N.WFMT_BF16X3):
            v = N.P2LVggLpips()
            v.wfmt = fmt
            per_fmt.append(smallest_accepted(v=C.byref(v)))
        assert per_fmt[0] == total and max(per_fmt) == nbytes
    else:
        assert total == nbytes

    required = {prepare: ('target',), fwd: ('img16', 'loss'), bwd: ('img16', 'gloss', 'dimg16')}
    for call, ptrs in required.items():
        assert call(shape=REFUSED[net]) == EINVAL
        assert call(shape=REFUSED[net], ws=null) == EINVAL        # the layout is checked first
        assert call(shape=(0, H, W), ws=null, c=None) == EINVAL
        assert call(n=total, ws=null) == EWS
        assert call(n=total - 1) == EWS
        assert call(n=total, c=None) == EWS
        for p in ptrs:
            assert call(n=total, **{p: null}) == EWS, p
    # ... and with everything in place the guards let the call through (see the docstring)
    assert prepare(n=total) == 0
    assert fwd(n=total) == EINVAL and bwd(n=total) == EINVAL
    # bwd with the LPIPS term asked for and no descriptor: P2L_EINVAL, but only behind the guards
    assert f_bwd(None, fake, fake, None, None, C.byref(cache), beta, 1, fake, B, H, W, null, C.c_size_t(total), fake,
                 None) == EWS
    assert f_bwd(None, fake, fake, None, None, C.byref(cache), beta, 1, fake, B, H, W, fake, C.c_size_t(total), fake,
                 None) == EINVAL

"""The launches whose epilogue is compiled for their class (csrc/p2l_conv_k.h EPI_*, p2l_conv_epilogue_class): one
descriptor per (kernel family, class) pair that ships.  tests/test_epilogue_class.py asks the classifier about them on
the host, tests/test_epilogue_forms_gpu.py launches them with and without P2L_FORM_GENERIC_EPI.

Shapes: the smallest at which the launch reaches its kernel and the kernel can go wrong.
  Winograd (fp16 x 2, 16x16- and 8x16-pixel blocks): B = 2, 16x16 (one tile) and 32x16 (two tiles), Cin = 32 (two
    chunks), Cout = 64 and 128, reached with P2L_FORM_WINO_ANY.
  1x1 full-tile: B = 2, 32x32 -- eight 128-pixel tiles; pw_shape (csrc/p2l_conv.hip) sends everything below 1024
    pixels to the small-grid form, which keeps the shared item -- Cin = 64, Cout = 64 and 128.
  direct 3x3 / sub-pixel input gradient: B = 2, 16x16 output grid, 64 -> 64.
"""
import ctypes as C

# csrc/p2l_conv_k.h
GENERIC, BIAS_PS, BIAS_RES_PS, BIAS_RESUP_PS, BIAS_RELU, BIAS_RELU_POOL, MASK, ARB, ARB_SKIP, ARB_SKIP_UP = range(10)
FORM_GENERIC_EPI = 8192
FORM_WINO_ANY, FORM_WINO_H2_8X16, FORM_WINO_H2_16X16, FORM_NO_H2R = 2, 64, 128, 256
ACT_NONE, ACT_RELU = 0, 1
POOL_NONE, POOL_MAX = 0, 1
PRO_NONE, PRO_AFFINE_RELU = 0, 1
WFMT_BF16X3W, WFMT_PW = 2, 3


def case(fam, ec, H, W, Cin, Cout, taps, **kw):
    c = dict(fam=fam, ec=ec, B=2, H=H, W=W, Cin=Cin, Cout=Cout, taps=taps, ups=0, pro=PRO_NONE, act=ACT_NONE,
             pool=POOL_NONE, bias=False, res=None, mask=False, next_affine=False, arb=False, skip=None, form=0,
             handed=False, oscale=False, noise=False, alpha=1.0)
    c.update(kw)
    return c


def case_id(c):
    return '%s-ec%d-%dx%dx%d-%dto%d-form%d' % (c['fam'], c['ec'], c['B'], c['H'], c['W'], c['Cin'], c['Cout'],
                                              c['form'])


_FWD = {BIAS_PS: dict(pro=PRO_AFFINE_RELU, bias=True, next_affine=True),
        BIAS_RES_PS: dict(pro=PRO_AFFINE_RELU, bias=True, next_affine=True, res='same'),
        BIAS_RESUP_PS: dict(pro=PRO_AFFINE_RELU, bias=True, next_affine=True, res='ups'),
        BIAS_RELU: dict(bias=True, act=ACT_RELU),
        BIAS_RELU_POOL: dict(bias=True, act=ACT_RELU, pool=POOL_MAX),
        MASK: dict(mask=True),
        ARB: dict(arb=True), ARB_SKIP: dict(arb=True, skip='same'), ARB_SKIP_UP: dict(arb=True, skip='ups')}

WINO_CLASSES = (BIAS_PS, BIAS_RELU, BIAS_RELU_POOL, MASK, ARB)
PW_CLASSES = (BIAS_PS, BIAS_RES_PS, BIAS_RESUP_PS, ARB, ARB_SKIP, ARB_SKIP_UP)

CASES = []
for _ec in WINO_CLASSES:
    for _form in (FORM_WINO_ANY | FORM_WINO_H2_16X16, FORM_WINO_ANY | FORM_WINO_H2_8X16):
        for (_H, _W, _Cout) in ((16, 16, 64), (32, 16, 128)):
            CASES.append(case('wino', _ec, _H, _W, 32, _Cout, 9, form=_form, **_FWD[_ec]))
for _ec in PW_CLASSES:
    for _Cout in (64, 128):
        CASES.append(case('pw', _ec, 32, 32, 64, _Cout, 1, handed=True, **_FWD[_ec]))
# the chunked direct kernel (an input gradient never runs on the register-resident one) and the sub-pixel input
# gradient: H, W = the HIGH-resolution gradient, the result is 16x16
CASES.append(case('direct', ARB, 16, 16, 64, 64, 9, **_FWD[ARB]))
CASES.append(case('subpix', ARB, 32, 32, 64, 64, 9, ups=3, **_FWD[ARB]))

# one fallback per family: a 12x12 grid is no whole tile of any of them (P2LConv wants even extents; the Winograd and
# full-tile 1x1 kernels take whole tiles only, so the launch lands on the kernel that owns partial grids)
FALLBACK = [case('wino', GENERIC, 12, 12, 32, 64, 9, form=FORM_WINO_ANY, **_FWD[BIAS_RELU]),
            case('pw', GENERIC, 12, 12, 64, 64, 1, handed=True, **_FWD[BIAS_PS]),
            case('direct', GENERIC, 12, 12, 64, 64, 9, **_FWD[MASK])]


def wfmt_of(c):
    return WFMT_PW if c['taps'] == 1 else WFMT_BF16X3W


def out_hw(c):
    return (c['H'] // 2, c['W'] // 2) if c['ups'] == 3 else (c['H'], c['W'])


def descriptor(N, c, B=None, form=None):
    """the P2LConv of case c (pitches = channel counts, except the nearest-up residual: res_ld > channels)"""
    d = N.P2LConv()
    d.B, d.H, d.W, d.Cin, d.Cout, d.taps, d.ups = c['B'] if B is None else B, c['H'], c['W'], c['Cin'], c['Cout'], \
        c['taps'], c['ups']
    d.x_ld, d.pro, d.alpha, d.act, d.pool = c['Cin'], c['pro'], c['alpha'], c['act'], c['pool']
    d.pro_bstride = c['Cin'] if c['pro'] else 0
    d.y_ld = d.yp_ld = d.n_store = c['Cout']
    if c['res']:
        d.res_ld, d.res_ups = (c['Cout'] + 32, 1) if c['res'] == 'ups' else (c['Cout'], 0)
    if c['mask']:
        d.mask_ld = c['Cout']
    d.splitk, d.wfmt, d.form = 1, wfmt_of(c), c['form'] if form is None else form
    return d


def classify(N, c, B=None, form=None, fake=0x10000):
    """p2l_conv_epilogue_class of case c with made-up addresses: only whether a pointer is NULL matters"""
    lib = N.lib()
    d = descriptor(N, c, B, form)
    p = C.c_void_p(fake)
    ws_bytes = lib.p2l_conv_workspace_bytes(C.byref(d))
    am = N.P2LAmax()
    am.out = fake
    if c['pool'] == POOL_MAX:
        am.outp = fake
    if c['handed']:
        am.in_, am.in_n = fake, 1
    if c['next_affine']:
        am.next_s, am.next_t, am.next_bstride = fake, fake, c['Cout']
    ex = arb = None
    if c['arb']:
        arb = N.P2LArb()
        arb.x, arb.x_ld, arb.s, arb.t, arb.st_bstride = fake, c['Cout'], fake, fake, c['Cout']
        arb.partial = arb.ds = arb.dt = fake
        arb.dsdt_bstride = c['Cout']
        if c['skip']:
            arb.skip, arb.skip_ld, arb.skip_C, arb.skip_ups = fake, c['Cout'], c['Cout'] // 2, int(c['skip'] == 'ups')
        arb.amax = am
    else:
        ex = N.P2LConvExtra()
        if c['oscale']:
            ex.oscale, ex.oscale_bstride = fake, c['Cout']
        if c['noise']:
            ex.noise, ex.noise_w = fake, 0.5
        ex.amax = am
    return lib.p2l_conv_epilogue_class(
        C.byref(d), C.byref(ex) if ex is not None else None, C.byref(arb) if arb is not None else None,
        p if c['bias'] else None, p if c['res'] else None, p if c['mask'] else None, p,
        p if c['pool'] == POOL_MAX else None, p if ws_bytes else None, C.c_size_t(ws_bytes))

"""p2l_conv_epilogue_class on the host (no device call): which compiled epilogue a launch runs with is decided from
its descriptor alone -- the class of every (family, class) pair that ships, 0 for every disqualifier taken one at a
time, and the same answer for every batch size."""
import os

import pytest

import _epilogue_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def N():
    so = os.path.join(ROOT, 'pix2latent_amd', 'libp2l_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from pix2latent_amd import _native
    _native.lib()
    return _native


def test_the_python_constants_are_the_headers():
    import re
    hdr = open(os.path.join(ROOT, 'include', 'p2l.h')).read()
    assert int(re.search(r'P2L_FORM_GENERIC_EPI = (\d+)', hdr).group(1)) == E.FORM_GENERIC_EPI
    assert int(re.search(r'P2L_FORM_SP_PAIR = (\d+)', hdr).group(1)) * 2 == E.FORM_GENERIC_EPI   # the next free bit
    k = open(os.path.join(ROOT, 'pix2latent_amd', 'csrc', 'p2l_conv_k.h')).read()
    for name in ('GENERIC', 'BIAS_PS', 'BIAS_RES_PS', 'BIAS_RESUP_PS', 'BIAS_RELU', 'BIAS_RELU_POOL', 'MASK', 'ARB',
                 'ARB_SKIP', 'ARB_SKIP_UP'):
        assert int(re.search(r'\bEPI_%s = (\d+)' % name, k).group(1)) == getattr(E, name)


@pytest.mark.parametrize('c', E.CASES, ids=E.case_id)
def test_every_shipped_pair_gets_its_class(N, c):
    assert c['ec'] != E.GENERIC
    assert E.classify(N, c) == c['ec']


@pytest.mark.parametrize('c', E.CASES, ids=E.case_id)
def test_the_descriptor_alone_decides(N, c):
    """the batch does not: B = 1 and B = 9 (the Winograd block shape, left to the grid, moves with it)"""
    forms = [c['form']] if c['fam'] != 'wino' else [c['form'], E.FORM_WINO_ANY]
    for form in forms:
        assert E.classify(N, c, B=1, form=form) == E.classify(N, c, B=9, form=form) == c['ec']


@pytest.mark.parametrize('c', E.CASES, ids=E.case_id)
def test_generic_epi_bit_gives_the_shared_item(N, c):
    assert E.classify(N, c, form=c['form'] | E.FORM_GENERIC_EPI) == E.GENERIC


def _first(fam, ec):
    return next(c for c in E.CASES if c['fam'] == fam and c['ec'] == ec)


@pytest.mark.parametrize('fam,ec', [('wino', E.BIAS_RELU), ('pw', E.BIAS_PS), ('wino', E.BIAS_PS)])
@pytest.mark.parametrize('what', ['oscale', 'noise'])
def test_stylegan2_terms_disqualify(N, fam, ec, what):
    c = _first(fam, ec)
    assert E.classify(N, c) == ec
    assert E.classify(N, dict(c, **{what: True})) == E.GENERIC


@pytest.mark.parametrize('c', E.FALLBACK, ids=E.case_id)
def test_a_partial_grid_disqualifies(N, c):
    whole = dict(c, H=32, W=32)                                # the same launch on whole tiles has a class ...
    if c['fam'] != 'direct':                                   # (masked launches have none on the direct kernel)
        assert E.classify(N, whole) != E.GENERIC
    assert E.classify(N, c) == E.GENERIC                       # ... on a 12x12 grid it has none


def test_a_sub_pixel_output_phase_disqualifies(N):
    """the sub-pixel FORWARD launch writes output phases (osh = 1): the shared item; its input gradient has a class"""
    bwd = _first('subpix', E.ARB)
    assert E.classify(N, bwd) == E.ARB
    fwd = E.case('subpix', E.GENERIC, 32, 32, 64, 64, 9, ups=2, pro=E.PRO_AFFINE_RELU, bias=True, next_affine=True)
    assert E.classify(N, fwd) == E.GENERIC


def test_other_disqualifiers(N):
    c = _first('pw', E.BIAS_PS)
    assert E.classify(N, dict(c, handed=False)) == E.GENERIC        # bf16 x 3 kernel: no maxima handed over
    assert E.classify(N, dict(c, act=E.ACT_RELU)) == E.GENERIC      # a combination no class describes
    assert E.classify(N, dict(c, next_affine=False)) == E.GENERIC
    assert E.classify(N, dict(c, pro=E.PRO_NONE)) == E.GENERIC      # (prologue, class) pairs the plans do not launch
    w = _first('wino', E.ARB)
    assert E.classify(N, dict(w, skip='same')) == E.GENERIC
    assert E.classify(N, dict(w, form=E.FORM_WINO_ANY | 4)) == E.GENERIC     # P2L_FORM_WINO_8X16: the bf16 x 3 kernel
    assert E.classify(N, dict(_first('direct', E.ARB), form=32)) == E.GENERIC   # P2L_FORM_WINO_BF3: bf16 x 3 direct

"""Colour transformations (reference pix2latent/transform/color_transform.py) on the host:
the module under both of the reference's names, its class attributes, the host restatement of
the Pillow integer rules against tests/golden/color_transform.npz (tools/make_color_golden.py)
and, where Pillow is installed, against Pillow itself.  CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'color_transform.npz')
NAMES = ('brightness', 'saturation', 'contrast', 'gamma', 'hue')      # op codes 0 .. 4


def gold():
    return np.load(GOLD, allow_pickle=False)


def expected(k):
    """what the reference's to_tensor + 2 (y - 0.5) makes of the golden's PIL bytes"""
    return 2.0 * (torch.from_numpy(k).float().div(255) - 0.5)


def golden_cases(g):
    """(set, name, ops, params [n_ops, B], bytes) of every single op and chain in the golden"""
    for s in ('a', 'b', 'c'):
        for op, name in enumerate(NAMES):
            for r in range(3):
                key = '%s_%s_%d' % (s, name, r)
                yield s, key, [op], g[key + '_p'][None], g[key + '_out']
        for chain in ('chain5', 'chain3'):
            key = '%s_%s' % (s, chain)
            yield s, key, list(g[chain + '_ops']), g[key + '_p'], g[key + '_out']


def test_modules_and_class_attributes():
    import pix2latent.transform.color_transform as CT
    import pix2latent.transform.transform_functions as TF
    from pix2latent_amd.transform import color_transform as impl
    assert CT is impl
    for name in ('ColorTransform', 'HueTransform', 'GammaTransform', 'SaturationTransform',
                 'BrightnessTransform', 'ContrastTransform'):
        assert getattr(TF, name) is getattr(CT, name)
    hue = CT.HueTransform()
    assert hue.t.dtype == np.float32 and list(hue.t) == [0.0]
    assert (hue.t_min, hue.t_max) == (-0.5 + 1e-6, 0.5 - 1e-6)
    assert hue.t_inv_fn is CT._negate
    for cls in (CT.GammaTransform, CT.SaturationTransform, CT.BrightnessTransform, CT.ContrastTransform):
        fn = cls()
        assert list(fn.t) == [1.0] and (fn.t_min, fn.t_max) == (0.667, 1.5)
        assert fn.t_inv_fn is CT._invert
        assert fn.is_spatial is False and fn.optimize is True
        assert fn.get_opt_param() is fn.t
        assert str(fn).startswith('ColorTransform: adjust_')
    fn = CT.BrightnessTransform(t=[1.2], t_min=0.5, t_max=2.0)
    assert (fn.t_min, fn.t_max) == (0.5, 2.0) and fn.t[0] == np.float32(1.2)
    off = CT.ColorTransform(CT.OP_GAMMA, optimize=False)
    assert off.get_opt_param() == []
    with pytest.raises(AssertionError):
        CT.ColorTransform(CT.OP_GAMMA, t_range=(1.0, 1.0))
    x = torch.tensor([[2.0]])
    assert CT._negate(x).item() == -2.0 and CT._invert(x).item() == 0.5


def test_host_path_equals_golden():
    from pix2latent_amd.transform import color_transform as CT
    g = gold()
    assert str(g['pillow_version'])
    n = 0
    for s, key, ops, ps, k in golden_cases(g):
        ims = torch.from_numpy(g[s + '_ims'])
        got = CT.host_chain(ims, ops, list(ps))
        assert torch.equal(got, expected(k)), key
        n += 1
    assert n == 3 * (5 * 3 + 2)


def test_classes_equal_golden_single_ops():
    """ColorTransform.apply on CPU tensors: the clamp of in-range values is the identity, the result
    is a detached CPU fp32 tensor"""
    from pix2latent_amd.transform import color_transform as CT
    g = gold()
    classes = [CT.BrightnessTransform, CT.SaturationTransform, CT.ContrastTransform, CT.GammaTransform,
               CT.HueTransform]
    ims = torch.from_numpy(g['b_ims']).requires_grad_(True)
    for op, name in enumerate(NAMES):
        key = 'b_%s_0' % name
        t = torch.from_numpy(g[key + '_p']).view(-1, 1)
        out = classes[op]()(ims, t)
        assert out.device.type == 'cpu' and out.dtype == torch.float32 and not out.requires_grad
        assert torch.equal(out, expected(g[key + '_out'])), name


def test_host_path_matches_pillow():
    pytest.importorskip('PIL')
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_color_golden as M
    from pix2latent_amd.transform import color_transform as CT
    gen = torch.Generator().manual_seed(123)
    ims = torch.rand(5, 3, 13, 21, generator=gen) * 2.2 - 1.1          # a few values outside [-1, 1] too
    for op in range(5):
        lo, hi = M.RANGES[op]
        for _ in range(3):
            p = (torch.rand(5, generator=gen) * (hi - lo) + lo).numpy()
            ref = CT.from_bytes(M.pil_apply(ims, op, p))
            assert torch.equal(CT.host_chain(ims, [op], [p]), ref), (op, p)
    ops = list(M.CHAINS['chain5'])
    ps = [(torch.rand(5, generator=gen) * (M.RANGES[o][1] - M.RANGES[o][0]) + M.RANGES[o][0]).numpy() for o in ops]
    assert torch.equal(CT.host_chain(ims, ops, ps), CT.from_bytes(M.pil_chain(ims, ops, ps)))


def test_compose_of_spatial_hue_brightness_is_its_parts_in_sequence():
    from pix2latent_amd.transform import ComposeTransform, SpatialTransform
    from pix2latent_amd.transform.color_transform import HueTransform, BrightnessTransform
    gen = torch.Generator().manual_seed(5)
    ims = torch.rand(4, 3, 12, 10, generator=gen) * 2 - 1
    sp, hue, br = SpatialTransform(), HueTransform(), BrightnessTransform()
    comp = ComposeTransform([(sp, 1.0), (hue, 5.0), (br, 5.0)])
    t = torch.cat([torch.tensor([[1.0, 0.0, 0.0]]) + 0.05 * torch.randn(4, 3, generator=gen),
                   0.03 * torch.randn(4, 1, generator=gen),
                   1.0 + 0.05 * torch.randn(4, 1, generator=gen)], 1)
    for invert in (False, True):
        seq = sp(ims, t[:, :3], invert=invert)
        seq = hue(seq, 5.0 * (t[:, 3:4] - 0.0) + 0.0, invert=invert)
        seq = br(seq, 5.0 * (t[:, 4:5] - 1.0) + 1.0, invert=invert)
        assert torch.equal(comp(ims, t, invert=invert), seq)
    # colour ops are skipped by only_spatial, and a single t row is broadcast over the batch
    assert torch.equal(comp(ims, t, only_spatial=True), sp(ims, t[:, :3]))
    assert torch.equal(comp(ims, t[:1]), comp(ims, t[:1].repeat(4, 1)))
    assert comp.get_opt_param().shape == (5,)


def test_invert_applies_t_inv_fn_before_the_clamp():
    from pix2latent_amd.transform import color_transform as CT
    gen = torch.Generator().manual_seed(9)
    ims = torch.rand(2, 3, 6, 7, generator=gen) * 2 - 1
    br = CT.BrightnessTransform()
    t = torch.tensor([[0.5], [0.8]])
    # 1 / 0.5 = 2 -> clamped to 1.5 (the clamp first would give 1 / 0.667)
    want = CT.host_chain(ims, [CT.OP_BRIGHTNESS], [np.array([1.5, 1.0 / 0.8], dtype=np.float32)])
    assert torch.equal(br(ims, t, invert=True), want)
    assert np.allclose(br.clamped(t, invert=True).numpy(), [1.5, 1.25])
    hue = CT.HueTransform()
    th = torch.tensor([[0.7], [-0.2]])
    assert np.allclose(hue.clamped(th, invert=True).numpy(), [np.float32(-0.5 + 1e-6), 0.2])
    assert np.allclose(hue.clamped(th).numpy(), [np.float32(0.5 - 1e-6), -0.2])
    want = CT.host_chain(ims, [CT.OP_HUE], [hue.clamped(th, invert=True).numpy()])
    assert torch.equal(hue(ims, th, invert=True), want)


def test_byte_conversion_wraps_and_round_trip_is_kept():
    """mul(255).byte() truncates and wraps modulo 256; the float -> byte -> float round trip between
    two chained ops is not always the identity, and a chain keeps it"""
    from pix2latent_amd.transform import color_transform as CT
    x = torch.tensor([256.5, -3.2, 255.99, 0.0]).mul(2.0 / 255).sub(1.0).view(1, 1, 1, 4).repeat(1, 3, 1, 1)
    k = CT.to_bytes(x)[0, 0, 0]
    assert list(k) == [0, 253, 255, 0]
    y = CT.from_bytes(np.arange(256, dtype=np.uint8).reshape(1, 1, 1, 256).repeat(3, 1))
    assert (CT.to_bytes(y)[0, 0, 0] != np.arange(256)).any()


def test_chain_struct_matches_the_compiled_header(tmp_path):
    """ctypes mirror of P2LColorChain / P2LColorOp against include/p2l.h compiled by gcc"""
    import shutil
    import subprocess
    import ctypes as C
    from pix2latent_amd.transform import color_transform as CT
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "p2l.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(P2LColorChain), sizeof(P2LColorOp),\n'
                   ' offsetof(P2LColorChain, n_ops), offsetof(P2LColorChain, ops), offsetof(P2LColorOp, param),\n'
                   ' offsetof(P2LColorOp, lut), P2L_COLOR_MAX_OPS);\n'
                   'printf("%d %d %d %d %d\\n", P2L_COLOR_BRIGHTNESS, P2L_COLOR_SATURATION, P2L_COLOR_CONTRAST,\n'
                   ' P2L_COLOR_GAMMA, P2L_COLOR_HUE);\nreturn 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split('\n')
    got = [int(v) for v in lines[0].split()]
    assert got == [C.sizeof(CT.P2LColorChain), C.sizeof(CT.P2LColorOp), CT.P2LColorChain.n_ops.offset,
                   CT.P2LColorChain.ops.offset, CT.P2LColorOp.param.offset, CT.P2LColorOp.lut.offset, CT._MAX_OPS]
    assert [int(v) for v in lines[1].split()] == [CT.OP_BRIGHTNESS, CT.OP_SATURATION, CT.OP_CONTRAST,
                                                  CT.OP_GAMMA, CT.OP_HUE]

"""`lpips_size` without a device: the definition of the area pooling (`LF.area_pool_torch`), the host-side guards of
the three entry points of csrc/p2l_pool.hip, and the ValueErrors of the Python layer (shape arithmetic alone)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import pix2latent_amd.loss_functions as LF


@pytest.fixture(scope='module')
def lib():
    from pix2latent_amd import _native as N
    return N.lib()


def test_f2_is_the_four_cell_means():
    x = torch.tensor([[1., 2., 5., 7.],
                      [3., 6., 9., 11.],
                      [-1., -2., 0.5, 0.25],
                      [-3., -4., 1.0, 0.25]]).view(1, 1, 4, 4)
    want = torch.tensor([[3.0, 8.0], [-2.5, 0.5]]).view(1, 1, 2, 2)
    assert torch.equal(LF.area_pool_torch(x, 2), want)
    assert LF.area_pool_torch(x, 1) is x or torch.equal(LF.area_pool_torch(x, 1), x)
    # the association: ((a + b) + (c + d)) * 0.25 in fp32, not a sum in another order
    a, b, c, d = 1.0, 2.0 ** -24, 2.0 ** -24, -1.0
    y = torch.tensor([[a, b], [c, d]]).view(1, 1, 2, 2)
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    assert torch.equal(LF.area_pool_torch(y, 2).view(()), ((t(a) + t(b)) + (t(c) + t(d))) * 0.25)
    assert LF.area_pool_torch(y, 2).item() == 2.0 ** -26        # (1 + 2^-24 rounds to 1; 2^-24 - 1 is exact)


def test_f4_is_f2_twice_and_any_leading_shape():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 5, 16, 24, generator=g) * 2 - 1
    assert torch.equal(LF.area_pool_torch(x, 4), LF.area_pool_torch(LF.area_pool_torch(x, 2), 2))
    assert torch.equal(LF.area_pool_torch(x, 8), LF.area_pool_torch(LF.area_pool_torch(x, 4), 2))
    assert LF.area_pool_torch(x, 8).shape == (2, 5, 2, 3)
    assert torch.equal(LF.area_pool_torch(x[0, 0], 4), LF.area_pool_torch(x, 4)[0, 0])
    for bad in (3, 32, 0):
        with pytest.raises(ValueError):
            LF.area_pool_torch(x, bad)
    with pytest.raises(ValueError):
        LF.area_pool_torch(x, 16)                               # 24 % 16


@pytest.mark.parametrize('f', [2, 4, 8, 16])
def test_against_avg_pool_fp64(f):
    """an fp32 sum of f^2 terms in any order is within (f^2 - 1) 2^-24 max|x| of the exact one; the division by
    f^2 is exact"""
    g = torch.Generator().manual_seed(f)
    x = torch.rand(2, 3, 64, 48, generator=g) * 2 - 1
    got = LF.area_pool_torch(x, f).double()
    ref = F.avg_pool2d(x.double(), f)
    err = (got - ref).abs().max().item()
    bound = (f * f - 1) * 2.0 ** -24 * x.abs().max().item()
    print('f=%d: max err %.3g, bound %.3g' % (f, err, bound))
    assert err <= bound


def test_symbols_and_host_guards(lib):
    """the three entry points exist and refuse before any launch (fake non-null pointers: no device is needed)"""
    from pix2latent_amd import _native as N
    for name in ('p2l_area_pool3_to_nhwc16', 'p2l_area_pool_nchw', 'p2l_area_unpool16_add_nchw3'):
        assert name in N.EXPORTS and hasattr(lib, name)
    fake = C.c_void_p(4096)
    pack, pool, unpool = lib.p2l_area_pool3_to_nhwc16, lib.p2l_area_pool_nchw, lib.p2l_area_unpool16_add_nchw3
    EINVAL = -1
    # NULL pointers
    assert pack(None, fake, 1, 8, 8, 2, None) == EINVAL
    assert pack(fake, None, 1, 8, 8, 2, None) == EINVAL
    assert pool(None, None, fake, 1, 3, 8, 8, 2, None) == EINVAL
    assert pool(fake, None, None, 1, 3, 8, 8, 2, None) == EINVAL
    assert unpool(None, fake, fake, 1, 8, 8, 2, None) == EINVAL
    assert unpool(fake, fake, None, 1, 8, 8, 2, None) == EINVAL
    assert unpool(fake, None, None, 1, 8, 8, 2, None) == EINVAL
    # f = 3 (and the other factors the kernels do not take)
    for f in (3, 0, 1, 32, -2):
        assert pack(fake, fake, 1, 96, 96, f, None) == EINVAL, f
        assert pool(fake, fake, fake, 1, 3, 96, 96, f, None) == EINVAL, f
        assert unpool(fake, fake, fake, 1, 96, 96, f, None) == EINVAL, f
    # H % f != 0, W % f != 0
    for H, W in ((10, 8), (8, 10)):
        assert pack(fake, fake, 1, H, W, 4, None) == EINVAL
        assert pool(fake, None, fake, 1, 3, H, W, 4, None) == EINVAL
        assert unpool(fake, None, fake, 1, H, W, 4, None) == EINVAL
    # Bn < 1 (and C < 1, H < 1)
    for Bn in (0, -1):
        assert pack(fake, fake, Bn, 8, 8, 2, None) == EINVAL
        assert pool(fake, None, fake, Bn, 3, 8, 8, 2, None) == EINVAL
        assert unpool(fake, None, fake, Bn, 8, 8, 2, None) == EINVAL
    assert pool(fake, None, fake, 1, 0, 8, 8, 2, None) == EINVAL
    assert pack(fake, fake, 1, 0, 8, 2, None) == EINVAL
    # misaligned
    odd = C.c_void_p(4100)
    assert pack(odd, fake, 1, 8, 8, 2, None) == EINVAL
    assert pool(fake, odd, fake, 1, 3, 8, 8, 2, None) == EINVAL
    assert unpool(fake, odd, fake, 1, 8, 8, 2, None) == EINVAL
    assert N.ABI_VERSION == lib.p2l_version() == 101


def test_python_layer_value_errors():
    """raised from the shapes alone: no tensor, no device"""
    assert LF.lpips_pool_factor((9, 3, 1024, 1024), None) == 1
    assert LF.lpips_pool_factor((9, 3, 1024, 1024), 1024) == 1
    assert LF.lpips_pool_factor((9, 3, 1024, 1024), 256) == 4
    assert LF.lpips_pool_factor((9, 3, 512, 256), 256) == 2
    assert LF.lpips_pool_factor((1, 3, 1024, 1024), 64) == 16
    with pytest.raises(ValueError, match=r'100, 128'):
        LF.lpips_pool_factor((2, 3, 100, 128), 64)              # H % s != 0
    with pytest.raises(ValueError, match=r'2048, 2048'):
        LF.lpips_pool_factor((2, 3, 2048, 2048), 64)            # f = 32
    with pytest.raises(ValueError, match=r'128, 130'):
        LF.lpips_pool_factor((2, 3, 128, 130), 32)              # W % f != 0
    with pytest.raises(ValueError):
        LF.lpips_pool_factor((2, 3, 192, 192), 64)              # f = 3
    with pytest.raises(ValueError):
        LF.lpips_pool_factor((2, 3, 128, 128), 0)


def test_loss_call_raises_before_anything_else():
    """the loss objects' __call__ asks the same function first: a stand-in that has only `lpips_size`"""
    class Stub(object):
        lpips_size, beta, _engine = 64, 10, None
    out = torch.zeros(1, 3, 100, 128)
    for cls in (LF.ProjectionLoss, LF.PerceptualLoss):
        with pytest.raises(ValueError, match=r'100, 128'):
            cls.__call__(Stub(), out, out)

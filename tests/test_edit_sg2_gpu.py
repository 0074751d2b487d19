"""pix2latent.edit for StyleGAN2 on the MI355X: the wide fp64 Gram kernel (p2l_gram_f64_wide) against numpy
float64, its guard bands, determinism and refusals; w_covariance and stylegan2_components on a size-64
synthetic-weight model; StyleGAN2LatentEditor's renders against direct syntheses, bit for bit."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (1, 17, 4099, 65539)
COLS = (1, 128, 129, 130, 255, 256, 257, 384, 511, 512)
SIZE = 64


def _data(rows, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, 512, generator=g) + 0.25


def _padded(Xd, rows, cols, ld):
    """device buffer with the panel Xd[:, :cols] at row stride ld: the padding columns and three rows behind
    the panel are NaN, so a read outside the panel shows"""
    buf = torch.full((rows + 3, ld), float('nan'), device=Xd.device)
    buf[:rows, :cols] = Xd[:, :cols]
    return buf


@pytest.mark.parametrize('rows', ROWS)
def test_gram_f64_wide_matches_numpy(dev, rows):
    """the bounds of the 128-column kernel (tests/test_edit_gpu.py).  The reference is good for them: at
    65539 x 512 numpy's float64 Gram is within 5.9e-17 |ref|.max() of an np.longdouble Gram (300 sampled
    entries, worst 4.1e-12 against a largest entry of 7.1e4), and its column sums are equal to the longdouble
    ones after rounding -- far below a tenth of 1e-12.  The column counts straddle every 16-column tile and
    128-column panel edge; the row counts are less than one 32-row chunk, a ragged chunk, 17 row ranges and
    the capped 51 ranges of the 10-pair layout."""
    from pix2latent_amd.edit.ganspace import gram_f64_wide
    X = _data(rows, 7 * rows)
    X64 = X.double().numpy()
    ref, ref_sum, ref_abs = X64.T @ X64, X64.sum(0), np.abs(X64).sum(0)
    Xd = X.to(dev)
    for cols in COLS:
        ld = cols + 3
        g, s = gram_f64_wide(_padded(Xd, rows, cols, ld), rows, cols, ld)
        g, s = g.cpu().numpy(), s.cpu().numpy()
        r = ref[:cols, :cols]
        assert g.shape == (cols, cols) and s.shape == (cols,)
        eg, es = np.abs(g - r).max(), np.abs(s - ref_sum[:cols]).max()
        print('rows %d cols %d: |G - ref| %.3g (bound %.3g), |s - ref| %.3g (bound %.3g)'
              % (rows, cols, eg, 1e-12 * np.abs(r).max(), es, 1e-12 * ref_abs[:cols].max()))
        assert eg <= 1e-12 * np.abs(r).max(), (rows, cols)
        assert es <= 1e-12 * ref_abs[:cols].max(), (rows, cols)
        assert (g == g.T).all(), (rows, cols)


@pytest.mark.parametrize('cols', (1, 130, 257, 512))
def test_gram_f64_wide_writes_nothing_outside_its_outputs(dev, cols):
    from pix2latent_amd import _native as N
    L = N.lib()
    rows, ld, guard = 4099, cols + 3, 1024
    X = _data(rows, 3).to(dev)
    buf = _padded(X, rows, cols, ld)
    gbuf = torch.full((cols * cols + 2 * guard,), float('nan'), dtype=torch.float64, device=dev)
    sbuf = torch.full((cols + 2 * guard,), float('nan'), dtype=torch.float64, device=dev)
    need = L.p2l_gram_f64_wide_ws_bytes(rows, cols)
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    assert L.p2l_gram_f64_wide(buf.data_ptr(), rows, cols, ld, gbuf.data_ptr() + 8 * guard,
                               sbuf.data_ptr() + 8 * guard, ws.data_ptr(), need, N.stream()) == 0
    torch.cuda.synchronize()
    for b, n in ((gbuf, cols * cols), (sbuf, cols)):
        assert torch.isnan(b[:guard]).all() and torch.isnan(b[guard + n:]).all()
        assert torch.isfinite(b[guard:guard + n]).all()
    X64 = X[:, :cols].double()
    ref = X64.t() @ X64
    assert (gbuf[guard:guard + cols * cols].view(cols, cols) - ref).abs().max() <= 1e-11 * ref.abs().max()


def test_gram_f64_wide_is_bit_identical_from_call_to_call(dev):
    from pix2latent_amd.edit.ganspace import gram_f64_wide
    rows = 100003
    d = _data(rows, 5).to(dev)
    a = gram_f64_wide(d, rows, 512, 512)
    torch.randn(1 << 20, device=dev)                     # (other work in between)
    b = gram_f64_wide(d, rows, 512, 512)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.isfinite(a[0]).all() and torch.equal(a[0], a[0].t())


def test_gram_f64_wide_refuses_bad_arguments(dev):
    from pix2latent_amd import _native as N
    from pix2latent_amd.edit.ganspace import gram_f64_wide
    L = N.lib()
    x = torch.zeros(64, 512, device=dev)
    g = torch.zeros(512, 512, dtype=torch.float64, device=dev)
    s = torch.zeros(512, dtype=torch.float64, device=dev)
    need = L.p2l_gram_f64_wide_ws_bytes(64, 512)
    ws = torch.zeros(need // 8, dtype=torch.float64, device=dev)
    P = lambda t: t.data_ptr()  # noqa: E731

    def call(rows, cols, ld, X=P(x), G=P(g), S=P(s), nbytes=need, w=P(ws)):
        return L.p2l_gram_f64_wide(X, rows, cols, ld, G, S, w, nbytes, N.stream())
    for args in ((0, 4, 512), (-3, 4, 512), (64, 0, 512), (64, 513, 513), (64, 8, 7), (64, 512, 511)):
        assert call(*args) == -1, args
    assert call(64, 8, 512, X=None) == -1
    assert call(64, 8, 512, G=None) == -1
    assert call(64, 8, 512, S=None) == -1
    assert call(64, 512, 512, nbytes=need - 8) == -3
    assert call(64, 512, 512, w=None) == -3
    for args in ((0, 4), (64, 0), (64, 513)):
        assert L.p2l_gram_f64_wide_ws_bytes(*args) == 0
    x.fill_(1.0)
    torch.cuda.synchronize()
    assert not g.any() and not s.any()                   # nothing was launched
    assert call(64, 512, 512) == 0
    torch.cuda.synchronize()
    assert (g == 64.0).all() and (s == 64.0).all()
    with pytest.raises(ValueError):
        gram_f64_wide(x, 65, 512, 512)                   # the panel does not fit the tensor
    with pytest.raises(ValueError):
        gram_f64_wide(x, 32, 513, 1024)
    with pytest.raises(ValueError):
        gram_f64_wide(x.double(), 64, 512, 512)


# ------------------------------------------------------------------------------------------- the model side
@pytest.fixture(scope='module')
def weights():
    from pix2latent_amd.utils import synthetic as S
    return S.stylegan2_weights(SIZE, 0)


def _model(weights, search, dev):
    from pix2latent_amd.model.stylegan2 import StyleGAN2
    warnings.simplefilter('ignore')
    return StyleGAN2(model='cars', search=search, weights=weights, size=SIZE, device=dev)


@pytest.fixture(scope='module')
def model_z(weights, dev):
    return _model(weights, 'z', dev)


@pytest.fixture(scope='module')
def model_w(weights, dev):
    return _model(weights, 'w+', dev)


def _host_covariance(model, seed, n, chunk):
    """numpy float64 covariance and mean of the same w: the draws of w_covariance under the seed, mapped on
    the device and copied to the host"""
    torch.manual_seed(seed)
    ws = []
    with torch.no_grad():
        for start in range(0, n, chunk):
            ws.append(model.mapping(torch.randn(min(chunk, n - start), 512)).cpu())
    w = torch.cat(ws).double().numpy()
    return np.cov(w, rowvar=False), w.mean(0), np.abs(w).mean(0)


@pytest.mark.parametrize('chunk', (4096, 65536))
def test_w_covariance_matches_numpy(model_z, chunk):
    """8197 samples: three chunks of 4096 with a ragged last one, or one chunk.  The second term of the bound
    covers the centring subtraction G / N - mean mean^T.  The mean is a column sum over N: the kernel's
    column-sum bound, 1e-12 sum |w|, over N."""
    from pix2latent_amd.edit.ganspace import w_covariance
    n = 8197
    torch.manual_seed(21)
    C, mean = w_covariance(model_z, n, chunk_rows=chunk)
    assert C.shape == (512, 512) and mean.shape == (512,)
    assert C.dtype == mean.dtype == torch.float64 and C.device.type == mean.device.type == 'cpu'
    ref_C, ref_mean, ref_abs = _host_covariance(model_z, 21, n, chunk)
    bound = 1e-12 * np.abs(ref_C).max() + 1e-12 * np.abs(ref_mean).max() ** 2
    err = np.abs(C.numpy() - ref_C).max()
    print('chunk %d: |C - ref| %.3g, bound %.3g (|C| %.3g, |mean| %.3g)'
          % (chunk, err, bound, np.abs(ref_C).max(), np.abs(ref_mean).max()))
    assert err <= bound
    assert np.abs(mean.numpy() - ref_mean).max() <= 1e-12 * ref_abs.max()
    assert torch.equal(C, C.t())


def test_stylegan2_components(model_z):
    from pix2latent_amd.edit.ganspace import stylegan2_components
    torch.manual_seed(3)
    V, stdev, mean = stylegan2_components(model_z, num_components=24, num_samples=8197)
    assert V.shape == (24, 512) and stdev.shape == (24,) and mean.shape == (512,)
    for t in (V, stdev, mean):
        assert t.dtype == torch.float32 and t.device.type == 'cuda'
    assert (V @ V.t() - torch.eye(24, device=V.device)).abs().max().item() < 1e-5
    assert (stdev[1:] <= stdev[:-1]).all() and (stdev > 0).all()
    again = stylegan2_components(model_z, num_components=24, num_samples=8197)
    assert all(a is b for a, b in zip(again, (V, stdev, mean)))         # cached on the model
    other = stylegan2_components(model_z, num_components=8, num_samples=8197)
    assert other[0].shape == (8, 512) and other[0] is not V


def _saved_result(path, model, dev):
    """three candidates, the second the best (as tests/test_edit_gpu.py builds its BigGAN result)"""
    from pix2latent_amd import VariableManager, save_variables
    vm = VariableManager(device=dev)
    if model.search == 'z':
        vm.register('z', (512,), 'input')
    else:
        vm.register('z', (model._desc.n_latent, 512), 'input')
        vm.register('noises', (model._desc.noise_total,), 'input')
    torch.manual_seed(4)
    v = vm.initialize(3)
    v['loss'] = [[5, {'loss': np.array([0.3, 0.1, 0.2])}]]
    save_variables(path, v)
    return v


def _stored(model, v, dev):
    """latent [1, n_latent, 512] and noise list of candidate 1, built without the editor"""
    from pix2latent_amd.edit import editor as E
    z = v.input.z.data[1].detach().float().to(dev)
    with torch.no_grad():
        if model.search == 'z':
            latent = model.mapping(z.unsqueeze(0)).unsqueeze(1).repeat(1, model._desc.n_latent, 1)
            g = torch.Generator().manual_seed(E.NOISE_SEED)
            noises = [torch.randn(1, 1, s[-2], s[-1], generator=g).to(dev) for s in model.noise_shape]
        else:
            latent = z.unsqueeze(0)
            noises = model.reshape_noise(v.input.noises.data[1].detach().float().to(dev).unsqueeze(0))
    return latent, noises


@pytest.fixture(scope='module', params=['z', 'w+'])
def edited(request, dev, model_z, model_w, tmp_path_factory):
    from pix2latent_amd.edit import StyleGAN2LatentEditor
    model = model_z if request.param == 'z' else model_w
    path = str(tmp_path_factory.mktemp('edit_sg2') / 'vars.npy')
    v = _saved_result(path, model, dev)
    e = StyleGAN2LatentEditor(model)
    assert e.model is model
    e.load_result(path)
    assert e._idx == 1
    latent, noises = _stored(model, v, dev)
    return e, model, latent, noises


def _synth(model, latent, noises):
    with torch.no_grad():
        return model.synthesis(latent, noises)[0]


def test_editor_renders_are_direct_syntheses(edited):
    e, model, latent, noises = edited
    n_latent = model._desc.n_latent
    assert n_latent == 10 and latent.shape == (1, n_latent, 512)
    base = _synth(model, latent, noises)
    assert base.shape == (3, SIZE, SIZE)
    assert torch.equal(e.default(), base)
    assert torch.equal(e.default(), base)                # (fixed noise: a second render is the same image)
    assert torch.equal(e.edit_w(3, 0.0), base)
    U, sd = e.components, e.stdev
    assert U.shape == (32, 512) and sd.shape == (32,)
    for k, sigma, layers in ((2, 1.5, None), (0, -2.0, range(2, 6)), (5, 3.0, [9])):
        lat = latent.clone()
        rows = list(range(n_latent)) if layers is None else list(layers)
        lat[:, rows] = lat[:, rows] + sigma * sd[k] * U[k]
        want = _synth(model, lat, noises)
        assert torch.equal(e.edit_w(k, sigma, layers), want), (k, sigma, layers)
        assert not torch.equal(want, base)
    all_layers = e.edit_w(2, 1.5)
    assert torch.equal(all_layers, e.edit_w(2, 1.5, range(n_latent)))
    assert not torch.equal(all_layers, e.edit_w(2, 1.5, range(2, 6)))
    for bad in ([n_latent], [-1], [0, 3, n_latent + 2]):
        with pytest.raises(ValueError):
            e.edit_w(0, 1.0, bad)
        with pytest.raises(ValueError):
            e.render_w_sweep([0], [1.0], bad)


@pytest.mark.parametrize('layers', (None, (2, 3, 4, 5)))
def test_render_w_sweep_rows_are_single_renders(edited, layers):
    e = edited[0]
    comps, sigmas = [0, 3], [-2, 0, 2]
    out = e.render_w_sweep(comps, sigmas, layers)
    assert out.shape == (6, 3, SIZE, SIZE)
    for i, k in enumerate(comps):
        for j, s in enumerate(sigmas):
            assert torch.equal(out[i * len(sigmas) + j], e.edit_w(k, s, layers)), (k, s)
    assert e.render_w_sweep([], sigmas).shape == (0, 3, SIZE, SIZE)


def test_render_w_sweep_in_more_than_one_batch(edited):
    e = edited[0]
    comps, sigmas = list(range(7)), [-2.0, 0.5, 3.0]     # 21 images: two batches (18 + 3)
    out = e.render_w_sweep(comps, sigmas, range(4))
    assert out.shape == (21, 3, SIZE, SIZE)
    for i, j in ((0, 0), (5, 2), (6, 0), (6, 2)):        # both sides of the batch edge
        assert torch.equal(out[i * 3 + j], e.edit_w(comps[i], sigmas[j], range(4)))

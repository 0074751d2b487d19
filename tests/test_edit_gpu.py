"""pix2latent.edit on the MI355X: the fp64 Gram kernel (p2l_gram_f64) against numpy float64 in both
layouts, its determinism and refusals; biggan_components against the host path fed by numpy Grams; the
editor's renders against direct forwards, bit for bit; and the reference's example call sequence on a
result that a short inversion saved."""
import os.path as osp
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (1, 17, 4099, 12800, 1 << 20)
COLS = (1, 3, 16, 127, 128)


def _panel(rows, trans, seed):
    """[rows, 128] fp32 data (non-zero mean) and a padded device copy with ld > cols: padding is NaN, so
    a read outside the panel shows"""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(rows, 128, generator=g) + 0.25
    if trans == 0:
        ld = 131
        buf = torch.full((rows, ld), float('nan'))
        buf[:, :128] = X
    else:
        ld = rows + 5
        buf = torch.full((128, ld), float('nan'))
        buf[:, :rows] = X.t()
    return X, buf, ld


@pytest.mark.parametrize('trans', (0, 1))
@pytest.mark.parametrize('rows', ROWS)
def test_gram_f64_matches_numpy(dev, rows, trans):
    from pix2latent_amd.edit.ganspace import gram_f64
    X, buf, ld = _panel(rows, trans, 7 * rows + trans)
    X64 = X.double().numpy()
    ref, ref_sum, ref_abs = X64.T @ X64, X64.sum(0), np.abs(X64).sum(0)
    d = buf.to(dev)
    for cols in COLS:
        g, s = gram_f64(d, rows, cols, ld, trans)
        g, s = g.cpu().numpy(), s.cpu().numpy()
        r = ref[:cols, :cols]
        assert g.shape == (cols, cols) and s.shape == (cols,)
        assert np.abs(g - r).max() <= 1e-12 * np.abs(r).max(), (rows, cols, trans)
        assert np.abs(s - ref_sum[:cols]).max() <= 1e-12 * ref_abs[:cols].max(), (rows, cols, trans)
        assert (g == g.T).all()


def test_gram_f64_is_bit_identical_from_call_to_call(dev):
    from pix2latent_amd.edit.ganspace import gram_f64
    for trans in (0, 1):
        _, buf, ld = _panel(100003, trans, 5)
        d = buf.to(dev)
        a = gram_f64(d, 100003, 128, ld, trans)
        torch.randn(1 << 20, device=dev)                 # (other work in between)
        b = gram_f64(d, 100003, 128, ld, trans)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_gram_f64_refuses_bad_arguments(dev):
    from pix2latent_amd import _native as N
    from pix2latent_amd.edit.ganspace import gram_f64
    L = N.lib()
    x = torch.zeros(64, 128, device=dev)
    g = torch.zeros(128, 128, dtype=torch.float64, device=dev)
    s = torch.zeros(128, dtype=torch.float64, device=dev)
    need = L.p2l_gram_f64_ws_bytes(64, 128, 0)
    ws = torch.zeros(need // 8, dtype=torch.float64, device=dev)
    P = lambda t: t.data_ptr()  # noqa: E731

    def call(rows, cols, ld, trans, X=P(x), nbytes=need, w=P(ws)):
        return L.p2l_gram_f64(X, rows, cols, ld, trans, P(g), P(s), w, nbytes, N.stream())
    for args in ((0, 4, 128, 0), (64, 0, 128, 0), (64, 129, 129, 0), (64, 8, 7, 0), (64, 8, 63, 1),
                 (64, 8, 128, 3)):
        assert call(*args) == -1, args
    assert call(64, 8, 128, 0, X=None) == -1
    assert call(64, 128, 128, 0, nbytes=need - 8) == -3
    assert call(64, 128, 128, 0, w=None) == -3
    torch.cuda.synchronize()
    assert not g.any()                                   # nothing was launched
    assert call(64, 128, 128, 0) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        gram_f64(x, 65, 128, 128, 0)                     # the panel does not fit the tensor
    with pytest.raises(ValueError):
        gram_f64(x, 64, 128, 128, 1)
    with pytest.raises(ValueError):
        gram_f64(x.double(), 64, 128, 128, 0)


@pytest.fixture(scope='module')
def model(dev):
    from pix2latent_amd.model.biggan import BigGAN
    from pix2latent_amd.utils import synthetic as S
    warnings.simplefilter('ignore')
    return BigGAN(weights=S.biggan_weights(0), device=dev)


def _host_reference(model, seed, n, k, method='sgd'):
    """the CPU path fed by S and G computed in numpy from the same draws"""
    from pix2latent_amd.edit import ganspace as GS
    torch.manual_seed(seed)
    z = torch.randn(n, 128)
    u0 = torch.randn(128, k) if method == 'sgd' else None
    z64 = z.double().numpy()
    zc = z64 - z64.mean(0)
    Wz = model._w['generator.gen_z.weight'][:, :128].double().numpy()
    S, G = torch.from_numpy(zc.T @ zc), torch.from_numpy(Wz.T @ Wz)
    return GS.components_from_grams(S, G, n, u0, k, method)


def test_biggan_components_match_the_host_path(dev, model):
    from pix2latent_amd.edit.ganspace import biggan_components
    torch.manual_seed(11)
    got = biggan_components(model, 207)
    assert got.shape == (32, 128) and got.dtype == torch.float32 and got.device.type == 'cuda'
    ref = _host_reference(model, 11, 12800, 32)
    assert (got.cpu().double() - ref).abs().max().item() < 1e-5
    assert model._ganspace_gram.shape == (128, 128)      # G is cached on the model
    torch.manual_seed(11)
    again = biggan_components(model, model.get_class_embedding(3))     # (the class does not matter)
    assert torch.equal(got, again)
    torch.manual_seed(12)
    got = biggan_components(model, 0, num_components=10, num_samples=5000, method='lstsq')
    ref = _host_reference(model, 12, 5000, 10, 'lstsq')
    assert (got.cpu().double() - ref).abs().max().item() < 1e-5


def _saved_result(path, model, dev):
    from pix2latent_amd import VariableManager, save_variables
    vm = VariableManager(device=dev)
    vm.register('z', (128,), 'input')
    vm.register('c', (128,), 'input', default=model.get_class_embedding(153)[0])
    torch.manual_seed(4)
    v = vm.initialize(3)
    v['loss'] = [[5, {'loss': np.array([0.3, 0.1, 0.2])}]]
    save_variables(path, v)
    return v


@pytest.fixture(scope='module')
def editor(dev, model, tmp_path_factory):
    from pix2latent_amd.edit import BigGANLatentEditor
    path = str(tmp_path_factory.mktemp('edit') / 'vars.npy')
    v = _saved_result(path, model, dev)
    e = BigGANLatentEditor(model)
    assert e.model is model
    e.load_result(path)
    assert e._idx == 1
    assert torch.equal(e._z.cpu(), v.input.z.data[1].detach().cpu().unsqueeze(0))
    return e


def test_editor_renders_are_direct_forwards(editor, model):
    z, c = editor._z, editor._c
    with torch.no_grad():
        base = model(z, c)[0]
    assert base.shape == (3, 256, 256)
    assert torch.equal(editor.default(), base)
    assert torch.equal(editor.edit_z(3, 0.0), base)
    assert torch.equal(editor.edit_class(220, 0.0), base)
    U = editor.components
    assert U.shape == (32, 128)
    with torch.no_grad():
        ez = model(z + 1.5 * U[2:3], c)[0]
        ec = model(z, 0.7 * model.get_class_embedding(220) + (1.0 - 0.7) * c)[0]
    assert torch.equal(editor.edit_z(2, 1.5), ez)
    assert torch.equal(editor.edit_class(220, 0.7), ec)
    assert not torch.equal(ez, base) and not torch.equal(ec, base)


def test_render_z_sweep_rows_are_single_renders(editor):
    comps, sigmas = list(range(7)), [-2.0, 0.5, 3.0]           # 21 images: two batches (18 + 3)
    out = editor.render_z_sweep(comps, sigmas)
    assert out.shape == (21, 3, 256, 256)
    for i, k in enumerate(comps):
        for j, s in enumerate(sigmas):
            assert torch.equal(out[i * len(sigmas) + j], editor.edit_z(k, s)), (k, s)


def test_invert_save_then_edit_like_the_example(dev, model, tmp_path):
    """a short inversion, save_variables, then the reference's examples/edit_biggan.py call sequence"""
    warnings.simplefilter('ignore')
    from pix2latent_amd import VariableManager, save_variables, distribution
    from pix2latent_amd.edit import BigGANLatentEditor
    from pix2latent_amd.optimizer import GradientOptimizer
    from pix2latent_amd.utils import synthetic as S, function_hooks as hook
    import pix2latent_amd.loss_functions as LF
    loss_fn = LF.ProjectionLoss(lpips_net='vgg', weights=S.lpips_vgg_weights(1), device=dev)
    vm = VariableManager(device=dev)
    vm.register('z', (128,), 'input', distribution=distribution.TruncatedNormalModulo(sigma=1.0, trunc=2.0),
                learning_rate=0.05, hook_fn=hook.Clamp(2.0))
    vm.register('c', (128,), 'input', default=model.get_class_embedding(153)[0], learning_rate=0.01)
    vm.register('target', (3, 256, 256), 'output', requires_grad=False, default=S.synthetic_target(256, 1))
    vm.register('weight', (3, 256, 256), 'output', requires_grad=False, default=S.synthetic_weight_mask(256))
    torch.manual_seed(5)
    opt = GradientOptimizer(model, vm, loss_fn, max_batch_size=9, log=False)
    variables, out, loss = opt.optimize(num_samples=3, grad_steps=2)
    variables.loss = loss
    path = osp.join(str(tmp_path), 'vars.npy')
    save_variables(path, variables)

    editor = BigGANLatentEditor(model)
    editor.load_result(path)
    out_z = editor.edit_z(component=0, sigma=1.0)
    out_c = editor.edit_class(cls_idx=220, alpha=1.0)
    idx = int(np.argmin(loss[-1][1]['loss']))
    z = variables.input.z.data[idx].detach().unsqueeze(0).float()
    c = variables.input.c.data[idx].detach().unsqueeze(0).float()
    with torch.no_grad():
        best = model(z, c)[0]
        moved = model(z + 1.0 * editor.components[0:1], c)[0]
        swapped = model(z, model.get_class_embedding(220))[0]
    assert out_z.shape == out_c.shape == (3, 256, 256)
    assert torch.isfinite(out_z).all() and torch.isfinite(out_c).all()
    assert torch.equal(editor.default(), best)
    assert torch.equal(out_z, moved) and torch.equal(out_c, swapped)
    assert not torch.equal(out_z, best)

"""StyleSpace (S) search of StyleGAN2 on the device: the synthesis behind the affines (pixels, bits, gradients, chain
rule, invariance) against the CPU oracle composed in tests/_sg2_style_ref.py, the column moments and the StylePrior
term against fp64, the closure with the styles as the optimised variable, and the channel editor.

Networks: the 64^2 synthetic ones of tests/test_stylegan2_gpu.py in its `wide` and `narrow` width tables, 3 candidates.
Gradients are held to that file's rule, unchanged (`grad_close`, `free_running_bound`)."""
import warnings

import numpy as np
import pytest
import torch

import _sg2_style_ref as SR
from test_stylegan2_gpu import SIZE, WIDTHS, d64, free_running_bound, grad_close, rel_rows

pytestmark = pytest.mark.gpu
B = 3
STAT_SAMPLES = 4096


@pytest.fixture(scope='module', params=['wide', 'narrow'])
def sg(request, dev):
    warnings.simplefilter('ignore')
    from pix2latent_amd.utils import synthetic as S
    from pix2latent_amd.model.stylegan2 import StyleGAN2
    from oracle import stylegan2_ref as R
    W = S.stylegan2_weights(SIZE, 0, channels=WIDTHS[request.param])
    model = StyleGAN2(model='cars', search='s', weights=W, size=SIZE, device=dev)
    g = torch.Generator().manual_seed(4)
    wplus = torch.randn(B, R.n_latent(SIZE), 512, generator=g) * 0.5
    flat = torch.cat([torch.randn(B, s[2] * s[3], generator=g) for s in R.noise_shapes(SIZE)], dim=1)
    probe = torch.randn(B, 3, SIZE, SIZE, generator=g) / SIZE
    other = torch.randn(B, R.n_latent(SIZE), 512, generator=g) * 0.5
    with torch.no_grad():
        # the oracle's own styles, moved off the range of the affines by 0.1 std of noise; computed once, left unchanged
        s0 = SR.styles(W, wplus, SIZE)
        styles = (s0 + 0.1 * s0.std() * torch.randn(s0.shape, generator=torch.Generator().manual_seed(104))).contiguous()
        ref = SR.forward_s(W, styles, flat, SIZE)
    return dict(W=W, model=model, wplus=wplus, flat=flat, probe=probe, other=other, R=R, width=request.param,
                styles=styles, ref=ref)


# ---- 0. layout of the model ------------------------------------------------------------------------------------------
def test_model_layout_and_styles_against_the_oracle(sg, dev):
    from pix2latent_amd.model.stylegan2 import style_layout
    model = sg['model']
    sl = SR.slices(sg['W'], SIZE)
    assert [(e.name, e.kind, e.offset, e.channels) for e in model.style_layout] == [(p, k, o, c) for p, k, _, o, c in sl]
    assert list(model.style_layout) == style_layout(SIZE, WIDTHS[sg['width']])
    assert model.n_styles == sl[-1][3] + sl[-1][4] == sg['styles'].shape[1]
    st = model.styles(sg['wplus'].to(dev))
    assert st.shape == (B, model.n_styles) and not st.requires_grad
    ref = SR.styles(sg['W'], sg['wplus'], SIZE)
    assert (st.cpu() - ref).abs().max().item() < 1e-5 * ref.abs().max().item()
    # one w for all layers
    w1 = sg['wplus'][:, 0].to(dev)
    assert torch.equal(model.styles(w1), model.styles(w1.unsqueeze(1).repeat(1, model._desc.n_latent, 1)))
    # a copy: a later forward leaves it alone
    keep = st.clone()
    with torch.no_grad():
        model.forward_w(sg['other'].to(dev), sg['flat'].to(dev))
    assert torch.equal(st, keep)
    assert model.latent_mean.shape == (512,) and model.latent_std.dim() == 0      # what W+ search sets
    with pytest.raises(ValueError, match='S_total = %d' % model.n_styles):
        model(sg['styles'][:, :-1].to(dev), sg['flat'].to(dev))
    with pytest.raises(ValueError, match='feat / skip'):
        model(sg['styles'].to(dev), sg['flat'].to(dev), feat=torch.zeros(1), skip=torch.zeros(1))


# ---- 1. forward pixels -----------------------------------------------------------------------------------------------
def test_forward_pixels_against_the_oracle(sg, dev):
    model = sg['model']
    with torch.no_grad():
        model.forward_w(sg['other'].to(dev), sg['flat'].to(dev))       # a stale workspace must not pass
        out = model(sg['styles'].to(dev), sg['flat'].to(dev))
    assert out.shape == sg['ref'].shape
    err = (out.cpu() - sg['ref']).abs().max().item()
    print('%s: max |forward_s - oracle| = %.3g' % (sg['width'], err))
    assert err < 2e-5


# ---- 2. forward_w = forward_s(styles) --------------------------------------------------------------------------------
def test_forward_w_is_forward_s_of_its_styles(sg, dev):
    model = sg['model']
    wd, nd = sg['wplus'].to(dev), sg['flat'].to(dev)
    with torch.no_grad():
        full = model.forward_w(wd, nd).clone()
        st = model.styles(wd)
        model.forward_w(sg['other'].to(dev), nd)
        part = model.forward_s(st, nd)
    print('%s: max |forward_w - forward_s(styles)| = %.3g' % (sg['width'], (full - part).abs().max().item()))
    assert torch.equal(full, part)


# ---- 3. gradients ----------------------------------------------------------------------------------------------------
def test_gradients_against_the_oracle(sg, dev):
    model, W = sg['model'], sg['W']
    dev_in = [t.to(dev).requires_grad_(True) for t in (sg['styles'], sg['flat'])]
    out = model.forward_s(*dev_in)
    (out * sg['probe'].to(dev)).sum().backward()
    tape = SR.decisions(model, B, out)
    got = [t.grad for t in dev_in]

    def oracle(dtype, tape):
        Wd = W if dtype == torch.float32 else d64(W)
        leaves = [t.to(dtype).clone().requires_grad_(True) for t in (sg['styles'], sg['flat'])]
        if tape is None:
            (SR.forward_s(Wd, *leaves, SIZE) * sg['probe'].to(dtype)).sum().backward()
        else:
            with sg['R'].replay(tape):
                (SR.forward_s(Wd, *leaves, SIZE) * sg['probe'].to(dtype)).sum().backward()
        return [t.grad for t in leaves]

    g32, g64, free = oracle(torch.float32, tape), oracle(torch.float64, tape), oracle(torch.float64, None)
    for name, a, r32, r64, rf in zip(('dstyles', 'dnoise'), got, g32, g64, free):
        assert a.shape == r64.shape, name
        print(name, 'native vs fp64', rel_rows(a, r64), 'fp32 oracle vs fp64', rel_rows(r32, r64))
        grad_close(a, r32, r64, name)
        free_running_bound(a, rf, name)
    for e in model.style_layout:
        assert got[0][:, e.offset:e.offset + e.channels].abs().max().item() > 0, e
    # NULL gradients: without a noise gradient none is computed, and dstyles keeps its bits
    part = [sg['styles'].to(dev).requires_grad_(True), sg['flat'].to(dev)]
    (model.forward_s(*part) * sg['probe'].to(dev)).sum().backward()
    assert torch.equal(part[0].grad, got[0]) and part[1].grad is None
    only_n = [sg['styles'].to(dev), sg['flat'].to(dev).requires_grad_(True)]
    (model.forward_s(*only_n) * sg['probe'].to(dev)).sum().backward()
    assert torch.equal(only_n[1].grad, got[1]) and only_n[0].grad is None


# ---- 4. chain rule against the W+ path -------------------------------------------------------------------------------
def test_chain_rule_against_the_wplus_path(sg, dev):
    model = sg['model']
    wd = sg['wplus'].to(dev).requires_grad_(True)
    nd = sg['flat'].to(dev)
    (model.forward_w(wd, nd) * sg['probe'].to(dev)).sum().backward()
    st = model.styles(sg['wplus'].to(dev)).requires_grad_(True)
    (model.forward_s(st, nd) * sg['probe'].to(dev)).sum().backward()
    pushed = SR.affine_transpose(sg['W'], st.grad, SIZE, model._desc.n_latent)
    dist = rel_rows(wd.grad, pushed)
    print('%s: dW+ vs dstyles through the affine transposes, per candidate: %s' % (sg['width'], dist))
    assert bool((dist < 1e-5).all()), dist


# ---- 5. bits ---------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch(sg, dev):
    model = sg['model']
    base = [t.to(dev) for t in (sg['styles'], sg['flat'])]
    probe = sg['probe'].to(dev)

    def run(rows):
        idx = torch.tensor(rows, device=dev)
        leaves = [t[idx].clone().requires_grad_(True) for t in base]
        out = model.forward_s(*leaves)
        (out * probe[idx]).sum().backward()
        return [out.detach().clone()] + [t.grad.clone() for t in leaves]

    names = ('image', 'dstyles', 'dnoise')
    a = run([0, 1, 2])
    for x, y, what in zip(a, run([0, 1, 2]), names):
        assert torch.equal(x, y), 'a repeated forward + backward differs in %s' % what
    for x, y, what in zip(a, run([1]), names):
        assert torch.equal(x[1:2], y), '%s of a candidate depends on the batch composition' % what
    perm = [2, 0, 1]
    for x, y, what in zip(a, run(perm), names):
        assert torch.equal(x[perm], y), '%s of a candidate depends on its row' % what


# ---- 6. column moments -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1), (7, 130), (4096, 33), (1000, 'S_total')], ids=lambda s: '%sx%s' % s)
def test_col_moments_against_fp64(dev, shape):
    from pix2latent_amd import ops
    from pix2latent_amd.model.stylegan2 import style_layout
    lay = style_layout(SIZE, WIDTHS['narrow'])
    rows, cols = shape[0], (lay[-1].offset + lay[-1].channels if shape[1] == 'S_total' else shape[1])
    assert cols != 'S_total' and (shape[1] != 'S_total' or cols == 1120)      # the narrow network's S_total
    g = torch.Generator().manual_seed(rows + cols)
    x = (torch.randn(rows, cols, generator=g) * 3.0 + 1.0)
    xd = x.to(dev)
    s, q = ops.col_moments_f64(xd)
    assert s.dtype == q.dtype == torch.float64 and s.shape == q.shape == (cols,)
    x64 = x.numpy().astype(np.float64)
    # rows * 2^-53 relative to the sum of magnitudes: 4.6e-13 at 4096 rows
    assert (np.abs(s.cpu().numpy() - x64.sum(0)) <= 1e-12 * np.abs(x64).sum(0)).all()
    assert (np.abs(q.cpu().numpy() - (x64 * x64).sum(0)) <= 1e-12 * (x64 * x64).sum(0)).all()
    # two accumulated chunks cut at a fixed row give the bits of the one call; a one-row matrix cannot be cut, so
    # there the accumulating call continues from zeros
    cut = min(3, rows - 1)
    if cut:
        s2, q2 = ops.col_moments_f64(xd[:cut].contiguous())
    else:
        s2, q2 = torch.zeros_like(s), torch.zeros_like(q)
    r2 = ops.col_moments_f64(xd[cut:].contiguous(), s2, q2)
    assert r2[0] is s2 and torch.equal(s2, s) and torch.equal(q2, q)
    # ld padding: the same columns inside a wider matrix
    wide = torch.full((rows, cols + 3), 7.0, device=dev)
    wide[:, :cols] = xd
    s3, q3 = ops.col_moments_f64(wide[:, :cols])
    assert torch.equal(s3, s) and torch.equal(q3, q)


def test_style_stats_are_the_moments_of_mapped_styles(sg, dev):
    model = sg['model']
    mean, std = model.style_stats(num_samples=STAT_SAMPLES, seed=11)
    assert mean.dtype == std.dtype == torch.float64 and mean.shape == std.shape == (model.n_styles,)
    assert model.style_stats(num_samples=STAT_SAMPLES, seed=11)[0] is mean                   # cached
    z = torch.randn(STAT_SAMPLES, 512, generator=torch.Generator().manual_seed(11)).to(dev)
    with torch.no_grad():
        st = model.styles(model.mapping(z)).double()
    rm, rs = st.mean(0), st.std(0, unbiased=False)
    em, es = ((mean - rm).abs() / rm.abs()).max().item(), ((std - rs).abs() / rs).max().item()
    print('%s: style_stats vs torch fp64: mean %.3g, std %.3g relative; std range %.3g .. %.3g'
          % (sg['width'], em, es, rs.min().item(), rs.max().item()))
    assert em <= 1e-9 and es <= 1e-9
    # chunked: the sums go on from chunk to chunk, the bits of the one call
    m2, s2 = model.style_stats(num_samples=STAT_SAMPLES, chunk_rows=STAT_SAMPLES, seed=11)
    assert torch.equal(m2, mean) and torch.equal(s2, std)


# ---- 7. StylePrior ---------------------------------------------------------------------------------------------------
def _ulp_close(got, ref64):
    """within one fp32 ulp of the fp64 reference rounded to fp32 (tests/test_sg2_feature_gpu.py, restated)"""
    ref32 = ref64.astype(np.float32)
    return np.abs(got.astype(np.float64) - ref32.astype(np.float64)) <= np.spacing(np.abs(ref32)).astype(np.float64)


@pytest.mark.parametrize('nb', [1, 3])
@pytest.mark.parametrize('n', [1, 63, 513, 4097, 9088])
def test_style_prior_against_fp64(dev, n, nb):
    import pix2latent_amd.loss_functions as LF
    g = torch.Generator().manual_seed(n + nb)
    weight = 0.37
    x = torch.randn(nb, n, generator=g) + 1.0
    center = torch.randn(n, generator=g, dtype=torch.float64) + 1.0
    scale = torch.rand(n, generator=g, dtype=torch.float64) + 0.05
    gloss = torch.tensor([1.0, 2.0, -1.0][:nb])
    reg = LF.StylePrior(center, scale, weight=weight)

    def run(xx, gl):
        xd = xx.to(dev).requires_grad_(True)
        loss = reg(xd)
        (loss * gl.to(dev)).sum().backward()
        return loss.detach().cpu(), xd.grad.cpu()

    loss, grad = run(x, gloss)
    assert loss.shape == (nb,) and loss.dtype == torch.float32 and grad.shape == x.shape
    d = (x.double().numpy() - center.numpy()[None]) / scale.numpy()[None]
    ref_loss = weight * (d * d).sum(1) / n
    ref_grad = gloss.double().numpy()[:, None] * (2.0 * weight / n) * d / scale.numpy()[None]
    assert _ulp_close(loss.numpy(), ref_loss).all(), (loss.numpy(), ref_loss)
    assert _ulp_close(grad.numpy(), ref_grad).all()
    assert torch.equal(reg(x.to(dev)).cpu(), loss)                      # forward-only, and twice: the same bits
    assert _ulp_close(LF.style_prior_torch(x, center, scale, weight).numpy(), ref_loss).all()
    _, unit = run(x, torch.ones(nb))
    assert torch.equal(grad[0], unit[0])
    if nb == 3:
        assert torch.equal(grad[1], 2 * unit[1]) and torch.equal(grad[2], -unit[2])
        for b in range(nb):
            l1, g1 = run(x[b:b + 1], gloss[b:b + 1])
            assert torch.equal(l1, loss[b:b + 1]) and torch.equal(g1, grad[b:b + 1])
        perm = [2, 0, 1]
        lp, gp = run(x[perm], gloss[perm])
        assert torch.equal(lp, loss[perm]) and torch.equal(gp, grad[perm])


def test_style_prior_constructors(sg, dev):
    import pix2latent_amd.loss_functions as LF
    model = sg['model']
    mean, std = model.style_stats(num_samples=STAT_SAMPLES)
    reg = LF.StylePrior.stylegan2(model, num_samples=STAT_SAMPLES, weight=2.0, min_std=1e-3)
    assert torch.equal(reg.center, mean.cpu()) and torch.equal(reg.scale, std.cpu().clamp(min=1e-3))
    # in-distribution styles score about the weight
    z = torch.randn(64, 512, generator=torch.Generator().manual_seed(5)).to(dev)
    score = reg(model.styles(model.mapping(z))).double().mean().item()
    print('%s: StylePrior.stylegan2 on mapped z: %.4g at weight 2' % (sg['width'], score))
    assert 1.0 < score < 4.0
    # a floor above every std: a finite term
    floor = 2.0 * std.max().item()
    flat_reg = LF.StylePrior.stylegan2(model, num_samples=STAT_SAMPLES, min_std=floor)
    assert bool((flat_reg.scale == floor).all()) and bool(torch.isfinite(flat_reg(sg['styles'].to(dev))).all())
    s0 = model.styles(sg['wplus'][:1].to(dev))
    around = LF.StylePrior.around(s0[0], model, num_samples=STAT_SAMPLES)
    assert torch.equal(around.scale, LF.StylePrior.stylegan2(model, num_samples=STAT_SAMPLES).scale)
    assert around(s0).item() == 0.0 and around(sg['styles'][1:2].to(dev)).item() > 0.0


# ---- 8. closure ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def problem(dev):
    warnings.simplefilter('ignore')
    from pix2latent_amd.utils import synthetic as S
    from pix2latent_amd.model.stylegan2 import StyleGAN2
    import pix2latent_amd.loss_functions as LF
    W = S.stylegan2_weights(SIZE, 0, channels=WIDTHS['narrow'])
    model = StyleGAN2(model='cars', search='s', weights=W, size=SIZE, device=dev)
    loss_fn = LF.ProjectionLoss(lpips_net='vgg', weights=S.lpips_vgg_weights(1), device=dev)
    n_lat = model._desc.n_latent
    g = torch.Generator().manual_seed(4)
    w0 = model.latent_mean.cpu().view(1, 512).repeat(n_lat, 1) + 0.3 * torch.randn(n_lat, 512, generator=g)
    w0 = torch.stack([w0, 1.25 * w0])
    n0 = torch.randn(model._desc.noise_total, generator=g)
    s0 = model.styles(w0.to(dev)).cpu()                                 # styles from a W+ start
    unit = LF.StylePrior.around(s0[0], model, num_samples=STAT_SAMPLES)
    # the weight at which the term of candidate 1 (anchored at candidate 0's start) begins at half the projection
    # loss's O(1)
    aw = 0.5 / unit(s0[1:2]).item()
    print('prior weight %.4g' % aw)
    return dict(aw=aw, model=model, loss_fn=loss_fn, target=S.synthetic_target(SIZE, 1),
                weight=S.synthetic_weight_mask(SIZE), s0=s0, n0=n0)


def _prior(p, **kw):
    import pix2latent_amd.loss_functions as LF
    kw = dict(dict(styles0=p['s0'][0], weight=p['aw']), **kw)
    return LF.StylePrior.around(kw['styles0'], p['model'], num_samples=STAT_SAMPLES, weight=kw['weight'])


def _steps(p, dev, n_steps, use_graph, reg):
    """n_steps optimise steps of 2 different candidates on z (the styles, under the prior) and noises"""
    from pix2latent_amd import VariableManager
    from pix2latent_amd.optimizer import GradientOptimizer
    s0 = p['s0']
    vm = VariableManager(device=dev)
    vm.register('z', tuple(s0.shape[1:]), 'input', learning_rate=0.05, default=s0[0], regularizer=reg)
    vm.register('noises', tuple(p['n0'].shape), 'input', learning_rate=0.05, default=p['n0'])
    vm.register('target', (3, SIZE, SIZE), 'output', requires_grad=False, default=p['target'])
    vm.register('weight', (3, SIZE, SIZE), 'output', requires_grad=False, default=p['weight'])
    opt = GradientOptimizer(p['model'], vm, p['loss_fn'], max_batch_size=9, use_graph=use_graph)
    variables = vm.initialize(num_samples=2)
    with torch.no_grad():
        variables.input.z.buf[1].copy_(s0[1])
    losses = []
    for _ in range(n_steps):
        _, l, _ = opt.step(variables, optimize=True, transform=False)
        losses.append(np.array(l, dtype=np.float64))
    if use_graph:
        assert any(isinstance(v, tuple) for v in opt._graphs.values()), 'no graph was captured'
    return np.stack(losses), variables.input.z.buf.detach().cpu().clone(), opt


def test_closure_optimises_the_styles_under_the_prior(problem, dev):
    import pix2latent_amd.loss_functions as LF
    p = problem
    model, loss_fn = p['model'], p['loss_fn']
    reg = _prior(p)
    losses, z_end, opt = _steps(p, dev, 3, False, reg)
    assert tuple(opt.tracked['z'][0].shape) == tuple(p['s0'].shape)
    for i in range(3):
        z, n = (opt.tracked[k][i].to(dev) for k in ('z', 'noises'))
        with torch.no_grad():
            out = model(z=z, noises=n)
            t = p['target'].to(dev).unsqueeze(0).expand(2, -1, -1, -1).contiguous()
            w = p['weight'].to(dev).unsqueeze(0).expand(2, -1, -1, -1).contiguous()
            base = loss_fn(out, t, w).view(2, -1).mean(1).double().cpu().numpy()
            term = reg(z).double().cpu().numpy()
        ref = LF.style_prior_torch(z.cpu(), reg.center, reg.scale, p['aw']).double().numpy()
        print('step %d: loss_fn %s  prior term %s (fp64 definition %s)  reported %s' % (i, base, term, ref, losses[i]))
        assert (np.abs(term - ref) <= 1e-6 * np.abs(ref)).all()
        assert (np.abs(losses[i] - (base + term)) <= 1e-5 * (base + term)).all()
        # candidate 0 starts on the centre, candidate 1 at its own styles; both terms show at the 1e-5 bound
        assert term[1] > 0.01 * base[1] and (term[0] == 0.0) == (i == 0)
        if i > 0:
            assert term[0] > 1e-4 * base[0]
    assert (z_end - p['s0']).abs().max(1)[0].min().item() > 0.01       # the styles move in both candidates


def test_closure_graph_replay_is_the_eager_trajectory(problem, dev):
    p = problem
    eager = _steps(p, dev, 3, False, _prior(p))
    graph = _steps(p, dev, 3, True, _prior(p))
    assert np.array_equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
    # the key of a captured step tells the centres and the weights apart
    opt = graph[2]
    (_, _, _, _, variables, _), = [v for v in opt._graphs.values() if isinstance(v, tuple)]
    k0 = opt._graph_key(variables, 0, 2)
    assert k0 in opt._graphs
    variables.input.z['regularizer'] = _prior(p, weight=2.0 * p['aw'])
    k1 = opt._graph_key(variables, 0, 2)
    variables.input.z['regularizer'] = _prior(p, styles0=p['s0'][1])
    k2 = opt._graph_key(variables, 0, 2)
    variables.input.z['regularizer'] = _prior(p)
    assert len({k0, k1, k2}) == 3 and opt._graph_key(variables, 0, 2) == k0


# ---- 9. editor -------------------------------------------------------------------------------------------------------
def _saved(path, dev, search, z, noises):
    """three candidates, the second the best, all holding the given z / noises"""
    from pix2latent_amd import VariableManager, save_variables
    vm = VariableManager(device=dev)
    vm.register('z', tuple(z.shape), 'input', default=z)
    vm.register('noises', tuple(noises.shape), 'input', default=noises)
    v = vm.initialize(3)
    v['loss'] = [[5, {'loss': np.array([0.3, 0.1, 0.2])}]]
    save_variables(path, v)


def test_editor_moves_single_channels(dev, tmp_path):
    warnings.simplefilter('ignore')
    from pix2latent_amd.utils import synthetic as S
    from pix2latent_amd.model.stylegan2 import StyleGAN2
    from pix2latent_amd.edit import StyleGAN2LatentEditor
    from pix2latent_amd.edit import editor as E
    W = S.stylegan2_weights(SIZE, 0, channels=WIDTHS['narrow'])
    ms = StyleGAN2(model='cars', search='s', weights=W, size=SIZE, device=dev)
    mw = StyleGAN2(model='cars', search='w+', weights=W, size=SIZE, device=dev)
    g = torch.Generator().manual_seed(9)
    wplus = torch.randn(ms._desc.n_latent, 512, generator=g) * 0.5
    flat = torch.randn(ms._desc.noise_total, generator=g)
    styles = ms.styles(wplus.unsqueeze(0).to(dev))
    _saved(str(tmp_path / 's.npy'), dev, 's', styles[0].cpu(), flat)
    _saved(str(tmp_path / 'w.npy'), dev, 'w+', wplus, flat)
    es, ew = StyleGAN2LatentEditor(ms, style_samples=STAT_SAMPLES), StyleGAN2LatentEditor(mw, style_samples=STAT_SAMPLES)
    es.load_result(str(tmp_path / 's.npy'))
    ew.load_result(str(tmp_path / 'w.npy'))
    assert es._idx == ew._idx == 1 and torch.equal(es._styles, ew._styles) and torch.equal(es._styles, styles)
    nd = flat.view(1, -1).to(dev)
    with torch.no_grad():
        base = ms.forward_s(styles, nd)[0]
    assert torch.equal(es.default(), base) and torch.equal(ew.default(), base)
    std = ms.style_stats(num_samples=STAT_SAMPLES)[1].float()
    assert torch.equal(std, mw.style_stats(num_samples=STAT_SAMPLES)[1].float())
    layout = ms.style_layout
    last = len(layout) - 1
    edits = [(0, 5), (1, 0), (6, layout[6].channels - 1), (last, 3)]
    for layer, ch in edits:
        i = layout[layer].offset + ch
        moved = styles.clone()
        moved[:, i] = moved[:, i] + 2.5 * std[i]
        with torch.no_grad():
            want = ms.forward_s(moved, nd)[0]
        assert torch.equal(es.edit_s(layer, ch, 2.5), want), (layer, ch)
        assert torch.equal(ew.edit_s(layer, ch, 2.5), want), (layer, ch)     # a W+ result renders the same bits
        assert not torch.equal(want, base)
    assert torch.equal(es.edit_s(3, 1, 0.0), base)
    # the sweep, in more than one chunk: every image is the single edit
    sigmas = [-3.0, -1.0, 0.0, 1.0, 3.0]
    out = es.render_s_sweep(edits, sigmas)
    assert out.shape == (20, 3, SIZE, SIZE) and E.SWEEP_CHUNK < 20
    for i, (layer, ch) in enumerate(edits):
        for j, s in enumerate(sigmas):
            assert torch.equal(out[i * len(sigmas) + j], es.edit_s(layer, ch, s)), (layer, ch, s)
    assert torch.equal(ew.render_s_sweep(edits[:1], sigmas[:2]), out[:2])
    assert es.render_s_sweep([], sigmas).shape == (0, 3, SIZE, SIZE)
    for bad in ((len(layout), 0), (-1, 0), (0, layout[0].channels), (2, -1), (1.5, 0)):
        with pytest.raises(ValueError):
            es.edit_s(bad[0], bad[1], 1.0)
        with pytest.raises(ValueError):
            es.render_s_sweep([bad], [1.0])
    with pytest.raises(ValueError):
        es.edit_w(0, 1.0)                                                 # no W latent behind an s result

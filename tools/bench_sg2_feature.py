"""Feature-space (F/W+) inversion of StyleGAN2 inside the optimise step: one step of the
cars-512 generator at 9 candidates, synthetic weights, ProjectionLoss (VGG),
  (w+)    z (W+) and the noises optimised, as the projector examples run it;
  (f@16)  z, noises and feat [512,16,16] optimised under LF.FeatureAnchor, skip fixed: the cut at 16;
  (f@32)  the same with feat [512,32,32]: the cut at 32;
and, for each cut, the three pieces the feature path adds to the launches of the W+ step, timed alone on the tensors
of the step: p2l_nchw_to_nhwc of feat (forward), p2l_nhwc_to_nchw of its gradient (backward), and the anchor term's
forward + backward.  Their sum over the step time is the share the table reports.
Device events around every step (and every call of a piece); the median of `--steps` after `--warmup`.
    python tools/bench_sg2_feature.py [--steps 20] [--warmup 5] [--out profiles/sg2_feature.txt]"""
import argparse
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pix2latent_amd.loss_functions as LF  # noqa: E402
from pix2latent_amd import ops  # noqa: E402
from pix2latent_amd.utils import synthetic as S  # noqa: E402

SIZE, CANDIDATES = 512, 9


def median_ms(fn, warm, calls):
    """median over `calls` of the device time of one fn(), each between its own pair of events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return 0.5 * (t[(calls - 1) // 2] + t[calls // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join('profiles', 'sg2_feature.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_sg2_feature.py measures the MI355X'
    warnings.simplefilter('ignore')
    from pix2latent_amd import VariableManager
    from pix2latent_amd.model.stylegan2 import StyleGAN2
    from pix2latent_amd.optimizer import GradientOptimizer
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    Wg = S.stylegan2_weights(SIZE, 0)
    loss_fn = LF.ProjectionLoss(lpips_net='vgg', weights=S.lpips_vgg_weights(1), device=dev)
    target, weight = S.synthetic_target(SIZE, 1), S.synthetic_weight_mask(SIZE)
    g = torch.Generator().manual_seed(2)
    say('cars-%d, %d candidates, ProjectionLoss(vgg); median of %d steps after %d, device events per step'
        % (SIZE, CANDIDATES, a.steps, a.warmup))
    rows = []
    for res in (None, 16, 32):
        gen = StyleGAN2(model='cars', search='w+' if res is None else 'f', f_res=res or 32, weights=Wg, size=SIZE,
                        device=dev)
        n_lat, n_noise = gen._desc.n_latent, gen._desc.noise_total
        z0 = gen.latent_mean.cpu().view(1, 512).repeat(n_lat, 1)
        noise0 = torch.randn(n_noise, generator=g)
        vm = VariableManager(device=dev)
        vm.register('z', (n_lat, 512), 'input', learning_rate=0.05, default=z0)
        vm.register('noises', (n_noise,), 'input', learning_rate=0.05, default=noise0)
        pieces = None
        if res is not None:
            feat0, skip0 = gen.features(z0.unsqueeze(0).to(dev), noise0.view(1, -1).to(dev))
            reg = LF.FeatureAnchor(feat0[0], weight=1.0)
            vm.register('feat', tuple(feat0.shape[1:]), 'input', learning_rate=0.01, default=feat0[0], regularizer=reg)
            vm.register('skip', tuple(skip0.shape[1:]), 'input', requires_grad=False, default=skip0[0])
        vm.register('target', (3, SIZE, SIZE), 'output', requires_grad=False, default=target)
        vm.register('weight', (3, SIZE, SIZE), 'output', requires_grad=False, default=weight)
        opt = GradientOptimizer(gen, vm, loss_fn, max_batch_size=CANDIDATES)
        variables = vm.initialize(num_samples=CANDIDATES)
        first = [True]

        def one():
            opt.step(variables, optimize=True, transform=first[0])
            first[0] = False
        ms = median_ms(one, a.warmup, a.steps)
        replay = bool(getattr(opt, '_graphs', None)) and any(isinstance(v, tuple) for v in opt._graphs.values())
        if res is not None:
            f = variables.input.feat.buf.detach()
            gl = torch.full((CANDIDATES,), 1.0 / CANDIDATES, device=dev)
            nhwc = ops.nchw_to_nhwc(f)
            t_in = median_ms(lambda: ops.nchw_to_nhwc(f), a.warmup, a.steps)
            t_out = median_ms(lambda: ops.nhwc_to_nchw(nhwc), a.warmup, a.steps)
            t_reg = median_ms(lambda: (ops.feature_anchor_fwd(f, reg.anchor, reg.weight),
                                       ops.feature_anchor_bwd(f, reg.anchor, reg.weight, gl)), a.warmup, a.steps)
            pieces = (t_in, t_out, t_reg)
        rows.append((res, ms, pieces, replay, [float(v) for v in opt.loss]))
        del opt, variables, vm, gen
        torch.cuda.empty_cache()
    base = rows[0][1]
    say('%-8s %10s %9s %14s %14s %14s %8s  %s' % ('search', 'step ms', 'vs w+', 'feat in us', 'dfeat out us',
                                                   'anchor f+b us', 'share', 'graph replay'))
    for res, ms, pieces, replay, losses in rows:
        name = 'w+' if res is None else 'f@%d' % res
        if pieces is None:
            say('%-8s %10.3f %9s %14s %14s %14s %8s  %s' % (name, ms, '1.000', '-', '-', '-', '-', replay))
        else:
            say('%-8s %10.3f %9.3f %14.1f %14.1f %14.1f %7.2f%%  %s'
                % (name, ms, ms / base, 1e3 * pieces[0], 1e3 * pieces[1], 1e3 * pieces[2],
                   100.0 * sum(pieces) / ms, replay))
        say('         last losses %s' % ['%.4g' % v for v in losses[:3]])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

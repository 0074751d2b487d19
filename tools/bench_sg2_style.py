"""StyleSpace (S) search of StyleGAN2 inside the optimise step: one step of the cars-512
generator at 9 candidates, synthetic weights, ProjectionLoss (VGG),
  (w+)  z (W+) and the noises optimised, as the projector examples run it;
  (s)   z (the styles [8960], started from the W+ start's styles) under LF.StylePrior.around and the noises;
both of the same library in one session, each measured `--repeats` times in turn (w+, s, w+, s, ...): the ratio
s / w+ is reported next to the spread of the repeated W+ timings, which is what it has to be read against.  Also the
prior term's forward + backward timed alone on the step's variable.
Device events around every step; a repeat is the median of `--steps` after `--warmup`.
    python tools/bench_sg2_style.py [--steps 20] [--warmup 5] [--repeats 3] [--out profiles/sg2_style.txt]"""
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
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--stat-samples', type=int, default=16384, help='mapped z behind the prior\'s channel stds')
    ap.add_argument('--out', default=os.path.join('profiles', 'sg2_style.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_sg2_style.py measures the MI355X'
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
    say('cars-%d, %d candidates, ProjectionLoss(vgg); %d repeats in turn, each the median of %d steps after %d, device '
        'events per step' % (SIZE, CANDIDATES, a.repeats, a.steps, a.warmup))
    runs = {}
    for search in ('w+', 's'):
        gen = StyleGAN2(model='cars', search=search, weights=Wg, size=SIZE, device=dev)
        n_lat, n_noise = gen._desc.n_latent, gen._desc.noise_total
        w0 = gen.latent_mean.cpu().view(1, 512).repeat(n_lat, 1)
        noise0 = torch.randn(n_noise, generator=g)
        vm = VariableManager(device=dev)
        reg = None
        if search == 'w+':
            vm.register('z', (n_lat, 512), 'input', learning_rate=0.05, default=w0)
        else:
            s0 = gen.styles(w0.unsqueeze(0).to(dev))[0].cpu()
            reg = LF.StylePrior.around(s0, gen, num_samples=a.stat_samples, weight=1.0)
            vm.register('z', (gen.n_styles,), 'input', learning_rate=0.01, default=s0, regularizer=reg)
        vm.register('noises', (n_noise,), 'input', learning_rate=0.05, default=noise0)
        vm.register('target', (3, SIZE, SIZE), 'output', requires_grad=False, default=target)
        vm.register('weight', (3, SIZE, SIZE), 'output', requires_grad=False, default=weight)
        opt = GradientOptimizer(gen, vm, loss_fn, max_batch_size=CANDIDATES)
        variables = vm.initialize(num_samples=CANDIDATES)
        first = [True]

        def one(opt=opt, variables=variables, first=first):
            opt.step(variables, optimize=True, transform=first[0])
            first[0] = False
        runs[search] = dict(one=one, opt=opt, variables=variables, reg=reg, gen=gen, ms=[])
    for r in range(a.repeats):
        for search in ('w+', 's'):
            runs[search]['ms'].append(median_ms(runs[search]['one'], a.warmup, a.steps))
    rs = runs['s']
    x = rs['variables'].input.z.buf.detach()
    gl = torch.full((CANDIDATES,), 1.0 / CANDIDATES, device=dev)
    center, inv = rs['reg']._device_tensors(dev)
    t_reg = median_ms(lambda: (ops.diag_prior_fwd(x, center, inv, 1.0), ops.diag_prior_bwd(x, center, inv, 1.0, gl)),
                      a.warmup, a.steps)
    med = {k: sorted(v['ms'])[len(v['ms']) // 2] for k, v in runs.items()}
    say('%-7s %10s  %-34s %s' % ('search', 'step ms', 'repeats ms', 'graph replay'))
    for search in ('w+', 's'):
        opt = runs[search]['opt']
        replay = bool(getattr(opt, '_graphs', None)) and any(isinstance(v, tuple) for v in opt._graphs.values())
        say('%-7s %10.3f  %-34s %s' % (search, med[search], ' '.join('%.3f' % t for t in runs[search]['ms']), replay))
        say('        last losses %s' % ['%.4g' % float(v) for v in opt.loss[:3]])
    wp = runs['w+']['ms']
    say('s / w+ = %.4f (medians of the repeats); the W+ repeats span %.3f .. %.3f ms = +-%.2f%% of their median'
        % (med['s'] / med['w+'], min(wp), max(wp), 50.0 * (max(wp) - min(wp)) / med['w+']))
    say('StylePrior forward + backward alone: %.1f us (%.2f%% of the s step)' % (1e3 * t_reg, 100.0 * t_reg / med['s']))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""Whitened latent prior alone and inside the C5 step.
  (a) native forward + backward (p2l_latent_prior_fwd / _bwd through the autograd Function) at the W+ shape of a
      22-candidate generation, B = 22, L = 18, D = K = 512, p_space on, eager;
  (b) the same 3 launches captured once and replayed from a graph: what the device spends.  The kernels are bound by
      the latency of their fp64 FMA chains, not by bandwidth: the figure is set against the 2 x 0.1 G FMA of work;
  (c) the torch restatement (`LF.latent_prior_torch`, forward + autograd backward) on the same device tensors;
  (d) the step of bench.py's `stylegan2_ffhq_1024_shard3_wplus` problem (3 candidates, W+ and noises optimised,
      synthetic weights) as it is, and with `LatentPrior.stylegan2` on z; `--rounds` alternating measurements of each,
      so that the difference can be read against the run-to-run spread.
Device events around 20 calls after the warm-up calls; (d) is skipped with --no-step.
    python tools/bench_latent_prior.py [--calls 20] [--rounds 3] [--no-step] [--out profiles/latent_prior.txt]"""
import argparse
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pix2latent_amd.loss_functions as LF  # noqa: E402
from pix2latent_amd.utils import synthetic as S  # noqa: E402

FP64_FMA_TFLOPS = 78.6          # vector fp64 peak of the MI355X, 2 flops per FMA


def per_call_ms(fn, warm, calls):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--samples', type=int, default=32768, help='z draws behind the statistics of (d)')
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_latent_prior.py measures the MI355X'
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, L, D = 22, 18, 512
    g = torch.Generator().manual_seed(0)
    # statistics of a 512-dimensional sample with a decaying spectrum: K = D = 512 kept
    X = torch.randn(4096, D, generator=g, dtype=torch.float64) * torch.logspace(0, -2, D, dtype=torch.float64).sqrt()
    prior = LF.LatentPrior.from_samples(X + 0.1, p_space=True, device=dev)
    K = prior.num_components
    x = (0.5 * torch.randn(B, L, D, generator=g)).to(dev).requires_grad_(True)
    gl = torch.linspace(0.5, 2.0, B).to(dev)

    def fwd_bwd(fn):
        x.grad = None
        (fn(x) * gl).sum().backward()

    ms_a = per_call_ms(lambda: fwd_bwd(lambda t: LF.latent_prior(t, prior)), 5, a.calls)
    g_a = x.grad.clone()
    basis, basis_t, mean, lw = prior._device_tensors(dev, L)
    ms_c = per_call_ms(lambda: fwd_bwd(lambda t: LF.latent_prior_torch(t, basis, mean, lw, True)), 3, a.calls)
    dg = ((x.grad - g_a).abs().max() / g_a.abs().max()).item()
    say('W+ shape B = %d, L = %d, D = %d, K = %d, p_space on, %d calls after warm-up' % (B, L, D, K, a.calls))
    say('(a) native forward + backward        : %9.1f us per call   through autograd, eager: 3 launches of ours + torch\'s '
        'mul / sum / fill and the autograd engine on the host' % (1e3 * ms_a))
    from pix2latent_amd import ops
    xd = x.detach()

    def graph_of(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            keep = fn()
        return gr, keep

    def native():
        P, ws = ops.latent_prior_fwd(xd, basis_t, mean, lw, True)
        return P, ws, ops.latent_prior_bwd(xd, basis, lw, True, ws, gl)
    gr_f, _ = graph_of(lambda: ops.latent_prior_fwd(xd, basis_t, mean, lw, True))
    gr_fb, keep = graph_of(native)
    ms_f = per_call_ms(gr_f.replay, 5, a.calls)
    ms_fb = per_call_ms(gr_fb.replay, 5, a.calls)
    assert torch.equal(keep[2], g_a), 'the replayed launches give other bits than the eager ones'
    fma = 2.0 * B * L * D * K
    say('(b) the 3 launches replayed from a graph: %6.1f us per call (forward\'s 2 alone %.1f us)   %.2f G fp64 FMA over '
        '%.1f MB of basis: %.2f TFLOP/s of %.1f -- latency-bound (chains of D / 4 dependent FMAs), not bandwidth-bound'
        % (1e3 * ms_fb, 1e3 * ms_f, fma / 1e9, 2 * D * K * 8 / 1e6, 2 * fma / (ms_fb * 1e-3) / 1e12, FP64_FMA_TFLOPS))
    say('(c) torch restatement fwd + autograd : %9.1f us per call   (%.1f x (a), %.1f x (b); gradients differ by %.1e of '
        'the largest entry)' % (1e3 * ms_c, ms_c / ms_a, ms_c / ms_fb, dg))

    if not a.no_step:
        warnings.simplefilter('ignore')
        from pix2latent_amd import VariableManager
        from pix2latent_amd.model.stylegan2 import StyleGAN2
        from pix2latent_amd.optimizer import GradientOptimizer
        gen = StyleGAN2(model='ffhq', search='w+', device=dev)
        n_noise = sum(s_[-2] * s_[-1] for s_ in gen.noise_shape)
        loss_fn = LF.ProjectionLoss(lpips_net='vgg', weights=S.lpips_vgg_weights(1), device=dev)
        g = torch.Generator().manual_seed(2)
        noise0 = torch.randn(n_noise, generator=g)
        torch.manual_seed(3)
        reg = LF.LatentPrior.stylegan2(gen, num_components=512, num_samples=a.samples)
        configs = (('as bench.py builds it', {}),
                   ('+ LatentPrior.stylegan2 on z (K = %d)' % reg.num_components, dict(regularizer=reg)))
        res = {name: [] for name, _ in configs}
        for rnd in range(a.rounds):
            for name, kw in configs:
                vm = VariableManager(device=dev)
                vm.register('z', (18, 512), 'input', learning_rate=0.05,
                            default=gen.latent_mean.cpu().view(1, 512).repeat(18, 1), **kw)
                vm.register('noises', (n_noise,), 'input', learning_rate=0.05, default=noise0)
                vm.register('target', (3, 1024, 1024), 'output', requires_grad=False,
                            default=S.synthetic_target(1024, 1))
                vm.register('weight', (3, 1024, 1024), 'output', requires_grad=False,
                            default=S.synthetic_weight_mask(1024))
                opt = GradientOptimizer(gen, vm, loss_fn, max_batch_size=9)
                variables = vm.initialize(num_samples=3)
                first = [True]

                def one():
                    opt.step(variables, optimize=True, transform=first[0])
                    first[0] = False
                res[name].append(per_call_ms(one, 4, a.calls))
                replay = bool(opt._graphs) and any(isinstance(v, tuple) for v in opt._graphs.values())
                say('(d) round %d, C5 step, %-40s: %8.2f ms per step (graph replay: %s; last losses %s)'
                    % (rnd, name, res[name][-1], replay, ['%.4g' % float(v) for v in opt.loss]))
                del opt, variables, vm
                torch.cuda.empty_cache()
        (n0, m0), (n1, m1) = res.items()
        mean0, mean1 = sum(m0) / len(m0), sum(m1) / len(m1)
        say('    without: mean %.3f ms, spread %.3f ms   with: mean %.3f ms, spread %.3f ms   difference of the means '
            '%.3f ms per step (%.2f %%)' % (mean0, max(m0) - min(m0), mean1, max(m1) - min(m1), mean1 - mean0,
                                            100.0 * (mean1 - mean0) / mean0))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

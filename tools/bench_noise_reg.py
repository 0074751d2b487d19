"""Noise regulariser and per-layer normalisation alone and inside the C5 step.
  (a) native forward + backward (p2l_sg2_noise_reg_fwd / _bwd through the autograd Function) at the FFHQ-1024
      layer list, B = 3, against the traffic floor: noises read twice and dnoises written once at 6.3 TB/s;
  (b) the torch restatement (`LF.noise_regularize_torch`, forward + autograd backward) on the same device tensors;
  (c) the step of bench.py's `stylegan2_ffhq_1024_shard3_wplus` problem (3 candidates, W+ and noises optimised,
      synthetic weights) as it is, and with `NoiseNormalize` + `NoiseRegularizer` on the noise variable.
Device events around 20 calls after the warm-up calls; (c) is skipped with --no-step.
    python tools/bench_noise_reg.py [--calls 20] [--no-step] [--out profiles/noise_reg_bench.txt]"""
import argparse
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pix2latent_amd.loss_functions as LF  # noqa: E402
from pix2latent_amd.utils import function_hooks as hook, synthetic as S  # noqa: E402

FFHQ1024 = [4] + [r for k in range(3, 11) for r in (2 ** k, 2 ** k)]
HBM_TBPS = 6.3


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
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_noise_reg.py measures the MI355X'
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T = 3, sum(r * r for r in FFHQ1024)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, generator=g).to(dev).requires_grad_(True)
    gl = torch.tensor([1.0, 0.5, 2.0], device=dev)

    def fwd_bwd(fn):
        x.grad = None
        (fn(x, FFHQ1024) * gl).sum().backward()

    floor_us = 3.0 * B * T * 4 / (HBM_TBPS * 1e12) * 1e6
    ms_a = per_call_ms(lambda: fwd_bwd(LF.noise_regularize), 5, a.calls)
    g_a = x.grad.clone()
    ms_b = per_call_ms(lambda: fwd_bwd(LF.noise_regularize_torch), 3, a.calls)
    dg = ((x.grad - g_a).abs().max() / g_a.abs().max()).item()
    say('layer list FFHQ-1024 (17 layers, 73 levels, %d floats per candidate), B = %d, %d calls after warm-up' % (T, B, a.calls))
    say('(a) native forward + backward        : %9.1f us per call   through autograd, eager: 4 launches of ours + torch\'s '
        'mul / sum / fill and the autograd engine on the host' % (1e3 * ms_a))
    # the same 4 launches alone, captured once and replayed: what the device spends
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
    gr_f, _ = graph_of(lambda: ops.noise_reg_fwd(xd, FFHQ1024))
    gr_fb, keep = graph_of(lambda: (lambda l, c, ws: (l, ws, ops.noise_reg_bwd(xd, FFHQ1024, ws, gl)))(
        *ops.noise_reg_fwd(xd, FFHQ1024)))
    ms_f = per_call_ms(gr_f.replay, 5, a.calls)
    ms_fb = per_call_ms(gr_fb.replay, 5, a.calls)
    assert torch.equal(keep[2], g_a), 'the replayed launches give other bits than the eager ones'
    say('    the 4 launches replayed from a graph: %8.1f us per call (forward\'s 3 alone %.1f us)   floor %.1f us = 3 passes '
        'over %.2f MB at %.1f TB/s -> %.2f of the floor rate'
        % (1e3 * ms_fb, 1e3 * ms_f, floor_us, B * T * 4 / 1e6, HBM_TBPS, floor_us / (1e3 * ms_fb)))
    say('(b) torch restatement fwd + autograd : %9.1f us per call   (%.1f x (a); gradients differ by %.1e of the largest entry)'
        % (1e3 * ms_b, ms_b / ms_a, dg))
    rows = x.detach().clone()
    h = hook.NoiseNormalize(FFHQ1024)
    say('    NoiseNormalize, one call          : %9.1f us per call' % (1e3 * per_call_ms(lambda: h.apply_batched(rows), 5, a.calls)))

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
        res = {}
        for name, kw in (('as bench.py builds it', {}),
                         ('+ NoiseNormalize + NoiseRegularizer', dict(hook_fn=hook.NoiseNormalize(gen.noise_shape),
                                                                      regularizer=LF.NoiseRegularizer(gen.noise_shape)))):
            vm = VariableManager(device=dev)
            vm.register('z', (18, 512), 'input', learning_rate=0.05,
                        default=gen.latent_mean.cpu().view(1, 512).repeat(18, 1))
            vm.register('noises', (n_noise,), 'input', learning_rate=0.05, default=noise0, **kw)
            vm.register('target', (3, 1024, 1024), 'output', requires_grad=False, default=S.synthetic_target(1024, 1))
            vm.register('weight', (3, 1024, 1024), 'output', requires_grad=False,
                        default=S.synthetic_weight_mask(1024))
            opt = GradientOptimizer(gen, vm, loss_fn, max_batch_size=9)
            variables = vm.initialize(num_samples=3)
            first = [True]

            def one():
                opt.step(variables, optimize=True, transform=first[0])
                first[0] = False
            res[name] = per_call_ms(one, 4, a.calls)
            replay = bool(opt._graphs) and any(isinstance(v, tuple) for v in opt._graphs.values())
            say('(c) C5 step, %-36s: %8.2f ms per step (graph replay: %s; last losses %s)'
                % (name, res[name], replay, ['%.4g' % float(v) for v in opt.loss]))
            del opt, variables, vm
            torch.cuda.empty_cache()
        ms = list(res.values())
        say('    difference: %.3f ms per step (%.2f %%)' % (ms[1] - ms[0], 100.0 * (ms[1] - ms[0]) / ms[0]))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

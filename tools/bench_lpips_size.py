"""What `lpips_size` is worth on the device.  The comparison point is lpips_size=None on the
same build: the parent's kernels.
  (a) the loss alone, forward + backward, ProjectionLoss('vgg') on B = 9 images: 1024^2 with lpips_size in
      {None, 512, 256}, 512^2 with {None, 256}; device events around `--calls` calls after the warm-up calls;
  (b) the two per-step launches the option adds (pool + pack, unpool + add) on the same shapes, alone, against
      their traffic floor at 6.3 TB/s: the image read once + the pooled NHWC16 written, and the two 16-channel
      gradients read (the full one in whole 64-byte pixels: the layout p2l_l1_loss_bwd writes) + the gradient
      written; the once-per-target launch (p2l_area_pool_nchw) is listed and not counted.  The 20 calls run on the
      same buffers, so up to 256 MB of them may stay in the Infinity Cache from call to call (as the image the
      generator has just written may in a step): the floors are HBM figures;
  (c) one step of bench.py's `stylegan2_ffhq_1024_shard3_wplus` and `stylegan2_cars_512_n32` problems (synthetic
      weights) with lpips_size in {None, 256}: the median of 3 timings of `--steps` steps, as bench.py takes them.
    python tools/bench_lpips_size.py [--calls 10] [--steps 6] [--no-step] [--out profiles/lpips_size.txt]"""
import argparse
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pix2latent_amd.loss_functions as LF  # noqa: E402
from pix2latent_amd import ops  # noqa: E402
from pix2latent_amd.utils import function_hooks as hook, synthetic as S  # noqa: E402

HBM_TBPS = 6.3
B = 9


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


def median_step_s(fn, n_warm, n, reps=3):
    """bench.py `_time_steps`"""
    for i in range(n_warm):
        fn(i == 0)
    per = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn(False)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / n)
    return sorted(per)[len(per) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_lpips_size.py measures the MI355X'
    warnings.simplefilter('ignore')
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    Wv = S.lpips_vgg_weights(1)
    say('(a) ProjectionLoss(vgg) alone, forward + backward, B = %d, %d calls after 3 warm-up calls (device events)'
        % (B, a.calls))
    loss_ms = {}
    for size, sizes in ((1024, (None, 512, 256)), (512, (None, 256))):
        g = torch.Generator().manual_seed(size)
        target = S.synthetic_target(size, 1).unsqueeze(0).repeat(B, 1, 1, 1).to(dev)
        weight = S.synthetic_weight_mask(size).unsqueeze(0).repeat(B, 1, 1, 1).to(dev)
        out = (target + 0.2 * torch.randn(B, 3, size, size, generator=g).to(dev)).clamp(-1, 1).requires_grad_(True)
        for s in sizes:
            loss_fn = LF.ProjectionLoss(lpips_net='vgg', weights=Wv, device=dev, lpips_size=s)

            def fwd_bwd():
                out.grad = None
                loss_fn(out, target, weight).mean().backward()
            ms = loss_ms[(size, s)] = per_call_ms(fwd_bwd, 3, a.calls)
            base = loss_ms[(size, None)]
            say('    %4d^2  lpips_size=%-4s : %9.3f ms per call   x %.2f of lpips_size=None   (f = %d, f^2 = %d)'
                % (size, s, ms, ms / base, size // (s or size), (size // (s or size)) ** 2))
            del loss_fn
            torch.cuda.empty_cache()
        say('(b) the added launches alone at %d^2, B = %d' % (size, B))
        x = out.detach()
        for s in sizes[1:]:
            f = size // s
            small16 = torch.empty(B, s, s, 16, device=dev)
            d_small = torch.randn(B, s, s, 16, device=dev)
            d_full = torch.randn(B, size, size, 16, device=dev)
            dout = torch.empty(B, 3, size, size, device=dev)
            img = B * 3 * size * size * 4
            ms_p = per_call_ms(lambda: ops.area_pool3_to_nhwc16(x, f, out=small16), 3, 20)
            ms_u = per_call_ms(lambda: ops.area_unpool16_add_nchw3(d_small, d_full, f, out=dout), 3, 20)
            ms_n = per_call_ms(lambda: ops.area_pool_nchw(x, f, mul=x), 3, 20)
            fl_p = (img + B * s * s * 64) / (HBM_TBPS * 1e12) * 1e3
            fl_u = (B * size * size * 64 + B * s * s * 64 + img) / (HBM_TBPS * 1e12) * 1e3
            tot = loss_ms[(size, s)]
            say('    f = %-2d pool + pack %7.1f us (floor %6.1f us)   unpool + add %7.1f us (floor %6.1f us)   together '
                '%.1f %% of the %.3f ms of lpips_size=%d   [once per target: pool_nchw with mul %.1f us]'
                % (f, 1e3 * ms_p, 1e3 * fl_p, 1e3 * ms_u, 1e3 * fl_u, 100.0 * (ms_p + ms_u) / tot, tot, s, 1e3 * ms_n))
            del small16, d_small, d_full, dout
        del target, weight, out, x
        torch.cuda.empty_cache()

    if not a.no_step:
        from pix2latent_amd import VariableManager, distribution
        from pix2latent_amd.model.stylegan2 import StyleGAN2
        from pix2latent_amd.optimizer import GradientOptimizer
        say('(c) optimiser steps of bench.py\'s config.extra problems: median of 3 timings of %d steps after 4 untimed '
            'ones' % a.steps)
        g = torch.Generator().manual_seed(2)

        def steps(name, model, make_vm, n, **kw):
            res = {}
            for s in (None, 256):
                loss_fn = LF.ProjectionLoss(lpips_net='vgg', weights=Wv, device=dev, lpips_size=s)
                vm = make_vm()
                opt = GradientOptimizer(model, vm, loss_fn, max_batch_size=9, **kw)
                variables = vm.initialize(num_samples=n)
                dt = res[s] = median_step_s(lambda first: opt.step(variables, optimize=True, transform=first), 4,
                                            a.steps)
                replay = bool(opt._graphs) and any(isinstance(v, tuple) for v in opt._graphs.values())
                say('    %-34s lpips_size=%-4s : %8.2f ms per step  %7.1f evals/s  (graph replay: %s)'
                    % (name, s, 1e3 * dt, n / dt, replay))
                del opt, variables, loss_fn, vm
                torch.cuda.empty_cache()
            say('    %-34s step time x %.2f, evals/s x %.2f' % (name, res[256] / res[None], res[None] / res[256]))

        gen = StyleGAN2(model='ffhq', search='w+', device=dev)
        n_noise = sum(s_[-2] * s_[-1] for s_ in gen.noise_shape)
        noise0 = torch.randn(n_noise, generator=g)

        def vm_ffhq():
            vm = VariableManager(device=dev)
            vm.register('z', (18, 512), 'input', learning_rate=0.05,
                        default=gen.latent_mean.cpu().view(1, 512).repeat(18, 1))
            vm.register('noises', (n_noise,), 'input', learning_rate=0.05, default=noise0)
            vm.register('target', (3, 1024, 1024), 'output', requires_grad=False, default=S.synthetic_target(1024, 1))
            vm.register('weight', (3, 1024, 1024), 'output', requires_grad=False,
                        default=S.synthetic_weight_mask(1024))
            return vm
        steps('stylegan2_ffhq_1024_shard3_wplus', gen, vm_ffhq, 3)
        del gen
        torch.cuda.empty_cache()

        gen = StyleGAN2(model='cars', search='z', device=dev)
        fixed = [torch.randn(1, 1, s_[2], s_[3], generator=g).to(dev) for s_ in gen.noise_shape]

        class FixedNoise(torch.nn.Module):
            def forward(self, z=None):
                return gen.forward_z(z, noises=[n_.expand(z.size(0), -1, -1, -1).contiguous() for n_ in fixed])

        def vm_cars():
            vm = VariableManager(device=dev)
            vm.register('z', (512,), 'input', distribution=distribution.TruncatedNormalModulo(), learning_rate=0.05,
                        hook_fn=hook.Compose(hook.NormalPerturb(sigma=0.05), hook.Clamp(2.0)))
            mask = torch.zeros(3, 512, 512)
            mask[:, 64:-64, :] += 1.0
            for nm, t in (('target', S.synthetic_target(512, 1)), ('weight', torch.ones(3, 512, 512)),
                          ('loss_mask', mask)):
                vm.register(nm, (3, 512, 512), 'output', requires_grad=False, default=t)
            return vm
        steps('stylegan2_cars_512_n32', FixedNoise(), vm_cars, 32, exec_batch_size='all')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

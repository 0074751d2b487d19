"""What the weighted L2 pixel term and the scheduled Adam step cost on the device.  GPU only.
  (1) the L2 term, forward + backward, on B = 9 images of 1024^2 and of 512^2 (weight, no mask):
        l2 kernels   p2l_l2_loss_fwd + p2l_l2_loss_bwd (accumulate = 0) on staged NHWC16 images
        l1 kernels   p2l_l1_loss_fwd + p2l_l1_loss_bwd on the same buffers
        l2 native    ReconstructionLoss('l2') end to end: staging, kernels, unpack (what a caller pays)
        l2 torch     the torch expression on the device with autograd: what 'l2' ran before the kernels existed
      The algorithmic bytes are from the shapes: per pixel 16 B of the image (floats 0..3 of its 64-byte pixel) and
      12 B of each plane read (target, weight), forward and backward, plus the 64-byte gradient pixel written.
  (2) p2l_adam_step_sched against p2l_adam_step_dev at 8.4 M elements (the StyleGAN2 noise variable) and at 18 x 128;
      `_dev` is measured twice, so its own spread is known.
Variants alternate inside one process: `--rounds` rounds, each timing every variant once over `--calls` calls between
two device events after warm-up calls; the table gives the median over rounds and [min, max].
    python tools/bench_pixel_sched.py [--rounds 5] [--calls 20] [--out profiles/pixel_sched.txt]"""
import argparse
import ctypes as C
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pix2latent_amd.loss_functions as LF  # noqa: E402
from pix2latent_amd import _native as N  # noqa: E402
from pix2latent_amd.utils import synthetic as S  # noqa: E402

B = 9


def timed_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(variants, rounds, calls, warm=3):
    """{name: fn} -> {name: (median, min, max) ms per call}; every round times every variant once, in order"""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    seen = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            seen[k].append(timed_ms(fn, calls))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in seen.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_pixel_sched.py measures the MI355X'
    warnings.simplefilter('ignore')
    dev = torch.device('cuda:0')
    lib = N.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('(1) weighted pixel term, forward + backward, B = %d: median of %d rounds x %d calls [min, max] (device events)'
        % (B, a.rounds, a.calls))
    for size in (1024, 512):
        g = torch.Generator().manual_seed(size)
        HW = size * size
        target = S.synthetic_target(size, 1).unsqueeze(0).repeat(B, 1, 1, 1).to(dev)
        weight = S.synthetic_weight_mask(size).unsqueeze(0).repeat(B, 1, 1, 1).to(dev)
        out = (target + 0.2 * torch.randn(B, 3, size, size, generator=g).to(dev)).clamp(-1, 1).requires_grad_(True)
        img16 = torch.empty(B, HW, 16, device=dev)
        N.check(lib.p2l_nchw3_to_nhwc16(N.ptr(out.detach()), N.ptr(img16), B, size, size, N.stream()))
        dimg16 = torch.empty(B, HW, 16, device=dev)
        wsum, loss, gs = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.full((B,), 1.0 / B, device=dev)
        N.check(lib.p2l_weight_sum(N.ptr(weight), None, N.ptr(wsum), B, 3 * HW, N.stream()))
        part = torch.empty(B * max(lib.p2l_l1_loss_nblk(size, size), lib.p2l_l2_loss_nblk(size, size)), device=dev)
        st = N.stream()

        def kernels(fwd, bwd):
            def run():
                N.check(fwd(N.ptr(img16), N.ptr(target), N.ptr(weight), None, N.ptr(wsum), N.ptr(loss), N.ptr(part),
                            B, size, size, st))
                N.check(bwd(N.ptr(img16), N.ptr(target), N.ptr(weight), None, N.ptr(wsum), N.ptr(gs), N.ptr(dimg16),
                            B, size, size, 0, st))
            return run

        rl2 = LF.ReconstructionLoss('l2')

        def native():
            out.grad = None
            rl2(out, target, weight).mean().backward()

        def torch_expr():
            out.grad = None
            (torch.sum(LF.l2_loss(out, target) * weight, [1, 2, 3]) / torch.sum(weight, [1, 2, 3])).mean().backward()

        res = alternate({'l2 kernels': kernels(lib.p2l_l2_loss_fwd, lib.p2l_l2_loss_bwd),
                         'l1 kernels': kernels(lib.p2l_l1_loss_fwd, lib.p2l_l1_loss_bwd),
                         'l2 native': native, 'l2 torch': torch_expr}, a.rounds, a.calls)
        nbytes = B * HW * ((16 + 2 * 12) * 2 + 64)
        say('    %d^2: algorithmic bytes of the two kernels %.1f MB (reads 2 x %d B, write 64 B per pixel)'
            % (size, nbytes / 1e6, 16 + 2 * 12))
        for k, (med, lo, hi) in res.items():
            rate = '  %7.0f GB/s' % (nbytes / (med * 1e-3) / 1e9) if k.endswith('kernels') else ''
            say('      %-11s %9.3f ms  [%.3f, %.3f]%s' % (k, med, lo, hi, rate))
        say('      l2 kernels / l1 kernels = %.2f   l2 native / l2 torch = %.2f'
            % (res['l2 kernels'][0] / res['l1 kernels'][0], res['l2 native'][0] / res['l2 torch'][0]))
        del target, weight, out, img16, dimg16, part, rl2
        torch.cuda.empty_cache()

    say('(2) Adam step, lr as a launch argument (dev) and from a device table (sched): median of %d rounds x %d calls '
        '[min, max]' % (a.rounds, 10 * a.calls))
    table = torch.full((1000,), 0.05, device=dev)
    for n, n_counters in ((8400000, 3), (18 * 128, 18)):
        g = torch.Generator().manual_seed(n)
        p = torch.randn(n, generator=g).to(dev)
        grad = (1e-3 * torch.randn(n, generator=g)).to(dev)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        steps = torch.zeros(n_counters, dtype=torch.int32, device=dev)
        sp, st = C.c_void_p(steps.data_ptr()), N.stream()

        def adam_dev():
            N.check(lib.p2l_adam_step_dev(N.ptr(p), N.ptr(grad), N.ptr(m), N.ptr(v), n, 0.05, 0.9, 0.999, 1e-8, sp,
                                          n_counters, st))

        def adam_sched():
            N.check(lib.p2l_adam_step_sched(N.ptr(p), N.ptr(grad), N.ptr(m), N.ptr(v), n, N.ptr(table), 1000, 0.9,
                                            0.999, 1e-8, sp, n_counters, st))

        res = alternate({'dev (a)': adam_dev, 'sched': adam_sched, 'dev (b)': adam_dev}, a.rounds, 10 * a.calls)
        say('    n = %d, %d counters (7 floats of traffic per element: %.1f MB)' % (n, n_counters, 28.0 * n / 1e6))
        for k, (med, lo, hi) in res.items():
            say('      %-8s %9.2f us  [%.2f, %.2f]' % (k, 1e3 * med, 1e3 * lo, 1e3 * hi))
        dev_lo = min(res['dev (a)'][1], res['dev (b)'][1])
        dev_hi = max(res['dev (a)'][2], res['dev (b)'][2])
        say('      sched median %s dev\'s own spread [%.2f, %.2f] us'
            % ('within' if dev_lo <= res['sched'][0] <= dev_hi else 'OUTSIDE', 1e3 * dev_lo, 1e3 * dev_hi))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

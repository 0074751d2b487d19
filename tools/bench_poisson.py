"""Poisson blend alone: ms per call of poisson_blend_tensors (p2l_poisson_blend, one block per system) for disk
masks of radius 0.4 * S at S = 256, 512 and 1024, B = 1 and 18, three channels, default tol = 1e-8; the CG
iterations of the slowest system and the achieved rate of state traffic.  State traffic per unknown and iteration:
9 fp64 accesses (p for the p.Ap pass; p, x, r read and x, r written by the update pass; r, p read and p written by
the direction pass -- the four stencil neighbours of p counted as cache hits), i.e. 72 bytes.  Device events; the
first call is a warm-up, the number of timed calls follows its duration.
--forward adds the yardstick the blend is held against: one BigGAN-deep-256 forward of 18 (synthetic weights).
    python tools/bench_poisson.py [--sizes 256,512,1024] [--batches 1,18] [--forward] [--json out.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pix2latent_amd.utils import image as I  # noqa: E402


def images(B, S, dev, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing='ij')
    return (0.5 * (0.6 * yy - 0.4 * xx + 2 * torch.rand(B, 3, S, S, generator=g) - 1)).to(dev)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='256,512,1024')
    ap.add_argument('--batches', default='1,18')
    ap.add_argument('--forward', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_poisson.py measures the MI355X'
    dev = torch.device('cuda:0')
    rows = []
    for S in [int(s) for s in a.sizes.split(',')]:
        yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing='ij')
        mask = ((yy - S / 2) ** 2 + (xx - S / 2) ** 2 <= (0.4 * S) ** 2).to(dev)
        n = int(mask[1:-1, 1:-1].sum())
        for B in [int(b) for b in a.batches.split(',')]:
            target, gen = images(1, S, dev, 0), images(B, S, dev, 1)
            fn = lambda: I.poisson_blend_tensors(target, mask, gen, return_info=True)  # noqa: E731
            warm, _ = timed(fn)
            reps = 1 if warm > 500 else 3 if warm > 50 else 10
            ms = []
            for _ in range(reps):
                t, (out, iters, relres) = timed(fn)
                ms.append(t)
            ms = sorted(ms)[len(ms) // 2]
            it = iters.flatten().tolist()
            gbps = 72.0 * n * sum(it) / ms / 1e6
            rows.append({'size': S, 'B': B, 'unknowns': n, 'ms': ms, 'reps': reps, 'iters_max': max(it),
                         'iters_min': min(it), 'relres_max': float(relres.max()), 'state_GBps': gbps})
            print('%4d^2  B %2d  n %6d x %2d systems : %9.2f ms per call (median of %2d)  iters %4d..%4d  relres <= %.1e  '
                  '%7.1f GB/s state traffic' % (S, B, n, 3 * B, ms, reps, min(it), max(it), float(relres.max()), gbps))
    if a.forward:
        from pix2latent_amd.model.biggan import BigGAN
        from pix2latent_amd.utils import synthetic
        model = BigGAN(weights=synthetic.biggan_weights(0), device=dev)
        g = torch.Generator().manual_seed(2)
        z = torch.fmod(torch.randn(18, 128, generator=g), 2.0).to(dev)
        c = (0.05 * torch.randn(1, 128, generator=g)).repeat(18, 1).to(dev)
        with torch.no_grad():
            fwd = lambda: model(z=z, c=c)  # noqa: E731
            timed(fwd)
            ms = sorted(timed(fwd)[0] for _ in range(10))[5]
        rows.append({'biggan_forward_18_ms': ms})
        print('BigGAN-deep-256 forward of 18: %.2f ms (median of 10)' % ms)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()

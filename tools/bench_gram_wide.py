"""The wide fp64 Gram kernel (p2l_gram_f64_wide) on the MI355X at 512 columns and the GANSpace paper's sample
counts, next to its two yardsticks, all in one run:
  * the torch route on the same panel: X.double().T @ X.double(), the conversion included;
  * the 128-column kernel (p2l_gram_f64) at 10^6 rows: its fraction of the fp64 matrix peak.
and stylegan2_components end to end at its default size.

A figure is the mean over `--calls` calls between two device events, after 3 warm-up calls; it is taken five
times and reported as median [min, max], so that the spread is on record with it.  A Gram call is two
launches (the Gram kernel and its finish kernel).  Rates:
  * fp64 TFLOP/s, algorithmic: rows * cols * (cols + 1) (one multiply-add per entry of the upper triangle),
    and as issued: 2 * 16 * 16 * rows per 16 x 16 tile, 36 tiles per diagonal and 64 per off-diagonal pair of
    128-column panels (528 tiles at 512 columns); the torch route issues the full 2 * rows * cols^2;
  * GB/s: the panel read once, rows * cols * 4 bytes.
  * of peak: issued TFLOP/s over 78.6 (fp64 matrix, AMD's specification).
stylegan2_components: host clock around the whole call with an empty cache (CPU draw of z, upload, mapping,
Gram per chunk, 512 x 512 eigh on the host), median of 3 after 1 warm-up call.
    python tools/bench_gram_wide.py [--json out.json]"""
import argparse
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pix2latent_amd.edit import ganspace as GS  # noqa: E402

PEAK_TFLOPS = 78.6
REPEATS = 5


def timed(fn, calls):
    """median, min and max over REPEATS of the mean ms per call"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    out.sort()
    return out[REPEATS // 2], out[0], out[-1]


def issued_tiles(cols):
    npan = (cols + 127) // 128
    return 36 * npan + 64 * (npan * (npan - 1) // 2)


def report(name, rows, cols, t, flop, issued):
    ms, lo, hi = t
    r = {'case': name, 'rows': rows, 'cols': cols, 'ms': ms, 'ms_min': lo, 'ms_max': hi,
         'TFLOPs': flop / ms / 1e9, 'issued_TFLOPs': issued / ms / 1e9,
         'of_peak': issued / ms / 1e9 / PEAK_TFLOPS, 'GBps': rows * cols * 4.0 / ms / 1e6}
    print('%-22s rows %8d cols %3d: %8.4f ms [%8.4f, %8.4f]  %6.2f TFLOP/s (%6.2f issued, %4.2f of peak)  '
          '%6.0f GB/s' % (name, rows, cols, ms, lo, hi, r['TFLOPs'], r['issued_TFLOPs'], r['of_peak'], r['GBps']))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--calls', type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_gram_wide.py measures the MI355X'
    dev = torch.device('cuda:0')
    warnings.simplefilter('ignore')
    out = []
    for rows in (100000, 1000000):
        cols = 512
        x = torch.randn(rows, cols, device=dev)
        tri = rows * cols * (cols + 1.0)
        t_k = timed(lambda: GS.gram_f64_wide(x, rows, cols, cols), a.calls)
        out.append(report('p2l_gram_f64_wide', rows, cols, t_k, tri, issued_tiles(cols) * 512.0 * rows))

        def torch_route():
            xd = x.double()
            return xd.t() @ xd
        t_t = timed(torch_route, a.calls)
        out.append(report('torch double().T @', rows, cols, t_t, tri, 2.0 * rows * cols * cols))
        verdict = 'not slower' if t_k[0] <= t_t[0] + max(t_t[2] - t_t[1], t_k[2] - t_k[1]) else 'SLOWER'
        print('  the kernel is %s than the torch route at %d rows: %.4f against %.4f ms (spreads %.4f and %.4f)'
              % (verdict, rows, t_k[0], t_t[0], t_k[2] - t_k[1], t_t[2] - t_t[1]))
        if rows == 1000000:
            x128 = x[:, :128].contiguous()
            t_n = timed(lambda: GS.gram_f64(x128, rows, 128, 128), a.calls)
            out.append(report('p2l_gram_f64 (128)', rows, 128, t_n, rows * 128 * 129.0, 36 * 512.0 * rows))
            del x128
        del x
    torch.cuda.empty_cache()
    from pix2latent_amd.model.stylegan2 import StyleGAN2
    from pix2latent_amd.utils import synthetic as S
    model = StyleGAN2(model='cars', search='z', weights=S.stylegan2_weights(64, 0), size=64, device=dev)
    t = []
    for i in range(4):
        model._ganspace_w = {}
        torch.manual_seed(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        GS.stylegan2_components(model)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(t[1:])[1]
    C = torch.eye(512, dtype=torch.float64) + 0.1
    t0 = time.perf_counter()
    GS.components_from_covariance(C, 32)
    host = (time.perf_counter() - t0) * 1e3
    z = torch.randn(65536, 512)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        model.mapping(z)
    torch.cuda.synchronize()
    mapping = (time.perf_counter() - t0) * 1e3
    out.append({'case': 'stylegan2_components', 'num_samples': 100000, 'ms': ms, 'host_eigh_ms': host,
                'mapping_65536_ms': mapping})
    print('stylegan2_components num_samples   100000: %8.1f ms (the host eigh alone: %.1f ms; the upload and '
          'mapping of one 65536-row chunk alone: %.1f ms)' % (ms, host, mapping))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()

"""GANSpace editing on the MI355X: the fp64 Gram kernel (p2l_gram_f64) alone and biggan_components end to
end, at the reference's N = 12 800 samples and the GANSpace paper's 10^6.

Gram kernel: device events over 20 calls after 3 warm-up calls (the two launches of one call: the Gram
kernel and its finish kernel).  Rates over that time:
  * fp64 TFLOP/s, algorithmic: rows * cols * (cols + 1) (one multiply-add per entry of the upper triangle)
    and as issued: 36 tiles * 2 * 16 * 16 * rows (v_mfma_f64_16x16x4_f64, diagonal tiles in full);
  * GB/s: the panel read once, rows * cols * 4 bytes.
biggan_components: host clock around the whole call, which ends in a device-to-host copy (CPU draw of z,
upload, kernel, 128 x 128 algebra and 100 Adam steps on the host), median of 3 after 1 warm-up call.
    python tools/bench_edit.py [--json out.json]"""
import argparse
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pix2latent_amd.edit import ganspace as GS  # noqa: E402


def time_gram(x, rows, cols, ld, trans, reps=20):
    for _ in range(3):
        GS.gram_f64(x, rows, cols, ld, trans)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        GS.gram_f64(x, rows, cols, ld, trans)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_edit.py measures the MI355X'
    dev = torch.device('cuda:0')
    warnings.simplefilter('ignore')
    from pix2latent_amd.model.biggan import BigGAN
    from pix2latent_amd.utils import synthetic as S
    model = BigGAN(weights=S.biggan_weights(0), device=dev)
    rows_out = []
    w = model._genz_wt
    cases = [('samples', 12800, 0, None), ('samples', 1000000, 0, None),
             ('genz_w (G)', w.shape[1], 1, w)]
    for name, rows, trans, x in cases:
        cols = 128
        if x is None:
            x = torch.randn(rows, cols, device=dev)
        ld = cols if trans == 0 else x.shape[1]
        ms = time_gram(x, rows, cols, ld, trans)
        flop = rows * cols * (cols + 1.0)
        mfma_flop = 36 * 2 * 16 * 16 * float(rows)
        nbytes = rows * cols * 4.0
        r = {'case': 'gram ' + name, 'rows': rows, 'trans': trans, 'ms': ms, 'TFLOPs': flop / ms / 1e9,
             'mfma_TFLOPs': mfma_flop / ms / 1e9, 'GBps': nbytes / ms / 1e6}
        rows_out.append(r)
        print('p2l_gram_f64 %-10s rows %8d trans %d: %8.4f ms  %6.2f TFLOP/s (%6.2f issued)  %7.0f GB/s'
              % (name, rows, trans, ms, r['TFLOPs'], r['mfma_TFLOPs'], r['GBps']))
        del x
    for n in (12800, 1000000):
        GS.biggan_components(model, 0, num_samples=n)
        t = []
        for i in range(3):
            torch.manual_seed(i)
            t0 = time.perf_counter()
            GS.biggan_components(model, 0, num_samples=n)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        ms = sorted(t)[1]
        S_ = torch.eye(128, dtype=torch.float64) * n
        t0 = time.perf_counter()
        GS.components_from_grams(S_ + 0.1, model._ganspace_gram, n, torch.randn(128, 32))
        host = (time.perf_counter() - t0) * 1e3
        rows_out.append({'case': 'biggan_components', 'num_samples': n, 'ms': ms, 'host_algebra_ms': host})
        print('biggan_components num_samples %8d: %8.1f ms (the host algebra + Adam alone: %.1f ms)' % (n, ms, host))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(rows_out, f, indent=1)


if __name__ == '__main__':
    main()

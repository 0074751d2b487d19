"""Colour-transform kernel alone: GB/s of p2l_color_adjust per launch (algorithmic bytes: the image read
once and written once per launch; a contrast op's pre-pass reads it once more) at 18 x 3 x 256^2 and
22 x 3 x 1024^2, per op and for the reference's five-op chain.  Device events over 20 calls after 3
warm-up calls.  The 256^2 batch (14 MB each way) stays in the 256 MB Infinity Cache between calls; the
1024^2 batch (277 MB each way) does not.  Compare with tools/micro/mem_rate.hip (HBM copy rate).
    python tools/bench_color.py [--json out.json]"""
import argparse
import ctypes as ct
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pix2latent_amd import _native as N  # noqa: E402
from pix2latent_amd.transform import color_transform as CT  # noqa: E402

CASES = [('brightness', [CT.OP_BRIGHTNESS]), ('saturation', [CT.OP_SATURATION]), ('gamma', [CT.OP_GAMMA]),
         ('hue', [CT.OP_HUE]), ('contrast', [CT.OP_CONTRAST]),
         ('chain5', [CT.OP_HUE, CT.OP_GAMMA, CT.OP_SATURATION, CT.OP_BRIGHTNESS, CT.OP_CONTRAST])]
VALUE = {CT.OP_HUE: 0.13, CT.OP_GAMMA: 1.2, CT.OP_SATURATION: 0.8, CT.OP_BRIGHTNESS: 1.1, CT.OP_CONTRAST: 0.9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_color.py measures the MI355X'
    dev = torch.device('cuda:0')
    L = N.lib()
    rows = []
    for B, S in ((18, 256), (22, 1024)):
        x = torch.rand(B, 3, S, S, device=dev) * 2 - 1
        y = torch.empty_like(x)
        for name, ops in CASES:
            ps = [torch.full((B,), VALUE[o], device=dev) + 0.001 * torch.arange(B, device=dev) for o in ops]
            chain, keep = CT.native_chain(ops, ps, B, dev)       # the launch alone: no host work timed
            nws = L.p2l_color_adjust_ws_bytes(ct.byref(chain), B)
            ws = torch.empty(max(nws // 8, 1), dtype=torch.int64, device=dev)
            fn = lambda: N.check(L.p2l_color_adjust(ct.byref(chain), N.ptr(x), N.ptr(y), B, 3, S, S,  # noqa: E731
                                                    ct.c_void_p(ws.data_ptr()), ct.c_size_t(nws), N.stream()))
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 20
            passes = 2 + ops.count(CT.OP_CONTRAST)                  # read + write, + one read per contrast op
            nbytes = 4.0 * x.numel() * passes
            rows.append({'case': name, 'B': B, 'size': S, 'ms': ms, 'GBps': nbytes / ms / 1e6})
            print('%-10s B %2d  %4d^2 : %7.3f ms per launch %6.0f GB/s' % (name, B, S, ms, nbytes / ms / 1e6))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()

"""Writes tests/golden/loss_layout.json: workspace sizes, cache offsets and test-hook lookups of the three
projection-loss plans (vgg, alex, squeeze) as the library built from the checked-out tree lays them out.
Host calls only.  Run it on the commit whose layout is to be pinned, BEFORE changing the plans
(tests/test_loss_layout.py compares later builds against the file)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pix2latent_amd import _native as N  # noqa: E402

SHAPES = [(1, 64, 64), (3, 64, 64), (5, 256, 256), (2, 128, 256), (3, 32, 32), (2, 100, 100), (2, 34, 34)]
# net -> (ws_bytes, cache_floats, taps, ws_lookup, number of lookup indices)
NETS = {'vgg': ('p2l_projloss_ws_bytes', 'p2l_loss_cache_floats', 5, 'p2l_projloss_ws_lookup', 13),
        'alex': ('p2l_alexloss_ws_bytes', 'p2l_alex_cache_floats', 5, None, 0),
        'squeeze': ('p2l_sqzloss_ws_bytes', 'p2l_sqz_cache_floats', 7, 'p2l_sqzloss_ws_lookup', 17)}


def record(lib, net, B, H, W):
    ws, cache, taps, lookup, n_idx = NETS[net]
    nft, wt, wsum = (C.c_size_t * taps)(), (C.c_size_t * taps)(), C.c_size_t(0)
    out = {'ws_bytes': getattr(lib, ws)(B, H, W),
           'cache_floats': getattr(lib, cache)(B, H, W, nft, wt, C.byref(wsum)),
           'nft_off': list(nft), 'wt_off': list(wt), 'wsum_off': wsum.value, 'lookup': []}
    for idx in range(n_idx):
        off, shape = C.c_size_t(0), (C.c_int32 * 4)()
        rc = getattr(lib, lookup)(B, H, W, idx, C.byref(off), shape)
        out['lookup'].append([rc, off.value, list(shape)])
    return out


if __name__ == '__main__':
    lib = N.lib()
    gold = {net: {'%dx%dx%d' % s: record(lib, net, *s) for s in SHAPES} for net in NETS}
    with open(os.path.join(ROOT, 'tests', 'golden', 'loss_layout.json'), 'w') as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write('\n')

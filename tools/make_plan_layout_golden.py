"""Writes tests/golden/plan_layout.json: workspace sizes and test-hook lookups of the BigGAN and StyleGAN2
plans as the library built from the checked-out tree lays them out, per batch size and weight format.
Host calls only: the descriptors carry extents and `wfmt`, every pointer is null (the layouts read nothing
else).  Run it on the commit whose layout is to be pinned, BEFORE changing the plans
(tests/test_plan_layout.py compares later builds against the file, in this order and in the reverse one)."""
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pix2latent_amd import _native as N  # noqa: E402
from pix2latent_amd.utils import synthetic as S  # noqa: E402

BG_BATCH = (1, 3, 18)
# plain formats, then flag sets a model can carry: PW | THIN | NO_AMAX on the Winograd format, ATTN_GEMM on it
BG_WFMT = (0x0, 0x1, 0x2, 0x12, 0x32, 0x92, 0x42)
SG_BATCH = (1, 3)
SG_WFMT = (0, 1, 2)
# name -> (size, width table override): the real width tables, and the `narrow` toy of tests/test_stylegan2_gpu.py
SG_NETS = {'64': (64, None), '512': (512, None), '1024': (1024, None),
           '64-narrow': (64, {4: 128, 8: 128, 16: 64, 32: 32, 64: 32})}


def biggan_desc(wfmt):
    """extents of biggan-deep-256 as model/biggan.py fills them (utils/synthetic.LAYERS, ch 128)"""
    d = N.P2LBigGAN()
    blocks = [s for s in S.layer_table() if s[0] == 'block']
    d.n_blocks, d.attn_before, d.ch, d.z_dim, d.c_dim = len(blocks), S.ATTN_POS, S.CH, S.Z_DIM, S.Z_DIM
    off = 0
    for bi, (_, up, cin, cout) in enumerate(blocks):
        g = d.blocks[bi]
        g.cin, g.cout, g.up = cin, cout, int(up)
        for k, ch in enumerate((cin, cin // 4, cin // 4, cin // 4)):
            g.cbn_off[k] = off
            off += ch
    d.cbn_total = off
    d.attn_ch = [s for s in S.layer_table() if s[0] == 'attn'][0][1]
    d.wfmt = wfmt
    return d


def sg2_desc(net, wfmt):
    """extents of the rosinality generator as model/stylegan2.py fills them"""
    size, widths = SG_NETS[net]
    ch = dict(S.sg2_channels(2))
    ch.update(widths or {})
    d = N.P2LStyleGAN2()
    log_size = int(math.log2(size))
    d.size, d.style_dim, d.n_latent = size, 512, 2 * log_size - 2
    d.n_conv, d.n_rgb = 2 * (log_size - 2) + 1, log_size - 1
    noise_off = 0
    for l in range(d.n_conv):
        c = d.conv[l]
        c.res = 4 if l == 0 else 2 ** ((l + 1) // 2 + 2)
        c.up = int(l % 2 == 1)
        c.cin = ch[c.res // 2] if c.up else ch[c.res]
        c.cout = ch[c.res]
        c.latent_idx, c.noise_off = l, noise_off
        noise_off += c.res * c.res
    d.noise_total = noise_off
    for j in range(d.n_rgb):
        r = d.rgb[j]
        r.res = 4 * 2 ** j
        r.cin, r.after_conv, r.latent_idx = ch[r.res], 2 * j, 2 * j + 1
    d.wfmt = wfmt
    return d


def _lookup(fn, *args):
    off, shape = C.c_size_t(0), (C.c_int32 * 4)()
    rc = fn(*args, C.byref(off), shape)
    return [rc, off.value, list(shape)]


def queries():
    """[(case, field, call)]: call(lib) makes ONE library call and returns what the file records for it"""
    out = []
    for B in BG_BATCH:
        for wfmt in BG_WFMT:
            case, d = 'biggan B=%d wfmt=0x%x' % (B, wfmt), biggan_desc(wfmt)
            out.append((case, 'ws_bytes', lambda lib, d=d, B=B: lib.p2l_biggan_ws_bytes(C.byref(d), B)))
            for what in range(13):                    # (12: no such item)
                # ModuleList indices (what 0) and bn inputs (what 7), each with the indices next to the valid range
                idx = range(-1, d.n_blocks + 2) if what == 0 else range(-1, 3 * d.n_blocks + 1) if what == 7 else (0,)
                for i in idx:
                    out.append((case, '%d:%d' % (what, i), lambda lib, d=d, B=B, what=what, i=i: _lookup(
                        lib.p2l_biggan_ws_lookup, C.byref(d), B, what, i)))
    for net in SG_NETS:
        for B in SG_BATCH:
            for wfmt in SG_WFMT:
                case, d = 'sg2 %s B=%d wfmt=%d' % (net, B, wfmt), sg2_desc(net, wfmt)
                out.append((case, 'ws_bytes', lambda lib, d=d, B=B: lib.p2l_sg2_ws_bytes(C.byref(d), B)))
                for l in range(-1, d.n_conv + 1):
                    out.append((case, str(l), lambda lib, d=d, B=B, l=l: _lookup(
                        lib.p2l_sg2_ws_lookup, C.byref(d), B, l)))
    return out


def record(lib, qs):
    gold = {}
    for case, field, call in qs:
        gold.setdefault(case, {})[field] = call(lib)
    return gold


if __name__ == '__main__':
    gold = record(N.lib(), queries())
    with open(os.path.join(ROOT, 'tests', 'golden', 'plan_layout.json'), 'w') as f:
        f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(gold[k], sort_keys=True,
                                                                        separators=(',', ':')))
                                    for k in sorted(gold)) + '\n}\n')

"""Host-side comparison of two builds of libp2l_hip.so over the conv launcher's ROUTING decisions
(csrc/p2l_conv.hip): for a refactor of the launcher or of its size queries every answer must stay what it was.

    python tools/route_sweep.py --lib A/libp2l_hip.so --lib B/libp2l_hip.so [--out FILE] [--stride N]

enumerates descriptors and asks each library, in ONE fresh child process per library, every NON-LAUNCHING entry
point about them: p2l_conv_suggest_splitk, _amax_slots, _workspace_bytes, _arb_fusable, _arb_nblk,
_arb_split_fusable, _arb_nblk_ws, p2l_conv_epilogue_class (the launcher's whole decision path, nothing launched),
p2l_packed_weight_floats and p2l_packed_subpix_weight_floats.  Nothing else is called -- no p2l_conv_fwd*, no
dgrad -- so the tool runs anywhere, with or without a GPU.  Exit status 1 on any difference.  Not a test and no
golden: a change of a routing rule moves both columns.

Descriptors.  SHAPES = the full product of taps {1, 9} x (ups, ext) {0 .. 3} x {0, 1} x H x W (each of 4 6 8 12 16
32 64 128 256) x Cin x Cout (each of 16 32 48 64 96 128 256 512 1024) x every weight format (the formats a tap
count does not take, and taps = 1 with an upsample, are refused by the launcher: those shapes get the base
descriptor only).  Around the BASE descriptor of a shape (B = 3, form 0, the suggested slice count, no pooling, no
activation, pitches = channel counts) ONE field moves at a time: splitk {0, 1, 2, 4, 8, 64}; B {1, 9, 18}; every
P2L_FORM_* bit alone and the pairs the tests use; pool {max, sum}; act {relu, tanh, leaky}; y_ld, res_ld, n_store no
multiple of four.  The epilogue class is asked with a workspace of p2l_conv_workspace_bytes and with none, for one
recipe per class of tests/_epilogue_cases.py (bias / residual / mask / pooling / fused activation backward with
and without shortcut, maxima handed over or not) plus the StyleGAN2 terms on the base descriptor, for three of them
on the others.

So that "0 differ" cannot be vacuous the child also counts, from the answers alone: shapes with more than one K
slice under each of the three slicing rules (sub-pixel gradient: ups = 3; Winograd: its slices always meet in the
16-byte finish kernel, so a y_ld that is no multiple of four leaves the maxima slots alone; direct / pointwise: the
rest), descriptors with maxima slots per family, and epilogue classes seen.
--stride N takes every N-th shape (a quick look while working; the committed summary is a full run)."""
import argparse
import ctypes as C
import hashlib
import itertools
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4, 6, 8, 12, 16, 32, 64, 128, 256)
CHANNELS = (16, 32, 48, 64, 96, 128, 256, 512, 1024)
WFMT = {'f32': 0, 'bf16x3': 1, 'bf16x3w': 2, 'pw': 3, 'bf16x3t': 4}
FORM_BITS = [1 << i for i in range(14)]
FORM_PAIRS = [2 | 4, 2 | 64, 2 | 128, 2 | 8192, 2 | 32, 1 | 256]      # WINO_ANY with ..., NO_WINO | NO_H2R
SPLITK = (0, 1, 2, 4, 8, 64)
FAKE = 0x10000
# tests/_epilogue_cases.py _FWD: what a launch of each class carries
RECIPES = {'plain': {}, 'bias_ps': dict(pro=1, bias=1, nxt=1, handed=1),
           'bias_res_ps': dict(pro=1, bias=1, nxt=1, handed=1, res=1),
           'bias_resup_ps': dict(pro=1, bias=1, nxt=1, handed=1, res=2), 'bias_relu': dict(bias=1, act=1),
           'bias_relu_pool': dict(bias=1, act=1, pool=1), 'mask': dict(mask=1), 'arb': dict(arb=1),
           'arb_skip': dict(arb=1, skip=1, handed=1), 'arb_skip_up': dict(arb=1, skip=2, handed=1), 'arb_handed': dict(arb=1, handed=1),
           'oscale': dict(bias=1, oscale=1, handed=1), 'noise': dict(bias=1, noise=1), 'no_amax': dict(bias=1, noamax=1)}
LITE = ('bias_ps', 'arb', 'bias_relu')


def sweep_group(job):
    """one (taps, ups, ext, format) group of shapes: its BLOCK / LINE lines and its coverage counts"""
    (taps, ups, ext), fmt, first_index, stride, dump = job
    from pix2latent_amd import _native as N          # (the structs of include/p2l.h; P2L_LIB_PATH names the library)
    lib = N.lib()
    lib.p2l_packed_weight_floats.argtypes = [C.c_int] * 4
    lib.p2l_packed_subpix_weight_floats.argtypes = [C.c_int] * 3
    q_int = [getattr(lib, 'p2l_conv_' + n) for n in ('suggest_splitk', 'amax_slots', 'arb_fusable', 'arb_nblk',
                                                      'arb_split_fusable', 'arb_nblk_ws')]
    for f in q_int + [lib.p2l_conv_workspace_bytes]:
        f.argtypes = [C.c_void_p]
    epi = lib.p2l_conv_epilogue_class
    d, ex, arb = N.P2LConv(), N.P2LConvExtra(), N.P2LArb()
    pd, pex, parb = C.addressof(d), C.addressof(ex), C.addressof(arb)

    def classes(recipes, both):
        """p2l_conv_epilogue_class of d under each recipe; made-up addresses: only NULL or not matters"""
        out = []
        act0, pool0, pro0, pb0 = d.act, d.pool, d.pro, d.pro_bstride
        for name in recipes:
            r = RECIPES[name]
            d.act, d.pool = r.get('act', act0), r.get('pool', pool0)
            d.pro = r.get('pro', pro0)
            d.pro_bstride = d.Cin if d.pro else 0
            d.res_ups = 1 if r.get('res') == 2 else 0
            am = N.P2LAmax()
            if not r.get('noamax'):
                am.out = FAKE
                if d.pool:
                    am.outp = FAKE
            if r.get('handed'):
                am.in_, am.in_n = FAKE, 1
            if r.get('nxt'):
                am.next_s, am.next_t, am.next_bstride = FAKE, FAKE, d.Cout
            if r.get('arb'):
                C.memset(parb, 0, C.sizeof(arb))
                arb.x, arb.x_ld, arb.s, arb.t, arb.st_bstride = FAKE, d.Cout, FAKE, FAKE, d.Cout
                arb.partial = arb.ds = arb.dt = FAKE
                arb.dsdt_bstride = d.Cout
                if r.get('skip'):
                    arb.skip, arb.skip_ld, arb.skip_C, arb.skip_ups = FAKE, d.Cout, d.Cout // 2, r['skip'] - 1
                arb.amax = am
                a, e = parb, None
            else:
                C.memset(pex, 0, C.sizeof(ex))
                if r.get('oscale'):
                    ex.oscale, ex.oscale_bstride = FAKE, d.Cout
                if r.get('noise'):
                    ex.noise, ex.noise_w = FAKE, 0.5
                ex.amax = am
                a, e = None, pex
            ws = lib.p2l_conv_workspace_bytes(pd)
            for with_ws in ((1, 0) if both else (1,)):
                use = ws if with_ws else 0
                out.append(epi(pd, e, a, FAKE if r.get('bias') else None, FAKE if r.get('res') else None,
                               FAKE if r.get('mask') else None, FAKE, FAKE if d.pool else None,
                               FAKE if use else None, use))
        d.act, d.pool, d.pro, d.pro_bstride, d.res_ups = act0, pool0, pro0, pb0, 0
        return out

    def record(recipes, both):
        return [f(pd) for f in q_int] + [lib.p2l_conv_workspace_bytes(pd)] + classes(recipes, both)

    cover = {'descriptors': 0, 'shapes': 0}

    def bump(key, n=1):
        cover[key] = cover.get(key, 0) + n

    def family(fmt):
        if d.ups >= 2:
            return 'sub-pixel forward' if d.ups == 2 else 'sub-pixel gradient'
        if d.taps == 1:
            return '1x1 ' + fmt
        if fmt == 'bf16x3w':
            return '3x3 bf16x3w' + (' NO_WINO' if d.form & 1 else ' WINO_ANY' if d.form & 2 else '')
        return '3x3 ' + fmt

    def note(rec, fmt):
        cover['descriptors'] += 1
        if rec[1] > 0:
            bump('maxima slots > 0: ' + family(fmt))
        for ec in rec[7:]:
            if ec:
                bump('epilogue class %d' % ec)

    out = []
    index = first_index
    if True:
        valid = (taps == 9 and fmt != 'pw') or (taps == 1 and ups == 0 and fmt in ('f32', 'pw'))
        for H, W in itertools.product(SIZES, SIZES):
            key = 'taps%d ups%d ext%d %s %dx%d' % (taps, ups, ext, fmt, H, W)
            h = hashlib.sha256()
            lines = []
            for Cin, Cout in itertools.product(CHANNELS, CHANNELS):
                index += 1
                if index % stride:
                    continue
                cover['shapes'] += 1
                C.memset(pd, 0, C.sizeof(d))
                d.B, d.H, d.W, d.Cin, d.Cout, d.taps, d.ups, d.ext = 3, H, W, Cin, Cout, taps, ups, ext
                d.x_ld, d.alpha, d.wfmt = Cin, 1.0, WFMT[fmt]
                d.y_ld = d.yp_ld = d.n_store = d.res_ld = d.mask_ld = Cout
                d.splitk = 1
                sug = lib.p2l_conv_suggest_splitk(pd)
                d.splitk = sug
                rows = [('base', [lib.p2l_packed_weight_floats(taps, Cout, Cin, WFMT[fmt]),
                                  lib.p2l_packed_subpix_weight_floats(Cout, Cin, WFMT[fmt])] + record(RECIPES, True))]
                note(rows[0][1][2:], fmt)
                if valid:
                    sliced = {}
                    for s in SPLITK:
                        d.splitk = s
                        rows.append(('splitk=%d' % s, record(LITE, False)))
                        sliced[s] = rows[-1][1][4] or rows[-1][1][5] != rows[-1][1][3]
                    d.splitk = sug
                    at_sug = rows[0][1][6] or rows[0][1][7] != rows[0][1][5]
                    for B in (1, 9, 18):
                        d.B = B
                        rows.append(('B=%d' % B, record(LITE, False)))
                    d.B = 3
                    for form in FORM_BITS + FORM_PAIRS:
                        d.form = form
                        d.splitk = 1
                        d.splitk = lib.p2l_conv_suggest_splitk(pd)      # (the Winograd rule follows the form)
                        rows.append(('form=%d' % form, record(LITE, True)))
                    d.form, d.splitk = 0, sug
                    for pool in (1, 2):
                        d.pool = pool
                        rows.append(('pool=%d' % pool, record(LITE, False)))
                    d.pool = 0
                    for act in (1, 2, 3):
                        d.act = act
                        rows.append(('act=%d' % act, record(('plain', 'oscale', 'arb'), False)))
                    d.act = 0
                    for field in ('y_ld', 'res_ld', 'n_store'):
                        setattr(d, field, Cout + 2 if field != 'n_store' else Cout - 2)
                        rows.append((field, record(LITE, False)))
                        setattr(d, field, Cout)
                    if at_sug and sug > 1:
                        # (a pitch that is no multiple of four sends the direct kernels' slices to the scalar finish
                        #  kernel, four times the maxima slots; the Winograd slices always end in the 16-byte one)
                        y_ld_slots = dict(rows)['y_ld'][1]
                        rule = 'sub-pixel gradient' if ups == 3 else \
                            'Winograd' if y_ld_slots == rows[0][1][3] > 0 else 'direct / pointwise'
                        bump('K slices > 1: %s rule' % rule)
                    for name, rec in rows[1:]:
                        d.form = int(name[5:]) if name.startswith('form=') else 0
                        note(rec, fmt)
                    d.form = 0
                for name, rec in rows:
                    text = '%d->%d %s %s' % (Cin, Cout, name, ' '.join(map(str, rec)))
                    h.update(text.encode())
                    if dump == key:
                        lines.append(text)
            if h.digest() != hashlib.sha256().digest():
                out.append('BLOCK %s|%s' % (key, h.hexdigest()[:24]))
            out += ['LINE ' + text for text in lines]
    return out, cover


def child(stride, dump):
    import multiprocessing
    combos = [(t, u, e) for t in (1, 9) for u in range(4) for e in (0, 1)]
    per_group = len(SIZES) ** 2 * len(CHANNELS) ** 2
    jobs = [(c, fmt, i * per_group, stride, dump) for i, (c, fmt) in enumerate(itertools.product(combos, WFMT))]
    cover = {}
    # (the library is loaded in the workers: this process stays the one child of its library and only adds up)
    with multiprocessing.Pool(min(4, os.cpu_count() or 1)) as pool:
        for lines, cov in pool.imap(sweep_group, jobs):
            print('\n'.join(lines), flush=True)
            for k, v in cov.items():
                cover[k] = cover.get(k, 0) + v
    for k in sorted(cover):
        print('COVER %s|%d' % (k, cover[k]))
    print('SWEEP-DONE', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', action='append', default=[], help='a libp2l_hip.so; give it twice or more')
    ap.add_argument('--out', help='also write the summary to this file')
    ap.add_argument('--stride', type=int, default=1, help='take every N-th shape only')
    ap.add_argument('--dump', default='', help='print every answer of one block, e.g. "taps9 ups0 ext0 bf16x3w 16x16"')
    ap.add_argument('--child', action='store_true')
    args = ap.parse_args()
    if args.child:
        return child(args.stride, args.dump)
    procs = []
    for lib in args.lib:                 # (host code only: the libraries may run side by side)
        env = dict(os.environ, P2L_LIB_PATH=os.path.abspath(lib))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), '--child', '--stride',
                                       str(args.stride), '--dump', args.dump], env=env, cwd=ROOT,
                                      stdout=subprocess.PIPE, universal_newlines=True))
    cols, covers = [], []
    for lib, p in zip(args.lib, procs):
        lines = p.communicate()[0].splitlines()
        if p.returncode != 0 or not any(l.startswith('SWEEP-DONE') for l in lines):
            sys.exit('route_sweep: the run with %s ended with status %d\n%s' % (lib, p.returncode, '\n'.join(lines[-20:])))
        cols.append(dict(l[6:].split('|') for l in lines if l.startswith('BLOCK ')))
        covers.append(dict(l[6:].split('|') for l in lines if l.startswith('COVER ')))
        if args.dump:
            with open('route_sweep_dump_%d.txt' % len(cols), 'w') as f:
                f.write('\n'.join(l[5:] for l in lines if l.startswith('LINE ')) + '\n')
    bad = sorted(set(k for c in cols for k in c if any(o.get(k) != c[k] for o in cols)))
    empty = [k for k, v in covers[0].items() if int(v) == 0]
    want = ['K slices > 1: %s rule' % r for r in ('direct / pointwise', 'Winograd', 'sub-pixel gradient')] + \
           ['epilogue class %d' % i for i in range(1, 10)]
    empty += [k for k in want if k not in covers[0]]
    text = ['# tools/route_sweep.py%s: every host query of the conv launcher; libraries: %s'
            % (' --stride %d' % args.stride if args.stride > 1 else '', ' | '.join(args.lib))]
    text += ['%-48s %s' % (k, '  '.join(c.get(k, '0') for c in covers)) for k in sorted(covers[0])]
    text += ['DIFFERS  ' + k for k in bad[:40]]
    text += ['NOT COVERED  ' + k for k in empty]
    text.append('# %s descriptors in %d blocks, %d blocks differ' % (covers[0]['descriptors'], len(cols[0]), len(bad)))
    print('\n'.join(text))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(text) + '\n')
    sys.exit(1 if bad or empty or len(cols) < 2 else 0)


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    main()

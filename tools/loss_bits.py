"""Bit-for-bit comparison of two trees through the native image losses (pix2latent_amd/loss_functions.py): for a
host-side refactor of the autograd Functions every output must keep its bits -- a factor applied on the other side
of a rounding, another beta, another buffer shows in the last ones.  GPU only.

    python tools/loss_bits.py --tree A --tree B [--label a --label b] [--out FILE]

runs the cases of tools/loss_trace.py (every form of the three loss classes; B = 3 at 64^2, at 128^2 with
lpips_size = 64) on seeded synthetic LPIPS weights, each tree in ONE fresh child process, one after the other, and
takes one sha256 per tensor -- the loss, `last_l1`, `last_lpips` of its engine, d output -- and prints per case one
digest over those four for every tree side by side, and every tensor that differs on a line of its own.  Each case runs eager on one lane; the first case of each form also on lane 1, on a side stream.  A tree is a
directory that holds a `pix2latent_amd` package; one without a built library runs on this checkout's.  Exit status
1 when a digest differs.  Not a test and no golden: the next kernel change moves the digests of both columns."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    import warnings
    warnings.simplefilter('ignore')
    import torch
    from loss_trace import B, cases
    from pix2latent_amd import lanes
    from pix2latent_amd.utils import synthetic as S
    import pix2latent_amd.loss_functions as LF
    dev = torch.device('cuda:0')
    weights = {'vgg': S.lpips_vgg_weights(1), 'alex': S.lpips_alex_weights(2), 'squeeze': S.lpips_squeeze_weights(3)}
    probe = torch.tensor([1.0, 0.5, 2.0], device=dev)
    side = lanes.side_streams(dev, 1)[0]

    def sha(t):
        if t is None:
            return '-' * 24
        torch.cuda.synchronize()
        return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:24]

    def run(case, fn, t, lane):
        out = t['output']
        out.grad = None
        if lane:
            side.wait_stream(torch.cuda.current_stream())
            with lanes.use(lane), torch.cuda.stream(side):
                loss = fn(out, t['target'], t['weight'], t['loss_mask'])
                (loss * probe).sum().backward()
            torch.cuda.current_stream().wait_stream(side)
        else:
            loss = fn(out, t['target'], t['weight'], t['loss_mask'])
            (loss * probe).sum().backward()
        eng = fn._engine
        for name, x in (('loss', loss), ('last_l1', getattr(eng, 'last_l1', None)),
                        ('last_lpips', getattr(eng, 'last_lpips', None)), ('d output', out.grad)):
            print('BITS %s|%s|%s' % (case + (' lane %d' % lane if lane else ''), name, sha(x)), flush=True)

    for cls, kw, div, mask, wk, first in cases():
        size = 128 if div else 64
        kw = dict(kw)
        net = kw.get('lpips_net', kw.get('net'))
        if net:
            kw['weights'] = weights[net]
        if div:
            kw['lpips_size'] = size // div
        case = '%s(%s) %dx%d mask=%s %s' % (cls, ', '.join('%s=%r' % i for i in sorted(kw.items()) if i[0] != 'weights'),
                                            size, size, 'yes' if mask else 'no', wk)
        g = torch.Generator().manual_seed(size + 7)
        r = lambda c: torch.rand(B, c, size, size, generator=g)
        t = dict(output=(r(3) * 2 - 1).to(dev).requires_grad_(True), target=(r(3) * 2 - 1).to(dev),
                 weight={'w3': r(3) + 0.5, 'w1': r(1) + 0.5, 'none': None}[wk],
                 loss_mask=(r(1) > 0.3).float().to(dev) if mask else None)
        if t['weight'] is not None:
            t['weight'] = t['weight'].to(dev)
        fn = getattr(LF, cls)(device=dev, **kw) if net else getattr(LF, cls)(**kw)
        run(case, fn, t, 0)
        if first:
            run(case, fn, t, 1)
    print('BITS-DONE', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', action='append', default=[], help='a checkout (holds pix2latent_amd/); give it twice')
    ap.add_argument('--label', action='append', default=[], help='what the header calls a tree, e.g. its commit')
    ap.add_argument('--out', help='also write the table to this file')
    ap.add_argument('--child', action='store_true')
    args = ap.parse_args()
    if args.child:
        return child()
    labels = (args.label + args.tree[len(args.label):])[:len(args.tree)]
    cols = []
    for tree in args.tree:
        tree = os.path.abspath(tree)
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([tree, os.path.join(ROOT, 'tools')]))
        if not os.path.exists(os.path.join(tree, 'pix2latent_amd', 'libp2l_hip.so')):
            env.setdefault('P2L_LIB_PATH', os.path.join(ROOT, 'pix2latent_amd', 'libp2l_hip.so'))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, cwd=tree,
                           stdout=subprocess.PIPE, universal_newlines=True)
        lines = p.stdout.splitlines()
        if p.returncode != 0 or 'BITS-DONE' not in lines:
            # (a tree that faulted is not started again, nor is the next one started behind it)
            sys.exit('loss_bits: the run of %s ended with status %d\n%s' % (tree, p.returncode, p.stdout[-2000:]))
        cols.append({l[5:-25]: l[-24:] for l in lines if l.startswith('BITS ')})
    keys = list(cols[0])
    bad = [k for k in keys if any(c.get(k) != cols[0][k] for c in cols)] + \
          [k for c in cols[1:] for k in c if k not in cols[0]]
    # one line per case: the sha256 (16 hex digits) over the digests of its four tensors, per tree; a tensor that
    # differs gets a line of its own
    text = ['# tools/loss_bits.py: per case one sha256 over the digests of loss, last_l1, last_lpips, d output; '
            'columns: ' + ' | '.join(labels)]
    for case in dict.fromkeys(k.split('|')[0] for k in keys):
        mine = [k for k in keys if k.split('|')[0] == case]
        text.append('%-100s %s' % (case, '  '.join(
            hashlib.sha256(''.join(c.get(k, '-') for k in mine).encode()).hexdigest()[:16] for c in cols)))
    text += ['DIFFERS %-104s %s' % (k, '  '.join(c.get(k, '-') for c in cols)) for k in bad]
    text.append('# %d tensors in %d cases, %d differ' % (len(keys), len(text) - 1 - len(bad), len(bad)))
    print('\n'.join(text[-40:] if len(text) > 40 else text))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(text) + '\n')
    sys.exit(1 if bad or len(cols) < 2 else 0)


if __name__ == '__main__':
    main()

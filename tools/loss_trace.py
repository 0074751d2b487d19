"""Host-side comparison of two trees over the LIBRARY CALLS the native image losses make
(pix2latent_amd/loss_functions.py): for a refactor of the autograd Functions, of `_apply` or of the engine every
form must go on making the same calls with the same scalars on the same buffers.

    python tools/loss_trace.py --tree A --tree B [--label a --label b] [--out FILE] [--dump FILE]

drives every form through the recording stand-in of tests/_loss_recorder.py (this checkout's, for every tree), in
ONE fresh child process per tree, and makes one line per library call: scalars as they are, pointers as the role
of the buffer (see the recorder).  The trees are compared line by line; every line that differs is printed for each
tree.  --out gets one line per case (its calls and the sha256 of its trace, per tree), --dump the whole trace of the
first tree.  A tree is a directory that holds a `pix2latent_amd` package; one without a
built library borrows this checkout's for the pure size queries, the only calls that reach it.  Nothing is
launched, no GPU is needed.  Exit status 1 on any difference.  Not a test and no golden: a change of what a form
launches moves both columns; tests/test_loss_forms.py holds the call-name sequences.

Cases.  ProjectionLoss: pixel_loss {l1, l2} x pixel_weight {1, 0, 0.37} x lpips_size {None, H/2} x loss_mask
{no, yes} x weight {three-channel, one-channel, None} on the VGG plan, and the twelve (pixel_loss, pixel_weight,
lpips_size) forms on the Alex and Squeeze plans.  PerceptualLoss: lpips_size x loss_mask x weight on VGG, lpips_size
on the other two.  ReconstructionLoss: {l1, l2} x loss_mask x weight {three-channel, one-channel}.  B = 3 at 64^2,
at 128^2 with lpips_size = 64.  Every case: a first call (forward + backward) and a second on the same tensors.
The first case of each form also: the same call under lanes.use(1); B = 3, 2, 3 on a fresh loss object (no
re-allocation on the way back up); a backward behind a later forward on its lane (the error, no call recorded).
Behind every step: `Scratch.generation`, the number of cache slots, what each lane holds, and which buffers
`last_l1` / `last_lpips` are."""
import argparse
import hashlib
import itertools
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 3


def cases():
    """(class, constructor arguments, lpips_size as a divisor of H or None, loss_mask?, weight kind, first of form?)"""
    for net in ('vgg', 'alex', 'squeeze'):
        full = net == 'vgg'
        for pl, pw, div in itertools.product(('l1', 'l2'), (1.0, 0.0, 0.37), (None, 2)):
            for k, (mask, wk) in enumerate(itertools.product((False, True), ('w3', 'w1', 'none')) if full
                                           else [(False, 'w3')]):
                yield 'ProjectionLoss', dict(lpips_net=net, pixel_loss=pl, pixel_weight=pw), div, mask, wk, k == 0
        for div in (None, 2):
            for k, (mask, wk) in enumerate(itertools.product((False, True), ('w3', 'w1', 'none')) if full
                                           else [(False, 'w3')]):
                yield 'PerceptualLoss', dict(net=net), div, mask, wk, k == 0
    for lt in ('l1', 'l2'):
        for k, (mask, wk) in enumerate(itertools.product((False, True), ('w3', 'w1'))):
            yield 'ReconstructionLoss', dict(loss_type=lt), None, mask, wk, k == 0


def child():
    import warnings
    warnings.simplefilter('ignore')
    import torch
    import _loss_recorder as R
    import pix2latent_amd.loss_functions as LF
    from pix2latent_amd import _native as N, lanes

    def say(s):
        print('TRACE ' + s, flush=True)

    def make(cls, kw, div, size):
        kw = dict(kw)
        if div:
            kw['lpips_size'] = size // div
        fn = getattr(LF, cls)(**kw)
        if fn._engine is None:                 # (ReconstructionLoss makes its engine at the first native call)
            fn._engine = LF._LossEngine(None)
        return fn

    def tensors(size, mask, wk):
        g = torch.Generator().manual_seed(size + 7)
        r = lambda c: torch.rand(B, c, size, size, generator=g)
        return dict(output=(r(3) * 2 - 1).requires_grad_(True), target=r(3) * 2 - 1,
                    weight={'w3': r(3) + 0.5, 'w1': r(1) + 0.5, 'none': None}[wk],
                    loss_mask=(r(1) > 0.3).float() if mask else None)

    def forward(fn, t, n, lane=0):
        with lanes.use(lane):
            return fn(*(None if v is None else v[:n] for v in (t['output'], t['target'], t['weight'], t['loss_mask'])))

    def state(rec, eng):
        held = ' '.join('lane%d[%s]' % (k, ' '.join(f for f in ('ws', 'full16', 'dfull16', 'pix_part')
                                                    if getattr(s, f, None) is not None))
                        for k, s in sorted(eng._scratch.lanes.items()))
        role = lambda t: '-' if t is None else rec.role(t.data_ptr())
        say('  state: generation=%d slots=%d %s last_l1=%s last_lpips=%s'
            % (eng._scratch.generation, len(set(map(id, eng.slots.values()))), held,
               role(getattr(eng, 'last_l1', None)), role(getattr(eng, 'last_lpips', None))))

    def step(rec, fn, t, what, n=B, lane=0):
        mark = len(rec.calls)
        say(' ' + what)
        t['output'].grad = None
        forward(fn, t, n, lane).sum().backward()
        for c in rec.calls[mark:]:
            say('  ' + c.text)
        state(rec, fn._engine)
        rec.step_end()

    with R.recording() as rec:
        for cls, kw, div, mask, wk, first in cases():
            size = 128 if div else 64
            say('CASE %s(%s) %s %dx%d loss_mask=%s weight=%s'
                % (cls, ', '.join('%s=%r' % i for i in sorted(kw.items())),
                   'lpips_size=%s' % (size // div if div else None), size, size, 'yes' if mask else 'no', wk))
            t = tensors(size, mask, wk)
            rec.reset()
            fn = make(cls, kw, div, size)
            rec.watch(fn._engine, **t)
            step(rec, fn, t, 'first call')
            step(rec, fn, t, 'second call, same tensors')
            if not first:
                continue
            step(rec, fn, t, 'under lanes.use(1)', lane=1)
            rec.reset()
            fn = make(cls, kw, div, size)
            rec.watch(fn._engine, **t)
            for n in (3, 2, 3):
                step(rec, fn, t, 'fresh object, B = %d' % n, n=n)
            say(' a backward behind a later forward on its lane')
            early = forward(fn, t, B)
            forward(fn, t, B)
            mark = len(rec.calls)
            try:
                early.sum().backward()
                say('  no error')
            except N.NativeError as e:
                say('  NativeError: %s; %d calls recorded' % (e, len(rec.calls) - mark))
            rec.step_end()
    print('TRACE-DONE', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', action='append', default=[], help='a checkout (holds pix2latent_amd/); give it twice')
    ap.add_argument('--label', action='append', default=[], help='what the header calls a tree, e.g. its commit')
    ap.add_argument('--out', help='also write the table (one line per case) and the verdict to this file')
    ap.add_argument('--dump', help='write the whole trace of the first tree, one line per call, to this file')
    ap.add_argument('--child', action='store_true')
    args = ap.parse_args()
    if args.child:
        return child()
    trees = args.tree or [ROOT]
    labels = (args.label + trees[len(args.label):])[:len(trees)]
    cols = []
    for tree in trees:
        tree = os.path.abspath(tree)
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([tree, os.path.join(ROOT, 'tests')]))
        if not os.path.exists(os.path.join(tree, 'pix2latent_amd', 'libp2l_hip.so')):
            env.setdefault('P2L_LIB_PATH', os.path.join(ROOT, 'pix2latent_amd', 'libp2l_hip.so'))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, cwd=tree,
                           stdout=subprocess.PIPE, universal_newlines=True)
        lines = p.stdout.splitlines()
        if p.returncode != 0 or 'TRACE-DONE' not in lines:
            sys.exit('loss_trace: the run of %s ended with status %d\n%s' % (tree, p.returncode, p.stdout[-2000:]))
        cols.append([l[6:] for l in lines if l.startswith('TRACE ')])
    bad = [i for i in range(max(map(len, cols))) if any(i >= len(c) or c[i] != cols[0][i] for c in cols)]

    def per_case(lines):
        """[(case line, its calls, sha256 of its lines)]"""
        out = []
        for l in lines:
            if l.startswith('CASE '):
                out.append([l[5:], 0, hashlib.sha256()])
            out[-1][1] += l.startswith(('  p2l_', '  slot.used'))
            out[-1][2].update((l + '\n').encode())
        return [(name, n, h.hexdigest()[:16]) for name, n, h in out]
    cases_of = [per_case(c) for c in cols]
    text = ['# tools/loss_trace.py: every library call of the native image losses; per case the recorded calls and the '
            'sha256 (16 hex digits) of its trace; trees: ' + ' | '.join(labels)]
    for k, (name, n, h) in enumerate(cases_of[0]):
        others = ['%d %s' % c[k][1:] if k < len(c) else '-' for c in cases_of[1:]]
        text.append('%-110s %d %s  %s' % (name, n, h, '  '.join(others)))
    for i in bad[:40]:
        text += ['DIFFERS line %d' % (i + 1)] + ['    %s: %s' % (lab, c[i] if i < len(c) else '(none)')
                                                 for lab, c in zip(labels, cols)]
    text.append('# %d cases, %d calls, %d lines, %d differ'
                % (len(cases_of[0]), sum(l.startswith('  p2l_') for l in cols[0]), len(cols[0]), len(bad)))
    print('\n'.join(text[-60:] if len(text) > 60 else text))
    for path, body in ((args.out, text), (args.dump, cols[0])):
        if path:
            with open(path, 'w') as f:
                f.write('\n'.join(body) + '\n')
    sys.exit(1 if bad or len(cols) < 2 else 0)


if __name__ == '__main__':
    main()

"""Bit-for-bit comparison of two builds of libp2l_hip.so through the plans (csrc/p2l_plan.hip, p2l_plan_sg2.hip):
for a host-side refactor of the plans every output must keep its bits -- a maxima hand-over taken or missed
differently, another split or another argument shows in the last ones.

    python tools/plan_bits.py --lib A/libp2l_hip.so --lib B/libp2l_hip.so [--out FILE]

runs the cases below once per library, each library in ONE fresh child process (pix2latent_amd/_native.py
loads the library P2L_LIB_PATH names), on seeded synthetic weights, and prints one sha256 per output tensor
for every library side by side.  Exit status 1 when a digest differs.  Not a test and no golden: the next
kernel change moves the digests of both columns.

Cases: the bench problem (generator + VGG loss at 256^2; image, loss, d image, dz, dc and the CBN gradients
ds / dt) at 18 and at 3 candidates (the small batch takes the split-K forms); 3 candidates again under every
switch that is read when a model is built; the VGG loss alone at 512^2 x 2, the smallest size at which a
producer leaves >= 4 096 partial maxima per image and the registry compacts them; the `wide` and `narrow`
StyleGAN2 toys of tests/test_stylegan2_gpu.py at 3 candidates, z and w+ with noise gradients, three formats."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = [{}, {'P2L_AMAX': '0'}, {'P2L_ATTN': '0'}, {'P2L_PW': '0'}, {'P2L_THIN': '0'},
            {'P2L_CONV_WFMT': 'f32'}, {'P2L_CONV_WFMT': 'bf16x3-direct'}]
SG_WIDTHS = {'wide': None, 'narrow': {4: 128, 8: 128, 16: 64, 32: 32, 64: 32}}
SG_FORMATS = ('bf16x3', 'bf16x3-direct', 'f32')


def sha(t):
    import torch
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:24]


def with_env(env):
    for k in ('P2L_AMAX', 'P2L_ATTN', 'P2L_PW', 'P2L_THIN', 'P2L_CONV_WFMT'):
        os.environ.pop(k, None)
    os.environ.update(env)
    import pix2latent_amd.loss_functions as LF
    LF._VGG_PARAMS.clear()         # (descriptors are built from the switches: none is carried over)
    return ','.join('%s=%s' % kv for kv in sorted(env.items())) or 'default'


def child():
    import warnings
    warnings.simplefilter('ignore')
    import torch
    from pix2latent_amd.utils import synthetic as S
    from pix2latent_amd.model.biggan import BigGAN
    from pix2latent_amd.model.stylegan2 import StyleGAN2
    import pix2latent_amd.loss_functions as LF
    dev = torch.device('cuda:0')
    W, Wv = S.biggan_weights(0), S.lpips_vgg_weights(1)

    def emit(case, name, t):
        print('BITS %s %s %s' % (case, name, sha(t)), flush=True)

    def bench_problem(case, n):
        model = BigGAN(weights=W, device=dev)
        loss_fn = LF.ProjectionLoss(lpips_net='vgg', weights=Wv, device=dev)
        g = torch.Generator().manual_seed(2)
        z = torch.fmod(torch.randn(n, 128, generator=g), 2.0).to(dev).requires_grad_(True)
        c = (0.05 * torch.randn(1, 128, generator=g)).repeat(n, 1).to(dev).requires_grad_(True)
        target = S.synthetic_target(256, 1).unsqueeze(0).repeat(n, 1, 1, 1).to(dev)
        weight = S.synthetic_weight_mask(256).unsqueeze(0).repeat(n, 1, 1, 1).to(dev)
        out = model(z=z, c=c)
        out.retain_grad()
        loss = loss_fn(out, target, weight)
        loss.mean().backward()
        for name, t in (('image', out), ('loss', loss), ('dimg', out.grad), ('dz', z.grad), ('dc', c.grad),
                        ('cbn_ds', model.saved_activation(4)), ('cbn_dt', model.saved_activation(5))):
            emit(case, name, t)

    for env in SWITCHES:
        tag = with_env(env)
        if not env:
            bench_problem('bench B=18 ' + tag, 18)
        bench_problem('bench B=3 ' + tag, 3)

    with_env({})
    loss_fn = LF.ProjectionLoss(lpips_net='vgg', weights=Wv, device=dev)
    g = torch.Generator().manual_seed(5)
    img = (torch.rand(2, 3, 512, 512, generator=g) * 2 - 1).to(dev).requires_grad_(True)
    target = (torch.rand(2, 3, 512, 512, generator=g) * 2 - 1).to(dev)
    loss = loss_fn(img, target, torch.ones(2, 3, 512, 512, device=dev))
    loss.mean().backward()
    emit('vgg 512^2 B=2', 'loss', loss)
    emit('vgg 512^2 B=2', 'dimg', img.grad)

    from oracle import stylegan2_ref as R
    B, SIZE = 3, 64
    for fmt in SG_FORMATS:
        with_env({'P2L_CONV_WFMT': fmt})
        for widths in SG_WIDTHS:
            case = 'sg2 %s %s' % (widths, fmt)
            Ws = S.stylegan2_weights(SIZE, 0, channels=SG_WIDTHS[widths])
            g = torch.Generator().manual_seed(3)
            z = torch.randn(B, 512, generator=g).to(dev).requires_grad_(True)
            noises = [torch.randn(B, 1, s[2], s[3], generator=g) for s in R.noise_shapes(SIZE)]
            probe = (torch.randn(B, 3, SIZE, SIZE, generator=g) / SIZE).to(dev)
            model = StyleGAN2(model='cars', search='z', weights=Ws, size=SIZE, device=dev)
            out = model.forward_z(z, noises=[n.to(dev) for n in noises])
            (out * probe).sum().backward()
            emit(case, 'z image', out)
            emit(case, 'dz', z.grad)
            model = StyleGAN2(model='cars', search='w+', weights=Ws, size=SIZE, device=dev)
            g = torch.Generator().manual_seed(4)
            wplus = (torch.randn(B, R.n_latent(SIZE), 512, generator=g) * 0.5).to(dev).requires_grad_(True)
            flat = torch.cat([n.reshape(B, -1) for n in noises], dim=1).to(dev).requires_grad_(True)
            out = model(wplus, flat)
            (out * probe).sum().backward()
            emit(case, 'w+ image', out)
            emit(case, 'dw+', wplus.grad)
            emit(case, 'dnoise', flat.grad)
    print('BITS-DONE', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', action='append', default=[], help='a libp2l_hip.so; give it twice or more')
    ap.add_argument('--out', help='also write the table to this file')
    ap.add_argument('--child', action='store_true')
    args = ap.parse_args()
    if args.child:
        return child()
    cols = []
    for lib in args.lib:
        env = dict(os.environ, P2L_LIB_PATH=os.path.abspath(lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, universal_newlines=True)
        lines = p.stdout.splitlines()
        if p.returncode != 0 or 'BITS-DONE' not in lines:
            # (a library that faulted is not started again, nor is the next one started behind it)
            sys.exit('plan_bits: the run with %s ended with status %d\n%s' % (lib, p.returncode, p.stdout[-2000:]))
        cols.append({l[5:-25]: l[-24:] for l in lines if l.startswith('BITS ')})
    keys = list(cols[0])
    bad = [k for k in keys if any(c.get(k) != cols[0][k] for c in cols)] + \
          [k for c in cols[1:] for k in c if k not in cols[0]]
    text = ['# tools/plan_bits.py: sha256 (first 24 hex digits) per output tensor; columns: ' + ' | '.join(args.lib)]
    text += ['%-52s %s%s' % (k, '  '.join(c.get(k, '-') for c in cols), '   DIFFERS' if k in bad else '') for k in keys]
    text.append('# %d tensors, %d differ' % (len(keys), len(bad)))
    print('\n'.join(text))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(text) + '\n')
    sys.exit(1 if bad or len(cols) < 2 else 0)


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    main()

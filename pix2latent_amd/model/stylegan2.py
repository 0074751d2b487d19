"""StyleGAN2 generator on the native MI355X path.

Host-side mirror of `pix2latent.model.StyleGAN2` (reference
pix2latent/model/stylegan2.py:66-138): `StyleGAN2(model='cars'|'ffhq', search='z'|'w+')`,
`__call__(z, noises=None, truncation=1.0)`, `forward_z`, `forward_w`, `reshape_noise`,
attributes `noise_shape`, `mean_latent` (z search) / `latent_mean`, `latent_std` (w+
search), `im_res`.  The arithmetic is libp2l_hip (`p2l_sg2_mapping_*`,
`p2l_sg2_synthesis_*`) instead of the git-cloned rosinality model + its two CUDA
extensions.  Generator parameters are frozen: gradients go to the latents and, in w+
search, to the noise inputs.

Not in the reference: `search='f'` (feature-space / F/W+ inversion) optimises the activation at
`f_res` -- `feat`, with the partial RGB `skip` -- next to the W+ rows and noise maps of the layers above it:
`features(z, noises)` captures both out of a W+ forward, `forward_f` / `__call__(z, noises, feat=, skip=)` run the
synthesis from there (`p2l_sg2_synthesis_from_*`), `feature_cut` is the arithmetic of the cut.
`search='s'` (StyleSpace) optimises the per-channel modulation scalars themselves, one flat
vector [S_total] per candidate named `z`: `styles(wplus)` computes them, `forward_s` runs the synthesis behind the
affines (`p2l_sg2_synthesis_s_*`), `style_layout` names the layers, `style_stats` gives the channel means and stds.

Weights: `$P2L_STYLEGAN2_<MODEL>_WEIGHTS` (a torch-loadable rosinality checkpoint with a
'g_ema' entry) if set, else seeded random-init tensors of the same architecture (no
network access here).  As in the reference, z-search draws fresh per-layer noise on
every forward unless `noises` is given.
"""
import collections
import ctypes as C
import math
import os
import warnings

import torch
import torch.nn as nn

from .. import _native as N
from .. import lanes
from ..utils import synthetic

IM_DIM = {'cars': 512, 'ffhq': 1024}
LR_MLP = 0.01


class _SynthFn(torch.autograd.Function):
    """latent [B, n_latent, 512] (+ layer-major noise) -> image [B,3,S,S]"""

    @staticmethod
    def forward(ctx, latent, noise_lm, model, want_dnoise):
        B = latent.shape[0]
        latent = latent.contiguous().float()
        noise_lm = noise_lm.contiguous().float()
        lib, S = model._lib, model.im_res
        s = model._ensure_ws(B)
        N.check(lib.p2l_sg2_synthesis_fwd(C.byref(model._desc), N.ptr(latent), N.ptr(noise_lm), B,
                                          N.ptr(s.ws), C.c_size_t(s.ws_bytes),
                                          N.ptr(s.img16), N.stream()), 'p2l_sg2_synthesis_fwd')
        out = torch.empty(B, 3, S, S, device=latent.device, dtype=torch.float32)
        N.check(lib.p2l_nhwc16_to_nchw3(N.ptr(s.img16), N.ptr(out), B, S, S, N.stream()),
                'p2l_nhwc16_to_nchw3')
        ctx.model, ctx.stamp, ctx.want_dnoise = model, model._scratch.stamp(), want_dnoise
        ctx.save_for_backward(latent, noise_lm)
        return out

    @staticmethod
    def backward(ctx, dout):
        with lanes.use(ctx.stamp[0]):    # (the saved activations live in the forward's lane)
            return _SynthFn._backward(ctx, dout)

    @staticmethod
    def _backward(ctx, dout):
        model = ctx.model
        latent, noise_lm = ctx.saved_tensors
        if model._scratch.stale(ctx.stamp):
            raise N.NativeError('StyleGAN2 workspace was reused by a later forward before '
                                'backward(); use one model object per in-flight graph')
        s = model._scratch.here()
        B, S, lib = latent.shape[0], model.im_res, model._lib
        N.check(lib.p2l_nchw3_to_nhwc16(N.ptr(dout.contiguous().float()), N.ptr(s.dimg16), B, S,
                                        S, N.stream()), 'p2l_nchw3_to_nhwc16')
        dlatent = torch.empty_like(latent)
        dnoise = torch.empty_like(noise_lm) if ctx.want_dnoise else None
        N.check(lib.p2l_sg2_synthesis_bwd(C.byref(model._desc), N.ptr(latent), N.ptr(noise_lm), B,
                                          N.ptr(s.ws), C.c_size_t(s.ws_bytes),
                                          N.ptr(s.dimg16), N.ptr(dlatent), N.ptr(dnoise),
                                          N.stream()), 'p2l_sg2_synthesis_bwd')
        return dlatent, dnoise, None, None


class _SynthFromFn(torch.autograd.Function):
    """(latent [B, n_latent, 512], layer-major noise, feat [B,C,r,r], skip [B,3,r,r]) -> image [B,3,S,S]: the
    synthesis from the cut at resolution r on (p2l_sg2_synthesis_from_fwd / _bwd), in the lane workspace of _SynthFn
    and under its stamp / stale check.  Each input gets a gradient only when autograd asks for it."""

    @staticmethod
    def forward(ctx, latent, noise_lm, feat, skip, model, res):
        B = latent.shape[0]
        latent = latent.contiguous().float()
        noise_lm = noise_lm.contiguous().float()
        feat = feat.contiguous().float()
        skip = skip.contiguous().float()
        lib, S = model._lib, model.im_res
        s = model._ensure_ws(B)
        N.check(lib.p2l_sg2_synthesis_from_fwd(C.byref(model._desc), res, N.ptr(feat), N.ptr(skip), N.ptr(latent),
                                               N.ptr(noise_lm), B, N.ptr(s.ws), C.c_size_t(s.ws_bytes),
                                               N.ptr(s.img16), N.stream()), 'p2l_sg2_synthesis_from_fwd')
        out = torch.empty(B, 3, S, S, device=latent.device, dtype=torch.float32)
        N.check(lib.p2l_nhwc16_to_nchw3(N.ptr(s.img16), N.ptr(out), B, S, S, N.stream()),
                'p2l_nhwc16_to_nchw3')
        ctx.model, ctx.stamp, ctx.res = model, model._scratch.stamp(), res
        ctx.shapes = (feat.shape, skip.shape)
        ctx.save_for_backward(latent, noise_lm)
        return out

    @staticmethod
    def backward(ctx, dout):
        with lanes.use(ctx.stamp[0]):    # (the saved activations live in the forward's lane)
            return _SynthFromFn._backward(ctx, dout)

    @staticmethod
    def _backward(ctx, dout):
        model = ctx.model
        latent, noise_lm = ctx.saved_tensors
        if model._scratch.stale(ctx.stamp):
            raise N.NativeError('StyleGAN2 workspace was reused by a later forward before '
                                'backward(); use one model object per in-flight graph')
        s = model._scratch.here()
        B, S, lib = latent.shape[0], model.im_res, model._lib
        N.check(lib.p2l_nchw3_to_nhwc16(N.ptr(dout.contiguous().float()), N.ptr(s.dimg16), B, S,
                                        S, N.stream()), 'p2l_nchw3_to_nhwc16')
        need = ctx.needs_input_grad
        # (the library always writes dlatent: the style gradients are what the pass reduces into)
        dlatent = torch.empty_like(latent)
        dnoise = torch.empty_like(noise_lm) if need[1] else None
        dfeat = torch.empty(ctx.shapes[0], device=latent.device, dtype=torch.float32) if need[2] else None
        dskip = torch.empty(ctx.shapes[1], device=latent.device, dtype=torch.float32) if need[3] else None
        N.check(lib.p2l_sg2_synthesis_from_bwd(C.byref(model._desc), ctx.res, N.ptr(latent), N.ptr(noise_lm), B,
                                               N.ptr(s.ws), C.c_size_t(s.ws_bytes), N.ptr(s.dimg16),
                                               N.ptr(dlatent), N.ptr(dnoise), N.ptr(dfeat), N.ptr(dskip),
                                               N.stream()), 'p2l_sg2_synthesis_from_bwd')
        return (dlatent if need[0] else None), dnoise, dfeat, dskip, None, None


class _SynthStyleFn(torch.autograd.Function):
    """(styles [B, S_total], layer-major noise) -> image [B,3,S,S]: the synthesis behind the affine layers
    (p2l_sg2_synthesis_s_fwd / _bwd), in the lane workspace of _SynthFn and under its stamp / stale check.  The noise
    gets a gradient only when autograd asks for it."""

    @staticmethod
    def forward(ctx, styles, noise_lm, model):
        B = styles.shape[0]
        styles = styles.contiguous().float()
        noise_lm = noise_lm.contiguous().float()
        lib, S = model._lib, model.im_res
        s = model._ensure_ws(B)
        N.check(lib.p2l_sg2_synthesis_s_fwd(C.byref(model._desc), N.ptr(styles), N.ptr(noise_lm), B, N.ptr(s.ws),
                                            C.c_size_t(s.ws_bytes), N.ptr(s.img16), N.stream()),
                'p2l_sg2_synthesis_s_fwd')
        out = torch.empty(B, 3, S, S, device=styles.device, dtype=torch.float32)
        N.check(lib.p2l_nhwc16_to_nchw3(N.ptr(s.img16), N.ptr(out), B, S, S, N.stream()),
                'p2l_nhwc16_to_nchw3')
        ctx.model, ctx.stamp = model, model._scratch.stamp()
        ctx.save_for_backward(styles, noise_lm)
        return out

    @staticmethod
    def backward(ctx, dout):
        with lanes.use(ctx.stamp[0]):    # (the saved activations live in the forward's lane)
            return _SynthStyleFn._backward(ctx, dout)

    @staticmethod
    def _backward(ctx, dout):
        model = ctx.model
        styles, noise_lm = ctx.saved_tensors
        if model._scratch.stale(ctx.stamp):
            raise N.NativeError('StyleGAN2 workspace was reused by a later forward before '
                                'backward(); use one model object per in-flight graph')
        s = model._scratch.here()
        B, S, lib = styles.shape[0], model.im_res, model._lib
        N.check(lib.p2l_nchw3_to_nhwc16(N.ptr(dout.contiguous().float()), N.ptr(s.dimg16), B, S,
                                        S, N.stream()), 'p2l_nchw3_to_nhwc16')
        need = ctx.needs_input_grad
        # (the library always writes dstyles: the style gradients are what the pass reduces into)
        dstyles = torch.empty_like(styles)
        dnoise = torch.empty_like(noise_lm) if need[1] else None
        N.check(lib.p2l_sg2_synthesis_s_bwd(C.byref(model._desc), N.ptr(styles), N.ptr(noise_lm), B, N.ptr(s.ws),
                                            C.c_size_t(s.ws_bytes), N.ptr(s.dimg16), N.ptr(dstyles), N.ptr(dnoise),
                                            N.stream()), 'p2l_sg2_synthesis_s_bwd')
        return (dstyles if need[0] else None), dnoise, None


StyleEntry = collections.namedtuple('StyleEntry', 'name kind index offset channels res')


def _style_entries(convs, rgbs):
    """network order from (cin, res) per conv and (cin, res, after_conv) per ToRGB"""
    out, off, rj = [], 0, 0
    for l, (cin, res) in enumerate(convs):
        out.append(StyleEntry('conv1' if l == 0 else 'convs.%d' % (l - 1), 'conv', l, off, int(cin), int(res)))
        off += int(cin)
        while rj < len(rgbs) and rgbs[rj][2] == l:
            out.append(StyleEntry('to_rgb1' if rj == 0 else 'to_rgbs.%d' % (rj - 1), 'rgb', rj, off, int(rgbs[rj][0]),
                                  int(rgbs[rj][1])))
            off += int(rgbs[rj][0])
            rj += 1
    return out


def style_layout(size, channels=None):
    """The StyleSpace layout of a generator of size `size` -- host arithmetic, no device: a list of
    (name, kind 'conv' | 'rgb', index, offset, channels, res) in network order (conv1, to_rgb1, then per resolution
    convs.{2j}, convs.{2j+1}, to_rgbs.{j}: the layer numbering of Wu et al., "StyleSpace Analysis", 2021).  An
    entry's `channels` is the layer's input width, the length of its modulation vector; `index` counts within the
    kind; the last offset + channels is S_total (9088 at 1024^2, 8960 at 512^2 with the released width table;
    `channels`: {resolution: width} overrides it)."""
    size = int(size)
    if size < 8 or size & (size - 1):
        raise ValueError('style layout of a %s^2 generator: the size is a power of two >= 8' % size)
    widths = dict(synthetic.sg2_channels())
    widths.update(channels or {})
    log_size = size.bit_length() - 1
    convs = []
    for l in range(2 * (log_size - 2) + 1):
        res = 4 if l == 0 else 2 ** ((l + 1) // 2 + 2)
        convs.append((widths[res // 2] if l % 2 == 1 else widths[res], res))
    rgbs = [(widths[4 * 2 ** j], 4 * 2 ** j, 2 * j) for j in range(log_size - 1)]
    return _style_entries(convs, rgbs)


FeatureCut = collections.namedtuple('FeatureCut', 'l0 j0 C rows noise_off')


def feature_cut(size, res, channels=None):
    """The cut of the feature-space (F/W+) run of a generator of size `size` at resolution `res` (a power of two,
    4 <= res <= size / 2; ValueError otherwise) -- host arithmetic, no device:
        l0        the first styled conv that still runs, 2 (log2 res - 2) + 1: the up conv to 2 res
        j0        the last ToRGB that no longer runs, log2 res - 2
        C         channels of the activation at res (`channels`: {resolution: width}, default the width table
                  of the released models)
        rows      the W+ rows the run reads (conv l reads row l, ToRGB j row 2 j + 1)
        noise_off the first element of a candidate's flat noise vector the run reads (sum of h w of conv[0 .. l0-1])
    The run reads feat = y[l0 - 1] and skip = skip[j0]; the W+ rows outside `rows` and the noise in front of
    `noise_off` are not read and get zero gradients."""
    size, r = int(size), int(res)
    if r != res or r < 4 or r & (r - 1) or size < 8 or size & (size - 1) or r > size // 2:
        raise ValueError('feature cut of a %s^2 generator at %s: the resolution is a power of two in 4 .. %d'
                         % (size, res, size // 2))
    k, log_size = r.bit_length() - 1, size.bit_length() - 1
    j0 = k - 2
    l0 = 2 * j0 + 1
    n_conv, n_rgb = 2 * (log_size - 2) + 1, log_size - 1
    rows = sorted(set(range(l0, n_conv)) | set(2 * j + 1 for j in range(j0 + 1, n_rgb)))
    noise_off = sum((4 if l == 0 else 2 ** ((l + 1) // 2 + 2)) ** 2 for l in range(l0))
    widths = dict(synthetic.sg2_channels())
    widths.update(channels or {})
    return FeatureCut(l0, j0, int(widths[r]), rows, noise_off)


class _NoiseLayoutFn(torch.autograd.Function):
    """noises [B, noise_total] (the reference's variable, model/stylegan2.py:128-138 slices it per layer) ->
    layer-major flat vector for the synthesis entry points; one launch each way (p2l_sg2_noise_relayout)
    where 17 slices + cat and their autograd transposes were 1.3 ms of a 25 ms FFHQ-1024 step"""

    @staticmethod
    def forward(ctx, noises, model):
        x = noises.contiguous().float()
        assert x.dim() == 2 and x.size(1) == model._desc.noise_total      # (reference stylegan2.py:137)
        out = torch.empty(x.numel(), device=x.device, dtype=torch.float32)
        N.check(model._lib.p2l_sg2_noise_relayout(C.byref(model._desc), N.ptr(x), N.ptr(out), x.size(0), 1,
                                                  N.stream()), 'p2l_sg2_noise_relayout')
        ctx.model, ctx.B = model, x.size(0)
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous().float()
        dx = torch.empty(ctx.B, ctx.model._desc.noise_total, device=g.device, dtype=torch.float32)
        N.check(ctx.model._lib.p2l_sg2_noise_relayout(C.byref(ctx.model._desc), N.ptr(g), N.ptr(dx), ctx.B, 0,
                                                      N.stream()), 'p2l_sg2_noise_relayout')
        return dx, None


class _MappingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, model):
        z = z.contiguous().float()
        B, D = z.shape
        w = torch.empty_like(z)
        acts = torch.empty(9, B, D, device=z.device, dtype=torch.float32)
        N.check(model._lib.p2l_sg2_mapping_fwd(C.byref(model._desc), N.ptr(z), N.ptr(w), N.ptr(acts),
                                               B, N.stream()), 'p2l_sg2_mapping_fwd')
        ctx.model = model
        ctx.save_for_backward(z, acts)
        model._last_acts = acts              # (test hook: oracle/replay.py reads the run's decisions)
        return w

    @staticmethod
    def backward(ctx, dw):
        z, acts = ctx.saved_tensors
        B, D = z.shape
        dz = torch.empty_like(z)
        scratch = torch.empty(2, B, D, device=z.device, dtype=torch.float32)
        N.check(ctx.model._lib.p2l_sg2_mapping_bwd(C.byref(ctx.model._desc), N.ptr(z), N.ptr(acts),
                                                   N.ptr(dw.contiguous().float()), N.ptr(dz),
                                                   N.ptr(scratch), B, N.stream()),
                'p2l_sg2_mapping_bwd')
        return dz, None


class StyleGAN2(nn.Module):
    def __init__(self, model='cars', search='z', weights=None, size=None, device='cuda', seed=0,
                 wfmt=None, f_res=32):
        super(StyleGAN2, self).__init__()
        if search == 'f':
            feature_cut(size if size is not None else IM_DIM[model], f_res)      # (ValueError for a bad f_res)
        self._dev = torch.device(device)
        if self._dev.type != 'cuda':
            raise N.NativeError('StyleGAN2 needs a ROCm device: the generator only exists as HIP '
                                'kernels (no CPU fallback)')
        self.im_res = size if size is not None else IM_DIM[model]
        if weights is None:
            path = os.environ.get('P2L_STYLEGAN2_%s_WEIGHTS' % model.upper())
            if path:
                ck = torch.load(path, map_location='cpu')
                weights = ck['g_ema'] if 'g_ema' in ck else ck
            else:
                warnings.warn('StyleGAN2: no checkpoint available (no network); using seeded '
                              'random-init weights of the %s architecture' % model)
                weights = synthetic.stylegan2_weights(self.im_res, seed)
        self._lib = N.lib()
        self._keep = []
        self._desc = N.P2LStyleGAN2()
        self._wfmt = N.default_wfmt() if wfmt is None else wfmt
        # (P2L_AMAX=0: every fp16 x 2 launch reduces the maxima of its input itself -- model descriptor flag)
        self._desc.wfmt = self._wfmt | (N.WFMT_FLAG_NO_AMAX if N.default_no_amax() else 0)
        self._scratch = lanes.Scratch()      # arena + image staging per lane (one per stream)
        self._pack(weights)
        self.search = search
        self.f_res = int(f_res) if search == 'f' else None
        with torch.no_grad():
            n_mean_latent = 4096
            g = torch.Generator(device='cpu').manual_seed(seed + 1)
            zs = torch.randn(n_mean_latent, 512, generator=g).to(self._dev)
            latent_out = self.mapping(zs)
            if search == 'z':
                self.mean_latent = latent_out.mean(0, keepdim=True)
            elif search in ('w+', 'f', 's'):       # ('s': a W+ start is the usual way into StyleSpace)
                self.latent_mean = latent_out.mean(0)
                latent_std = (latent_out - self.latent_mean).pow(2).sum()
                self.latent_std = (latent_std / n_mean_latent) ** 0.5
        return

    # ------------------------------------------------------------------ setup
    def _t(self, t):
        t = t.detach().to(self._dev, torch.float32).contiguous()
        self._keep.append(t)
        return t.data_ptr()

    def _pack_w(self, w, taps, n_pad, k_pad, flip, subpix=False):
        dst = N.pack_conv_weight(w.detach().to(self._dev, torch.float32), taps, n_pad, k_pad, flip,
                                 self._wfmt, subpix_mode=1 if subpix else None)
        torch.cuda.current_stream().synchronize()
        self._keep.append(dst)
        return dst.data_ptr()

    def _pack(self, W):
        d = self._desc
        S = self.im_res
        log_size = int(math.log2(S))
        d.size, d.style_dim = S, 512
        d.n_latent = log_size * 2 - 2
        for i in range(8):
            wt = W['style.%d.weight' % (i + 1)].float() * (LR_MLP / math.sqrt(512))
            d.map_w[i] = self._t(wt.t())
            d.map_b[i] = self._t(W['style.%d.bias' % (i + 1)].float() * LR_MLP)
        d.const_input = self._t(W['input.input'][0].permute(1, 2, 0))
        names = ['conv1'] + ['convs.%d' % i for i in range(2 * (log_size - 2))]
        self.noise_shape = []
        self._widths = {}
        noise_off = 0
        for l, nm in enumerate(names):
            c = d.conv[l]
            w = W[nm + '.conv.weight'][0].float()                 # [out, in, 3, 3]
            cout, cin = w.shape[0], w.shape[1]
            up = (l >= 1) and (l % 2 == 1)
            res = 4 if l == 0 else 2 ** ((l + 1) // 2 + 2)
            ws = w / math.sqrt(cin * 9)
            c.cin, c.cout, c.up, c.res = cin, cout, int(up), res
            self._widths[res] = cout
            c.w = self._pack_w(ws, 9, cout, cin, False, subpix=up)
            c.wt = self._pack_w(ws, 9, cin, cout, True, subpix=up)
            c.wsq = self._t((ws ** 2).sum((2, 3)).t())            # [cin][cout]
            c.mod_w = self._t((W[nm + '.conv.modulation.weight'].float() / math.sqrt(512)).t())
            c.mod_b = self._t(W[nm + '.conv.modulation.bias'].float())
            c.act_b = self._t(W[nm + '.activate.bias'].float())
            c.noise_w = float(W[nm + '.noise.weight'].reshape(-1)[0])
            c.latent_idx = l
            c.noise_off = noise_off
            noise_off += res * res
            self.noise_shape.append([1, 1, res, res])
        d.n_conv = len(names)
        d.noise_total = noise_off
        rgb_names = ['to_rgb1'] + ['to_rgbs.%d' % j for j in range(log_size - 2)]
        for j, nm in enumerate(rgb_names):
            r = d.rgb[j]
            w = W[nm + '.conv.weight'][0].float()                 # [3, cin, 1, 1]
            cin = w.shape[1]
            ws = w / math.sqrt(cin)
            r.cin, r.res = cin, 4 * (2 ** j)
            r.after_conv = 2 * j
            r.latent_idx = 2 * j + 1
            r.w = self._pack_w(ws, 1, 32, cin, False)
            r.wt = self._pack_w(ws, 1, cin, 16, True)
            r.mod_w = self._t((W[nm + '.conv.modulation.weight'].float() / math.sqrt(512)).t())
            r.mod_b = self._t(W[nm + '.conv.modulation.bias'].float())
            b32 = torch.zeros(32)
            b32[:3] = W[nm + '.bias'].reshape(-1)
            r.bias = self._t(b32)
        d.n_rgb = len(rgb_names)
        self._noise_sizes = [s[-1] * s[-2] for s in self.noise_shape]
        # StyleSpace layout in network order; the library's walk of the same descriptor has to agree (a library built
        # before the entry point existed -- P2L_LIB_PATH, the A/B runs of tools/plan_bits.py -- is not asked)
        self.style_layout = _style_entries([(d.conv[l].cin, d.conv[l].res) for l in range(d.n_conv)],
                                           [(d.rgb[j].cin, d.rgb[j].res, d.rgb[j].after_conv) for j in range(d.n_rgb)])
        self.n_styles = self.style_layout[-1].offset + self.style_layout[-1].channels
        if hasattr(self._lib, 'p2l_sg2_style_layout'):
            co, ro, total = (C.c_int32 * d.n_conv)(), (C.c_int32 * d.n_rgb)(), C.c_int32(0)
            N.check(self._lib.p2l_sg2_style_layout(C.byref(d), co, ro, C.byref(total)), 'p2l_sg2_style_layout')
            offs = {'conv': co, 'rgb': ro}
            assert all(offs[e.kind][e.index] == e.offset for e in self.style_layout) and total.value == self.n_styles
        self._style_stats = {}

    lanes_ok = True              # per-lane workspaces: chunks of one step may run on several streams
    _lanes = property(lambda self: self._scratch.lanes)

    def _ws_bytes(self, B, H, W):
        nbytes = self._lib.p2l_sg2_ws_bytes(C.byref(self._desc), B)
        if nbytes == 0:
            raise N.NativeError('p2l_sg2_ws_bytes rejected batch %d' % B)
        return nbytes

    def _ensure_ws(self, B):
        # (32 samples = chunks of 9,9,9,5 alternate B)
        return self._scratch.grow(B, self.im_res, self.im_res, self._ws_bytes, self._dev)

    def saved_activation(self, layer, B):
        """test hook: view of the post-activation output of styled conv `layer` inside the workspace
        of the last synthesis forward on B candidates, NHWC"""
        off = C.c_size_t(0)
        shape = (C.c_int32 * 4)()
        N.check(self._lib.p2l_sg2_ws_lookup(C.byref(self._desc), B, layer, C.byref(off), shape),
                'p2l_sg2_ws_lookup')
        n = shape[0] * shape[1] * shape[2] * shape[3]
        return self._scratch.here().ws[off.value:off.value + n].view(*list(shape))

    def saved_skip(self, j, B):
        """test hook: view of the unclamped partial RGB behind ToRGB `j` inside the workspace of the last synthesis
        forward on B candidates, NHWC16 (3 real channels)"""
        return self.saved_activation(1000 + j, B)          # (P2L_SG2_WS_SKIP, include/p2l_test.h)

    # -------------------------------------------------------------- pieces
    def mapping(self, z):
        """PixelNorm + 8 EqualLinear/fused-lrelu layers: z [B,512] -> w [B,512]"""
        return _MappingFn.apply(z.to(self._dev), self)

    def _noise_layer_major(self, noises, B):
        """list of [B,1,h,w] (or None -> fresh normal noise, as NoiseInjection does)"""
        if noises is None:
            noises = [torch.randn(B, 1, s[-2], s[-1], device=self._dev) for s in self.noise_shape]
        return torch.cat([n.reshape(B, -1).reshape(-1) for n in noises])

    def synthesis(self, latent, noises=None, want_dnoise=False):
        B = latent.shape[0]
        if torch.is_tensor(noises) and noises.dim() == 1:
            noise_lm = noises
        else:
            noise_lm = self._noise_layer_major(noises, B)
        return _SynthFn.apply(latent, noise_lm, self, want_dnoise)

    # ------------------------------------------------------------- public API
    def __call__(self, z, noises=None, truncation=1.0, feat=None, skip=None):
        if self.search == 'f':
            return self.forward_f(z, noises, feat, skip)
        if feat is not None or skip is not None:
            raise ValueError("feat / skip are the inputs of search='f'; this model searches %r" % (self.search,))
        if self.search == 'w+':
            return self.forward_w(z, noises)
        if self.search == 's':
            return self.forward_s(z, noises)
        return self.forward_z(z, noises=noises)

    class _CutMethod(object):
        """`model.feature_cut(res)`: the cut of THIS generator (C, the W+ rows and the noise offset come from its
        descriptor); `StyleGAN2.feature_cut(size, res, channels=None)`: the same arithmetic without a model or a
        device (the module's `feature_cut`)."""

        def __get__(self, obj, cls):
            return feature_cut if obj is None else obj._feature_cut

    feature_cut = _CutMethod()

    def _feature_cut(self, res):
        cut = feature_cut(self.im_res, res, self._widths)
        d = self._desc
        rows = sorted(set(d.conv[l].latent_idx for l in range(cut.l0, d.n_conv)) |
                      set(d.rgb[j].latent_idx for j in range(cut.j0 + 1, d.n_rgb)))
        return FeatureCut(cut.l0, cut.j0, d.conv[cut.l0].cin, rows, d.conv[cut.l0].noise_off)

    def _feat_shapes(self, B, res):
        return (B, self._feature_cut(res).C, res, res), (B, 3, res, res)

    def features(self, z, noises, res=None):
        """(feat [B,C,r,r], skip [B,3,r,r]) of the W+ latents z and the flat noises at resolution `res` (default
        `f_res`): the activation behind the plain styled conv at r and the unclamped partial RGB there, as
        `forward_f` takes them.  One full forward under no_grad, then p2l_sg2_capture: the results are copies,
        not views of the workspace."""
        res = self.f_res if res is None else res
        if res is None:
            raise ValueError('features: give res (the model was not built with search=\'f\')')
        B = z.shape[0]
        fs, ss = self._feat_shapes(B, res)
        with torch.no_grad():
            self.forward_w(z.detach().to(self._dev), noises.detach())
            s = self._scratch.here()
            feat = torch.empty(fs, device=self._dev, dtype=torch.float32)
            skip = torch.empty(ss, device=self._dev, dtype=torch.float32)
            N.check(self._lib.p2l_sg2_capture(C.byref(self._desc), int(res), B, N.ptr(s.ws), C.c_size_t(s.ws_bytes),
                                              N.ptr(feat), N.ptr(skip), N.stream()), 'p2l_sg2_capture')
        return feat, skip

    def forward_f(self, z, noises, feat, skip, res=None):
        """the synthesis from resolution r = `f_res` on: z [B, n_latent, 512] (or [B,512]) W+ latents, of which the
        rows `feature_cut(r).rows` are read; noises [B, sum(h*w)] flat, read from `feature_cut(r).noise_off` on;
        feat [B,C,r,r] the activation at r and skip [B,3,r,r] the partial RGB there (`features`).  Gradients go to
        all four; what is not read gets zeros."""
        res = self.f_res if res is None else res
        if res is None:
            raise ValueError('forward_f: give res (the model was not built with search=\'f\')')
        B = z.shape[0]
        fs, ss = self._feat_shapes(B, res)
        if feat is None or skip is None or tuple(feat.shape) != fs or tuple(skip.shape) != ss:
            raise ValueError("search='f' at resolution %d takes feat %s and skip %s, got %s and %s"
                             % (res, list(fs), list(ss), None if feat is None else list(feat.shape),
                                None if skip is None else list(skip.shape)))
        if noises is None:
            raise ValueError("search='f' takes the flat noises [B, %d]" % self._desc.noise_total)
        latent = z if z.dim() == 3 else z.unsqueeze(1).expand(-1, self._desc.n_latent, -1)
        noise_lm = _NoiseLayoutFn.apply(noises.to(self._dev), self)
        return _SynthFromFn.apply(latent, noise_lm, feat.to(self._dev), skip.to(self._dev), self, int(res))

    # ----------------------------------------------------- StyleSpace (S) search
    style_layout = staticmethod(style_layout)      # (on the class: no model, no device; an instance holds its list)

    def styles(self, wplus):
        """[B, S_total]: every layer's affine of its row of the W+ latents wplus [B, n_latent, 512] (or [B, 512], one
        w for all layers), in the order of `style_layout` -- the bits a forward_w leaves in its style slots
        (p2l_sg2_styles: the affines alone, no synthesis).  Under no_grad; the result is a new tensor."""
        with torch.no_grad():
            w = wplus.detach().to(self._dev, torch.float32)
            latent = (w if w.dim() == 3 else w.unsqueeze(1).expand(-1, self._desc.n_latent, -1)).contiguous()
            B = latent.shape[0]
            if tuple(latent.shape) != (B, self._desc.n_latent, 512):
                raise ValueError('styles: W+ latents are [B, %d, 512] or [B, 512], got %s'
                                 % (self._desc.n_latent, list(wplus.shape)))
            out = torch.empty(B, self.n_styles, device=self._dev, dtype=torch.float32)
            N.check(self._lib.p2l_sg2_styles(C.byref(self._desc), N.ptr(latent), B, N.ptr(out), N.stream()),
                    'p2l_sg2_styles')
        return out

    def style_stats(self, num_samples=100000, chunk_rows=65536, seed=0):
        """(mean, std) fp64 [S_total] on the device: the channel statistics of styles(mapping(z)) over `num_samples`
        normal z, drawn chunk by chunk (`chunk_rows` rows at a time) from one CPU generator seeded with `seed`.  The
        moments are p2l_col_moments_f64 sums continued from chunk to chunk; std is the population one,
        sqrt(E x^2 - mean^2).  Cached on the model per (num_samples, chunk_rows, seed)."""
        from .. import ops
        key = (int(num_samples), int(chunk_rows), int(seed))
        if key[0] < 1 or key[1] < 1:
            raise ValueError('style_stats: num_samples and chunk_rows are at least 1')
        if key not in self._style_stats:
            g = torch.Generator(device='cpu').manual_seed(key[2])
            sums = None
            with torch.no_grad():
                for lo in range(0, key[0], key[1]):
                    rows = min(key[1], key[0] - lo)
                    z = torch.randn(rows, 512, generator=g).to(self._dev)
                    # (the mapping in batches of the size the constructor uses)
                    w = torch.cat([self.mapping(z[i:i + 4096]) for i in range(0, rows, 4096)])
                    st = torch.cat([self.styles(w[i:i + 4096]) for i in range(0, rows, 4096)])
                    sums = ops.col_moments_f64(st, *(sums or ()))
            mean = sums[0] / key[0]
            var = (sums[1] / key[0] - mean * mean).clamp_(min=0.0)
            self._style_stats[key] = (mean, var.sqrt())
        return self._style_stats[key]

    def forward_s(self, z, noises):
        """the synthesis behind the affine layers: z [B, S_total] the styles (`styles`, `style_layout`), noises
        [B, sum(h*w)] flat.  Gradients go to both."""
        if z.dim() != 2 or z.shape[1] != self.n_styles:
            raise ValueError("search='s' takes the styles [B, S_total = %d], got %s" % (self.n_styles, list(z.shape)))
        if noises is None:
            raise ValueError("search='s' takes the flat noises [B, %d]" % self._desc.noise_total)
        noise_lm = _NoiseLayoutFn.apply(noises.to(self._dev), self)
        return _SynthStyleFn.apply(z.to(self._dev), noise_lm, self)

    def forward_z(self, z, truncation=1.0, noises=None):
        """generator([z], truncation=1.0).clamp_(-1, 1); `noises` (list of [B,1,h,w]) makes
        the per-layer noise explicit (the reference draws it fresh on every call)."""
        w = self.mapping(z)
        latent = w.unsqueeze(1).expand(-1, self._desc.n_latent, -1)
        return self.synthesis(latent, noises)

    def forward_w(self, z, noises, truncation=1.0):
        """z: w+ latents [B, n_latent, 512] (or [B,512]); noises: [B, sum(h*w)] flat."""
        B = z.shape[0]
        latent = z if z.dim() == 3 else z.unsqueeze(1).expand(-1, self._desc.n_latent, -1)
        noise_lm = _NoiseLayoutFn.apply(noises.to(self._dev), self)
        return _SynthFn.apply(latent, noise_lm, self, bool(noises.requires_grad))

    def reshape_noise(self, z):
        st_idx = 0
        noises = []
        for d in self.noise_shape:
            en_idx = st_idx + (d[-2] * d[-1])
            noises.append(z[:, st_idx:en_idx].reshape(-1, 1, d[-2], d[-1]))
            st_idx = en_idx

        assert z.size(1) == en_idx
        return noises

    def cuda(self, device=None):
        return self

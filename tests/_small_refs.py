"""Plain float64 references of the small entry points of include/p2l.h (the HBM-bound glue of both generators, the
losses and the optimiser), written from the formulas in the header comments and the reference arithmetic they cite
-- not from the kernels.  Forwards are direct restatements; every backward is autograd through its forward in
float64 (`vjp`).  Everything runs on torch-CPU.  tests/test_small_refs.py checks these functions against
independent formulations, tests/test_small_kernels_gpu.py, tests/test_loss_kernels_gpu.py and
tests/test_glue_kernels_gpu.py hold the kernels to them.  (The closed-form lpips_tap_bwd and the pool backwards are the exceptions to "autograd through the forward":
the first because autograd has no value at ||f|| == 0, the second are autograd through F.max_pool2d.)

Layouts are those of the ABI: activations NHWC, images NHWC16 (3 channels in 16 floats), targets / weights NCHW3.
Every function takes tensors of any float dtype and computes in the dtype of its first argument, so that the same
text is the fp64 reference and -- called with float32 tensors -- the "straightforward fp32 restatement" the GPU
tests use as a yardstick for the error bars."""
import math

import torch
import torch.nn.functional as F

SQRT2 = math.sqrt(2.0)
SLOPE = 0.2
U = 2.0 ** -24          # unit round-off of fp32


def vjp(fn, inputs, grad_out, wrt=None):
    """gradients of sum(fn(*inputs) * grad_out) w.r.t. inputs[i], i in wrt (default: all), by autograd."""
    wrt = list(range(len(inputs))) if wrt is None else list(wrt)
    xs = [t.detach().clone().requires_grad_(i in wrt) for i, t in enumerate(inputs)]
    out = fn(*xs)
    outs = out if isinstance(out, (tuple, list)) else (out,)
    gos = grad_out if isinstance(grad_out, (tuple, list)) else (grad_out,)
    total = sum((o * g.to(o.dtype)).sum() for o, g in zip(outs, gos))
    grads = torch.autograd.grad(total, [xs[i] for i in wrt], allow_unused=True)
    grads = [torch.zeros_like(xs[i]) if g is None else g for i, g in zip(wrt, grads)]
    return grads if len(grads) > 1 else grads[0]


def lrelu(v):
    """leaky_relu(0.2): the branch torch.where(v > 0, ...) takes (0 and -0 go down the negative slope)."""
    return torch.where(v > 0, v, SLOPE * v)


# ---- StyleGAN2 mapping network ---------------------------------------------------------------------------------
def pixelnorm(z):                                   # PixelNorm: x * rsqrt(mean(x^2, dim=1) + 1e-8)
    return z * torch.rsqrt((z * z).mean(dim=1, keepdim=True) + 1e-8)


def bias_lrelu(x, bias, bias_mul):                  # fused_leaky_relu(x, bias * lr_mul)
    return lrelu(x + bias.to(x.dtype) * bias_mul) * SQRT2


def lrelu_bwd(y, g):
    """g * d(lrelu(v) * sqrt2)/dv at a pre-activation of the sign of the saved output y."""
    return vjp(lambda v: lrelu(v) * SQRT2, [y], g)


# ---- StyleGAN2 modulation ----------------------------------------------------------------------------------------
def demod(s, Wsq):                                  # d[b,o] = rsqrt(sum_i s[b,i]^2 Wsq[i][o] + 1e-8)
    return torch.rsqrt((s * s) @ Wsq.to(s.dtype) + 1e-8)


def demod_bwd(s, Wsq, dd):
    return vjp(lambda s_: demod(s_, Wsq), [s], dd)


def scale_fwd(x, s):                                # a[b,p,c] = x[b,p,c] * s[b,c]
    return x * s.to(x.dtype)[:, None, :]


def scale_bwd(da, x, s, skip=None, skip_C=0):
    """dx = da * s (+ skip on channels < skip_C), ds[b,c] = sum_p da * x; x, da: [B, P, C]"""
    dx, ds = vjp(scale_fwd, [x, s.to(x.dtype)], da)
    if skip is not None:
        dx = dx.clone()
        dx[:, :, :skip_C] += skip.to(dx.dtype)[:, :, :skip_C]
    return dx, ds


# ---- StyleGAN2 styled-conv activation -----------------------------------------------------------------------------
def styled_act(c, d, noise, nw, bias):
    """y = lrelu(c * d[b,ch] + nw * noise[b,p] + bias[ch]) * sqrt2 ; c: [B, P, C], noise: [B, P] or None"""
    pre = c * d[:, None, :] + bias[None, None, :]
    if noise is not None:
        pre = pre + nw * noise[:, :, None]
    return lrelu(pre) * SQRT2


def styled_act_bwd(dy, c, d, noise, nw, bias):
    """-> gd (gradient of the un-scaled conv result c), dd [B, C], dnoise [B, P] (or None) from the TRUE c"""
    if noise is None:
        gd, dd = vjp(lambda c_, d_: styled_act(c_, d_, None, nw, bias), [c, d], dy)
        return gd, dd, None
    gd, dd, dn = vjp(lambda c_, d_, n_: styled_act(c_, d_, n_, nw, bias), [c, d, noise], dy)
    return gd, dd, dn


# ---- StyleGAN2 image tail -----------------------------------------------------------------------------------------
def upfirdn2d_up2(x):
    """upfirdn2d(x, [1,3,3,1] x [1,3,3,1] / 16 * 4, up=2, pad=(2,1)) on [B, C, h, w]: zero-insert, zero-pad, FIR
    with the flipped kernel."""
    b, c, h, w = x.shape
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=x.dtype)
    k = torch.outer(k1, k1)
    k = k / k.sum() * 4
    o = x.new_zeros(b, c, h, 2, w, 2)
    o[:, :, :, 0, :, 0] = x
    o = F.pad(o.reshape(b, c, 2 * h, 2 * w), [2, 1, 2, 1])
    wk = torch.flip(k, [0, 1]).view(1, 1, 4, 4)
    return F.conv2d(o.reshape(b * c, 1, 2 * h + 3, 2 * w + 3), wk).view(b, c, 2 * h, 2 * w)


def rgb_up(skip16):
    """[B, h, w, 16] -> [B, 2h, 2w, 16]: channels 0..3 filtered, 4..15 zero (p2l.h)."""
    x = skip16[..., :4].permute(0, 3, 1, 2)
    up = upfirdn2d_up2(x).permute(0, 2, 3, 1)
    return torch.cat([up, up.new_zeros(up.shape[:3] + (12,))], dim=3)


def rgb_up_bwd(dout16, h, w):
    B = dout16.shape[0]
    return vjp(rgb_up, [dout16.new_zeros(B, h, w, 16)], dout16)


def clamp16(x16):
    """channels 0..2 clamped to [-1, 1], 3..15 zero."""
    y = torch.zeros_like(x16)
    idx = torch.zeros(16, dtype=torch.bool)
    idx[:3] = True
    return torch.where(idx, torch.clamp(x16, -1.0, 1.0), y)


def clamp16_bwd(x16, dy16):
    return vjp(clamp16, [x16], dy16)


# ---- BigGAN conditioning ------------------------------------------------------------------------------------------
def cbn_fold(g_raw, b_raw, mean, rstd):             # s = (1 + g) * rstd ; t = b - mean * s
    s = (1.0 + g_raw) * rstd.to(g_raw.dtype)
    return s, b_raw - mean.to(g_raw.dtype) * s


def cbn_fold_bwd(ds, dt, mean, rstd):
    z = torch.zeros_like(ds)
    return vjp(lambda g_, b_: cbn_fold(g_, b_, mean.to(ds.dtype), rstd.to(ds.dtype)), [z, z.clone()], (ds, dt))


def linear(x, W, bias=None):                        # y[b][n] = sum_k x[b][k] W[k][n] + bias[n]
    y = x @ W.to(x.dtype)
    return y if bias is None else y + bias.to(x.dtype)


def linear_bwd(dy, W):
    K = W.shape[0]
    return vjp(lambda x_: linear(x_, W.to(dy.dtype)), [dy.new_zeros(dy.shape[0], K)], dy)


# ---- image layout -------------------------------------------------------------------------------------------------
def nchw3_to_nhwc16(src):
    B, _, H, W = src.shape
    out = src.new_zeros(B, H, W, 16)
    out[..., :3] = src.permute(0, 2, 3, 1)
    return out


def nhwc16_to_nchw3(src16):
    return src16[..., :3].permute(0, 3, 1, 2).contiguous()


def tanh_bwd16(img16, dimg16):
    """d(pre-tanh) on channels 0..2 = autograd through tanh at pre = atanh(img); channel 3 -> 0, 4..15 unchanged"""
    img = img16[..., :3]
    pre = torch.atanh(img.clamp(-1 + 1e-12, 1 - 1e-12))
    out = dimg16.clone()
    out[..., :3] = vjp(torch.tanh, [pre], dimg16[..., :3])
    out[..., 3] = 0
    return out


def relu_mask(y, g):
    return vjp(torch.relu, [y], g)                  # torch.relu's gradient at 0 (and -0) is 0


# ---- losses -------------------------------------------------------------------------------------------------------
def _w(weight, loss_mask):
    return weight if loss_mask is None else loss_mask.to(weight.dtype) * weight


def weight_sum(weight, loss_mask=None):             # [B,3,H,W] -> [B]
    return _w(weight, loss_mask).sum(dim=(1, 2, 3))


def weight_map(weight, loss_mask=None):             # [B,3,H,W] -> [B,H,W]
    return _w(weight, loss_mask).sum(dim=1)


def l1_loss(img16, target, weight, loss_mask=None):
    """sum |target - out| * w / sum w over (c, p): ReconstructionLoss with weights (loss_functions.py:117-124)."""
    out = nhwc16_to_nchw3(img16)
    w = _w(weight.to(img16.dtype), loss_mask)
    return (torch.abs(target.to(img16.dtype) - out) * w).sum(dim=(1, 2, 3)) / w.sum(dim=(1, 2, 3))


def l1_loss_bwd(img16, target, weight, loss_mask, gscale):
    return vjp(lambda i_: l1_loss(i_, target, weight, loss_mask), [img16], gscale)


def reduce_rows(partial, scale, div=None):
    s = partial.sum(dim=1) * scale
    return s if div is None else s / div.to(s.dtype)


def vec_scale_div(a, scale, div=None):
    return a * scale if div is None else a * scale / div.to(a.dtype)


# ---- LPIPS loss path (tests/test_loss_kernels_gpu.py) -------------------------------------------------------------
# features are NHWC: f, nft [B, P, C] (or [B, H, W, C]); a target shared by the batch is nft [P, C] / wt [P]
def lpips_normalize(f):                             # nf = f / (||f||_2 + 1e-10), the norm over the channels
    return f / (torch.sqrt((f * f).sum(dim=-1, keepdim=True)) + 1e-10)


def lpips_tap(f, nft, lin, wt):
    """[B]: sum_p wt[p] * sum_c lin_c (nf - nft)^2"""
    d = (lin.to(f.dtype) * (lpips_normalize(f) - nft.to(f.dtype)) ** 2).sum(dim=-1)
    return (d * wt.to(f.dtype)).sum(dim=-1)


def lpips_tap_bwd(f, nft, lin, wt, gscale):
    """df[b,p,:] = gscale[b] * wt[b,p] * d(sum_c lin_c (nf - nft)^2) / df in closed form: with u = 2 lin (nf - nft)
    and inv = 1 / (nrm + 1e-10), df = gscale wt (u inv - c2 f), c2 = (u . f) inv^2 / nrm -- and c2 = 0 where
    nrm == 0, where d nrm / df does not exist (autograd: NaN) and f = 0 removes the term: df = gscale wt u / 1e-10"""
    nrm = torch.sqrt((f * f).sum(dim=-1, keepdim=True))
    inv = 1.0 / (nrm + 1e-10)
    u = 2.0 * lin.to(f.dtype) * (f * inv - nft.to(f.dtype))
    uf = (u * f).sum(dim=-1, keepdim=True)
    c2 = torch.where(nrm > 0, uf * inv * inv / torch.where(nrm > 0, nrm, torch.ones_like(nrm)), torch.zeros_like(nrm))
    gsw = gscale.to(f.dtype).view(-1, 1) * wt.to(f.dtype)
    return gsw[..., None] * (u * inv - c2 * f)


def _pool_vjp(x, gp, k, s):
    """gradient of sum(max_pool2d(x, k, s) * gp) w.r.t. x, NHWC in and out: ATen sends the gradient of a window to
    its first maximum in scan order"""
    g = vjp(lambda x_: F.max_pool2d(x_.permute(0, 3, 1, 2), k, s), [x], gp.to(x.dtype).permute(0, 3, 1, 2))
    return g


def maxpool2_bwd(y, dyp, add=None, relu_mask=False):
    """y [B,H,W,C], dyp [B,H/2,W/2,C]: pool backward, then + add, then * (y > 0)"""
    dy = _pool_vjp(y, dyp, 2, 2)
    if add is not None:
        dy = dy + add.to(y.dtype)
    return dy * (y > 0).to(y.dtype) if relu_mask else dy


def maxpool3s2(x):                                  # [B,Hi,Wi,C] -> [B,Ho,Wo,C], 3x3 windows, stride 2, no padding
    return F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1).contiguous()


def maxpool3s2_bwd(x, gp, gtap=None):
    """(pool backward of gp + gtap) * (x > 0)"""
    dx = _pool_vjp(x, gp, 3, 2)
    if gtap is not None:
        dx = dx + gtap.to(x.dtype)
    return dx * (x > 0).to(x.dtype)


def lpips_tap_pool_bwd(f, nft, lin, wt, gscale, dyp):
    """f [B,H,W,C] is a tap and the input of relu -> 2x2 max pool: tap backward, then the pool backward with the tap
    gradient as the additive term and the ReLU mask"""
    B, H, W, C = f.shape
    tap = lpips_tap_bwd(f.reshape(B, H * W, C), nft, lin, wt, gscale).view(B, H, W, C)
    return maxpool2_bwd(f, dyp, tap, True)


def bilinear_adjoint(wsrc, h, w):
    """wsrc [B,H,W] -> [B,h,w]: the adjoint of F.interpolate(bilinear, align_corners=False) from h x w up to H x W"""
    B, H, W = wsrc.shape
    up = lambda m: F.interpolate(m, size=(H, W), mode='bilinear', align_corners=False)
    return vjp(up, [wsrc.new_zeros(B, 1, h, w)], wsrc[:, None])[:, 0]


def conv1_dgrad(g, w_t3, H, W, K, S, pad):
    """g [B,Ho,Wo,Co], w_t3 [K*K][3][Co] -> NHWC16 gradient of the H x W input of the stride-S KxK conv; pixels past
    the last window get nothing (output_padding), channels 3..15 are zero"""
    B, Ho, Wo, Co = g.shape
    wgt = w_t3.to(g.dtype).view(K, K, 3, Co).permute(3, 2, 0, 1)                      # [Co, 3, K, K]
    opad = (H + 2 * pad - K - (Ho - 1) * S, W + 2 * pad - K - (Wo - 1) * S)
    d = F.conv_transpose2d(g.permute(0, 3, 1, 2), wgt, stride=S, padding=pad, output_padding=opad)
    out = g.new_zeros(B, H, W, 16)
    out[..., :3] = d.permute(0, 2, 3, 1)
    return out


# ---- glue kernels (tests/test_glue_kernels_gpu.py) -----------------------------------------------------------------
def gemm(A, B, M, N, K, a_kmajor=False, b_kmajor=False, alpha=1.0, C0=None):
    """C[b] = alpha * op(A[b]) op(B[b]) (+ C0[b]).  A: [batch, M, lda] (K contiguous) or, K-major, [batch, K, lda]
    (M contiguous); B: [batch or 1, N, ldb] or [batch or 1, K, ldb]; C0: [batch, M, ldc].  Pitches may exceed the
    row: the gap columns are not read.  -> [batch, M, N]"""
    a = A[..., :K, :M].transpose(-1, -2) if a_kmajor else A[..., :M, :K]
    b = B[..., :K, :N] if b_kmajor else B[..., :N, :K].transpose(-1, -2)
    out = alpha * torch.matmul(a, b.to(a.dtype))
    return out if C0 is None else out + C0[..., :N].to(a.dtype)


def softmax_rows(S):                                # P = exp(S - max) / sum exp(S - max), over the last dimension
    e = torch.exp(S - S.max(dim=-1, keepdim=True)[0].detach())
    return e / e.sum(dim=-1, keepdim=True)


def softmax_rows_bwd(P, dP):
    """dS = P (dP - sum_row P dP) from the SAVED probabilities, as the kernel gets them (fp32-rounded: they need not
    add up to 1, and hold exact zeros, so there are no logits to differentiate at).  The exception to "autograd
    through the forward"; tests/test_small_refs.py holds it against vjp(softmax_rows) where P is the softmax itself."""
    return P * (dP.to(P.dtype) - (P * dP.to(P.dtype)).sum(dim=-1, keepdim=True))


def affine_relu_fwd(x, s, t):                       # a[b,p,c] = max(x[b,p,c] * s[b,c] + t[b,c], 0)
    return torch.relu(x * s.to(x.dtype)[:, None, :] + t.to(x.dtype)[:, None, :])


def skip_term(skip, skip_C, skip_ups, Bn, H, W, C):
    """[B, H*W, C]: skip on channels < skip_C, zero above; skip_ups: skip is [B, 2H, 2W, *] and its 2x2 children
    are summed (the backward of nearest x 2)"""
    out = skip.new_zeros(Bn, H * W, C)
    if skip_ups:
        sk = skip.reshape(Bn, H, 2, W, 2, skip.shape[-1]).sum(dim=(2, 4))
    else:
        sk = skip
    out[:, :, :skip_C] = sk.reshape(Bn, H * W, -1)[:, :, :skip_C]
    return out


def affine_relu_bwd(da, x, s, t, skip=None, skip_C=0, skip_ups=False, H=None, W=None):
    """-> dx [B,P,C] (+ the skip term), ds, dt [B,C]: autograd through affine_relu_fwd (no gradient at a == 0)"""
    dx, ds, dt = vjp(affine_relu_fwd, [x, s.to(x.dtype), t.to(x.dtype)], da)
    if skip is not None:
        Bn, P, C = x.shape
        if not skip_ups:
            H, W = P, 1
        dx = dx + skip_term(skip.to(x.dtype), skip_C, skip_ups, Bn, H, W, C)
    return dx, ds, dt


def warp_coords(theta, H, W):
    """sampling positions (ix, iy) [B, H, W] in source pixels of F.affine_grid + F.grid_sample(align_corners=False)
    for theta [B, 6]: g0 = (2 x + 1) / W - 1, g = theta (g0x, g0y, 1), i = ((g + 1) size - 1) / 2"""
    dt = theta.dtype
    gx0 = ((2 * torch.arange(W, dtype=dt) + 1) / W - 1)[None, None, :]
    gy0 = ((2 * torch.arange(H, dtype=dt) + 1) / H - 1)[None, :, None]
    th = theta.reshape(-1, 6)[:, :, None, None]
    gx = th[:, 0] * gx0 + th[:, 1] * gy0 + th[:, 2]
    gy = th[:, 3] * gx0 + th[:, 4] * gy0 + th[:, 5]
    return ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2


def warp_corners(src, theta):
    """the four corners of every sample: [(value [B,C,H,W] (0 outside the image), weight [B,1,H,W])] in the order
    (y0,x0), (y0,x1), (y1,x0), (y1,x1)"""
    B, C, H, W = src.shape
    ix, iy = warp_coords(theta.to(src.dtype), H, W)
    fx, fy = torch.floor(ix).detach(), torch.floor(iy).detach()
    wx1, wy1 = ix - fx, iy - fy
    x0, y0 = fx.long(), fy.long()
    flat = src.reshape(B, C, H * W)
    out = []
    for dy, wy in ((0, 1 - wy1), (1, wy1)):
        for dx, wx in ((0, 1 - wx1), (1, wx1)):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(B, 1, H * W).expand(B, C, H * W)
            v = torch.gather(flat, 2, idx).reshape(B, C, H, W) * ok[:, None].to(src.dtype)
            out.append((v, (wy * wx)[:, None]))
    return out


def affine_warp(src, theta):
    """bilinear warp with zero padding: dst[b,c,y,x] = sum over the 4 corners of src * weight.  src [B,C,H,W],
    theta [B,6]"""
    return sum(v * w for v, w in warp_corners(src, theta))


def affine_warp_bwd(src, theta, dout):              # -> dsrc [B,C,H,W], dtheta [B,6]
    return vjp(affine_warp, [src, theta.to(src.dtype)], dout)


FIR = (0.25, 0.75, 0.75, 0.25)


def blur4(u):
    """[B, H+2, W+2, C] -> [B, H, W, C]: sum_{j,i} a_j a_i u[Y+j-1, X+i-1], a = [1 3 3 1] / 4; row / column -1 are
    zero (rows 0..H and columns 0..W of the frame hold the transposed conv's result, the last ones are zero)"""
    B, UH, UW, C = u.shape
    H, W = UH - 2, UW - 2
    p = torch.cat([u.new_zeros(B, 1, UW, C), u], dim=1)
    p = torch.cat([p.new_zeros(B, UH + 1, 1, C), p], dim=2)          # p[y + 1, x + 1] = u[y, x]
    out = u.new_zeros(B, H, W, C)
    for j in range(4):
        for i in range(4):
            out = out + (FIR[j] * FIR[i]) * p[:, j:j + H, i:i + W]
    return out


def sg2_blur_fwd(u, d, noise, nw, bias):
    """y = lrelu(blur4(u) * d[b,c] + nw * noise[b,p] + bias[c]) * sqrt2; noise [B, H*W] or None"""
    return styled_act(blur4(u).flatten(1, 2), d.to(u.dtype), None if noise is None else noise.to(u.dtype), nw,
                      bias.to(u.dtype)).view(u.shape[0], u.shape[1] - 2, u.shape[2] - 2, u.shape[3])


def sg2_blur_bwd(g, H, W):
    """du [B, H+2, W+2, C] of sum(blur4(u) * g): the transpose of the FIR, the whole frame"""
    B, C = g.shape[0], g.shape[-1]
    return vjp(blur4, [g.new_zeros(B, H + 2, W + 2, C)], g)


# ---- optimiser ----------------------------------------------------------------------------------------------------
def adam_reference(p0, grads, lr, first_step=1, m0=None, v0=None):
    """torch.optim.Adam (defaults) stepped on the CPU in fp32 from step number `first_step`; returns the parameter
    after every step."""
    p = p0.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr)
    if first_step > 1 or m0 is not None:
        st = opt.state[p]
        st['step'] = torch.tensor(float(first_step - 1))
        st['exp_avg'] = (torch.zeros_like(p0) if m0 is None else m0.clone())
        st['exp_avg_sq'] = (torch.zeros_like(p0) if v0 is None else v0.clone())
    out = []
    for g in grads:
        p.grad = g.clone()
        opt.step()
        out.append(p.detach().clone())
    return out

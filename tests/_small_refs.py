"""Plain float64 references of the small entry points of include/p2l.h (the HBM-bound glue of both generators, the
losses and the optimiser), written from the formulas in the header comments and the reference arithmetic they cite
-- not from the kernels.  Forwards are direct restatements; every backward is autograd through its forward in
float64 (`vjp`).  Everything runs on torch-CPU.  tests/test_small_refs.py checks these functions against
independent formulations, tests/test_small_kernels_gpu.py, tests/test_loss_kernels_gpu.py,
tests/test_glue_kernels_gpu.py, tests/test_pw_kernels_gpu.py (the 1x1 convs: references, per-route fp32
restatements, host packers and the case tables) and tests/test_wino_kernels_gpu.py (the Winograd 3x3 routes: the
same), tests/test_direct_kernels_gpu.py (the direct 3x3 routes, ups 0 / 1: the same) and
tests/test_subpix_kernels_gpu.py (the sub-pixel routes, ups 2 / 3: the same) and tests/test_thin_kernels_gpu.py (the
thin 3-channel routes: the same) hold the kernels to them.  (The
closed-form lpips_tap_bwd and the pool backwards are the exceptions to "autograd through the forward":
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


def _cancellation_case(seed, Bn, P, Cc):
    """x [Bn, P, C], s, t [Bn, C] in fp32.  Channels 0..15 (kind A): in 32 pixels x s + t cancels so that the twice
    rounded fl(fl(x s) + t) is 0 but the once rounded fma(x, s, t) is the product's rounding error, of either sign.
    Channels 16..31 (kind B, magnitudes near 2^-126): x s = (n + 1/2) 2^-149 with n odd and t = -n 2^-149 (and the
    mirror image): fl(x s) is the even neighbour, so the twice rounded sum is 2^-149, and the once rounded one is the
    tie 2^-150 -> 0.  The other pixels of the kind B channels hold +-64 .. 128: a is 0 or about 2^-120 there, a normal
    number -- the bf16 pieces through which the 3x3 formats 1 and 2 are read back do not carry subnormals, so a
    positive a below 2^-126 would read as 0 whatever the prologue decided.  Everything else is ordinary."""
    D64 = torch.float64
    g = torch.Generator().manual_seed(4000 + seed)
    x = torch.randn(Bn, P, Cc, generator=g)
    s = (0.5 + torch.rand(Bn, Cc, generator=g)) * torch.where(torch.rand(Bn, Cc, generator=g) < 0.5, -1.0, 1.0)
    t = 0.3 * torch.randn(Bn, Cc, generator=g)
    special = torch.zeros(Bn, P, Cc, dtype=torch.int8)
    for b in range(Bn):
        for c in range(32):
            pix = torch.randperm(P, generator=g)[:32]
            if c < 16:
                xv = float(torch.randn(1, generator=g)) + 2.0
                prod = torch.tensor(xv, dtype=torch.float32) * s[b, c]            # fl(x s)
                x[b, pix, c], t[b, c] = xv, -prod
                special[b, pix, c] = 1
            else:
                n = 2 * int(torch.randint(2 ** 21, 2 ** 22, (1,), generator=g)) + 1                # odd, < 2^23
                sign = 1.0 if c % 2 == 0 else -1.0
                x[b, :, c] = (64.0 + 64.0 * torch.rand(P, generator=g)) * torch.where(torch.rand(P, generator=g) < 0.5, -1.0, 1.0)
                x[b, pix, c], s[b, c], t[b, c] = sign * (2 * n + 1) * 2.0 ** -24, 2.0 ** -126, -sign * n * 2.0 ** -149
                special[b, pix, c] = 2
    # both models of the decision on the host: fp64 holds the product exactly, and the sum wherever it cancels
    once = (x.to(D64) * s.to(D64)[:, None] + t.to(D64)[:, None]).float()         # fma: ONE rounding
    twice = x * s[:, None] + t[:, None]                                          # fp32 product, fp32 sum
    A, B = special == 1, special == 2
    assert int(A.sum()) >= 256 and int(B.sum()) >= 256
    assert bool((twice[A] == 0).all()) and bool((once[A] != 0).all())
    assert bool((once[A] > 0).any()) and bool((once[A] < 0).any())
    assert bool((once[B] == 0).all()) and bool((twice[B] != 0).all())
    assert bool((twice[B] > 0).any()) and bool((twice[B] < 0).any())
    assert bool(((once <= 0) | (once >= 2.0 ** -126)).all())                      # every positive a is a normal number
    return x, s, t, once > 0, twice > 0, A, B


# ---- 1x1 convs (tests/test_pw_kernels_gpu.py) ----------------------------------------------------------------------
# Activations are dense NHWC views [B, H, W, C] (the caller slices the pitch off), a weight is the [N, K] matrix the
# launch applies (the forward conv's [O, I]; its transpose for the input gradient), prologue / arb vectors are
# [1 or B, C].  Enumerations are those of include/p2l.h.
ACT_NONE, ACT_RELU, ACT_TANH, ACT_LRELU_SQRT2 = 0, 1, 2, 3
POOL_NONE, POOL_MAX, POOL_SUM = 0, 1, 2
PRO_NONE, PRO_AFFINE_RELU, PRO_AFFINE = 0, 1, 2


def fma(x, s, t):
    """x s + t with ONE rounding in the dtype of x (fp32: through fp64, which holds the product exactly)"""
    if x.dtype == torch.float32:
        return (x.double() * s.double() + t.double()).float()
    return x * s.to(x.dtype) + t.to(x.dtype)


def pw_prologue(x, pro, s, t):
    """-> a, and the same expression on absolute values (no ReLU)"""
    if pro == PRO_NONE:
        return x, x.abs()
    s_, t_ = s.to(x.dtype)[:, None, None, :], t.to(x.dtype)[:, None, None, :]
    a = fma(x, s_, t_)
    return (torch.relu(a) if pro == PRO_AFFINE_RELU else a), x.abs() * s_.abs() + t_.abs()


def quads(v):
    """[B, H, W, C] -> the four pixels of every 2x2 quad, [B, H/2, W/2, C] each, in the order (0,0) (0,1) (1,0) (1,1)"""
    return v[:, 0::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 0::2], v[:, 1::2, 1::2]


def quad_sum(v):
    v0, v1, v2, v3 = quads(v)
    return (v0 + v1) + (v2 + v3)


def up2(r):                                         # nearest x 2 of [B, h, w, C]
    return r.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def conv1x1(x, w, pro=PRO_NONE, s=None, t=None, alpha=1.0, oscale=None, noise=None, noise_w=0.0, bias=None,
            res=None, res_ups=False, act=ACT_NONE, mask=None, n_store=None, pool=POOL_NONE, acc=None, floor=None):
    """the 1x1 conv launch of include/p2l.h in the dtype of x, in the header's order:
        a = prologue(x) ; v = alpha sum_k a w ; v = v oscale[b][n] + bias[n] + noise_w noise[b][pixel] + res ; act ;
        mask ; channels < n_store ; 2x2 max / sum pool of what was stored.
    oscale [B, N], noise [B, H, W], res [B, H, W, >= n_store] (res_ups: [B, H/2, W/2, ..]), mask like y.
    `acc` replaces sum_k a w (a restatement's accumulator: every route feeds the same epilogue); `floor` [B, H, W, N]
    is added to sum_k |a| |w| (h2_floor: the absolute term of the fp16 x 2 contract).
    -> dict: y, den (sum |terms|: every operand's absolute value, activation and mask left out), yp, denp (pool sum:
    the quad's sum; max: the quad's maximum), a, aabs"""
    dt = x.dtype
    w = w.to(dt)
    Cout = w.shape[0]
    n_store = Cout if n_store is None else n_store
    a, aabs = pw_prologue(x, pro, s, t)
    v = (a @ w.t() if acc is None else acc.to(dt)) * alpha
    den = aabs @ w.abs().t()
    den = (den if floor is None else den + floor.to(dt)) * abs(alpha)
    out = conv_epilogue(v, den, oscale, noise, noise_w, bias, res, res_ups, act, mask, n_store, pool)
    out.update(a=a, aabs=aabs)
    return out


def conv_epilogue(v, den, oscale=None, noise=None, noise_w=0.0, bias=None, res=None, res_ups=False, act=ACT_NONE,
                  mask=None, n_store=None, pool=POOL_NONE):
    """the epilogue half of every conv launch (the shared epilogue item of csrc/p2l_conv_k.h), in the dtype of v: v =
    alpha-scaled accumulator [B, H, W, N], den the same expression on absolute values.
    -> dict: y, den, yp, denp"""
    dt = v.dtype
    n_store = v.shape[-1] if n_store is None else n_store
    if oscale is not None:
        v = v * oscale.to(dt)[:, None, None, :]
        den = den * oscale.to(dt).abs()[:, None, None, :]
    if bias is not None:
        v = v + bias.to(dt)
        den = den + bias.to(dt).abs()
    if noise is not None:
        v = v + noise_w * noise.to(dt)[..., None]
        den = den + abs(noise_w) * noise.to(dt).abs()[..., None]
    v, den = v[..., :n_store], den[..., :n_store]
    if res is not None:
        r = res.to(dt)[..., :n_store]
        r = up2(r) if res_ups else r
        v = v + r
        den = den + r.abs()
    if act == ACT_RELU:
        v = torch.relu(v)
    elif act == ACT_TANH:
        v = torch.tanh(v)
    elif act == ACT_LRELU_SQRT2:
        v = torch.where(v > 0, v * SQRT2, v * (SLOPE * SQRT2)) if dt == torch.float64 else \
            v * torch.where(v > 0, torch.tensor(1.41421356237, dtype=dt), torch.tensor(0.2 * 1.41421356237).to(dt))
    if mask is not None:
        v = torch.where(mask.to(dt)[..., :n_store] > 0, v, torch.zeros_like(v))
    out = dict(y=v, den=den, yp=None, denp=None)
    if pool == POOL_MAX:
        v0, v1, v2, v3 = quads(v)
        d0, d1, d2, d3 = quads(den)
        out['yp'] = torch.maximum(torch.maximum(v0, v1), torch.maximum(v2, v3))
        out['denp'] = torch.maximum(torch.maximum(d0, d1), torch.maximum(d2, d3))
    elif pool == POOL_SUM:
        out['yp'], out['denp'] = quad_sum(v), quad_sum(den)
    return out


def conv1x1_arb(dy, w, x, s, t, alpha=1.0, pool_sum=False, nomask=False, skip=None, skip_C=0, skip_ups=False,
                acc=None, floor=None):
    """the input-gradient launch fused with the backward of a = max(x s + t, 0) (p2l_conv_dgrad_arb), in the dtype of
    dy: da = alpha conv(dy, w) [2x2-summed when pool_sum], g = fma(x, s, t) > 0 ? da : 0 (nomask: g = da),
    dx = g s + shortcut (channels < skip_C; skip_ups: the sum of the four children of a [B, 2H, 2W, ..] gradient),
    ds = sum g x, dt = sum g over the pixels.  x is at the resolution of dx.
    -> dict: dx, den_dx, ds, den_ds (sum |g x|), dt, den_dt (sum |g|), g, den_g (sum |terms| of da)"""
    dtp = dy.dtype
    w = w.to(dtp)
    da = (dy @ w.t() if acc is None else acc.to(dtp)) * alpha
    dend = dy.abs() @ w.abs().t()
    dend = (dend if floor is None else dend + floor.to(dtp)) * abs(alpha)         # (h2_floor, as in conv1x1)
    return arb_epilogue(da, dend, x, s, t, pool_sum, nomask, skip, skip_C, skip_ups)


def arb_epilogue(da, dend, x, s, t, pool_sum=False, nomask=False, skip=None, skip_C=0, skip_ups=False):
    """the half of the fused input gradient behind da = alpha conv(dy, w) (dend: the same on absolute values), shared
    by the 1x1 and the 3x3 launches -> conv1x1_arb's dict"""
    dtp = da.dtype
    if pool_sum:
        da, dend = quad_sum(da), quad_sum(dend)
    x, s_, t_ = x.to(dtp), s.to(dtp)[:, None, None, :], t.to(dtp)[:, None, None, :]
    g = da if nomask else torch.where(fma(x, s_, t_) > 0, da, torch.zeros_like(da))
    dx, den = g * s_, dend * s_.abs()
    if skip is not None and skip_C > 0:
        sk = skip.to(dtp)[..., :skip_C]
        ska = sk.abs()
        if skip_ups:
            sk, ska = quad_sum(sk), quad_sum(ska)
        dx, den = dx.clone(), den.clone()
        dx[..., :skip_C] += sk
        den[..., :skip_C] += ska
    gx = g * x
    return dict(dx=dx, den_dx=den, ds=gx.sum(dim=(1, 2)), den_ds=gx.abs().sum(dim=(1, 2)), dt=g.sum(dim=(1, 2)),
                den_dt=g.abs().sum(dim=(1, 2)), g=g, den_g=dend)


def arb_finish_order32(part):
    """partial [Bn, nblk, C] (one half) -> [Bn, C] in the order csrc/p2l_ops.hip documents for p2l_arb_finish, in
    fp32: segment seg adds its rows seg, seg + 16, ... in four chains (row index / 16 mod 4), combined
    ((0 + 1) + (2 + 3)); then the 16 segments in sequence"""
    Bn, nblk, Cc = part.shape
    segs = []
    for seg in range(16):
        ch = [torch.zeros(Bn, Cc) for _ in range(4)]
        for j in range(seg, nblk, 16):
            q = (j // 16) % 4
            ch[q] = ch[q] + part[:, j]
        segs.append((ch[0] + ch[1]) + (ch[2] + ch[3]))
    out = segs[0]
    for k in range(1, 16):
        out = out + segs[k]
    return out


def npow2(v):
    p = 1
    while p < v:
        p *= 2
    return p


def arb_sums32(g, x, H, W, pool_sum, split):
    """ds, dt of fp32 g, x [B, Ho, Wo, C] (at the resolution of dx) for a launch on the H x W grid, the two stages
    in the kernels' order.  Stage one, per 2x2 quad of the grid: its pixels (one under pool_sum) onto the item's
    running sum in sequence, `sgx += g x` as a fused multiply-add, `sg += g`.  A split-K launch leaves one partial per
    quad, row-major (either finish kernel).  An unsplit one leaves one per 128-pixel tile (choose_tile: TW =
    min(16, W), TH = 128 / TW, one image per tile): the tile's quads row-major, eight per wave, meet in the tree
    q ^ 1, q ^ 2, q ^ 4 and the four waves as (0 + 1) + (2 + 3) (epi_arb_reduce); tiles row-major.  Stage two:
    p2l_arb_finish over the partials (arb_finish_order32)."""
    def quad_partials(prod):
        if pool_sum:
            return prod(g, x, None)
        acc = None
        for gq, xq in zip(quads(g), quads(x)):
            acc = prod(gq, xq, acc)
        return acc

    def stage(prod):
        q = quad_partials(prod)                                           # [B, H/2, W/2, C]
        Bn, Hq, Wq, Cc = q.shape
        assert (Hq, Wq) == (H // 2, W // 2)
        if split:
            return arb_finish_order32(q.reshape(Bn, Hq * Wq, Cc))
        TW = min(npow2(W), 16)
        TH = min(128 // TW, npow2(H))
        twh, thh = TW // 2, TH // 2
        assert twh * thh == 32 and Hq % thh == 0 and Wq % twh == 0, 'one image per whole 128-pixel tile'
        t = q.reshape(Bn, Hq // thh, thh, Wq // twh, twh, Cc).permute(0, 1, 3, 2, 4, 5)
        t = t.reshape(Bn, -1, 4, 8, Cc)                                   # [B, tile, wave, quad of the wave, C]
        w = ((t[:, :, :, 0] + t[:, :, :, 1]) + (t[:, :, :, 2] + t[:, :, :, 3])) + \
            ((t[:, :, :, 4] + t[:, :, :, 5]) + (t[:, :, :, 6] + t[:, :, :, 7]))
        return arb_finish_order32((w[:, :, 0] + w[:, :, 1]) + (w[:, :, 2] + w[:, :, 3]))
    return (stage(lambda gq, xq, acc: gq * xq if acc is None else fma(gq, xq, acc)),
            stage(lambda gq, xq, acc: gq if acc is None else acc + gq))


# -- restatements of each route's accumulator, fp32 on the CPU (a [B, H, W, K] after the prologue, w [N, K]) --------
def cdiv(a, b):
    return -(-a // b)


def splitk_slices(K, kc, splitk):
    """[(k_lo, k_hi)] of the K slices a request of `splitk` resolves to (conv_launch_impl: clamped to the chunk
    count, then to whole chunks per slice)"""
    nch = K // kc
    sk = max(1, min(splitk, nch))
    per = cdiv(nch, sk)
    return [(z * per * kc, min(K, (z + 1) * per * kc)) for z in range(cdiv(nch, per))]


def combine_slices(parts):
    """the finish kernels' order: lane z sums slices z, z + 4, ...; then (z0 + z1) + (z2 + z3)"""
    if len(parts) == 1:
        return parts[0]
    z = [torch.zeros_like(parts[0]) for _ in range(4)]
    for i, p in enumerate(parts):
        z[i % 4] = z[i % 4] + p
    return (z[0] + z[1]) + (z[2] + z[3])


def acc_fp32(a, w, splitk=1, kc=None):
    """route A (conv_mfma_kernel<1, ..>, exact fp32 products): one chain per output over k, per K slice; kc: the
    columns of one chunk (default: the 1x1 kernel's 32 / 16 channels; the 3x3 kernels' im2col: 9 x 16)"""
    K = a.shape[-1]
    kc = kc or (32 if K % 32 == 0 else 16)
    wt = w.t().contiguous()
    parts = []
    for lo, hi in splitk_slices(K, kc, splitk):
        acc = torch.zeros(a.shape[:-1] + (w.shape[0],), dtype=a.dtype)
        for k in range(lo, hi):
            acc = acc + a[..., k:k + 1] * wt[k]
        parts.append(acc)
    return combine_slices(parts)


def split3(x):
    """x = h + m + l, three round-to-nearest bf16 pieces (split3 / store_bf3), as fp32 tensors"""
    h = x.bfloat16().float()
    r1 = x - h
    m = r1.bfloat16().float()
    return h, m, (r1 - m).bfloat16().float()


def acc_bf3(a, w, splitk=1, kc=None):
    """route B (pw_bf3_kernel): per 16-channel step the six kept cross terms (a piece, w piece) in the kernel's
    order (3,1) (1,3) (2,2) (2,1) (1,2) (1,1), each an fp32 sum of 16 exact products onto the accumulator; in K
    slices of whole chunks of kc columns where the launch is sliced (the direct 3x3 kernel: kc = 9 x 16)"""
    a1, a2, a3 = split3(a)
    w1, w2, w3 = split3(w)
    K = a.shape[-1]
    parts = []
    for lo, hi in splitk_slices(K, kc or K, splitk):
        acc = torch.zeros(a.shape[:-1] + (w.shape[0],), dtype=a.dtype)
        for c in range(lo, hi, 16):
            sl = slice(c, c + 16)
            for p, q in ((a3, w1), (a1, w3), (a2, w2), (a2, w1), (a1, w2), (a1, w1)):
                acc = acc + p[..., sl] @ q[:, sl].t()
        parts.append(acc)
    return combine_slices(parts)


def h2_scales(mx):
    """(scale, inv) = 2^(139 - E), 2^(E - 139), E the biased exponent of the fp32 maxima `mx` clamped to 40 .. 254:
    a maximum with such an exponent lands in [2^12, 2^13)"""
    E = ((mx.float().contiguous().view(torch.int32) >> 23) & 0xff).clamp(40, 254).double()
    return (2.0 ** (139 - E)).float(), (2.0 ** (E - 139)).float()


def split2(x):
    """x = h + m, two round-to-nearest fp16 pieces, as fp32 tensors"""
    h = x.half().float()
    return h, (x - h).half().float()


def acc_h2(a, w, amax, wmax, splitk=1, kc=32):
    """routes C and D (pw_h2_kernel): operands scaled by the power of two of h2_scales (activations per image from
    amax [B], weights from wmax), two fp16 pieces each, per 16-channel step the three kept terms (m h) (h m) (h h);
    32-channel stages (kc; the direct 3x3 kernels: chunks of 9 x 16 im2col columns) in K slices; un-scaled exactly"""
    xs, xinv = h2_scales(amax)
    ws, winv = h2_scales(wmax.reshape(1))
    ah, am = split2(a * xs.view(-1, 1, 1, 1))
    wh, wm = split2(w * ws)
    parts = []
    for lo, hi in splitk_slices(a.shape[-1], kc, splitk):
        acc = torch.zeros(a.shape[:-1] + (w.shape[0],), dtype=a.dtype)
        for c in range(lo, hi, 16):
            sl = slice(c, c + 16)
            for p, q in ((am, wh), (ah, wm), (ah, wh)):
                acc = acc + p[..., sl] @ q[:, sl].t()
        parts.append(acc * (xinv * winv).view(-1, 1, 1, 1))
    return combine_slices(parts)


def h2_floor(aabs, w, amax, wmax):
    """what the fp16 x 2 contract adds to sum_k |a| |w|: 2^-13 (amax_b sum_k |w_nk| + wmax sum_k |a_pk|) -- in units
    of 2^-24 that is 2^-37 of the image's maximum per term, the absolute precision the header promises for elements
    more than 2^15 below it.  fp64, [B, H, W, N]"""
    return 2.0 ** -13 * (amax.double().view(-1, 1, 1, 1) * w.double().abs().sum(1) +
                         float(wmax) * aabs.double().sum(-1, keepdim=True))


# -- host packers, from the header's description of P2L_WFMT_PW (bit for bit what the device packers write) -----------
def _padded(w, N_pad, K_pad):
    o = torch.zeros(N_pad, K_pad, dtype=torch.float32)
    o[:w.shape[0], :w.shape[1]] = w
    return o


def pack_f32(w, N_pad, K_pad):
    """[K_pad / KC][N_pad][KC] floats, KC = 32 when K_pad % 32 == 0 and 16 otherwise"""
    kc = 32 if K_pad % 32 == 0 else 16
    return _padded(w, N_pad, K_pad).view(N_pad, K_pad // kc, kc).permute(1, 0, 2).contiguous().flatten()


def _rows16(p, N_pad, K_pad):
    """[N_pad, K_pad] -> [K_pad / 16, N_pad / 32, 32 rows, 2 halves, 8]"""
    return p.view(N_pad // 32, 32, K_pad // 16, 2, 8).permute(2, 0, 1, 3, 4)


def pack_bf3(w, N_pad, K_pad):
    """the bf16 x 3 image as int32 words: [K_pad / 16][N_pad / 32][32 rows][96 B], a row = [x1 k0-7 | x1 k8-15 | x2 ..
    | x3 ..], the 16-byte chunk index XOR-ed with bit 3 of the row"""
    out = torch.zeros(K_pad // 16, N_pad // 32, 32, 6, 8, dtype=torch.bfloat16)
    row = torch.arange(32)
    for i, piece in enumerate(split3(_padded(w, N_pad, K_pad))):
        src = _rows16(piece.bfloat16(), N_pad, K_pad)
        for half in (0, 1):
            for bit in (0, 1):
                rows = row[((row >> 3) & 1) == bit]
                out[:, :, rows, (2 * i + half) ^ bit] = src[:, :, rows, half]
    return out.view(torch.int16).flatten().view(torch.int32)


def pack_h2(w, N_pad, K_pad):
    """the fp16 x 2 image as int32 words: [K_pad / 16][N_pad / 32][32 rows][64 B], a row = [h k0-7 | h k8-15 | m k0-7
    | m k8-15] of the weight times the layer's power of two, the chunk index XOR-ed with bits 2-3 of the row; then
    four tail words, the first the bits of max |w|"""
    wmax = w.abs().max().reshape(1) if w.numel() else torch.zeros(1)
    scale, _ = h2_scales(wmax)
    out = torch.zeros(K_pad // 16, N_pad // 32, 32, 4, 8, dtype=torch.float16)
    row = torch.arange(32)
    for i, piece in enumerate(split2(_padded(w, N_pad, K_pad) * scale)):
        src = _rows16(piece.half(), N_pad, K_pad)
        for half in (0, 1):
            for bits in range(4):
                rows = row[((row >> 2) & 3) == bits]
                out[:, :, rows, (2 * i + half) ^ bits] = src[:, :, rows, half]
    tail = torch.zeros(4, dtype=torch.int32)
    tail[0] = wmax.float().view(torch.int32)[0]
    return torch.cat([out.view(torch.int16).flatten().view(torch.int32), tail])


def pack_pw(w, N_pad, K_pad):
    """a P2L_WFMT_PW buffer as int32 words: fp32 layout | bf16 x 3 image | fp16 x 2 image | tail"""
    return torch.cat([pack_f32(w, N_pad, K_pad).view(torch.int32), pack_bf3(w, N_pad, K_pad), pack_h2(w, N_pad, K_pad)])


# -- the cases of tests/test_pw_kernels_gpu.py: shared with tests/test_small_refs.py, which holds every case's inputs
#    to "the restatement's own figure is at most k / 4" on the host ---------------------------------------------------
def _pwc(route, HW, B, Cin, Cout, **kw):
    c = dict(route=route, H=HW[0], W=HW[1], B=B, Cin=Cin, Cout=Cout, pro=PRO_NONE, pro_b=1, alpha=1.0, bias=False,
             res=None, mask=False, act=ACT_NONE, pool=POOL_NONE, want_y=True, oscale=False, noise=False,
             n_store=Cout, splitk=1, wfmt=0 if route == 'A' else 3, form=0, ws=route == 'D', amax=None, finish='v4')
    assert not set(kw) - set(c), kw
    c.update(kw)
    return c


def pw_id(c):
    d = _pwc(c['route'], (c['H'], c['W']), c['B'], c['Cin'], c['Cout'])
    return '%s-%dx%dx%d-%dto%d' % (c['route'], c['B'], c['H'], c['W'], c['Cin'], c['Cout']) + ''.join(
        '-%s%s' % (k, c[k]) for k in sorted(c) if c[k] != d[k])


EPI = [dict(bias=True, alpha=0.5, res='same'), dict(res='ups', pro=PRO_AFFINE_RELU), dict(mask=True, pro=PRO_AFFINE),
       dict(act=ACT_RELU, pool=POOL_MAX), dict(pool=POOL_SUM, want_y=False, pro=PRO_AFFINE, pro_b=0),
       dict(act=ACT_TANH), dict(act=ACT_LRELU_SQRT2, oscale=True, noise=True, bias=True)]
FORM_NO_PW, FORM_WINO_BF3 = 8, 32
PW_FWD_CASES = [
    # route A: TB = 8 with the last tile partly empty; TB = 2 and KC = 16; one image per tile; partial tiles; the
    # 32-channel tiles choose_bn picks on a full grid; P2L_WFMT_PW buffers on the exact-fp32 kernel
    _pwc('A', (4, 4), 9, 32, 32, **EPI[0]),
    _pwc('A', (8, 8), 3, 48, 64, **EPI[1]),
    _pwc('A', (8, 16), 1, 96, 96, **EPI[2]),
    _pwc('A', (16, 16), 3, 160, 64, **EPI[3]),
    _pwc('A', (16, 16), 1, 48, 32, **EPI[4]),
    _pwc('A', (12, 20), 1, 32, 32, **EPI[5]),
    _pwc('A', (6, 10), 3, 96, 96, n_store=68, pro=PRO_AFFINE_RELU, pro_b=0),
    _pwc('A', (64, 64), 9, 64, 64),
    _pwc('A', (16, 16), 3, 96, 64, wfmt=3, form=FORM_NO_PW, **EPI[6]),
    _pwc('A', (8, 8), 3, 64, 96, wfmt=3, bias=True),                         # Cout % 64 != 0
    _pwc('A', (12, 20), 3, 64, 64, wfmt=3, bias=True),                       # a partial grid
    _pwc('A', (8, 8), 3, 64, 64, wfmt=3, bias=True),                         # a small grid without workspace
    _pwc('A', (32, 32), 1, 64, 64, wfmt=3, form=FORM_NO_PW, act=ACT_RELU),
    # route A in K slices: 5 chunks; the requests 3 and 8 resolve to 3 and 5 slices, 2 to slices of 3 and 2 chunks
    _pwc('A', (8, 8), 3, 160, 64, splitk=2, ws=True, **EPI[0]),
    _pwc('A', (16, 16), 3, 160, 64, splitk=3, ws=True, **EPI[3]),
    _pwc('A', (8, 8), 9, 160, 32, splitk=8, ws=True, **EPI[2]),
    _pwc('A', (16, 16), 1, 160, 64, splitk=8, ws=True, **EPI[6]),
    _pwc('A', (8, 8), 3, 160, 64, splitk=3, ws=True, finish='scalar', **EPI[0]),
    _pwc('A', (16, 16), 3, 160, 64, splitk=2, ws=True, finish='scalar', **EPI[3]),
    _pwc('A', (8, 8), 3, 160, 64, splitk=8, ws=True, finish='scalar', res='ups', mask=True, act=ACT_TANH, n_store=36),
    # route B
    _pwc('B', (32, 32), 1, 64, 64, **EPI[0]),
    _pwc('B', (8, 128), 3, 192, 128, **EPI[1]),
    _pwc('B', (64, 16), 1, 64, 128, **EPI[2]),
    _pwc('B', (24, 48), 3, 192, 64, **EPI[3]),
    _pwc('B', (32, 32), 3, 64, 64, **EPI[4]),
    _pwc('B', (32, 32), 3, 64, 128, n_store=100, **EPI[5]),
    _pwc('B', (32, 32), 1, 192, 64, **EPI[6]),
    _pwc('B', (64, 16), 3, 64, 64, pro=PRO_AFFINE_RELU, pro_b=0),
    _pwc('B', (32, 32), 3, 64, 64, form=FORM_WINO_BF3, amax='true', bias=True),   # handed maxima, still bf16 x 3
    # route C: true maxima without a prologue, raw maxima under a prologue, in_applied maxima
    _pwc('C', (32, 32), 3, 64, 64, amax='true', **EPI[0]),
    _pwc('C', (8, 128), 3, 192, 128, amax='raw', **EPI[1]),
    _pwc('C', (24, 48), 3, 192, 64, amax='applied', **EPI[2]),
    _pwc('C', (64, 16), 1, 64, 128, amax='true', **EPI[3]),
    _pwc('C', (32, 32), 3, 64, 64, amax='raw', **EPI[4]),
    _pwc('C', (32, 32), 3, 64, 128, amax='true', n_store=100, **EPI[5]),      # (its all-zero image: exactly 0)
    _pwc('C', (32, 32), 3, 192, 64, amax='true', **EPI[6]),
    _pwc('C', (64, 16), 3, 64, 64, amax='raw', pro=PRO_AFFINE_RELU, pro_b=0),
    # route D: one, three and five 32-channel stages, in 1 .. 5 slices; maxima from the pass in front / handed over
    _pwc('D', (4, 4), 9, 32, 64, **EPI[0]),
    _pwc('D', (8, 8), 5, 96, 128, splitk=3, amax='raw', **EPI[1]),
    _pwc('D', (8, 16), 3, 160, 64, splitk=2, **EPI[2]),
    _pwc('D', (16, 16), 1, 160, 128, splitk=8, amax='true', **EPI[3]),
    _pwc('D', (16, 16), 3, 96, 64, **EPI[4]),
    _pwc('D', (8, 8), 3, 32, 64, n_store=36, **EPI[5]),
    _pwc('D', (8, 8), 3, 160, 64, **EPI[6]),
    _pwc('D', (8, 8), 3, 160, 64, splitk=3, **EPI[6]),
    _pwc('D', (16, 16), 5, 96, 64, splitk=3, amax='applied', pro=PRO_AFFINE_RELU, bias=True),
    _pwc('D', (8, 8), 3, 160, 64, splitk=8, finish='scalar', **EPI[0]),
    _pwc('D', (8, 8), 3, 96, 64, pro=PRO_AFFINE_RELU, pro_b=0),
]


def _arbc(route, HW, B, Cin, Cout, **kw):
    c = dict(route=route, H=HW[0], W=HW[1], B=B, Cin=Cin, Cout=Cout, splitk=1, skip=None, pool_sum=False,
             nomask=False, wfmt=0 if route == 'A' else 3, ws=route == 'D', amax='true' if route == 'C' else None,
             pro=PRO_NONE, alpha=1.0)
    assert not set(kw) - set(c), kw
    c.update(kw)
    return c


def arb_id(c):
    d = _arbc(c['route'], (c['H'], c['W']), c['B'], c['Cin'], c['Cout'])
    return '%s-%dx%dx%d-%dto%d' % (c['route'], c['B'], c['H'], c['W'], c['Cin'], c['Cout']) + ''.join(
        '-%s%s' % (k, c[k]) for k in sorted(c) if c[k] != d[k])


ARB_VARIANTS = [dict(), dict(skip='same'), dict(skip='ups'), dict(pool_sum=True, skip='same'), dict(nomask=True)]
PW_ARB_CASES = [_arbc(*base, **dict(kw, **v)) for base, kw in [
    (('A', (8, 16), 1, 96, 64), {}), (('A', (16, 16), 3, 48, 96), {}), (('A', (8, 8), 3, 160, 64), dict(splitk=3, ws=True)),
    (('B', (32, 32), 3, 64, 64), {}), (('C', (32, 32), 3, 192, 64), {}), (('D', (16, 16), 3, 96, 64), {}),
    (('D', (8, 8), 3, 160, 128), dict(splitk=3))] for v in ARB_VARIANTS]


def arb_inputs(g, c):
    """dy [B, H, W, Cin], w [Cout, Cin] (the matrix the launch applies), x, s, t of the consumer at the resolution of
    dx ([B, H/2, W/2, Cout] under pool_sum), the shortcut gradient with Cout channels (skip_C = Cout / 2)"""
    B, H, W, Cin, Cout = c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    rn = lambda *sh: torch.randn(*sh, generator=g)
    mg = mags(B).view(B, 1, 1, 1)
    Ho, Wo = (H // 2, W // 2) if c['pool_sum'] else (H, W)
    i = dict(x=rn(B, H, W, Cin) * mg, w=rn(Cout, Cin) / math.sqrt(Cin))
    if c['route'] in 'CD':
        i['x'][1] = 0.0
        i['x'][0, 0:2, 0:2] *= 2.0 ** -20
    i['ax'] = rn(B, Ho, Wo, Cout) * mg.flip(0)
    i['as'] = (0.5 + torch.rand(B, Cout, generator=g)) * torch.where(torch.rand(B, Cout, generator=g) < 0.5, -1.0, 1.0)
    i['at'] = 0.3 * rn(B, Cout) * mg.flip(0).view(B, 1)
    if c['skip'] == 'same':
        i['skip'] = rn(B, Ho, Wo, Cout) * mg
    elif c['skip'] == 'ups':
        i['skip'] = rn(B, 2 * Ho, 2 * Wo, Cout) * mg
    return i


def arb_refs(c, i):
    """-> conv1x1_arb's dict in fp64, the fp32 restatement's (its ds, dt in the kernels' two-stage order: arb_sums32)"""
    kw = dict(pool_sum=c['pool_sum'], nomask=c['nomask'], skip=i.get('skip'), skip_C=c['Cout'] // 2 if c['skip'] else 0,
              skip_ups=c['skip'] == 'ups')
    floor = h2_floor(i['x'].double().abs(), i['w'], pw_amax(c, i)[1], i['w'].abs().max()) if c['route'] in 'CD' else None
    r64 = conv1x1_arb(i['x'].double(), i['w'].double(), i['ax'].double(), i['as'].double(), i['at'].double(),
                      floor=floor, **kw)
    r32 = conv1x1_arb(i['x'], i['w'], i['ax'], i['as'], i['at'], acc=pw_acc32(c, i), **kw)
    split = c['route'] in 'AD' and len(splitk_slices(c['Cin'], 32 if c['Cin'] % 32 == 0 else 16, c['splitk'])) > 1
    r32['ds'], r32['dt'] = arb_sums32(r32['g'], i['ax'], c['H'], c['W'], c['pool_sum'], split)
    return r64, r32


def arb_positive(i):
    """the same case with |dy| and |w|: no term of da cancels, so sum |terms of g| = |g| (fp16 x 2: but for the floor)
    and the denominators sum |g x| and sum |g| carry the conv's own error of g -- the inputs on which ds and dt are
    held to their bar.  (With signed operands a channel with a few live pixels has sum |g| as small as one cancelled
    conv output: its figure measures that cancellation, without bound, and not the reduction; dx, whose denominator
    is sum |terms|, is held on the signed inputs, and ds, dt there to `arb_bound`.)"""
    return dict(i, x=i['x'].abs(), w=i['w'].abs())


def arb_k(c, conv_k=None):
    """-> (k of dx, of ds, of dt); conv_k: the conv's count (default pw_k; the 3x3 cases: wino_k).  dx: the conv's k (pw_k), the 2x2 sum of da (2), g s (1), the shortcut (1; the
    children's tree and the sum: 3).  ds, dt on `arb_positive` inputs: the conv's k on every g (+ 1 for the floor's
    share of sum |terms| on the fp16 x 2 routes), the sums (a quad's chain 4, the tile's tree of quads and waves 5, the
    rows of p2l_arb_finish's chains, their tree 2, the 16 segments 15) and the product g x (1)"""
    kg = (conv_k or pw_k)(dict(c, oscale=False, bias=False, noise=False, res=None, act=ACT_NONE, pool=POOL_NONE)) + \
        (2 if c['pool_sum'] else 0)
    Ho, Wo = (c['H'] // 2, c['W'] // 2) if c['pool_sum'] else (c['H'], c['W'])
    ksum = 4 + 5 + max(1, (Ho // 2) * (Wo // 2) // 64) + 2 + 15
    return kg + 1 + {None: 0, 'same': 1, 'ups': 3}[c['skip']], kg + 1 + 1 + ksum, kg + 1 + ksum


def arb_bound(c, r64, ax, conv_k=None):
    """a-priori bounds of |ds - ref|, |dt - ref| [B, C] in units of 2^-24 for operands of any sign: the conv's k on
    sum |terms of g| of every LIVE pixel (times |x| for ds), the sums' k on sum |g x| / sum |g|"""
    kdx, kds, kdt = arb_k(c, conv_k)
    kg = kdx - 1 - {None: 0, 'same': 1, 'ups': 3}[c['skip']]
    dg = r64['den_g'] * (r64['g'] != 0).double()
    return (kg * (dg * ax.double().abs()).sum(dim=(1, 2)) + (kds - kg) * r64['den_ds'],
            kg * dg.sum(dim=(1, 2)) + (kdt - kg) * r64['den_dt'])


def mags(Bn, lo=-2.0, hi=2.0):
    """one magnitude per image, 1e-2 .. 1e2"""
    return 10.0 ** torch.linspace(lo, hi, Bn) if Bn > 1 else torch.tensor([3.0])


def pw_inputs(g, c):
    """the operands of a forward case on the host, dense fp32: every image at a magnitude of its own; routes C and D:
    image 1 of a batch of three or more all zero and a 2x2 quad of image 0 2^-20 below its maximum; prologue: s in
    0.5 + U(0, 1), t scaled to the image, one heavy channel (|s| x 50) away from the channel of the largest |x|"""
    B, H, W, Cin, Cout = c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    rn = lambda *sh: torch.randn(*sh, generator=g)
    mg = mags(B)
    i = dict(x=rn(B, H, W, Cin) * mg.view(B, 1, 1, 1), w=rn(Cout, Cin) / math.sqrt(Cin))
    if c['route'] in 'CD':
        if B >= 3:
            i['x'][1] = 0.0
        i['x'][0, 0:2, 0:2] *= 2.0 ** -20
    xmax = i['x'].abs().amax(dim=(1, 2, 3))
    out_mag = torch.where(xmax > 0, mg, torch.ones_like(mg)).view(B, 1, 1, 1)
    if c['pro'] != PRO_NONE:
        Bs = B if c['pro_b'] else 1
        s = 0.5 + torch.rand(Bs, Cin, generator=g)
        t = 0.3 * rn(Bs, Cin) * (xmax[:Bs].view(Bs, 1) if c['pro_b'] else xmax[xmax > 0].min())
        for b in range(Bs):
            big = int(i['x'][b].abs().amax(dim=(0, 1)).argmax())
            s[b, (big + Cin // 2) % Cin] *= 50.0
        i['s'], i['t'] = s, t
    if c['bias']:
        i['bias'] = 0.1 * rn(Cout)
    if c['res'] == 'same':
        i['res'] = rn(B, H, W, Cout) * out_mag
    elif c['res'] == 'ups':
        i['res'] = rn(B, H // 2, W // 2, Cout) * out_mag
    if c['mask']:
        i['mask'] = rn(B, H, W, Cout)
    if c['oscale']:
        i['oscale'] = 0.5 + torch.rand(B, Cout, generator=g)
    if c['noise']:
        i['noise'], i['noise_w'] = rn(B, H, W) * out_mag[..., 0], 0.3
    return i


def pw_amax(c, i):
    """-> (what a case hands to P2LAmax.in [B] or None, amax_b [B]: the value the contract says the kernel scales by).
    Pass in front: the true maximum of the prologue's result; handed raw maxima under a prologue:
    (max |s| max |x| + max |t|) 1.001; in_applied: the handed maxima of |x s + t|; no prologue: the handed maxima"""
    B = c['B']
    x = i['x']
    xmax = x.abs().amax(dim=(1, 2, 3))
    if c['pro'] == PRO_NONE:
        return (xmax if c['amax'] else None), xmax
    s, t = i['s'].expand(B, -1), i['t'].expand(B, -1)
    pre = fma(x, s[:, None, None, :], t[:, None, None, :])
    if c['amax'] == 'raw':
        return xmax, (s.abs().amax(1) * xmax + t.abs().amax(1)) * 1.001
    if c['amax'] == 'applied':
        m = pre.abs().amax(dim=(1, 2, 3))
        return m, m * 1.001
    a = torch.relu(pre) if c['pro'] == PRO_AFFINE_RELU else pre
    return (xmax if c['amax'] else None), a.abs().amax(dim=(1, 2, 3))


def pw_kwargs(c, i, dtype):
    """the keyword arguments of conv1x1 for a case, operands in `dtype`"""
    cv = lambda name: i[name].to(dtype) if name in i else None
    return dict(pro=c['pro'], s=cv('s'), t=cv('t'), alpha=c['alpha'], oscale=cv('oscale'), noise=cv('noise'),
                noise_w=i.get('noise_w', 0.0), bias=cv('bias'), res=cv('res'), res_ups=c['res'] == 'ups', act=c['act'],
                mask=cv('mask'), n_store=c['n_store'], pool=c['pool'])


def pw_acc32(c, i, route=None):
    """the fp32 restatement of the accumulator of a case on route `route` (default: its own)"""
    route = route or c['route']
    a, _ = pw_prologue(i['x'], c['pro'], i.get('s'), i.get('t'))
    if route == 'A':
        return acc_fp32(a, i['w'], c['splitk'])
    if route == 'B':
        return acc_bf3(a, i['w'])
    return acc_h2(a, i['w'], pw_amax(c, i)[1], i['w'].abs().max(), c['splitk'] if route == 'D' else 1)


def pw_refs(c, i, route=None):
    """-> fp64 reference (conv1x1's dict, den with the fp16 x 2 floor on routes C and D) and the fp32 restatement's"""
    route = route or c['route']
    i64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in i.items()}
    floor = None
    if route in 'CD':
        _, aabs = pw_prologue(i64['x'], c['pro'], i64.get('s'), i64.get('t'))
        floor = h2_floor(aabs, i['w'], pw_amax(c, i)[1], i['w'].abs().max())
    r64 = conv1x1(i64['x'], i64['w'], floor=floor, **pw_kwargs(c, i, torch.float64))
    r32 = conv1x1(i['x'], i['w'], acc=pw_acc32(c, i, route), **pw_kwargs(c, i, torch.float32))
    return r64, r32


def pw_k(c, route=None, pooled=False):
    """the bar's k of a forward case, counted from the route's arithmetic: per k of the deepest K slice the
    additions onto the accumulator (fp32 MFMA: a product and an addition; bf16 x 3: six cross terms of exact
    products; fp16 x 2: three) and the slices in order; bf16 x 3: the pieces to 2^-24 relative of either operand (2)
    and the dropped terms <= 2^-23 (2); fp16 x 2: the pieces to 2^-22 relative of either operand (8), the dropped
    term (4) and the absolute floor that `h2_floor` puts into the denominator (1); the prologue's fma or product and
    sum (2); alpha, oscale, bias, noise (a product and a sum), residual one each; tanh 2; the leaky ReLU's factor
    sqrt 2 on everything before it and its own rounding; the pool's sum: two additions deep"""
    route = route or c['route']
    K = c['Cin']
    sl = splitk_slices(K, 32 if (route == 'D' or K % 32 == 0) else 16, c['splitk']) if route in 'AD' else [(0, K)]
    deep = max(hi - lo for lo, hi in sl)
    k = {'A': 2, 'B': 6, 'C': 3, 'D': 3}[route] * deep + (len(sl) - 1) + {'A': 0, 'B': 4, 'C': 13, 'D': 13}[route]
    k += (2 if c['pro'] != PRO_NONE else 0) + 1 + c['oscale'] + c['bias'] + 2 * c['noise'] + (c['res'] is not None)
    if c['act'] == ACT_TANH:
        k += 2
    if c['act'] == ACT_LRELU_SQRT2:
        k = 1.5 * k + 1
    return k + 2 if pooled and c['pool'] == POOL_SUM else k


# ---- Winograd F(2x2, 3x3) convs (tests/test_wino_kernels_gpu.py) ----------------------------------------------------
# Routes of a taps = 9, ups = 0, P2L_WFMT_BF16X3W launch into csrc/p2l_wino.hip: W8 wino_conv_kernel (8x16-pixel blocks,
# bf16 x 3), W16 wino16s_conv_kernel (16x16, bf16 x 3), H the same kernel in fp16 x 2 (blk 8 / 16: its two block
# shapes), HS its K-sliced small-grid form with conv_splitk_finish4; F is the exact-fp32 direct kernel (P2L_WFMT_F32),
# every case's twin.  A weight is the [N, K, 3, 3] correlation kernel the launch applies.  Frequencies are numbered
# 4 i + j, i the row of B^T d / G g and j the column, as in the packed image.
WFMT_BF16X3W = 2
FORM_WINO_ANY, FORM_WINO_8X16, FORM_WINO_H2_8X16, FORM_WINO_H2_16X16 = 2, 4, 64, 128
WINO_G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)


def wino_U(w):
    """G g G^T in fp64: [N, K, 3, 3] -> [16, N, K]"""
    u = torch.einsum('ia,nkab,jb->ijnk', WINO_G, w.double(), WINO_G)
    return u.reshape(16, w.shape[0], w.shape[1])


def _wino_bt(d0, d1, d2, d3, absolute):
    """the four rows of B^T d as p2l_wino.hip:133 writes them out: d0 - d2, d1 + d2, d2 - d1, d1 - d3 (absolute: of
    |B^T| |d|)"""
    if absolute:
        return d0 + d2, d1 + d2, d2 + d1, d1 + d3
    return d0 - d2, d1 + d2, d2 - d1, d1 - d3


def wino_V(a, absolute=False):
    """B^T d B of every 4x4 patch of the zero-padded a [B, H, W, K], in the dtype of a and in the kernels' two stages:
    the rows (one addition of two patch rows each), then the same combination of the columns -> [16, B, H/2, W/2, K]"""
    B, H, W, K = a.shape
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    Hq, Wq = H // 2, W // 2
    out = []
    for r in _wino_bt(*[ap[:, i:i + 2 * Hq:2] for i in range(4)], absolute):
        out.extend(_wino_bt(*[r[:, :, j:j + 2 * Wq:2] for j in range(4)], absolute))
    return torch.stack(out)


def wino_out(M, absolute=False):
    """A^T M A in the kernels' order: T0 = (m0 + m1) + m2, T1 = (m1 - m2) - m3 down the rows, then the same along the
    columns.  M [16, B, H/2, W/2, N] -> [B, H, W, N]"""
    def at(m0, m1, m2, m3):
        if absolute:
            return (m0 + m1) + m2, (m1 + m2) + m3
        return (m0 + m1) + m2, (m1 - m2) - m3
    T0, T1 = zip(*[at(M[j], M[4 + j], M[8 + j], M[12 + j]) for j in range(4)])
    v00, v01 = at(*T0)
    v10, v11 = at(*T1)
    _, B, Hq, Wq, Nn = M.shape
    y = torch.stack([torch.stack([v00, v01], dim=3), torch.stack([v10, v11], dim=3)], dim=2)    # [B, Hq, 2, Wq, 2, N]
    return y.reshape(B, 2 * Hq, 2 * Wq, Nn)


def wino_acc_bf3(V, U):
    """W8 / W16: V [16, M, K], U [16, N, K] in fp32; per 16-channel chunk and frequency the six kept cross terms
    (activation piece, weight piece) in the order both kernels issue them: (1,1) (1,2) (1,3) (2,1) (2,2) (3,1)"""
    v1, v2, v3 = split3(V)
    u1, u2, u3 = split3(U)
    acc = torch.zeros(16, V.shape[1], U.shape[1])
    for c in range(0, V.shape[2], 16):
        sl = slice(c, c + 16)
        for p, q in ((v1, u1), (v1, u2), (v1, u3), (v2, u1), (v2, u2), (v3, u1)):
            acc = acc + torch.bmm(p[:, :, sl], q[:, :, sl].transpose(1, 2))
    return acc


def wino_acc_h2(V, U, lo, hi):
    """H / HS: the scaled V, U in two fp16 pieces, channels lo .. hi; per chunk and frequency (h h) (h m) (m h)"""
    vh, vm = split2(V)
    uh, um = split2(U)
    acc = torch.zeros(16, V.shape[1], U.shape[1])
    for c in range(lo, hi, 16):
        sl = slice(c, c + 16)
        for p, q in ((vh, uh), (vh, um), (vm, uh)):
            acc = acc + torch.bmm(p[:, :, sl], q[:, :, sl].transpose(1, 2))
    return acc


def wino_acc32(c, i, route=None):
    """the fp32 restatement of a route's result in front of alpha and the epilogue, [B, H, W, N]: U = G g G^T in fp64
    rounded once; the input transform on the prologue's result (H, HS: times the image's power of two -- the scales
    are those of the RAW maxima, h2_scales' range leaves the transform its factor 4 and U its 2.25); the chunks; the
    output transform; H, HS: un-scaled exactly; HS: every slice through the output transform on its own
    (chunks_per_split = chunks / slices), then ((z0 + z1) + (z2 + z3)) as conv_splitk_finish4 adds them"""
    route = route or c['route']
    a, _ = pw_prologue(i['x'], c['pro'], i.get('s'), i.get('t'))
    B, H, W, K = a.shape
    Nn = i['w'].shape[0]
    U = wino_U(i['w']).float()
    shape = (16, B, H // 2, W // 2, Nn)
    if route in ('W8', 'W16'):
        return wino_out(wino_acc_bf3(wino_V(a).reshape(16, -1, K), U).reshape(shape))
    xs, xinv = h2_scales(pw_amax(c, i)[1])
    ws, winv = h2_scales(i['w'].abs().max().reshape(1))
    V, Us = wino_V(a * xs.view(-1, 1, 1, 1)).reshape(16, -1, K), U * ws
    sk = c['splitk'] if route == 'HS' else 1
    per = (K // 16 // sk) * 16
    parts = [wino_out(wino_acc_h2(V, Us, z * per, (z + 1) * per).reshape(shape)) * (xinv * winv).view(-1, 1, 1, 1)
             for z in range(sk)]
    if sk == 1:
        return parts[0]
    parts += [torch.zeros_like(parts[0])] * (4 - sk)
    return (parts[0] + parts[1]) + (parts[2] + parts[3])


def wino_den(aabs, w):
    """den_w = |A^T| (sum_k |U| (.) |B^T| |a| |B|) |A|: sum |terms| of the arithmetic the Winograd kernels perform, in
    the dtype of aabs, [B, H, W, N]"""
    B, H, W, K = aabs.shape
    Ua = wino_U(w).abs().to(aabs.dtype)
    M = torch.bmm(wino_V(aabs, True).reshape(16, -1, K), Ua.transpose(1, 2))
    return wino_out(M.reshape(16, B, H // 2, W // 2, w.shape[0]), True)


def wino_h2_floor(aabs, w, amax, wmax):
    """the absolute term of the fp16 x 2 contract in the transform domain, fp64 [B, H, W, N].  The header: an element
    more than 2^15 below the maximum of its image gets a denormal second piece -- "2^-37 of the maximum in absolute
    terms".  The operands the Winograd kernel splits are V = B^T a B times the image's power of two 2^p and U times
    the layer's 2^q, with amax 2^p and wmax 2^q in [2^12, 2^13) (h2_scales on the maxima the kernel scales by: of the
    raw image, or the bound (max |s| max |x| + max |t|) 1.001, or the handed-over |x s + t| maxima times 1.001; max
    |w| from the weight tail).  h + m misses a scaled value by at most half an fp16 subnormal step, 2^-25, i.e. V by
    2^-25 / 2^p <= 2^-37 amax and U by 2^-37 wmax.  To first order the product of a frequency is then off by at most
    2^-37 (amax |U| + wmax |V|), |V| <= |B^T| |a| |B|: summed over k and taken through |A^T| . |A| like the products
    themselves, in units of 2^-24 that is what this function returns,
        |A^T| ( 2^-13 (amax_b sum_k |U_nk| + wmax sum_k (|B^T| |a| |B|)_k) ) |A|
    -- h2_floor with |B^T| |a| |B| and |U| in place of |a| and |w|"""
    B, H, W, K = aabs.shape
    Ua = wino_U(w).abs()                                                      # [16, N, K]
    Va = wino_V(aabs.double(), True)                                          # [16, B, Hq, Wq, K]
    f = 2.0 ** -13 * (amax.double().view(1, B, 1, 1, 1) * Ua.sum(2).view(16, 1, 1, 1, -1) +
                      float(wmax) * Va.sum(-1, keepdim=True))
    return wino_out(f, True)


def conv3x3(x, w, pro=PRO_NONE, s=None, t=None, alpha=1.0, acc=None, floor=None, ups=False, den_w=True, **epi):
    """the stride-1 3x3 conv launch of include/p2l.h in the dtype of x: a = prologue(x); ups (P2LConv.ups = 1): x
    is the low-resolution [B, H/2, W/2, K] tensor, the prologue runs on it, then nearest x 2 (`up2`); zero padding
    AFTER the prologue (and the upsample); v = alpha sum a w; then conv_epilogue(**epi), the epilogue conv1x1 ends
    in -- res_ups and the pool as before, on the H x W output.  w [N, K, 3, 3].  `acc` replaces the conv (a
    restatement's result), `floor` (wino_h2_floor / direct_h2_floor) is added to both denominators.
    -> conv1x1's dict with den / denp on den_w (wino_den) and den_d / denp_d on the direct sum_taps,k |a| |w|;
    den_w = False (the direct routes): den / denp are den_d / denp_d"""
    dt = x.dtype
    w = w.to(dt)
    a, aabs = pw_prologue(x, pro, s, t)
    if ups:
        a, aabs = up2(a), up2(aabs)
    nchw = lambda v: v.permute(0, 3, 1, 2)
    v = F.conv2d(nchw(a), w, padding=1).permute(0, 2, 3, 1) if acc is None else acc.to(dt)
    den_d = F.conv2d(nchw(aabs), w.abs(), padding=1).permute(0, 2, 3, 1)
    den_w = wino_den(aabs, w) if den_w else den_d
    if floor is not None:
        den_w, den_d = den_w + floor.to(dt), den_d + floor.to(dt)
    out = conv_epilogue(v * alpha, den_w * abs(alpha), **epi)
    direct = conv_epilogue(v * alpha, den_d * abs(alpha), **epi)
    out.update(a=a, aabs=aabs, den_d=direct['den'], denp_d=direct['denp'])
    return out


def conv3x3_arb(dy, w, x, s, t, alpha=1.0, acc=None, floor=None, ups=False, den_w=True, **kw):
    """p2l_conv_dgrad_arb on a 3x3 launch: da = alpha conv3x3(dy, w) (ups: of the nearest x 2 of the low-resolution
    dy, as in conv3x3), then arb_epilogue -> conv1x1_arb's dict on den_w, and den_dx_d on the direct denominator
    (den_w = False, the direct routes: both are the direct one)"""
    dtp = dy.dtype
    w = w.to(dtp)
    dy = up2(dy) if ups else dy
    nchw = lambda v: v.permute(0, 3, 1, 2)
    da = (F.conv2d(nchw(dy), w, padding=1).permute(0, 2, 3, 1) if acc is None else acc.to(dtp)) * alpha
    den_d = F.conv2d(nchw(dy.abs()), w.abs(), padding=1).permute(0, 2, 3, 1)
    den_w = wino_den(dy.abs(), w) if den_w else den_d
    if floor is not None:
        den_w, den_d = den_w + floor.to(dtp), den_d + floor.to(dtp)
    out = arb_epilogue(da, den_w * abs(alpha), x, s, t, **kw)
    out['den_dx_d'] = arb_epilogue(da, den_d * abs(alpha), x, s, t, **kw)['den_dx']
    return out


def _wc(route, HW, B, Cin, Cout, **kw):
    c = dict(route=route, H=HW[0], W=HW[1], B=B, Cin=Cin, Cout=Cout, pro=PRO_NONE, pro_b=1, alpha=1.0, bias=False,
             res=None, mask=False, act=ACT_NONE, pool=POOL_NONE, want_y=True, oscale=False, noise=False,
             n_store=Cout, splitk=1, amax=None, blk=16 if route == 'H' else 0, relu_like=False, own=False)
    assert not set(kw) - set(c), kw
    c.update(kw)
    return c


def wino_id(c):
    d = _wc(c['route'], (c['H'], c['W']), c['B'], c['Cin'], c['Cout'])
    return '%s-%dx%dx%d-%dto%d' % (c['route'], c['B'], c['H'], c['W'], c['Cin'], c['Cout']) + ''.join(
        '-%s%s' % (k, c[k]) for k in sorted(c) if c[k] != d[k])


def wino_form(c, route=None):
    """P2LConv.form of a case: W8 forced (own: left to the dispatch, which takes the 8x16 kernel where H % 16 != 0),
    W16 = the 16x16 kernel kept on bf16 x 3, H with its block shape, HS by the product's own rule (form 0)"""
    route = route or c['route']
    if route == 'W8':
        return FORM_WINO_ANY | (0 if c['own'] else FORM_WINO_8X16)
    if route == 'W16':
        return FORM_WINO_ANY | FORM_WINO_BF3
    blk = {0: 0, 8: FORM_WINO_H2_8X16, 16: FORM_WINO_H2_16X16}[c['blk']]
    return blk if route == 'HS' else FORM_WINO_ANY | blk


# every term of EPI on every route; n_store < Cout rides on the tanh entry, the shared prologue on EPI[4]
WINO_SHAPES = {'8x16': ((8, 16), 1, 16, 64), '16x16': ((16, 16), 2, 16, 64), '24x16': ((24, 16), 2, 32, 64),
               '16x32': ((16, 32), 3, 48, 128), '32x16': ((32, 16), 1, 80, 192), '32x32': ((32, 32), 2, 64, 64),
               'hs2': ((16, 16), 2, 256, 512), 'hs4': ((32, 16), 1, 512, 256)}


def _wsh(route, name, **kw):
    HW, B, Cin, Cout = WINO_SHAPES[name]
    return _wc(route, HW, B, Cin, Cout, **kw)


WINO_FWD_CASES = [
    _wsh('W8', '8x16', **EPI[0]),
    _wsh('W8', '16x16', **EPI[1]),
    _wsh('W8', '24x16', own=True, **EPI[2]),
    _wsh('W8', '16x32', **EPI[3]),
    _wsh('W8', '32x16', relu_like=True, **EPI[4]),
    _wsh('W8', '32x32', n_store=36, **EPI[5]),
    _wsh('W8', '16x16', **EPI[6]),
    _wsh('W16', '16x16', **EPI[2]),
    _wsh('W16', '16x32', **EPI[0]),
    _wsh('W16', '32x16', **EPI[1]),
    _wsh('W16', '32x32', relu_like=True, **EPI[3]),
    _wsh('W16', '16x32', **EPI[4]),
    _wsh('W16', '32x16', n_store=100, **EPI[5]),
    _wsh('W16', '32x32', **EPI[6]),
    # H: the pass in front (amax None), maxima handed over (true / raw under a prologue), in_applied; both blocks
    _wsh('H', '16x16', blk=8, **EPI[3]),
    _wsh('H', '16x32', blk=16, amax='true', **EPI[0]),
    _wsh('H', '32x16', blk=8, amax='raw', **EPI[1]),
    _wsh('H', '32x32', blk=16, amax='applied', **EPI[2]),
    _wsh('H', '16x32', blk=8, **EPI[4]),
    _wsh('H', '16x32', blk=16, amax='true', n_store=100, **EPI[5]),           # (its all-zero image: exactly 0)
    _wsh('H', '32x16', blk=16, relu_like=True, **EPI[6]),
    _wsh('H', '32x32', blk=8, amax='raw', pro=PRO_AFFINE_RELU, pro_b=0),
    _wsh('HS', 'hs2', splitk=2, **EPI[0]),
    _wsh('HS', 'hs2', splitk=2, amax='raw', **EPI[1]),
    _wsh('HS', 'hs4', splitk=4, amax='applied', **EPI[2]),
    _wsh('HS', 'hs4', splitk=4, relu_like=True, **EPI[3]),
    _wsh('HS', 'hs2', splitk=2, blk=16, **EPI[4]),
    _wsh('HS', 'hs4', splitk=4, n_store=100, amax='true', **EPI[5]),
    _wsh('HS', 'hs2', splitk=2, blk=8, **EPI[6]),
]


def wino_inputs(g, c):
    """pw_inputs' operands for a 3x3 case (H, HS: its fp16 x 2 inputs -- the quad 2^-20 below the maximum, the all-zero
    image of a batch of three, the heavy channel under a prologue), w [Cout, Cin, 3, 3]; relu_like: a non-negative
    image; PRO_AFFINE: |t| of 2 .. 5 units of the image, so that padding in front of the prologue is far off"""
    i = pw_inputs(g, dict(c, route='C' if c['route'] in ('H', 'HS') else 'A'))
    i['w'] = torch.randn(c['Cout'], c['Cin'], 3, 3, generator=g) / math.sqrt(9 * c['Cin'])
    if c['relu_like']:
        i['x'] = torch.relu(i['x'])
    if c['pro'] == PRO_AFFINE:
        sign = torch.where(torch.rand(i['t'].shape, generator=g) < 0.5, -1.0, 1.0)
        xmax = i['x'].abs().amax(dim=(1, 2, 3))
        unit = xmax[:i['t'].shape[0]].view(-1, 1) if c['pro_b'] else xmax[xmax > 0].min()
        i['t'] = sign * (2.0 + 3.0 * torch.rand(i['t'].shape, generator=g)) * 0.3 * unit
    return i


def wino_refs(c, i, route=None):
    """-> conv3x3's dict in fp64 (H, HS: both denominators with wino_h2_floor) and the route's fp32 restatement's
    (route F, the exact-fp32 twin: no restatement, None)"""
    route = route or c['route']
    i64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in i.items()}
    floor = None
    if route in ('H', 'HS'):
        _, aabs = pw_prologue(i64['x'], c['pro'], i64.get('s'), i64.get('t'))
        floor = wino_h2_floor(aabs, i['w'], pw_amax(c, i)[1], i['w'].abs().max())
    r64 = conv3x3(i64['x'], i64['w'], floor=floor, **pw_kwargs(c, i, torch.float64))
    if route == 'F':
        return r64, None
    return r64, conv3x3(i['x'], i['w'], acc=wino_acc32(c, i, route), **pw_kwargs(c, i, torch.float32))


def wino_k(c, route=None, pooled=False):
    """the bar's k of a 3x3 case, counted like pw_k.  Winograd routes: the rounding of U (1); the two additions of the
    input transform (2); per k of the deepest slice the additions onto the accumulator (bf16 x 3: six cross terms,
    fp16 x 2: three) and the slices; the pieces and dropped terms with pw_k's constants (bf16 x 3: 2 + 2; fp16 x 2: 8
    + 4 + 1 for the floor in the denominator); the output transform, two additions down the rows and two along the
    columns (4).  Route F, the exact-fp32 direct kernel: a product and an addition per tap and k.  Then pw_k's
    prologue and epilogue terms"""
    route = route or c['route']
    K = c['Cin']
    if route == 'F':
        k = 2 * 9 * K
    else:
        bf3 = route in ('W8', 'W16', 'WS')                 # (WS: the K-sliced launch that was left on bf16 x 3)
        sk = c['splitk'] if route in ('HS', 'WS') else 1
        k = 1 + 2 + (6 if bf3 else 3) * (K // sk) + (sk - 1) + (4 if bf3 else 13) + 4
    k += (2 if c['pro'] != PRO_NONE else 0) + 1 + c['oscale'] + c['bias'] + 2 * c['noise'] + (c['res'] is not None)
    if c['act'] == ACT_TANH:
        k += 2
    if c['act'] == ACT_LRELU_SQRT2:
        k = 1.5 * k + 1
    return k + 2 if pooled and c['pool'] == POOL_SUM else k


def wino_onehot(c, tap, seed=0):
    """exact inputs: x with single power-of-two pixels at the corners, the edges, the seams of the 8x16 / 16x16 blocks
    and the interior, each in a channel of its own chunk; w with single power-of-two entries on tap (a, b) at a few
    (cout, cin).  G g G^T, B^T d B and A^T M A then hold sums of at most four powers of two within a few binades --
    exact in fp32, in three bf16 and in two fp16 pieces"""
    B, H, W, Cin, Cout = c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    x, w = torch.zeros(B, H, W, Cin), torch.zeros(Cout, Cin, 3, 3)
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, W // 2 - 1),
             (7, 15), (8, 15) if H > 8 else (7, 14), (7, W - 1), (H // 2, W // 2), (3, 5), (4, 6)]
    spots += [(15, 15), (16, 16), (15, 16), (16, 15)] if H > 16 and W > 16 else \
        [(7, 16), (8, 16)] if W > 16 else [(15, 7), (16, 8)] if H > 16 else []
    for n, (py, px) in enumerate(spots):
        x[(n + seed) % B, py, px, (5 * (n + seed)) % Cin] = 2.0 ** ((n + seed) % 5 - 2)
    for n in range(10):
        ci = (5 * (n + seed)) % Cin                                          # (channels the first ten pixels sit in)
        w[(37 * n + seed) % Cout, ci, tap // 3, tap % 3] = 2.0 ** (n % 3 - 1) * (-1.0) ** n
    return dict(x=x, w=w)


def direct_k(c, route=None, pooled=False):
    """the bar's k of a stride-1 direct 3x3 case (ups 0 / 1), counted like pw_k and wino_k's route-F branch from the
    arithmetic of csrc/p2l_conv.hip, p2l_h2.hip and p2l_h2r.hip.  A K slice is whole 16-channel chunks, a chunk nine
    taps of 16 channels: `deep` = the 9 x channels im2col columns of the deepest slice (splitk_slices on chunks of
    144 columns).  Per column onto the accumulator -- F (fp32 MFMA): a product and an addition (2); B (bf16 x 3):
    the six cross terms of exact products (6); H, R (fp16 x 2): three (3).  Then the slices, summed in the finish
    kernels' order (slices - 1); B: the pieces to 2^-24 relative of either operand (2) and the dropped terms <= 2^-23
    (2); H, R: the pieces to 2^-22 of either operand (8), the dropped term (4) and the absolute floor that
    `direct_h2_floor` puts into the denominator (1).  The nearest upsample of ups = 1 copies values: no term.  Then
    pw_k's prologue and epilogue terms: the prologue's fma (2); alpha, oscale, bias, noise (a product and a sum),
    residual one each; tanh 2; the leaky ReLU's factor sqrt 2 on everything before it and its own rounding; the
    pool's sum two additions deep.  R counts as H: the same order on the same pieces (the header of p2l_h2r.hip)"""
    route = route or c['route']
    sl = splitk_slices(9 * c['Cin'], 144, c['splitk'])
    deep = max(hi - lo for lo, hi in sl)
    k = {'F': 2, 'B': 6, 'H': 3, 'R': 3}[route] * deep + (len(sl) - 1) + {'F': 0, 'B': 4, 'H': 13, 'R': 13}[route]
    k += (2 if c['pro'] != PRO_NONE else 0) + 1 + c['oscale'] + c['bias'] + 2 * c['noise'] + (c['res'] is not None)
    if c['act'] == ACT_TANH:
        k += 2
    if c['act'] == ACT_LRELU_SQRT2:
        k = 1.5 * k + 1
    return k + 2 if pooled and c['pool'] == POOL_SUM else k


def direct_h2_floor(aabs, w, amax=None, wmax=None, ups=False):
    """h2_floor over the nine taps (the direct kernel splits a and w themselves), fp64 [B, H, W, N]: aabs the
    prologue's absolute values (no prologue: |x|) at the resolution of x, upsampled here under ups = 1; amax [B] the
    maxima the kernel scales by (pw_amax; default: those of aabs), wmax max |w|"""
    xa, wa = aabs.double(), w.double().abs()
    amax = xa.amax(dim=(1, 2, 3)) if amax is None else amax.double()
    wmax = float(wa.max()) if wmax is None else float(wmax)
    xa = up2(xa) if ups else xa
    near = F.conv2d(xa.permute(0, 3, 1, 2), torch.ones(1, xa.shape[-1], 3, 3, dtype=torch.float64), padding=1)
    return 2.0 ** -13 * (amax.view(-1, 1, 1, 1) * wa.sum(dim=(1, 2, 3)) + wmax * near.permute(0, 2, 3, 1))


def producer_amax(y, next_s=None, next_t=None):
    """[B]: what a maxima producer records for the y it stored, over all its slots: max |y|, or max |fma(y, s, t)| of
    the affine its reader will fuse (one rounding: the epilogue's y s + t is a fused multiply-add)"""
    v = y if next_s is None else fma(y, next_s[:, None, None], next_t[:, None, None])
    return v.abs().amax(dim=(1, 2, 3))


def _wac(route, HW, B, Cin, Cout, **kw):
    c = dict(route=route, H=HW[0], W=HW[1], B=B, Cin=Cin, Cout=Cout, splitk=1, skip=None, pool_sum=False,
             nomask=False, amax=None, blk=16 if route == 'H' else 0, pro=PRO_NONE, alpha=1.0, own=False)
    assert not set(kw) - set(c), kw
    c.update(kw)
    return c


def wino_arb_id(c):
    d = _wac(c['route'], (c['H'], c['W']), c['B'], c['Cin'], c['Cout'])
    return '%s-%dx%dx%d-%dto%d' % (c['route'], c['B'], c['H'], c['W'], c['Cin'], c['Cout']) + ''.join(
        '-%s%s' % (k, c[k]) for k in sorted(c) if c[k] != d[k])


# the launch's Cin -> Cout: the gradient of the 64 -> 64 and 128 -> 48 forward convs, and the 2-slice HS shape
WINO_ARB_CASES = [_wac(*base, **dict(kw, **v)) for base, kw in [
    (('W8', (16, 16), 2, 64, 64), {}), (('W16', (16, 16), 2, 64, 64), {}), (('H', (16, 16), 2, 64, 64), dict(blk=8)),
    (('W8', (16, 32), 2, 48, 128), {}), (('W16', (16, 32), 2, 48, 128), {}),
    (('H', (16, 32), 2, 48, 128), dict(amax='true')), (('HS', (16, 16), 2, 256, 512), dict(splitk=2))]
    for v in ARB_VARIANTS]


def wino_arb_inputs(g, c):
    i = arb_inputs(g, dict(c, route='C' if c['route'] in ('H', 'HS') else 'A'))
    i['w'] = torch.randn(c['Cout'], c['Cin'], 3, 3, generator=g) / math.sqrt(9 * c['Cin'])
    return i


def wino_arb_refs(c, i):
    """-> conv3x3_arb's dict in fp64 and the route's fp32 restatement's, ds and dt in the kernels' two stages
    (arb_sums32: an unsplit launch leaves one partial per 8x16-pixel tile in both block shapes, its quads row-major,
    one row per wave; the K-sliced one one per quad)"""
    kw = dict(pool_sum=c['pool_sum'], nomask=c['nomask'], skip=i.get('skip'), skip_C=c['Cout'] // 2 if c['skip'] else 0,
              skip_ups=c['skip'] == 'ups')
    floor = None
    if c['route'] in ('H', 'HS'):
        floor = wino_h2_floor(i['x'].double().abs(), i['w'], pw_amax(c, i)[1], i['w'].abs().max())
    r64 = conv3x3_arb(i['x'].double(), i['w'].double(), i['ax'].double(), i['as'].double(), i['at'].double(),
                      floor=floor, **kw)
    r32 = conv3x3_arb(i['x'], i['w'], i['ax'], i['as'], i['at'], acc=wino_acc32(c, i), **kw)
    r32['ds'], r32['dt'] = arb_sums32(r32['g'], i['ax'], c['H'], c['W'], c['pool_sum'], c['route'] == 'HS')
    return r64, r32


# ---- direct 3x3 convs, stride 1, ups 0 / 1 (tests/test_direct_kernels_gpu.py) ---------------------------------------
# Routes of a taps = 9 launch that the Winograd kernels do not take: F conv_mfma_kernel<9, .., BF3 = false>
# (P2L_WFMT_F32), B the same kernel in bf16 x 3 (wfmt 'bf3': P2L_WFMT_BF16X3; 'bf3w': P2L_WFMT_BF16X3W kept on it with
# P2L_FORM_NO_WINO | P2L_FORM_WINO_BF3; ups = 1 always), H conv_h2_kernel<9, ..> (fp16 x 2, chunked), R conv_h2r_kernel
# (64 -> 64, whole 8x16 tiles; seq: P2L_FORM_H2R_SEQ_EPI, the shared epilogue item).  H, W are those of the OUTPUT (ups
# = 1: x is [B, H/2, W/2, Cin]).  A weight is the [N, K, 3, 3] correlation kernel the launch applies.
WFMT_BF16X3 = 1
FORM_NO_WINO, FORM_NO_H2R, FORM_H2R_SEQ_EPI = 1, 256, 512


def direct_tile(H, W):
    """(TW, TH, TB) of choose_tile (csrc/p2l_conv.hip): 128 pixels, TW = min(16, npow2(W)), TH up to npow2(H), the
    rest images"""
    TW = min(npow2(W), 16)
    TH = min(128 // TW, npow2(H))
    TB = 128 // (TW * TH)
    while TB > 1 and TB * (TH + 2) * (TW + 2) > 320:      # (the 320 patch rows a block stages: 2-wide / 2-high grids)
        TH, TB = 2 * TH, TB // 2
    return TW, TH, TB


def direct_cols(a):
    """im2col of the zero-padded a [B, H, W, K] with the K axis in the order all three kernels walk it (read off their
    loops: `for c in chunks` outside, the unrolled `tap = u / NT` inside, 16 channels per MFMA group; tap = 3 dy + dx
    reads pixel (y + dy - 1, x + dx - 1)): 16-channel chunk, tap, channel -> [B, H, W, 9 K]"""
    B, H, W, K = a.shape
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    taps = torch.stack([ap[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], dim=3)    # [B, H, W, 9, K]
    return taps.reshape(B, H, W, 9, K // 16, 16).permute(0, 1, 2, 4, 3, 5).reshape(B, H, W, 9 * K)


def direct_wmat(w):
    """[N, K, 3, 3] -> [N, 9 K] in direct_cols' order"""
    N, K = w.shape[:2]
    return w.reshape(N, K // 16, 16, 9).permute(0, 1, 3, 2).reshape(N, 9 * K)


def direct_acc32(c, i, route=None):
    """the fp32 restatement of a route's accumulator in front of alpha and the epilogue, [B, H, W, N]: the prologue
    (on the low-resolution x under ups = 1, then up2), zero padding, and acc_fp32 / acc_bf3 / acc_h2 on the im2col in
    the kernels' order with chunks of 9 x 16 columns.  R shares H's restatement and never slices"""
    route = route or c['route']
    a, _ = pw_prologue(i['x'], c['pro'], i.get('s'), i.get('t'))
    a = up2(a) if c['ups'] else a
    cols, wm = direct_cols(a), direct_wmat(i['w'])
    if route == 'F':
        return acc_fp32(cols, wm, c['splitk'], 144)
    if route == 'B':
        return acc_bf3(cols, wm, c['splitk'], 144)
    return acc_h2(cols, wm, pw_amax(c, i)[1], i['w'].abs().max(), c['splitk'] if route == 'H' else 1, 144)


def _dc(route, HW, B, Cin, Cout, **kw):
    c = dict(route=route, H=HW[0], W=HW[1], B=B, Cin=Cin, Cout=Cout, pro=PRO_NONE, pro_b=1, alpha=1.0, bias=False,
             res=None, mask=False, act=ACT_NONE, pool=POOL_NONE, want_y=True, oscale=False, noise=False,
             n_store=Cout, splitk=1, amax=None, ups=0, wfmt='bf3', seq=False, finish='v4', relu_like=False)
    assert not set(kw) - set(c), kw
    c.update(kw)
    return c


def direct_id(c):
    d = _dc(c['route'], (c['H'], c['W']), c['B'], c['Cin'], c['Cout'])
    return '%s-%dx%dx%d-%dto%d' % (c['route'], c['B'], c['H'], c['W'], c['Cin'], c['Cout']) + ''.join(
        '-%s%s' % (k, c[k]) for k in sorted(c) if c[k] != d[k])


def direct_form(c, route=None):
    """-> (P2LConv.wfmt, P2LConv.form) of a case on `route`"""
    route = route or c['route']
    if route == 'F':
        return 0, 0
    if route == 'B':
        if c['wfmt'] == 'bf3':
            return WFMT_BF16X3, 0
        return WFMT_BF16X3W, 0 if c['ups'] else FORM_NO_WINO | FORM_WINO_BF3
    if route == 'H':
        return WFMT_BF16X3W, FORM_NO_WINO | FORM_NO_H2R
    return WFMT_BF16X3W, FORM_H2R_SEQ_EPI if c['seq'] else 0


# the smallest shapes at which each form of choose_tile / choose_bn / direct_split exists
DIRECT_SHAPES = {
    '4x4': ((4, 4), 5, 32, 64),            # eight images per tile, the last tile with three empty slots
    '8x8': ((8, 8), 3, 48, 64),            # two images per tile
    '32x4': ((32, 4), 2, 32, 96),          # one image per tile on the A_ITERS = 5 form; BN = 32 by the remainder
    '8x16': ((8, 16), 1, 32, 128),         # the `small` form, one tile; BN = 64 on a small grid
    '16x16': ((16, 16), 2, 16, 64),        # ... two tiles
    '12x20': ((12, 20), 2, 32, 64),        # partial tiles in both directions
    '24x16': ((24, 16), 1, 16, 64),        # three whole tile rows
    '6x6': ((6, 6), 3, 32, 64),            # two images per tile, both partial
    '16x32': ((16, 32), 3, 64, 64),        # route R: four tiles per image, a block's range changes image
    '64x64': ((64, 64), 10, 16, 64),       # choose_bn's grid rule: n64 = 320 -> BN = 32 with Cout % 64 == 0
    'k8': ((8, 8), 3, 256, 64),            # p2l_conv_suggest_splitk: 8 slices
    'k4': ((16, 16), 2, 128, 64),          # ... 4
    'k4s': ((4, 4), 5, 128, 128),          # ... 4, eight images per tile
    'k3': ((8, 8), 3, 128, 64),            # 8 chunks, a request of 3: slices of 3 + 3 + 2
}


def _dsh(route, name, **kw):
    HW, B, Cin, Cout = DIRECT_SHAPES[name]
    return _dc(route, HW, B, Cin, Cout, **kw)


def _direct_fb(r, w):
    """the cases routes F and B share (B: `w` alternates its two weight formats)"""
    w = w if r == 'B' else 'bf3'
    return [
        _dsh(r, '4x4', **EPI[0]), _dsh(r, '8x8', wfmt=w, **EPI[1]), _dsh(r, '32x4', **EPI[2]),
        _dsh(r, '16x16', wfmt=w, **EPI[3]), _dsh(r, '8x16', **EPI[4]), _dsh(r, '12x20', wfmt=w, n_store=36, **EPI[5]),
        _dsh(r, '24x16', **EPI[6]), _dsh(r, '6x6', wfmt=w, bias=True, pro=PRO_AFFINE_RELU, pro_b=0),
        _dsh(r, '64x64', act=ACT_RELU),
        # ups = 1: nearest x 2 inside the staging, the prologue on the low-resolution tensor
        _dsh(r, '8x8', ups=1, wfmt='bf3w', **EPI[0]), _dsh(r, '16x16', ups=1, wfmt='bf3w', **EPI[2]),
        _dsh(r, '16x32', ups=1, wfmt='bf3w', **EPI[1]),
        # K slices through conv_splitk_finish_v4, and one through the scalar conv_splitk_finish
        _dsh(r, 'k8', splitk=8, wfmt=w, **EPI[0]), _dsh(r, 'k4', splitk=4, **EPI[3]),
        _dsh(r, 'k4s', splitk=4, wfmt=w, **EPI[2]), _dsh(r, 'k3', splitk=3, **EPI[6]),
        _dsh(r, 'k3', splitk=4, ups=1, wfmt='bf3w', **EPI[4]),
        _dsh(r, 'k8', splitk=8, finish='scalar', wfmt=w, **EPI[0]),
    ]


DIRECT_FWD_CASES = _direct_fb('F', 'bf3') + _direct_fb('B', 'bf3w') + [
    # H: maxima from the pass in front (amax None), handed over (true / raw under a prologue), in_applied
    _dsh('H', '4x4', **EPI[0]), _dsh('H', '8x8', amax='raw', **EPI[1]), _dsh('H', '32x4', amax='applied', **EPI[2]),
    _dsh('H', '16x16', amax='true', **EPI[3]), _dsh('H', '8x16', **EPI[4]),
    _dsh('H', '12x20', amax='true', n_store=36, **EPI[5]), _dsh('H', '24x16', **EPI[6]),
    _dsh('H', '6x6', bias=True, pro=PRO_AFFINE_RELU, pro_b=0, amax='raw'),
    _dsh('H', '16x32', act=ACT_TANH),                                         # (its all-zero image: exactly 0)
    _dsh('H', '64x64', act=ACT_RELU, amax='true'),
    _dsh('H', 'k8', splitk=8, **EPI[0]), _dsh('H', 'k4', splitk=4, amax='true', **EPI[3]),
    _dsh('H', 'k4s', splitk=4, amax='applied', **EPI[2]), _dsh('H', 'k3', splitk=3, **EPI[6]),
    _dsh('H', 'k8', splitk=8, finish='scalar', amax='raw', **EPI[1]),
    # R: EPI 1 (plain), 2 (mask), 3 (max pool) by the epilogue; everything else on the shared item (seq)
    _dsh('R', '16x32', bias=True, act=ACT_RELU), _dsh('R', '16x32', amax='applied', **EPI[2]),
    _dsh('R', '16x32', amax='true', **EPI[3]), _dsh('R', '16x32', seq=True, **EPI[0]),
    _dsh('R', '16x32', seq=True, amax='raw', **EPI[1]), _dsh('R', '16x32', seq=True, **EPI[4]),
    _dsh('R', '16x32', seq=True, n_store=36, **EPI[5]), _dsh('R', '16x32', seq=True, amax='true', **EPI[6]),
]


def direct_inputs(g, c):
    """wino_inputs' operands for a direct case (H, R: the fp16 x 2 inputs -- the quad 2^-20 below the maximum, the
    all-zero image of a batch of three, the heavy channel under a prologue; PRO_AFFINE: |t| of 2 .. 5 units of the
    image) with the images of one launch scaled very differently on top of their magnitudes: the first x 1e-6, the
    last x 3e4 -- x, a per-image t, the residual and the noise alike (a prologue shared by the batch keeps pw_inputs'
    magnitudes: one t has to fit every image).  ups = 1: x is every other pixel of the draw, [B, H/2, W/2, Cin]"""
    i = wino_inputs(g, dict(c, route='H' if c['route'] in 'HR' else 'W8'))
    B = c['B']
    if c['ups']:
        i['x'] = i['x'][:, ::2, ::2].contiguous()
    if B >= 2 and (c['pro'] == PRO_NONE or c['pro_b']):
        f = torch.ones(B)
        f[0], f[B - 1] = 1e-6, 3e4
        i['x'] = i['x'] * f.view(B, 1, 1, 1)
        if 't' in i:
            i['t'] = i['t'] * f.view(B, 1)
        if 'res' in i:
            i['res'] = i['res'] * f.view(B, 1, 1, 1)
        if 'noise' in i:
            i['noise'] = i['noise'] * f.view(B, 1, 1)
    return i


def direct_refs(c, i, route=None, restate=True):
    """-> conv3x3's dict in fp64 on den_d (H, R: plus direct_h2_floor) and the route's fp32 restatement's (restate =
    False: None)"""
    route = route or c['route']
    i64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in i.items()}
    floor = None
    if route in 'HR':
        _, aabs = pw_prologue(i64['x'], c['pro'], i64.get('s'), i64.get('t'))
        floor = direct_h2_floor(aabs, i['w'], pw_amax(c, i)[1], i['w'].abs().max(), bool(c['ups']))
    ups = bool(c['ups'])
    r64 = conv3x3(i64['x'], i64['w'], floor=floor, ups=ups, den_w=False, **pw_kwargs(c, i, torch.float64))
    if not restate:
        return r64, None
    r32 = conv3x3(i['x'], i['w'], acc=direct_acc32(c, i, route), ups=ups, den_w=False,
                  **pw_kwargs(c, i, torch.float32))
    return r64, r32


def direct_spots(H, W, B):
    """(image, y, x) of the one-hot pixels: the corners, the edges, both sides of every seam of choose_tile's tiles,
    the last row / column (of a partial tile where the grid has one), the interior, and the first pixel and the last
    of the second image (in a multi-image tile: the neighbour of image 0's halo)"""
    TW, TH, TB = direct_tile(H, W)
    sp = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1), (0, 0, W // 2), (0, H // 2, 0),
          (0, H - 1, W // 2 - 1), (0, H // 2, W - 1), (0, H // 2, W // 2), (0, 1, 1), (0, H - 2, W - 2)]
    for ys in range(TH, H, TH):
        sp += [(0, ys - 1, W // 3), (0, ys, W // 3), (0, ys - 1, W - 1), (0, ys, 0)]
    for xs in range(TW, W, TW):
        sp += [(0, H // 3, xs - 1), (0, H // 3, xs), (0, 0, xs - 1), (0, H - 1, xs)]
    if B > 1:
        sp += [(1, 0, 0), (1, H - 1, W - 1), (B - 1, 0, W - 1), (B - 1, H - 1, 0)]
    out = []
    for s in sp:
        if s not in out:
            out.append(s)
    return out


def direct_onehot(c, tap, seed=0):
    """exact inputs: x with single power-of-two pixels at direct_spots (ups = 1: on the low-resolution grid), one per
    channel in turn; w with single power-of-two entries on tap (a, b) at a few (cout, cin).  Every output is a sum
    of a few powers of two within a few binades: exact in fp32, in three bf16 and in two fp16 pieces"""
    B, H, W, Cin, Cout = c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    h, w_ = (H // 2, W // 2) if c['ups'] else (H, W)
    x, w = torch.zeros(B, h, w_, Cin), torch.zeros(Cout, Cin, 3, 3)
    spots = direct_spots(h, w_, B)
    for n, (b, py, px) in enumerate(spots):
        x[b, py, px, (5 * (n + seed)) % Cin] = 2.0 ** ((n + seed) % 5 - 2)
    for n in range(min(len(spots), Cin)):
        ci = (5 * (n + seed)) % Cin
        w[(37 * n + seed) % Cout, ci, tap // 3, tap % 3] = 2.0 ** (n % 3 - 1) * (-1.0) ** n
    return dict(x=x, w=w)


def _dac(route, HW, B, Cin, Cout, **kw):
    c = dict(route=route, H=HW[0], W=HW[1], B=B, Cin=Cin, Cout=Cout, splitk=1, skip=None, pool_sum=False,
             nomask=False, amax=None, pro=PRO_NONE, alpha=1.0, ups=0, wfmt='bf3', seq=False, finish='v4',
             amax_out=False)
    assert not set(kw) - set(c), kw
    c.update(kw)
    return c


def direct_arb_id(c):
    d = _dac(c['route'], (c['H'], c['W']), c['B'], c['Cin'], c['Cout'])
    return '%s-%dx%dx%d-%dto%d' % (c['route'], c['B'], c['H'], c['W'], c['Cin'], c['Cout']) + ''.join(
        '-%s%s' % (k, c[k]) for k in sorted(c) if c[k] != d[k])


# the launch's Cin -> Cout.  Unsplit: one image per tile (F, B, H; R on the shared item); in K slices on the multi-image
# 4x4 / 8x8 tiles, where the finish kernel does the backward per quad.  amax_out: the launch records the maxima of dx
# (P2LArb.amax.out) -- what the plans' gradient launches do, and what makes the plain variant on H the class EPI_ARB
# with its compiled epilogue (csrc/p2l_conv_k.h epi_class); every other variant and case runs the shared item
DIRECT_ARB_CASES = [_dac(*base, **dict(kw, **v)) for base, kw in [
    (('F', (16, 16), 2, 32, 64), {}), (('B', (16, 16), 2, 32, 64), {}), (('B', (24, 16), 2, 16, 96), dict(wfmt='bf3w')),
    (('H', (16, 16), 2, 32, 64), {}), (('H', (16, 32), 2, 64, 64), dict(amax='true')),
    (('H', (16, 16), 2, 16, 64), dict(amax_out=True)), (('H', (32, 4), 2, 32, 96), dict(amax_out=True)),
    (('R', (16, 32), 2, 64, 64), dict(seq=True)),
    (('F', (4, 4), 5, 128, 128), dict(splitk=4)), (('B', (8, 8), 3, 128, 64), dict(splitk=3)),
    (('H', (8, 8), 3, 256, 64), dict(splitk=8)), (('H', (4, 4), 5, 128, 128), dict(splitk=4, amax='true'))]
    for v in ARB_VARIANTS]


def direct_arb_inputs(g, c):
    i = arb_inputs(g, dict(c, route='C' if c['route'] in 'HR' else 'A'))
    i['w'] = torch.randn(c['Cout'], c['Cin'], 3, 3, generator=g) / math.sqrt(9 * c['Cin'])
    return i


def direct_arb_refs(c, i):
    """-> conv3x3_arb's dict in fp64 on the direct denominator (H, R: plus direct_h2_floor) and the route's fp32
    restatement's, ds and dt in the kernels' two stages (arb_sums32: an unsplit launch leaves one partial per
    128-pixel tile through epilogue_vec_items -- the register-resident kernel fills the same dumps --, a K-sliced one
    one per quad)"""
    kw = dict(pool_sum=c['pool_sum'], nomask=c['nomask'], skip=i.get('skip'), skip_C=c['Cout'] // 2 if c['skip'] else 0,
              skip_ups=c['skip'] == 'ups')
    floor = None
    if c['route'] in 'HR':
        floor = direct_h2_floor(i['x'].abs(), i['w'], pw_amax(c, i)[1], i['w'].abs().max())
    r64 = conv3x3_arb(i['x'].double(), i['w'].double(), i['ax'].double(), i['as'].double(), i['at'].double(),
                      floor=floor, den_w=False, **kw)
    r32 = conv3x3_arb(i['x'], i['w'], i['ax'], i['as'], i['at'], acc=direct_acc32(c, i), den_w=False, **kw)
    split = len(splitk_slices(9 * c['Cin'], 144, c['splitk'])) > 1
    r32['ds'], r32['dt'] = arb_sums32(r32['g'], i['ax'], c['H'], c['W'], c['pool_sum'], split)
    return r64, r32


# ---- sub-pixel 3x3 convs, ups 2 / 3 (tests/test_subpix_kernels_gpu.py) ------------------------------------------------
# The four modes of a taps = 9 launch with P2LConv.ups >= 2 (include/p2l.h): ups = 2 the forward conv on the low-
# resolution x [B, H/2, W/2, Cin] -- ext = 0: the 3x3 conv of its nearest x 2 upsample, ext = 1: the stride-2 transposed
# conv, written into a [B, H+2, W+2, *] frame -- and ups = 3 its input gradient, from the high-resolution gradient (ext =
# 1: the frame, row / column H+1 zero) to [B, H/2, W/2, Cout].  H, W are the HIGH-resolution dims of the descriptor, Cin
# -> Cout those of the launch, and a case's weight is always the FORWARD conv's OIHW tensor: [Cout, Cin, 3, 3] for ups
# = 2, [Cin, Cout, 3, 3] for ups = 3 (packed through transpose_flip).  Routes: F conv_mfma_kernel<4, .., BF3 = false>
# (P2L_WFMT_F32), B the same kernel in bf16 x 3 (wfmt 'bf3': P2L_WFMT_BF16X3; 'bf3w': P2L_WFMT_BF16X3W with
# P2L_FORM_WINO_BF3; 'nows': P2L_WFMT_BF16X3W without the 256 B per image of workspace), H conv_h2_kernel<4, ..> (fp16 x
# 2, P2L_FORM_NO_SP_PAIR on a forward launch), P conv_h2_kernel<8, ..> (ups = 2: P2L_FORM_SP_PAIR, or pair = 'own': by
# the launcher's own rule, ext = 1 with 64-channel tiles).
FORM_NO_SP_SKIP, FORM_NO_SP_PAIR, FORM_SP_PAIR = 1024, 2048, 4096

# sp_tapset of csrc/p2l_conv.hip restated: (mode, flip) -> [p: phase | plane parity][i: window tap] -> the original taps
# (dy, or dx) whose weights the slab sums along that dimension (tests/test_small_refs.py ties it to the definition)
SP_TAPS = {
    (0, 0): (((0,), (1, 2)), ((0, 1), (2,))),
    (0, 1): (((1, 2), (0,)), ((2,), (0, 1))),
    (1, 0): (((2,), (0,)), ((1,), ())),
    (1, 1): (((0,), (2,)), ((), (1,))),
}


def subpix_slabs(w, mode, flip):
    """the 16 (phase | plane, window tap) weight slabs of pack_subpix_kernel from the forward conv's OIHW w, in the
    dtype of w: slab 4 p + t with p = 2 py + px, t = 2 i + j sums w[.., dy, dx] over SP_TAPS[py][i] x SP_TAPS[px][j]
    onto 0 in the kernel's dy-outer / dx-inner order (fp32: its pack-time roundings) -> [16, N, K]; flip (the input
    gradient): N, K = I, O"""
    src = w.permute(1, 0, 2, 3) if flip else w
    T = SP_TAPS[(mode, int(bool(flip)))]
    out = []
    for ph in range(4):
        for tap in range(4):
            v = torch.zeros(src.shape[:2], dtype=w.dtype)
            for dy in range(3):
                for dx in range(3):
                    if dy in T[ph >> 1][tap >> 1] and dx in T[ph & 1][tap & 1]:
                        v = v + src[:, :, dy, dx]
            out.append(v)
    return torch.stack(out)


def subpix_windows(a, ups, ext):
    """the 2x2 windows the kernels read, per phase (ups = 2: a the low-resolution [B, h, w, K] after the prologue,
    zero outside) or phase plane (ups = 3: a the high-resolution gradient [B, H + 2 ext, W + 2 ext, K]) -> four
    [B, gh, gw, 4, K].  Read off the staging and the fragment addressing of conv_mfma_kernel<4, ..> / conv_h2_kernel:
    a patch line holds low-resolution rows y0 - 1 .., window tap (i, j) of grid point (p, q) reads patch row p + oy + i:
    phase (py, px) pixel (p - 1 + py + i, q - 1 + px + j) of x; plane (cy, cx) -- oy = 1 - cy -- pixel (p - cy + i, q -
    cx + j) of the plane, i.e. row 2 (p - cy + i) + cy of the frame"""
    out = []
    if ups == 2:
        h, w = a.shape[1:3]
        gh, gw = h + ext, w + ext
        ap = F.pad(a, (0, 0, 1, 1 + ext, 1, 1 + ext))
        for ph in range(4):
            py, px = ph >> 1, ph & 1
            out.append(torch.stack([ap[:, py + i:py + i + gh, px + j:px + j + gw] for i in (0, 1) for j in (0, 1)], dim=3))
        return out
    for cls in range(4):
        cy, cx = cls >> 1, cls & 1
        pl = a[:, cy::2, cx::2]
        h, w = pl.shape[1] - ext, pl.shape[2] - ext
        ap = F.pad(pl, (0, 0, 1, 1, 1, 1))
        out.append(torch.stack([ap[:, 1 - cy + i:1 - cy + i + h, 1 - cx + j:1 - cx + j + w]
                                for i in (0, 1) for j in (0, 1)], dim=3))
    return out


def subpix_cols(win):
    """[B, gh, gw, 4, K] -> [B, gh, gw, 4 K] in the kernels' K order: 16-channel chunk, window tap, channel"""
    B, gh, gw, _, K = win.shape
    return win.reshape(B, gh, gw, 4, K // 16, 16).permute(0, 1, 2, 4, 3, 5).reshape(B, gh, gw, 4 * K)


def subpix_wmat(slabs4):
    """the four slabs [4, N, K] of one phase | plane -> [N, 4 K] in subpix_cols' order"""
    _, N, K = slabs4.shape
    return slabs4.reshape(4, N, K // 16, 16).permute(1, 2, 0, 3).reshape(N, 4 * K)


def subpix_map(a, w, ups, ext):
    """the plain linear map of the four modes in the dtype of a, from the definitions alone -- nothing here knows
    phases, planes or slabs.  w: the forward conv's [O, I, 3, 3].  ups = 2, ext = 0: zero pad and 3x3 of the nearest
    x 2 of a [B, h, w, I]; ext = 1: conv_transpose2d(stride 2) -- out[2 p + k] += a[p] w[k] -- in rows / columns 0 .. H
    of a [B, H + 2, W + 2, O] frame, row / column H + 1 zero.  ups = 3: the vjp of that forward at the gradient a [B,
    H + 2 ext, W + 2 ext, O] -> [B, h, w, I]"""
    nchw = lambda v: v.permute(0, 3, 1, 2)
    if ups == 2:
        if not ext:
            return F.conv2d(nchw(up2(a)), w, padding=1).permute(0, 2, 3, 1)
        u = F.conv_transpose2d(nchw(a), w.transpose(0, 1), stride=2).permute(0, 2, 3, 1)
        return F.pad(u, (0, 0, 0, 1, 0, 1))
    B, Hf, Wf, _ = a.shape
    z = torch.zeros(B, (Hf - 2 * ext) // 2, (Wf - 2 * ext) // 2, w.shape[1], dtype=a.dtype)
    return vjp(lambda z_: subpix_map(z_, w, 2, ext), [z], a)


def subpix_h2_wmax(w):
    """what p2l_pack_conv_weight_subpix_h2 records in its tail and scales every slab by: 4 max |w| over the OIHW
    tensor (h2_tail_x4_kernel: a slab sums up to four taps) -- a bound of the slabs, not their maximum"""
    return 4.0 * w.abs().max()


def subpix_h2_floor(aabs, w, ups, ext, amax, wmax):
    """direct_h2_floor for the sub-pixel forms, fp64 at the output's shape: 2^-13 (amax_b sum |w| + wmax sum |a|), both
    sums over the original taps and channels that reach the output from a real input position (subpix_map of ones).
    aabs: the prologue's absolute values (ups = 3: |gradient|), amax [B] the maxima the kernel scales by, wmax the pack
    tail (subpix_h2_wmax)"""
    xa, wa = aabs.double(), w.double().abs()
    one_a = torch.ones_like(xa[:1])
    if ups == 3 and ext:
        one_a[:, -1], one_a[:, :, -1] = 0.0, 0.0
    one_w = torch.ones_like(wa[:1]) if ups == 2 else torch.ones_like(wa[:, :1])
    return 2.0 ** -13 * (amax.double().view(-1, 1, 1, 1) * subpix_map(one_a, wa, ups, ext) +
                         float(wmax) * subpix_map(xa, one_w, ups, ext))


def subpix_acc32(c, i, route=None):
    """the fp32 restatement of a route's accumulator in front of alpha and the epilogue, read off the loops of
    conv_mfma_kernel<4, ..> (csrc/p2l_conv.hip) and conv_h2_kernel<4 | 8, ..> (csrc/p2l_h2.hip).  Weights: the fp32 slab
    sums of pack_subpix_kernel / h2_pack_kernel (subpix_slabs).  Forward (blockIdx.y = the phase; TAPS = 8: two phases,
    two accumulator sets, the same order per output): `for c in chunks` of 16 channels outside, the unrolled window taps
    u / NT (0 .. 3) inside, 16 channels per MFMA group -- per phase the columns (chunk, tap, channel) of subpix_cols,
    written to pixels (2 p + py, 2 q + px) of the [2 gh, 2 gw] buffer.  Gradient: chunk c = (plane cls = c / sp_ncc,
    channel chunk c % sp_ncc) -- `geom` -- with wslab = 4 cls: plane, chunk, tap, channel; K slices cut that chunk
    sequence by chunks_per_split = cdiv(4 Cin / 16, sk) (splitk_slices on chunks of 64 columns) and meet in the finish
    kernels' order (combine_slices).  The skipped taps of ext = 1 are zero slabs: their products add +0.  Accumulators:
    acc_fp32 / acc_bf3 / acc_h2 with chunks of 4 x 16 columns; fp16 x 2 scales by the per-image maxima of pw_amax and
    by the pack tail subpix_h2_wmax"""
    route = route or c['route']
    ups, ext = c['ups'], c['ext']
    a = pw_prologue(i['x'], c['pro'], i.get('s'), i.get('t'))[0] if ups == 2 else i['x']
    slabs = subpix_slabs(i['w'], ext, ups == 3)
    wins = subpix_windows(a, ups, ext)

    def acc(cols, wm, sk):
        if route == 'F':
            return acc_fp32(cols, wm, sk, 64)
        if route == 'B':
            return acc_bf3(cols, wm, sk, 64)
        return acc_h2(cols, wm, pw_amax(c, i)[1], subpix_h2_wmax(i['w']), sk, 64)
    if ups == 2:
        B, gh, gw = wins[0].shape[:3]
        out = torch.zeros(B, 2 * gh, 2 * gw, slabs.shape[1])
        for ph in range(4):
            out[:, ph >> 1::2, ph & 1::2] = acc(subpix_cols(wins[ph]), subpix_wmat(slabs[4 * ph:4 * ph + 4]), 1)
        return out
    cols = torch.cat([subpix_cols(wn) for wn in wins], dim=-1)
    wm = torch.cat([subpix_wmat(slabs[4 * cls:4 * cls + 4]) for cls in range(4)], dim=-1)
    return acc(cols, wm, c['splitk'])


def subpix_slices(c):
    """the (plane, chunk) slices of a ups = 3 launch as column ranges of the 16 Cin columns"""
    return splitk_slices(16 * c['Cin'], 64, c['splitk']) if c['ups'] == 3 else [(0, 4 * c['Cin'])]


def subpix_k(c, route=None, pooled=False):
    """the bar's k of a sub-pixel case, counted like direct_k.  Columns onto one accumulator: forward 4 window taps x
    Cin per phase, gradient 4 planes x 4 taps x Cin, the deepest K slice of it (whole (plane, chunk) chunks of 64
    columns) -- F a product and an addition (2), B six cross terms, H / P three per column; the slices in the finish
    kernels' order (slices - 1); B: pieces 2 + dropped terms 2; H / P: pieces 8 + dropped term 4 + the floor in the
    denominator 1.  The pack-time roundings of a summed slab, relative to sum |w_tap|: mode 0 (ext = 0) sums up to 2 x 2
    taps in ONE chain of fp32 additions -- 3 roundings, forward and gradient alike (the first addition onto 0 is exact);
    mode 1 (ext = 1) slabs are single taps: 0.  Then direct_k's prologue and epilogue terms"""
    route = route or c['route']
    sl = subpix_slices(c)
    deep = max(hi - lo for lo, hi in sl)
    k = {'F': 2, 'B': 6, 'H': 3, 'P': 3}[route] * deep + (len(sl) - 1) + {'F': 0, 'B': 4, 'H': 13, 'P': 13}[route]
    k += 0 if c['ext'] else 3
    k += (2 if c['pro'] != PRO_NONE else 0) + 1 + c['oscale'] + c['bias'] + 2 * c['noise'] + (c['res'] is not None)
    if c['act'] == ACT_TANH:
        k += 2
    if c['act'] == ACT_LRELU_SQRT2:
        k = 1.5 * k + 1
    return k


def subpix_bwd_split(H, W, Cin, Cout):
    """subpix_bwd_split of csrc/p2l_conv.hip for a ups = 3, ext = 1 fp16 x 2 launch on whole tiles (H, W the high-
    resolution dims, Cin the gradient's channels): 1 = unsliced"""
    p2f = lambda v: 1 if v < 2 else 2 ** (int(v).bit_length() - 1)
    hw = (H // 2) * (W // 2)
    s = min(p2f(Cin * 16 // 128), p2f(524288 // (hw * Cout)), 4 if hw >= 256 else 8)
    nchunks = 4 * (Cin // 16)
    while s > 1 and nchunks // s < 8:
        s //= 2
    return 1 if s <= 2 else s


def subpix_grid(c):
    """(gh, gw) of the low-resolution grid the kernel tiles, and direct_tile of it"""
    e = 1 if (c['ups'] == 2 and c['ext']) else 0
    gh, gw = c['H'] // 2 + e, c['W'] // 2 + e
    return (gh, gw), direct_tile(gh, gw)


def _sc(route, ups, ext, HW, B, Cin, Cout, **kw):
    c = dict(route=route, ups=ups, ext=ext, H=HW[0], W=HW[1], B=B, Cin=Cin, Cout=Cout, pro=PRO_NONE, pro_b=1, alpha=1.0,
             bias=False, res=None, mask=False, act=ACT_NONE, pool=POOL_NONE, want_y=True, oscale=False, noise=False,
             n_store=Cout, splitk=1, amax=None, wfmt='bf3', pair='form', skip=True, finish='v4', t0=False,
             cancel=False, relu_like=False)
    assert not set(kw) - set(c), kw
    c.update(kw)
    return c


def subpix_id(c):
    d = _sc(c['route'], c['ups'], c['ext'], (c['H'], c['W']), c['B'], c['Cin'], c['Cout'])
    return '%s-u%de%d-%dx%dx%d-%dto%d' % (c['route'], c['ups'], c['ext'], c['B'], c['H'], c['W'], c['Cin'], c['Cout']) + \
        ''.join('-%s%s' % (k, c[k]) for k in sorted(c) if c[k] != d[k])


def subpix_form(c, route=None):
    """-> (P2LConv.wfmt, P2LConv.form, with the fp16 x 2 share of the workspace) of a case on `route`"""
    route = route or c['route']
    noskip = 0 if c['skip'] else FORM_NO_SP_SKIP
    if route == 'F':
        return 0, 0, True
    if route == 'B':
        return {'bf3': (WFMT_BF16X3, 0, True), 'bf3w': (WFMT_BF16X3W, FORM_WINO_BF3, True),
                'nows': (WFMT_BF16X3W, 0, False)}[c['wfmt']]
    if route == 'H':
        return WFMT_BF16X3W, noskip | (FORM_NO_SP_PAIR if c['ups'] == 2 else 0), True
    assert c['ups'] == 2
    return WFMT_BF16X3W, noskip | (FORM_SP_PAIR if c['pair'] == 'form' else 0), True


# hi-res H x W, B, Cin, Cout of the launch: the smallest shapes that reach each path of choose_tile on the low-
# resolution grid (ext = 1 forward: H/2 + 1 points, every tile partial)
SUBPIX_SHAPES = {
    '16x32': ((16, 32), 1, 16, 32),        # grid 8x16: one whole tile, A_ITERS = 3 | ext forward 9x17: four partial tiles
    '32x32': ((32, 32), 2, 48, 64),        # grid 16x16: a seam in y | 17x17: four tiles, all partial
    '16x64': ((16, 64), 1, 16, 96),        # grid 8x32: a seam in x
    '8x8': ((8, 8), 3, 64, 32),            # grid 4x4: eight images per tile, A_ITERS = 5 | 5x5: two per tile, partial
    '8x8b9': ((8, 8), 9, 16, 64),          # ... a second tile
    '4x4': ((4, 4), 3, 16, 32),            # grid 2x2: the minimum choose_tile accepts | 3x3
    '4x4b9': ((4, 4), 9, 16, 32),          # ... nine images: a second tile of eight
    '16x16': ((16, 16), 2, 48, 96),        # grid 8x8: two images per tile | 9x9: TW = 16, two partial tile rows
    'bn64': ((16, 32), 16, 16, 256),       # ups = 2: n64 = 16 tiles x 4 channel tiles x 4 phases = 256 -> BN = 64
    'bn64e': ((16, 16), 8, 16, 256),       # ... ext = 1: grid 9x9, 2 tiles x 8 images x 4 x 4 = 256 -> BN = 64 unforced
    '4x4b32': ((4, 4), 32, 16, 32),        # grid 2x2: 32 images -- one tile of 512 patch rows by the 128-pixel rule
    's4': ((16, 16), 3, 128, 64),          # ups = 3, ext = 1: 4 K slices, two images per tile
    's8': ((16, 16), 1, 256, 32),          # ... 8 slices
    's4w': ((32, 32), 1, 256, 32),         # ... 4 slices (hw >= 256)
    'bn64g': ((16, 32), 64, 16, 256),      # ups = 3: 64 tiles x 4 channel tiles = 256 -> BN = 64 (slots query only: 4.7 s)
}


def _ssh(route, ups, ext, name, **kw):
    HW, B, Cin, Cout = SUBPIX_SHAPES[name]
    return _sc(route, ups, ext, HW, B, Cin, Cout, **kw)


# the epilogue terms of each mode (the issue's list): ups = 2, ext = 0 (BigGAN's conv_1) / ext = 1 (StyleGAN2's up conv)
SP_EPI_E0 = [dict(bias=True, alpha=0.5), dict(pro=PRO_AFFINE_RELU), dict(pro=PRO_AFFINE_RELU, pro_b=0, act=ACT_RELU),
             dict(pro=PRO_AFFINE, bias=True), dict(act=ACT_TANH)]
SP_EPI_E1 = [dict(pro=PRO_AFFINE, t0=True), dict(pro=PRO_AFFINE), dict(pro=PRO_AFFINE_RELU, bias=True),
             dict(pro=PRO_AFFINE, oscale=True, noise=True, bias=True, act=ACT_LRELU_SQRT2), dict(bias=True, alpha=0.5)]
SP_EPI_G = [dict(), dict(res='same', mask=True), dict(act=ACT_TANH), dict(res='same', alpha=0.5), dict(act=ACT_RELU)]


def _subpix_fwd(r, **rk):
    e0, e1 = SP_EPI_E0, SP_EPI_E1
    return [
        _ssh(r, 2, 0, '16x32', **dict(rk, **e0[0])), _ssh(r, 2, 0, '32x32', **dict(rk, **e0[1])),
        _ssh(r, 2, 0, '16x64', **dict(rk, **e0[2])), _ssh(r, 2, 0, '8x8', **dict(rk, **e0[3])),
        _ssh(r, 2, 0, '8x8b9', **dict(rk, **e0[4])), _ssh(r, 2, 0, '4x4', **dict(rk, **e0[0])),
        _ssh(r, 2, 0, '16x16', n_store=48, **dict(rk, **e0[1])), _ssh(r, 2, 0, '32x32', cancel=True, **rk),
        _ssh(r, 2, 1, '8x8', **dict(rk, **e1[0])), _ssh(r, 2, 1, '16x16', **dict(rk, **e1[1])),
        _ssh(r, 2, 1, '32x32', **dict(rk, **e1[2])), _ssh(r, 2, 1, '16x32', **dict(rk, **e1[3])),
        _ssh(r, 2, 1, '8x8b9', **dict(rk, **e1[4])), _ssh(r, 2, 1, '4x4', **dict(rk, **e1[1])),
        _ssh(r, 2, 1, '16x16', n_store=48, **dict(rk, **e1[2])),
    ]


def _subpix_bwd(r, **rk):
    g = SP_EPI_G
    return [
        _ssh(r, 3, 0, '16x32', **dict(rk, **g[0])), _ssh(r, 3, 0, '32x32', n_store=48, **dict(rk, **g[1])),
        _ssh(r, 3, 0, '16x64', **dict(rk, **g[2])), _ssh(r, 3, 0, '8x8', **dict(rk, **g[3])),
        _ssh(r, 3, 0, '4x4', **dict(rk, **g[4])), _ssh(r, 3, 0, '32x32', cancel=True, **rk),
        _ssh(r, 3, 1, '16x32', **dict(rk, **g[1])), _ssh(r, 3, 1, '32x32', **dict(rk, **g[0])),
        _ssh(r, 3, 1, '8x8b9', **dict(rk, **g[2])), _ssh(r, 3, 1, '4x4', **dict(rk, **g[3])),
        _ssh(r, 3, 1, '16x16', n_store=48, **dict(rk, **g[4])), _ssh(r, 3, 1, '16x64', **dict(rk, **g[0])),
    ]


SUBPIX_FWD_CASES = _subpix_fwd('F') + _subpix_fwd('B') + [
    _ssh('B', 2, 0, '16x32', wfmt='bf3w', bias=True), _ssh('B', 2, 1, '16x16', wfmt='nows', pro=PRO_AFFINE),
    # H: maxima from the pass in front (None), handed over (true / raw under a prologue), in_applied
    _ssh('H', 2, 0, '16x32', amax='true', **SP_EPI_E0[0]), _ssh('H', 2, 0, '32x32', amax='raw', **SP_EPI_E0[1]),
    _ssh('H', 2, 0, '16x64', amax='applied', **SP_EPI_E0[2]), _ssh('H', 2, 0, '8x8', **SP_EPI_E0[3]),
    _ssh('H', 2, 0, '8x8b9', amax='true', **SP_EPI_E0[4]), _ssh('H', 2, 0, '4x4', **SP_EPI_E0[0]),
    _ssh('H', 2, 0, '16x16', n_store=48, **SP_EPI_E0[1]), _ssh('H', 2, 0, '32x32', cancel=True),
    _ssh('H', 2, 1, '8x8', **SP_EPI_E1[0]), _ssh('H', 2, 1, '16x16', amax='raw', **SP_EPI_E1[1]),
    _ssh('H', 2, 1, '32x32', amax='applied', **SP_EPI_E1[2]), _ssh('H', 2, 1, '16x32', **SP_EPI_E1[3]),
    _ssh('H', 2, 1, '8x8b9', amax='true', **SP_EPI_E1[4]), _ssh('H', 2, 1, '4x4', **SP_EPI_E1[1]),
    _ssh('H', 2, 1, '16x16', n_store=48, skip=False, **SP_EPI_E1[2]),
    # P: two phases per block by the form bit, and by the launcher's own rule (ext = 1, 64-channel tiles)
    _ssh('P', 2, 0, '16x32', **SP_EPI_E0[0]), _ssh('P', 2, 0, '32x32', amax='raw', **SP_EPI_E0[1]),
    _ssh('P', 2, 0, '8x8', **SP_EPI_E0[3]), _ssh('P', 2, 0, '4x4', **SP_EPI_E0[4]),
    _ssh('P', 2, 0, 'bn64', bias=True),
    _ssh('P', 2, 1, '8x8', **SP_EPI_E1[0]), _ssh('P', 2, 1, '16x16', **SP_EPI_E1[1]),
    _ssh('P', 2, 1, '32x32', amax='applied', **SP_EPI_E1[2]), _ssh('P', 2, 1, '16x32', **SP_EPI_E1[3]),
    _ssh('P', 2, 1, 'bn64e', pair='own', **SP_EPI_E1[0]),
    # the 2x2 grid with 32 images: one 128-pixel tile would stage 32 x 16 = 512 patch rows, a block stages 320
    _ssh('F', 2, 0, '4x4b32', bias=True), _ssh('H', 2, 0, '4x4b32', bias=True),
]
SUBPIX_BWD_CASES = _subpix_bwd('F') + _subpix_bwd('B') + [
    _ssh('B', 3, 0, '16x32', wfmt='bf3w'), _ssh('B', 3, 1, '16x32', wfmt='nows'),
    _ssh('H', 3, 0, '16x32', amax='true'), _ssh('H', 3, 0, '32x32', n_store=48, **SP_EPI_G[1]),
    _ssh('H', 3, 0, '16x64', amax='true', **SP_EPI_G[2]), _ssh('H', 3, 0, '8x8', **SP_EPI_G[3]),
    _ssh('H', 3, 0, '4x4', **SP_EPI_G[4]), _ssh('H', 3, 0, '32x32', cancel=True),
    _ssh('H', 3, 1, '16x32', **SP_EPI_G[1]), _ssh('H', 3, 1, '32x32', amax='true', **SP_EPI_G[0]),
    _ssh('H', 3, 1, '8x8b9', **SP_EPI_G[2]), _ssh('H', 3, 1, '4x4', **SP_EPI_G[3]),
    _ssh('H', 3, 1, '16x16', n_store=48, skip=False, **SP_EPI_G[4]), _ssh('H', 3, 1, '16x64', **SP_EPI_G[0]),
    _ssh('H', 3, 0, '4x4b9', **SP_EPI_G[2]), _ssh('H', 3, 1, '8x8', **SP_EPI_G[3]),
    # K slices (ups = 3, ext = 1, fp16 x 2 only) through both finish kernels; s4: two images per tile
    _ssh('H', 3, 1, 's4', splitk=4, **SP_EPI_G[1]), _ssh('H', 3, 1, 's8', splitk=8, **SP_EPI_G[0]),
    _ssh('H', 3, 1, 's4w', splitk=4, amax='true', **SP_EPI_G[2]),
    _ssh('H', 3, 1, 's4', splitk=4, finish='scalar', **SP_EPI_G[3]),
    _ssh('H', 3, 1, 's8', splitk=8, skip=False, **SP_EPI_G[4]),
    _ssh('F', 3, 0, '4x4b32'), _ssh('H', 3, 1, '4x4b32'),
]


def subpix_inputs(g, c):
    """the operands of a case on the host, dense fp32: pw_inputs' draws (every image at a magnitude of its own; H, P:
    the all-zero image of a batch of three, the quad 2^-20 below the maximum, the heavy channel under a prologue) with
    direct_inputs' spread on top -- the first image x 1e-6, the last x 3e4: the images of one launch up to 3e14
    apart.  ups = 2: x the low-resolution tensor, w [Cout, Cin, 3, 3]; PRO_AFFINE: |t| of 2 .. 5 units of the image
    (t0: exactly 0, the launch the StyleGAN2 plan makes), so that a t at a padding position of the grid is far off;
    noise on the frame the launch writes.  ups = 3: x the high-resolution gradient (ext: the [H+2, W+2] frame, row /
    column H+1 zero), w the forward's [Cin, Cout, 3, 3], residual and mask at the low resolution.  cancel: weights
    whose taps cancel inside the 2 x 2 slab {1, 2} x {1, 2} of mode 0 (phase (0, 0), window tap (1, 1); the gradient's
    plane (0, 0), tap (0, 0)) the way fp32 cannot follow -- w[1][1] = b, w[2][1] = -b, w[1][2] and w[2][2] 2^-18 of b:
    the chain b + w12 rounds w12 to ulp(b) before -b takes b away again, so the packed slab is off by 2^-6 of |sum
    w_tap| and by 2^-24 of sum |w_tap| (two nearly opposite taps alone cancel exactly) -- on isolated input pixels, so
    that outputs exist which that slab alone feeds"""
    ups, ext, B, H, W, Cin, Cout = c['ups'], c['ext'], c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    h, w_ = H // 2, W // 2
    rt = 'C' if c['route'] in 'HP' else 'A'
    rn = lambda *sh: torch.randn(*sh, generator=g)
    if ups == 2:
        i = pw_inputs(g, dict(c, route=rt, H=h, W=w_, res=None, mask=False, noise=False))
        i['w'] = rn(Cout, Cin, 3, 3) / math.sqrt(9 * Cin)
    else:
        Hf, Wf = H + 2 * ext, W + 2 * ext
        i = pw_inputs(g, dict(c, route=rt, H=Hf, W=Wf, res=None, mask=False, noise=False))
        if ext:
            i['x'][:, Hf - 1], i['x'][:, :, Wf - 1] = 0.0, 0.0
        i['w'] = rn(Cin, Cout, 3, 3) / math.sqrt(9 * Cin)
    if c['relu_like']:
        i['x'] = torch.relu(i['x'])
    xmax = i['x'].abs().amax(dim=(1, 2, 3))
    out_mag = torch.where(xmax > 0, mags(B), torch.ones(B)).view(B, 1, 1, 1)
    if c['pro'] == PRO_AFFINE:
        sign = torch.where(torch.rand(i['t'].shape, generator=g) < 0.5, -1.0, 1.0)
        unit = xmax[:i['t'].shape[0]].view(-1, 1) if c['pro_b'] else xmax[xmax > 0].min()
        i['t'] = sign * (2.0 + 3.0 * torch.rand(i['t'].shape, generator=g)) * 0.3 * unit
        if c['t0']:
            i['t'] = torch.zeros_like(i['t'])
    if c['cancel']:
        b = i['w'][:, :, 1, 1].clone()
        i['w'][:, :, 2, 1] = -b
        i['w'][:, :, 1, 2] = 2.0 ** -18 * b.abs() * rn(*b.shape)
        i['w'][:, :, 2, 2] = 2.0 ** -18 * b.abs() * rn(*b.shape)
        keep = torch.zeros_like(i['x'])
        if ups == 2:
            keep[:, 1::3, 1::3] = 1.0
        else:
            keep[:, 2::6, 2::6] = 1.0
        i['x'] = i['x'] * keep
    if c['noise']:
        fr = (H + 2, W + 2) if (ups == 2 and ext) else ((H, W) if ups == 2 else (h, w_))
        i['noise'], i['noise_w'] = rn(B, *fr) * out_mag[..., 0], 0.3
    if c['res']:
        i['res'] = rn(B, h, w_, Cout) * out_mag
    if c['mask']:
        i['mask'] = rn(B, h, w_, Cout)
    if B >= 2 and (c['pro'] == PRO_NONE or c['pro_b']):
        f = torch.ones(B)
        f[0], f[B - 1] = 1e-6, 3e4
        i['x'] = i['x'] * f.view(B, 1, 1, 1)
        for name in ('t', 'res', 'noise'):
            if name in i and torch.is_tensor(i[name]):
                i[name] = i[name] * f.view([B] + [1] * (i[name].dim() - 1))
    return i


def subpix_launch(x, w, ups, ext, pro=PRO_NONE, s=None, t=None, alpha=1.0, acc=None, floor=None, **epi):
    """a sub-pixel launch of include/p2l.h in the dtype of x: a = prologue(x) on the input tensor itself -- before any
    upsampling or padding (ups = 3: no prologue) --, v = alpha subpix_map(a, w), then conv_epilogue(**epi) on the whole
    output (ext = 1 forward: the frame; its row / column H+1 holds the epilogue of 0).  `acc` replaces the map (a
    restatement's accumulator), `floor` is added to the denominator.  den = subpix_map(|a|, |w|): sum |a| |w| over the
    ORIGINAL 3x3 taps that reach the output -- a slab whose taps cancel keeps its denominator.
    -> conv_epilogue's dict, and a, aabs"""
    dt = x.dtype
    w = w.to(dt)
    a, aabs = pw_prologue(x, pro, s, t) if ups == 2 else (x, x.abs())
    v = subpix_map(a, w, ups, ext) if acc is None else acc.to(dt)
    den = subpix_map(aabs, w.abs(), ups, ext)
    den = den if floor is None else den + floor.to(dt)
    out = conv_epilogue(v * alpha, den * abs(alpha), **epi)
    out.update(a=a, aabs=aabs)
    return out


def subpix_refs(c, i, route=None, restate=True):
    """-> subpix_launch's dict in fp64 (H, P: with subpix_h2_floor) and the route's fp32 restatement's (restate =
    False: None)"""
    route = route or c['route']
    i64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in i.items()}
    kw64, kw32 = pw_kwargs(c, i, torch.float64), pw_kwargs(c, i, torch.float32)
    floor = None
    if route in 'HP':
        aabs = pw_prologue(i64['x'], c['pro'], i64.get('s'), i64.get('t'))[1] if c['ups'] == 2 else i64['x'].abs()
        floor = subpix_h2_floor(aabs, i['w'], c['ups'], c['ext'], pw_amax(c, i)[1], subpix_h2_wmax(i['w']))
    r64 = subpix_launch(i64['x'], i64['w'], c['ups'], c['ext'], floor=floor, **kw64)
    if not restate:
        return r64, None
    return r64, subpix_launch(i['x'], i['w'], c['ups'], c['ext'], acc=subpix_acc32(c, i, route), **kw32)


def subpix_spots(c):
    """(image, y, x) of the one-hot pixels on the INPUT tensor of a case: its corners, both sides of every seam of
    choose_tile's tiles of the low-resolution grid (ups = 3: the four high-resolution rows / columns around it), the
    last row / column -- of an ext = 1 forward the input pixel H/2 - 1 that alone reaches grid row H/2, of an ext = 1
    gradient row H of the frame --, the interior, and the first and last pixel of the second image"""
    ups, ext, B = c['ups'], c['ext'], c['B']
    (gh, gw), (TW, TH, TB) = subpix_grid(c)
    if ups == 2:
        ih, iw = c['H'] // 2, c['W'] // 2
        ys = [y for s in range(TH, gh, TH) for y in (s - 1, s)]
        xs = [x for s in range(TW, gw, TW) for x in (s - 1, s)]
    else:
        ih, iw = c['H'] + ext, c['W'] + ext                     # (the real rows / columns of the frame)
        ys = [y for s in range(TH, gh, TH) for y in (2 * s - 2, 2 * s - 1, 2 * s, 2 * s + 1)]
        xs = [x for s in range(TW, gw, TW) for x in (2 * s - 2, 2 * s - 1, 2 * s, 2 * s + 1)]
    sp = [(0, 0, 0), (0, 0, iw - 1), (0, ih - 1, 0), (0, ih - 1, iw - 1), (0, ih // 2, iw // 2), (0, 1, 1),
          (0, ih - 2, iw - 2), (0, 0, iw // 2), (0, ih // 2, 0)]
    sp += [(0, y, iw // 3) for y in ys if y < ih] + [(0, y, iw - 1) for y in ys if y < ih]
    sp += [(0, ih // 3, x) for x in xs if x < iw] + [(0, ih - 1, x) for x in xs if x < iw]
    if B > 1:
        sp += [(1, 0, 0), (1, ih - 1, iw - 1), (B - 1, 0, iw - 1), (B - 1, ih - 1, 0)]
    if ups == 3:        # all four phase planes at every spot: one tap of a transposed conv reaches one parity only
        sp = [(b, yy, xx) for b, y, x in sp for yy in (y, y ^ 1) for xx in (x, x ^ 1) if yy < ih and xx < iw]
    out = []
    for s in sp:
        if s not in out:
            out.append(s)
    return out


def subpix_onehot(c, tap, seed=0):
    """exact inputs: x with single power-of-two pixels at subpix_spots, one per channel in turn; the forward's w with
    single power-of-two entries on ORIGINAL tap (dy, dx) = (tap / 3, tap % 3) at the channels the pixels sit in.  A
    slab then holds one tap or none, every output is a sum of a few powers of two within a few binades: exact in fp32,
    in three bf16 and in two fp16 pieces, in any K slices"""
    ups, ext, B, H, W, Cin, Cout = c['ups'], c['ext'], c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    shape = (B, H // 2, W // 2, Cin) if ups == 2 else (B, H + 2 * ext, W + 2 * ext, Cin)
    x = torch.zeros(*shape)
    w = torch.zeros(Cout, Cin, 3, 3) if ups == 2 else torch.zeros(Cin, Cout, 3, 3)
    spots = subpix_spots(c)
    for n, (b, py, px) in enumerate(spots):
        x[b, py, px, (5 * (n + seed)) % Cin] = 2.0 ** ((n + seed) % 5 - 2)
    for n in range(min(len(spots), Cin)):
        ci, co = (5 * (n + seed)) % Cin, (37 * n + seed) % Cout
        v = 2.0 ** (n % 3 - 1) * (-1.0) ** n
        if ups == 2:
            w[co, ci, tap // 3, tap % 3] = v
        else:
            w[ci, co, tap // 3, tap % 3] = v
    return dict(x=x, w=w)


def _sac(route, ext, HW, B, Cin, Cout, **kw):
    c = dict(route=route, ups=3, ext=ext, H=HW[0], W=HW[1], B=B, Cin=Cin, Cout=Cout, splitk=1, skip_g=None,
             pool_sum=False, nomask=False, amax=None, pro=PRO_NONE, alpha=1.0, wfmt='bf3', pair='form', skip=True,
             finish='v4', amax_out=False, cancel=False, relu_like=False, t0=False)
    assert not set(kw) - set(c), kw
    c.update(kw)
    return c


def subpix_arb_id(c):
    d = _sac(c['route'], c['ext'], (c['H'], c['W']), c['B'], c['Cin'], c['Cout'])
    return '%s-u3e%d-%dx%dx%d-%dto%d' % (c['route'], c['ext'], c['B'], c['H'], c['W'], c['Cin'], c['Cout']) + ''.join(
        '-%s%s' % (k, c[k]) for k in sorted(c) if c[k] != d[k])


# the variants the launcher accepts for ups = 3 (it drops the pool: no pool_sum); skips live at the low resolution
SP_ARB_VARIANTS = [dict(), dict(skip_g='same'), dict(skip_g='ups'), dict(nomask=True)]
# unsplit: one image per whole tile of the low-resolution grid (8x16 and up); sliced: the finish kernel, per quad --
# multi-image tiles allowed
SUBPIX_ARB_CASES = [_sac(*base, **dict(kw, **v)) for base, kw in [
    (('F', 0, (16, 32), 2, 32, 64), {}), (('B', 0, (32, 32), 2, 16, 32), {}), (('B', 1, (16, 32), 2, 32, 64), dict(wfmt='bf3w')),
    (('H', 0, (16, 32), 2, 32, 64), dict(amax_out=True)), (('H', 0, (32, 32), 2, 16, 96), dict(amax='true')),
    (('H', 1, (16, 32), 2, 32, 64), {}), (('F', 1, (16, 64), 2, 16, 32), {}),
    (('H', 1, (16, 16), 3, 128, 64), dict(splitk=4)), (('H', 1, (16, 16), 2, 256, 32), dict(splitk=8, amax='true')),
    (('H', 1, (16, 16), 3, 128, 64), dict(splitk=4, finish='scalar')), (('H', 1, (32, 32), 2, 256, 32), dict(splitk=4))]
    for v in SP_ARB_VARIANTS]


def subpix_arb_inputs(g, c):
    """arb_inputs' consumer operands (ax, as, at, the shortcut gradient) at the low resolution of dx, the high-
    resolution gradient x (ext: the frame, row / column H+1 zero) and the forward's w [Cin, Cout, 3, 3]"""
    B, H, W, Cin, Cout, ext = c['B'], c['H'], c['W'], c['Cin'], c['Cout'], c['ext']
    rt = 'C' if c['route'] in 'HP' else 'A'
    i = arb_inputs(g, dict(c, route=rt, H=H // 2, W=W // 2, skip=c['skip_g'], pool_sum=False))
    mg = mags(B).view(B, 1, 1, 1)
    x = torch.randn(B, H + 2 * ext, W + 2 * ext, Cin, generator=g) * mg
    if rt == 'C':
        x[1] = 0.0
        x[0, 0:2, 0:2] *= 2.0 ** -20
    if ext:
        x[:, -1], x[:, :, -1] = 0.0, 0.0
    i['x'] = x
    i['w'] = torch.randn(Cin, Cout, 3, 3, generator=g) / math.sqrt(9 * Cin)
    return i


def subpix_arb_refs(c, i):
    """-> arb_epilogue's dict on da = subpix_map of the gradient in fp64 (H: with subpix_h2_floor) and the route's fp32
    restatement's, ds and dt in the kernels' two stages on the LOW-resolution grid (arb_sums32: an unsplit launch
    leaves one partial per 128-pixel tile, a K-sliced one one per quad)"""
    kw = dict(pool_sum=False, nomask=c['nomask'], skip=i.get('skip'), skip_C=c['Cout'] // 2 if c['skip_g'] else 0,
              skip_ups=c['skip_g'] == 'ups')
    x64, w64 = i['x'].double(), i['w'].double()
    dend = subpix_map(x64.abs(), w64.abs(), 3, c['ext'])
    if c['route'] in 'HP':
        dend = dend + subpix_h2_floor(x64.abs(), i['w'], 3, c['ext'], pw_amax(c, i)[1], subpix_h2_wmax(i['w']))
    r64 = arb_epilogue(subpix_map(x64, w64, 3, c['ext']), dend, i['ax'].double(), i['as'].double(), i['at'].double(), **kw)
    r32 = arb_epilogue(subpix_acc32(c, i), dend.float(), i['ax'], i['as'], i['at'], **kw)
    r32['ds'], r32['dt'] = arb_sums32(r32['g'], i['ax'], c['H'] // 2, c['W'] // 2, False, len(subpix_slices(c)) > 1)
    return r64, r32


def subpix_arb_k(c):
    """arb_k with the conv's count from subpix_k and the sums' over the low-resolution grid of dx"""
    return arb_k(dict(c, H=c['H'] // 2, W=c['W'] // 2, skip=c['skip_g'], oscale=False, bias=False, noise=False,
                      res=None, act=ACT_NONE), subpix_k)


def subpix_arb_bound(c, r64, ax):
    return arb_bound(dict(c, H=c['H'] // 2, W=c['W'] // 2, skip=c['skip_g'], oscale=False, bias=False, noise=False,
                          res=None, act=ACT_NONE), r64, ax, subpix_k)


# ---- generic gather conv (tests/test_gconv_kernels_gpu.py) ----------------------------------------------------------
# gconv_mfma_kernel behind p2l_gconv_fwd (csrc/p2l_alex.hip): every conv of the AlexNet and SqueezeNet LPIPS plans and,
# through transpose_flip packings, their input gradients.  A case is the LAUNCH: x [B, Hi, Wi, Cin] -> y [B, Ho, Wo,
# n_store of Cout], a weight of O x I real channels packed into Cout x Cin.  A `dgrad` case draws the OIHW weight wf [I,
# O, KH, KW] of the stride-1 forward conv it differentiates (padding K - 1 - pad), packs it with transpose_flip and is
# judged against that conv's float64 vjp.
def gconv_out(c):
    return (c['Hi'] + 2 * c['pad'] - c['KH']) // c['stride'] + 1, (c['Wi'] + 2 * c['pad'] - c['KW']) // c['stride'] + 1


def gconv(x, w, stride=1, pad=0, pro_s=None, pro_t=None, bias=None, res=None, mask=None, relu=False, acc=None):
    """the header's contract in the dtype of x: y = [mask > 0] relu?( conv(zero_pad(pro_s x + pro_t)) + bias + res ), x
    [B, Hi, Wi, C], w [N, C, KH, KW], pro_s / pro_t [C], bias [N], res / mask [B, Ho, Wo, N]; Ho = (Hi + 2 pad - KH)
    // stride + 1.  `acc` replaces the conv's sum (a restatement's accumulator, a vjp).  -> dict: y, den = sum over
    taps and channels of (|pro_s| |x| + |pro_t|) |w| + |bias| + |res|, carried through the ReLU and the mask"""
    dt = x.dtype
    w = w.to(dt)
    a, aabs = x, x.abs()
    if pro_s is not None:
        a, aabs = fma(x, pro_s.to(dt), pro_t.to(dt)), x.abs() * pro_s.to(dt).abs() + pro_t.to(dt).abs()
    conv = lambda u, v: F.conv2d(u.permute(0, 3, 1, 2), v, stride=stride, padding=pad).permute(0, 2, 3, 1)
    v = conv(a, w) if acc is None else acc.to(dt)
    den = conv(aabs, w.abs())
    if bias is not None:
        v, den = v + bias.to(dt), den + bias.to(dt).abs()
    if res is not None:
        v, den = v + res.to(dt), den + res.to(dt).abs()
    if relu:
        v = torch.relu(v)
    if mask is not None:
        v = torch.where(mask > 0, v, torch.zeros_like(v))
    return dict(y=v.contiguous(), den=den.contiguous())


def gconv_cols(a, c):
    """im2col of the zero-padded a [B, Hi, Wi, C] with the K axis in the order gconv_mfma_kernel walks it: tap (ky KW
    + kx; pixel (oy stride - pad + ky, ox stride - pad + kx)), 16-channel chunk, then the eight 32x32x2 MFMAs, each
    of which takes channels j and 8 + j -> [B, Ho, Wo, KH KW C]"""
    B, C = a.shape[0], a.shape[-1]
    Ho, Wo = gconv_out(c)
    s, p = c['stride'], c['pad']
    ap = F.pad(a, (0, 0, p, p, p, p))
    taps = torch.stack([ap[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s]
                        for ky in range(c['KH']) for kx in range(c['KW'])], dim=3)              # [B, Ho, Wo, T, C]
    return taps.reshape(B, Ho, Wo, -1, C // 16, 2, 8).transpose(-1, -2).reshape(B, Ho, Wo, -1)


def gconv_wmat(w):
    """[N, C, KH, KW] -> [N, KH KW C] in gconv_cols' order"""
    N, C = w.shape[:2]
    return w.reshape(N, C, -1).permute(0, 2, 1).reshape(N, -1, C // 16, 2, 8).transpose(-1, -2).reshape(N, -1)


def gconv_pack(w, N_pad, K_pad, flip=False, kc=16):
    """host statement of p2l_pack_gconv_weight (and of p2l_pack_conv_weight at taps 25 / 121): OIHW -> [tap][K_pad /
    kc][N_pad][kc], zero fill; flip: the input gradient's weight, N = I, K = O, taps reversed"""
    O, I = w.shape[:2]
    m = w.reshape(O, I, -1)
    if flip:
        m = m.permute(1, 0, 2).flip(2)
    T = m.shape[2]
    full = torch.zeros(N_pad, K_pad, T, dtype=w.dtype)
    full[:m.shape[0], :m.shape[1]] = m
    return full.permute(2, 1, 0).reshape(T, K_pad // kc, kc, N_pad).permute(0, 1, 3, 2).contiguous().reshape(-1)


def _gc(name, K, stride, pad, HW, B, Cin, Cout, **kw):
    KH, KW = K if isinstance(K, tuple) else (K, K)
    c = dict(name=name, KH=KH, KW=KW, stride=stride, pad=pad, Hi=HW[0], Wi=HW[1], B=B, Cin=Cin, Cout=Cout, I=Cin, O=Cout,
             pro=False, bias=False, relu=False, res=False, mask=False, n_store=None, tight=False, aux_tight=False,
             x_off=False, dgrad=False, y_ld=None, col=0)
    assert not set(kw) - set(c), kw
    c.update(kw)
    c['n_store'] = c['O'] if c['n_store'] is None else c['n_store']
    if c['y_ld'] is None:
        c['y_ld'] = c['n_store'] + (0 if c['tight'] else 4)
    return c


def gconv_id(c):
    return c['name']


_FIRST = dict(I=3, pro=True, bias=True, relu=True)
_BR = dict(bias=True, relu=True)
GCONV_CASES = [
    # the strided first convs on an NHWC16 image: three real channels, the scaling layer as the prologue
    _gc('alex0-11x11s4p2-23x19', 11, 4, 2, (23, 19), 2, 16, 64, **_FIRST),               # M = 40: one ragged block
    _gc('alex0-11x11s4p2-22x22', 11, 4, 2, (22, 22), 2, 16, 64, **_FIRST),               # the last row / column unused
    _gc('sqz0-3x3s2p0-9x12', 3, 2, 0, (9, 12), 2, 16, 64, **_FIRST),                     # the last column unused
    # M = 105: two pixel blocks, images straddling a block, three channel blocks
    _gc('alex1-5x5p2-64to192', 5, 1, 2, (7, 5), 3, 64, 192, **_BR),
    _gc('3x3p1-48to128', 3, 1, 1, (5, 7), 2, 48, 128, **_BR),                            # three K chunks
    _gc('3x3p1-192to64', 3, 1, 1, (4, 5), 2, 192, 64, **_BR),
    # squeeze convs: 64 padded outputs, n_store of them stored at pitch n_store / n_store + 4
    _gc('squeeze-1x1-ns16-tight', 1, 1, 0, (5, 7), 2, 64, 64, O=16, tight=True, **_BR),
    _gc('squeeze-1x1-ns16', 1, 1, 0, (5, 7), 2, 64, 64, O=16, **_BR),
    _gc('squeeze-1x1-ns48-tight', 1, 1, 0, (5, 7), 2, 64, 64, O=48, tight=True, **_BR),
    _gc('squeeze-1x1-ns48', 1, 1, 0, (5, 7), 2, 64, 64, O=48, **_BR),
    # block edges
    _gc('M1', 3, 1, 0, (3, 3), 1, 16, 64, bias=True),
    _gc('M64', 3, 1, 1, (8, 8), 1, 16, 64, res=True),
    _gc('M128', 3, 1, 1, (8, 8), 2, 16, 64, mask=True),
    _gc('M63-B3', 3, 1, 1, (3, 7), 3, 16, 64, **_BR),
    _gc('M65', 3, 1, 1, (5, 13), 1, 16, 64, res=True, mask=True, relu=True),
    # descriptors ops.gconv cannot express
    _gc('1x3p1-5x6', (1, 3), 1, 1, (5, 6), 2, 16, 64, pro=True, bias=True),             # rows 0 and Ho - 1: padding alone
    _gc('5x2s2p1-7x4', (5, 2), 2, 1, (7, 4), 2, 16, 64, pro=True, res=True),
    _gc('2x2s3p0-8x7', 2, 3, 0, (8, 7), 2, 32, 64, bias=True, mask=True),
    _gc('1x1p1-4x5', 1, 1, 1, (4, 5), 2, 16, 64, pro=True, bias=True),                   # the border: padding alone
    # input gradients: flipped and transposed packing, pad K - 1 - P, no bias, no ReLU
    _gc('dgrad-e3-64to16-xoff-res-mask', 3, 1, 1, (5, 7), 2, 64, 64, O=16, dgrad=True, x_off=True, res=True, mask=True,
        tight=True, aux_tight=True),
    _gc('dgrad-e3-64to32-xoff-res', 3, 1, 1, (5, 7), 2, 64, 64, O=32, dgrad=True, x_off=True, res=True, aux_tight=True),
    _gc('dgrad-e1-64to48-xoff-mask', 1, 1, 0, (5, 7), 2, 64, 64, O=48, dgrad=True, x_off=True, mask=True,
        aux_tight=True),
    _gc('dgrad-3x3-48to32', 3, 1, 1, (4, 9), 2, 48, 64, O=32, dgrad=True),
    _gc('dgrad-alex1-5x5-192to64', 5, 1, 2, (5, 4), 2, 192, 64, dgrad=True, res=True, mask=True),
]
# the expand pair of a fire: both write one tensor of pitch 128, at columns 0 and 64
GCONV_PAIR = (_gc('expand-1x1-16to64-of128', 1, 1, 0, (5, 7), 2, 16, 64, y_ld=128, col=0, **_BR),
              _gc('expand-3x3p1-16to64-of128', 3, 1, 1, (5, 7), 2, 16, 64, y_ld=128, col=64, **_BR))


def gconv_geometries():
    """the distinct (KH, KW, stride, pad) of the cases"""
    out = []
    for c in GCONV_CASES + list(GCONV_PAIR):
        g = (c['KH'], c['KW'], c['stride'], c['pad'])
        if g not in out:
            out.append(g)
    return out


def gconv_inputs(g, c):
    """the operands of a case on the host, dense fp32: every image at a magnitude of its own (x, the residual); x, pro_s
    and pro_t zero in the channels >= I of a first conv; the mask relu(randn) -- about half of it exact zeros -- with
    a few -0.0 and negative entries; dgrad: wf is the forward conv's weight [I, O, KH, KW], w the launch's equivalent
    [O, I, KH, KW] (transposed, taps reversed)"""
    B, Hi, Wi, Cin, Cout, I, O, ns = c['B'], c['Hi'], c['Wi'], c['Cin'], c['Cout'], c['I'], c['O'], c['n_store']
    KH, KW = c['KH'], c['KW']
    Ho, Wo = gconv_out(c)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    mg = mags(B).view(B, 1, 1, 1)
    i = dict(x=rn(B, Hi, Wi, Cin) * mg)
    i['x'][..., I:] = 0.0
    if c['dgrad']:
        i['wf'] = rn(I, O, KH, KW) / math.sqrt(I * KH * KW)
        i['w'] = i['wf'].permute(1, 0, 2, 3).flip(2, 3).contiguous()
    else:
        i['w'] = rn(O, I, KH, KW) / math.sqrt(I * KH * KW)
    if c['pro']:
        i['pro_s'], i['pro_t'] = 0.5 + torch.rand(Cin, generator=g), 0.3 * rn(Cin)
        i['pro_s'][I:] = 0.0
        i['pro_t'][I:] = 0.0
    if c['bias']:
        i['bias'] = 0.1 * rn(Cout)
    if c['res']:
        i['res'] = rn(B, Ho, Wo, ns) * mg
    if c['mask']:
        m = torch.relu(rn(B, Ho, Wo, ns))
        flat = m.view(-1)
        flat[1::97] = -0.0
        flat[5::89] = -1.5
        i['mask'] = m
    return i


def _gconv_kwargs(c, i, dtype):
    cv = lambda name: i[name].to(dtype) if name in i else None
    return dict(stride=c['stride'], pad=c['pad'], pro_s=cv('pro_s'), pro_t=cv('pro_t'),
                bias=None if cv('bias') is None else cv('bias')[:c['n_store']], res=cv('res'), mask=cv('mask'),
                relu=c['relu'])


def gconv_weight(c, i, dtype=torch.float32):
    """the launch's weight on its stored outputs and all Cin channels, [n_store, Cin, KH, KW]"""
    w = torch.zeros(c['n_store'], c['Cin'], c['KH'], c['KW'], dtype=dtype)
    w[:c['O'], :c['I']] = i['w'].to(dtype)[:c['n_store']]
    return w


def gconv_refs(c, i):
    """-> the float64 reference (gconv's dict; dgrad: the conv's sum is the vjp of the forward conv) and the fp32
    restatement: the same formula with the sum in gconv_mfma_kernel's order, one fp32 product and one fp32 addition
    per column"""
    x64, w64 = i['x'].double(), gconv_weight(c, i, torch.float64)
    acc = None
    if c['dgrad']:
        Ho, Wo = gconv_out(c)
        wf = torch.zeros(c['Cin'], c['n_store'], c['KH'], c['KW'], dtype=torch.float64)
        wf[:c['I'], :c['O']] = i['wf'].double()
        fwd = lambda X: F.conv2d(X, wf, padding=c['KH'] - 1 - c['pad'])
        X0 = torch.zeros(c['B'], c['n_store'], Ho, Wo, dtype=torch.float64)
        acc = vjp(fwd, [X0], x64.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    r64 = gconv(x64, w64, acc=acc, **_gconv_kwargs(c, i, torch.float64))
    x32, w32 = i['x'], gconv_weight(c, i)
    a = fma(x32, i['pro_s'], i['pro_t']) if c['pro'] else x32
    acc32 = acc_fp32(gconv_cols(a, c), gconv_wmat(w32), 1, 16)
    r32 = gconv(x32, w32, acc=acc32, **_gconv_kwargs(c, i, torch.float32))
    return r64, r32


def gconv_k(c):
    """the bar's k of a case, counted from gconv_mfma_kernel's arithmetic like direct_k's route F: one chain per
    output over the KH KW Cin columns (tap-major, 16-channel chunks, a 32x32x2 MFMA per channel pair j, 8 + j), a
    product and an addition each; the prologue's product and sum (2), the bias (1), the residual (1).  ReLU and mask
    select"""
    return 2 * c['KH'] * c['KW'] * c['Cin'] + 2 * c['pro'] + c['bias'] + c['res']


def gconv_spots(c):
    """(image, y, x) of one-hot input pixels: the four corners, an edge pixel of every side, and an interior pixel of
    every residue of (y, x) modulo the stride, on the last image"""
    B, Hi, Wi, s = c['B'], c['Hi'], c['Wi'], c['stride']
    b = B - 1
    sp = [(0, 0, 0), (b, 0, Wi - 1), (b, Hi - 1, 0), (0, Hi - 1, Wi - 1), (b, 0, Wi // 2), (b, Hi // 2, 0),
          (0, Hi - 1, Wi // 2), (b, Hi // 2, Wi - 1)]
    y0, x0 = max(1, Hi // 2 - s // 2), max(1, Wi // 2 - s // 2)
    sp += [(b, min(y0 + ry, Hi - 2), min(x0 + rx, Wi - 2)) for ry in range(s) for rx in range(s)]
    out = []
    for q in sp:
        if q not in out:
            out.append(q)
    return out


def gconv_onehot(c, spot, n=0):
    """exact inputs: x zero but for one power of two at `spot` in channel (5 n) % Cin; w[o, ci, tap] = (1 + (ci % 16) /
    16 + o / 1024) 2^(tap - taps // 2 + ci // 16): a value of its own for every (tap, channel, output), with an
    eleven-bit mantissa.  Every output is ONE product, exact in fp32, and names the tap and the channel that reached
    it"""
    B, Hi, Wi, Cin, Cout = c['B'], c['Hi'], c['Wi'], c['Cin'], c['Cout']
    T = c['KH'] * c['KW']
    assert Cin == 16 and Cout <= 64, 'with a second chunk (tap, chunk 1) would share its value with (tap + 1, chunk 0)'
    x = torch.zeros(B, Hi, Wi, Cin)
    x[spot[0], spot[1], spot[2], (5 * n) % Cin] = 2.0 ** (n % 5 - 2) * (-1.0) ** n
    ci, o, tap = torch.arange(Cin).view(1, Cin, 1), torch.arange(Cout).view(Cout, 1, 1), torch.arange(T).view(1, 1, T)
    w = (1.0 + (ci % 16) / 16.0 + o / 1024.0) * 2.0 ** (tap - T // 2 + ci // 16).double()
    return dict(x=x, w=w.float().view(Cout, Cin, c['KH'], c['KW']))


# ---- thin 3x3 convs: three real channels on one side (tests/test_thin_kernels_gpu.py) ---------------------------------
# Routes of a taps = 9, ups = 0, P2L_WFMT_BF16X3T launch (csrc/p2l_thin.hip): TI conv_thinin_kernel (16 (3 real) -> Cout
# > 32), TO conv_thinout_kernel (Cin > 16 -> 32 (3 real)), B the generic bf16 x 3 kernel on the first image of the same
# buffer -- by P2L_FORM_NO_THIN, by a shape thin_shape does not take, or by the launch's arguments (thin_takes: oscale /
# noise on either shape; a residual, a mask, a pool, y == NULL or a fused backward on a thin-output shape) -- and F
# (P2L_WFMT_F32) the recorded twin.  A case's weight is the [Cout, Cin, 3, 3] correlation kernel the launch applies,
# zero outside its real channels (the packer's zeros); the packer is handed the real channels alone (thin_weight).
WFMT_BF16X3T, FORM_NO_THIN = 4, 16


def thin_real(c):
    """(real input channels, real output channels): 3 of the 16 / 32 the thin side is padded to"""
    return (3 if c['Cin'] == 16 else c['Cin']), (3 if c['Cout'] == 32 else c['Cout'])


def thin_kind(c):
    """thin_shape (csrc/p2l_conv.hip) and p2l_thin_mode restated: 1 thin input, 0 thin output, -1 neither.  (x_ld % 4
    is in thin_shape too, but conv_prepare refuses such a pitch in front of the route: no launch gets that far.)"""
    if c['H'] % 8 or c['W'] % 16 or c['ups']:
        return -1
    if c['Cout'] == 32 and c['Cin'] > 16:
        return 0
    return 1 if c['Cin'] == 16 and c['Cout'] > 32 else -1


def thin_falls_back(c, arb=False):
    """thin_takes restated: a thin shape whose launch the generic kernel runs because of its ARGUMENTS"""
    kind = thin_kind(c)
    if kind < 0:
        return False
    if c.get('oscale') or c.get('noise'):
        return True
    return kind == 0 and bool(arb or c['res'] or c['mask'] or c['pool'] != POOL_NONE or not c['want_y'])


def thin_form(c, route=None):
    """-> (P2LConv.wfmt, P2LConv.form) of a case on `route`: B carries P2L_FORM_NO_THIN only where nothing else keeps
    the launch off the thin kernels"""
    route = route or c['route']
    if route == 'F':
        return 0, 0
    if route == 'B' and thin_kind(c) >= 0 and not thin_falls_back(c):
        return WFMT_BF16X3T, FORM_NO_THIN
    return WFMT_BF16X3T, 0


def _tc(route, HW, B, Cin, Cout, **kw):
    c = _dc(route, HW, B, Cin, Cout)
    c.update(wfmt='bf3t', y_gap=4, x_gap=4)             # y_ld = n_store + y_gap, x_ld = Cin + x_gap
    assert not set(kw) - set(c), kw
    c.update(kw)
    return c


def thin_id(c):
    d = _tc(c['route'], (c['H'], c['W']), c['B'], c['Cin'], c['Cout'])
    return '%s-%dx%dx%d-%dto%d' % (c['route'], c['B'], c['H'], c['W'], c['Cin'], c['Cout']) + ''.join(
        '-%s%s' % (k, c[k]) for k in sorted(c) if c[k] != d[k])


# the smallest shapes at which each form of the two kernels exists (a block is 8 x 16 pixels of one image)
THIN_SHAPES = {
    'i8x16': ((8, 16), 1, 16, 64),         # thin input: one block, all four borders in one patch; two 32-channel tiles
    'i16x32': ((16, 32), 2, 16, 64),       # 2 x 2 tiles per image: seams in both directions, a block range changes image
    'i24x16': ((24, 16), 3, 16, 96),       # three tile rows, nine blocks (xcd_remap: no multiple of 8); three tiles
    'i8x48': ((8, 48), 2, 16, 64),         # three tile columns
    'o8x16': ((8, 16), 1, 32, 32),         # thin output: one block; two 16-channel chunks, the fewest the mode admits
    'o16x32': ((16, 32), 2, 48, 32),       # 2 x 2 tiles; three chunks: the first stage buffer is written a second time
    'o24x16': ((24, 16), 3, 64, 32),       # three tile rows, nine blocks; four chunks
    'o8x48': ((8, 48), 2, 32, 32),         # three tile columns
    'o16x16': ((16, 16), 2, 32, 32),       # two tile rows (run at another x_ld: every multiple of four is a thin pitch)
    'n12x20': ((12, 20), 2, 16, 64),       # not thin: partial tiles in both directions
    'n8x8': ((8, 8), 3, 32, 32),           # not thin: W % 16, two images per tile
    'n32from16': ((16, 16), 2, 16, 32),    # not thin: 32 <- 16, which neither mode admits (and the packer refuses)
}


def _tsh(route, name, **kw):
    HW, B, Cin, Cout = THIN_SHAPES[name]
    return _tc(route, HW, B, Cin, Cout, **kw)


THIN_FWD_CASES = [
    # thin input: the epilogues the conv sections share (EPI[6], oscale + noise: the launch falls back to B) ...
    _tsh('TI', 'i8x16', **EPI[0]), _tsh('TI', 'i16x32', **EPI[1]), _tsh('TI', 'i24x16', **EPI[2]),
    _tsh('TI', 'i8x48', **EPI[3]), _tsh('TI', 'i16x32', **EPI[4]), _tsh('TI', 'i24x16', **EPI[5]),
    _tsh('B', 'i8x48', **EPI[6]),
    # ... the second 32-channel tile storing one float4 group / nothing, the prologues shared by the batch
    _tsh('TI', 'i16x32', n_store=36, pro=PRO_AFFINE_RELU, pro_b=0, bias=True),
    _tsh('TI', 'i8x16', n_store=16, pro=PRO_AFFINE, pro_b=1, act=ACT_LRELU_SQRT2),
    # ... the first VGG / LPIPS conv verbatim: shared scaling layer, bias, ReLU
    _tsh('TI', 'i16x32', pro=PRO_AFFINE, pro_b=0, bias=True, act=ACT_RELU),
    _tsh('B', 'i8x16', noise=True, bias=True), _tsh('B', 'i16x32', oscale=True, pro=PRO_AFFINE_RELU),
    # thin output: conv_to_rgb verbatim (shared affine-ReLU, bias, tanh, n_store = y_ld = 16) and the first VGG conv's
    # input gradient verbatim (64 -> 3 plain, n_store = y_ld = 16); then 2 / 3 / 4 chunks, n_store 4 / 16 / 32, every
    # prologue shared and per image, alpha, every activation
    _tsh('TO', 'o16x32', n_store=16, y_gap=0, pro=PRO_AFFINE_RELU, pro_b=0, bias=True, act=ACT_TANH),
    _tsh('TO', 'o24x16', n_store=16, y_gap=0),
    _tsh('TO', 'o8x16', n_store=4),
    _tsh('TO', 'o8x48', n_store=32, pro=PRO_AFFINE_RELU, pro_b=1, alpha=0.5, act=ACT_RELU),
    _tsh('TO', 'o16x32', n_store=32, pro=PRO_AFFINE, pro_b=0, bias=True, act=ACT_LRELU_SQRT2),
    _tsh('TO', 'o24x16', n_store=4, pro=PRO_AFFINE, pro_b=1, bias=True, alpha=0.7),
    _tsh('TO', 'o16x16', n_store=16, x_gap=8, bias=True, act=ACT_TANH),
    # a thin-output shape whose arguments send it to the generic kernel
    _tsh('B', 'o8x16', n_store=16, res='same', bias=True), _tsh('B', 'o16x32', n_store=16, mask=True, pro=PRO_AFFINE_RELU),
    _tsh('B', 'o24x16', n_store=32, act=ACT_RELU, pool=POOL_MAX), _tsh('B', 'o8x48', n_store=16, pool=POOL_SUM, want_y=False),
    _tsh('B', 'o8x16', n_store=16, oscale=True), _tsh('B', 'o16x32', n_store=16, y_gap=0, noise=True, act=ACT_TANH),
    # shapes thin_shape does not take, on the same format
    _tsh('B', 'n12x20', n_store=36, bias=True, act=ACT_TANH), _tsh('B', 'n8x8', n_store=16, y_gap=0, bias=True),
    _tsh('B', 'n32from16', n_store=16, pro=PRO_AFFINE, bias=True),
]


def _tac(route, HW, B, Cin, Cout, **kw):
    c = _dac(route, HW, B, Cin, Cout)
    c.update(wfmt='bf3t')
    assert not set(kw) - set(c), kw
    c.update(kw)
    return c


def thin_arb_id(c):
    d = _tac(c['route'], (c['H'], c['W']), c['B'], c['Cin'], c['Cout'])
    return '%s-%dx%dx%d-%dto%d' % (c['route'], c['B'], c['H'], c['W'], c['Cin'], c['Cout']) + ''.join(
        '-%s%s' % (k, c[k]) for k in sorted(c) if c[k] != d[k])


# conv_to_rgb's input gradient: dy with three real channels -> ch, the backward of relu(x s + t) fused, with and
# without the maxima of dx; the last: a thin-OUTPUT shape with a fused backward, which the generic kernel runs
THIN_ARB_CASES = [_tac(*base, **dict(kw, **v)) for base, kw in [
    (('TI', (16, 32), 2, 16, 64), {}), (('TI', (24, 16), 3, 16, 96), dict(amax_out=True)),
    (('TI', (8, 48), 2, 16, 64), dict(amax_out=True))] for v in ARB_VARIANTS] + [_tac('B', (16, 32), 2, 48, 32)]


def thin_inputs(g, c):
    """the operands of a forward case, dense fp32, at direct_inputs' magnitudes: every image at a magnitude of its own
    (mags), the first x 1e-6 and the last x 3e4 on top -- x, a per-image t, the residual and the noise alike (a
    prologue shared by the batch keeps `mags` alone: one t has to fit every image).  x and w are zero outside the real
    channels; s and t hold finite junk there, which no route may show.  |t| is 0.6 .. 1.5 of the image's max |x|, positive
    on channel 0 and negative on channel 1: relu(t) > 0 and t != 0, so padding in FRONT of the prologue shows at
    every border pixel under either prologue"""
    B, H, W, Cin, Cout = c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    ri, ro = thin_real(c)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    mg = mags(B)
    if B >= 2 and (c['pro'] == PRO_NONE or c['pro_b']):
        mg = mg.clone()
        mg[0], mg[B - 1] = mg[0] * 1e-6, mg[B - 1] * 3e4
    x = rn(B, H, W, Cin) * mg.view(B, 1, 1, 1)
    x[..., ri:] = 0.0
    w = torch.zeros(Cout, Cin, 3, 3)
    w[:ro, :ri] = rn(ro, ri, 3, 3) / math.sqrt(9 * ri)
    i = dict(x=x, w=w)
    xmax = x.abs().amax(dim=(1, 2, 3))
    out_mag = mg.view(B, 1, 1, 1)
    if c['pro'] != PRO_NONE:
        Bs = B if c['pro_b'] else 1
        s = 0.5 + torch.rand(Bs, Cin, generator=g)
        sign = torch.where(torch.rand(Bs, Cin, generator=g) < 0.5, -1.0, 1.0)
        sign[:, 0], sign[:, 1] = 1.0, -1.0
        unit = xmax[:Bs].view(Bs, 1) if c['pro_b'] else xmax.min()
        t = sign * (2.0 + 3.0 * torch.rand(Bs, Cin, generator=g)) * 0.3 * unit
        s[:, ri:], t[:, ri:] = 7.5, -3.25 * unit * torch.ones(Bs, Cin - ri)
        i['s'], i['t'] = s, t
    if c['bias']:
        i['bias'] = 0.1 * rn(Cout)
    if c['res'] == 'same':
        i['res'] = rn(B, H, W, Cout) * out_mag
    elif c['res'] == 'ups':
        i['res'] = rn(B, H // 2, W // 2, Cout) * out_mag
    if c['mask']:
        i['mask'] = rn(B, H, W, Cout)
    if c['oscale']:
        i['oscale'] = 0.5 + torch.rand(B, Cout, generator=g)
    if c['noise']:
        i['noise'], i['noise_w'] = rn(B, H, W) * out_mag[..., 0], 0.3
    return i


def thin_weight(c, i, flip=False):
    """the OIHW tensor the packer is handed: the real channels alone; flip: the forward conv's tensor whose input
    gradient the launch applies, for the packer's transpose_flip copy"""
    ri, ro = thin_real(c)
    w = i['w'][:ro, :ri]
    return (w.permute(1, 0, 2, 3).flip(2, 3) if flip else w).contiguous()


def thin_cols(a):
    """thin input: the zero-padded a [B, H, W, >= 3] -> [B, H, W, 32], column kk = 3 tap + c holds channel c of pixel
    (y + dy - 1, x + dx - 1), tap = 3 dy + dx; columns 27 .. 31 zero (read off the A-fragment loop)"""
    B, H, W, _ = a.shape
    ap = F.pad(a[..., :3], (0, 0, 1, 1, 1, 1))
    taps = [ap[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]
    return torch.cat(taps + [torch.zeros(B, H, W, 5, dtype=a.dtype)], dim=3)


def thin_wmat(w):
    """[N, >= 3, 3, 3] -> [N, 32] in thin_cols' order"""
    N = w.shape[0]
    return torch.cat([w[:, :3].permute(0, 2, 3, 1).reshape(N, 27), torch.zeros(N, 5, dtype=w.dtype)], dim=1)


def thin_acc32(c, i, route=None, mm=None):
    """the fp32 restatement of a route's accumulator in front of alpha, [B, H, W, Cout], in the order read off the
    kernels (mm: the matrix product in place of acc_bf3 -- tests/test_small_refs.py runs the same walk in fp64).  TI:
    acc_bf3 over the 32 columns kk = 3 tap + c in two 16-steps.  TO: Z = acc_bf3 of every pixel of the zero-padded
    (AFTER the prologue) tensor onto the 27 columns 3 tap + c over 16-channel chunks; an output is the sum of its
    nine Z values in fp32, tap 0 first, starting from 0; channels 3 .. 31 hold 0.  B: direct_acc32 unchanged"""
    route = route or c['route']
    if route == 'B':
        return direct_acc32(c, i, 'B')
    mm = mm or acc_bf3
    a, _ = pw_prologue(i['x'], c['pro'], i.get('s'), i.get('t'))
    B, H, W, Cin = a.shape
    if route == 'TI':
        return mm(thin_cols(a), thin_wmat(i['w']))
    assert route == 'TO'
    wz = i['w'][:3].permute(2, 3, 0, 1).reshape(27, Cin)                     # row 3 tap + c
    z = mm(F.pad(a, (0, 0, 1, 1, 1, 1)), wz)                                  # [B, H + 2, W + 2, 27]
    s = torch.zeros(B, H, W, 3, dtype=a.dtype)
    for tap in range(9):
        dy, dx = tap // 3, tap % 3
        s = s + z[:, dy:dy + H, dx:dx + W, 3 * tap:3 * tap + 3]
    acc = torch.zeros(B, H, W, c['Cout'], dtype=a.dtype)
    acc[..., :3] = s
    return acc


def thin_refs(c, i, route=None, restate=True):
    """-> conv3x3's dict in fp64 on den_d = sum_taps,k |a| |w| through the epilogue, and the route's fp32 restatement's
    (route F or restate = False: None)"""
    route = route or c['route']
    i64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in i.items()}
    r64 = conv3x3(i64['x'], i64['w'], den_w=False, **pw_kwargs(c, i, torch.float64))
    if not restate or route == 'F':
        return r64, None
    return r64, conv3x3(i['x'], i['w'], acc=thin_acc32(c, i, route), den_w=False, **pw_kwargs(c, i, torch.float32))


def thin_k(c, route=None, pooled=False):
    """the bar's k of a thin case, counted like direct_k from the arithmetic of csrc/p2l_thin.hip.  Per column onto an
    accumulator the six cross terms of exact products (6) -- TI: the 32 columns 3 tap + c of its two 16-steps (192);
    TO: the Cin columns of one Z value (6 Cin; the nine Z values of an output each carry that against their own share
    of sum |terms|), then the eight additions of the tap sum (8).  The pieces to 2^-24 relative of either operand (2)
    and the dropped terms <= 2^-23 (2).  Then pw_k's prologue and epilogue terms: the prologue's fma (2); alpha, oscale,
    bias, noise (a product and a sum), residual one each; tanh 2; the leaky ReLU's factor sqrt 2 on everything before
    it and its own rounding; the pool's sum two additions deep.  Route B from the same buffer: direct_k's"""
    route = route or c['route']
    if route == 'B':
        return direct_k(c, 'B', pooled)
    k = (6 * 32 if route == 'TI' else 6 * c['Cin'] + 8) + 4
    k += (2 if c['pro'] != PRO_NONE else 0) + 1 + c['oscale'] + c['bias'] + 2 * c['noise'] + (c['res'] is not None)
    if c['act'] == ACT_TANH:
        k += 2
    if c['act'] == ACT_LRELU_SQRT2:
        k = 1.5 * k + 1
    return k + 2 if pooled and c['pool'] == POOL_SUM else k


def thin_spots(H, W, B):
    """(image, y, x) of the one-hot pixels on a grid of whole 8 x 16 blocks: the corners and edge midpoints, both sides
    of every 8-row and 16-column seam, both sides of every wave boundary inside a block (rows 2 w + 1 | 2 w + 2), both
    sides of a quad boundary in x, the interior, and the first and last pixel of the second image"""
    sp = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1), (0, 0, W // 2), (0, H // 2, 0),
          (0, H - 1, W // 2 - 1), (0, H // 2, W - 1), (0, H // 2, W // 2), (0, 1, 1), (0, H - 2, W - 2)]
    for ys in range(8, H, 8):
        sp += [(0, ys - 1, W // 3), (0, ys, W // 3), (0, ys - 1, W - 1), (0, ys, 0)]
    for xs in range(16, W, 16):
        sp += [(0, H // 3, xs - 1), (0, H // 3, xs), (0, 0, xs - 1), (0, H - 1, xs)]
    for wv in range(3):
        sp += [(0, 2 * wv + 1, 5), (0, 2 * wv + 2, 5)]
    sp += [(0, 3, 7), (0, 3, 8), (0, 4, 9), (0, 4, 10)]
    if B > 1:
        sp += [(1, 0, 0), (1, H - 1, W - 1), (B - 1, 0, W - 1), (B - 1, H - 1, 0)]
    out = []
    for s in sp:
        if s not in out:
            out.append(s)
    return out


def thin_onehot(c, tap, seed=0):
    """exact inputs: x with single power-of-two pixels at thin_spots, in one of the real channels in turn; w with
    single power-of-two entries on `tap` at a few (cout, cin) whose input channels hold pixels.  Every output is a sum
    of a few powers of two within a few binades: exact in fp32 and in three bf16 pieces, through the 27-column K of
    TI and the Z columns and tap sum of TO alike"""
    B, H, W, Cin, Cout = c['B'], c['H'], c['W'], c['Cin'], c['Cout']
    ri, ro = thin_real(c)
    x, w = torch.zeros(B, H, W, Cin), torch.zeros(Cout, Cin, 3, 3)
    spots = thin_spots(H, W, B)
    for n, (b, py, px) in enumerate(spots):
        x[b, py, px, (5 * (n + seed)) % ri] = 2.0 ** ((n + seed) % 5 - 2)
    for n in range(min(len(spots), max(ri, 10))):
        w[(37 * n + seed) % ro, (5 * (n + seed)) % ri, tap // 3, tap % 3] = 2.0 ** (n % 3 - 1) * (-1.0) ** n
    return dict(x=x, w=w)


def thin_arb_inputs(g, c):
    """direct_arb_inputs with dy and w zero outside the real channels (the loss backward's NHWC16 gradient), and a
    dead unit: channel 5 of every image has x s + t < 0 at every pixel (ds = dt = 0 there, exactly, unless nomask)"""
    i = direct_arb_inputs(g, c)
    ri, ro = thin_real(c)
    i['at'][:, 5] = -2.0 * i['as'][:, 5].abs() * i['ax'][..., 5].abs().amax(dim=(1, 2))
    i['x'][..., ri:] = 0.0
    i['w'][ro:] = 0.0
    i['w'][:, ri:] = 0.0
    i['w'] *= math.sqrt(c['Cin'] / float(ri))
    return i


def thin_arb_sums32(g, x, H, W, pool_sum):
    """ds, dt of fp32 g, x [B, Ho, Wo, C] for a thin-input launch on the H x W grid, in the kernel's order.  An item
    is one 2x2 quad (one pixel under pool_sum) and four channels: its pixels onto the running sum in sequence, `sgx +=
    g x` fused, `sg += g`.  Lane 8 q + c4 holds quad q of the wave's two rows: the xor-shuffle over lanes >= 8 (offsets
    8, 16, 32) adds q ^ 1, q ^ 2, q ^ 4; wave w holds rows 2 w, 2 w + 1 of the block and the four waves meet as (0 + 1) +
    (2 + 3); one partial per 8 x 16 block, blocks row-major; then p2l_arb_finish (arb_finish_order32)"""
    def stage(prod):
        if pool_sum:
            q = prod(g, x, None)
        else:
            q = None
            for gq, xq in zip(quads(g), quads(x)):
                q = prod(gq, xq, q)
        Bn, Hq, Wq, Cc = q.shape
        assert (Hq, Wq) == (H // 2, W // 2) and H % 8 == 0 and W % 16 == 0
        t = q.reshape(Bn, Hq // 4, 4, Wq // 8, 8, Cc).permute(0, 1, 3, 2, 4, 5)    # [B, ty, tx, wave, quad, C]
        v = [t[..., j, :] for j in range(8)]
        for o in (1, 2, 4):
            v = [v[j] + v[j ^ o] for j in range(8)]
        wv = v[0]                                                                  # (every lane holds the same sum)
        blk = (wv[..., 0, :] + wv[..., 1, :]) + (wv[..., 2, :] + wv[..., 3, :])
        return arb_finish_order32(blk.reshape(Bn, -1, Cc))
    return (stage(lambda gq, xq, acc: gq * xq if acc is None else fma(gq, xq, acc)),
            stage(lambda gq, xq, acc: gq if acc is None else acc + gq))


def thin_arb_refs(c, i):
    """-> conv3x3_arb's dict in fp64 on the direct denominator and the route's fp32 restatement's, ds and dt in the
    kernel's two stages (TI: thin_arb_sums32; B: arb_sums32, one partial per 128-pixel tile)"""
    kw = dict(pool_sum=c['pool_sum'], nomask=c['nomask'], skip=i.get('skip'), skip_C=c['Cout'] // 2 if c['skip'] else 0,
              skip_ups=c['skip'] == 'ups')
    r64 = conv3x3_arb(i['x'].double(), i['w'].double(), i['ax'].double(), i['as'].double(), i['at'].double(),
                      den_w=False, **kw)
    r32 = conv3x3_arb(i['x'], i['w'], i['ax'], i['as'], i['at'], acc=thin_acc32(c, i), den_w=False, **kw)
    if c['route'] == 'TI':
        r32['ds'], r32['dt'] = thin_arb_sums32(r32['g'], i['ax'], c['H'], c['W'], c['pool_sum'])
    else:
        r32['ds'], r32['dt'] = arb_sums32(r32['g'], i['ax'], c['H'], c['W'], c['pool_sum'], False)
    return r64, r32


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

"""References of tests/test_pixel_sched.py and tests/test_pixel_sched_gpu.py, restated from the definitions (DESIGN.md
section 14) and not from the package's code: the weighted L2 pixel term and its gradient in numpy float64 from the
fp32 operands, and the three learning-rate schedules in Python floats."""
import math

import numpy as np


# ---- the weighted L2 term ------------------------------------------------------------------------------------------
def make_case(Bn, H, W, with_mask, seed):
    """fp32 operands: out / target in (-1, 1), weight in [0, 1] with exact zeros, a 0/1 mask (or None), the weight
    sum as an fp32 INPUT (any positive value would do: the entry points take it as given), mixed-sign gscale"""
    rs = np.random.RandomState(seed)
    out = rs.uniform(-0.999, 0.999, (Bn, 3, H, W)).astype(np.float32)
    target = rs.uniform(-0.999, 0.999, (Bn, 3, H, W)).astype(np.float32)
    weight = rs.uniform(0.0, 1.0, (Bn, 3, H, W)).astype(np.float32)
    weight[rs.uniform(size=weight.shape) < 0.2] = 0.0
    mask = (rs.uniform(size=weight.shape) < 0.7).astype(np.float32) if with_mask else None
    wm = weight.astype(np.float64) * (1.0 if mask is None else mask.astype(np.float64))
    wsum = wm.reshape(Bn, -1).sum(1).astype(np.float32)
    gscale = (rs.uniform(0.5, 1.5, Bn) * np.where(np.arange(Bn) % 2 == 0, 1.0, -1.0)).astype(np.float32)
    assert (wsum > 0).all()
    return out, target, weight, mask, wsum, gscale


def pad16(x, fill=None, rs=None):
    """[B,3,H,W] -> [B,H*W,16]: channels in floats 0..2, the rest `fill` (a number) or draws of `rs`"""
    Bn, _, H, W = x.shape
    if rs is not None:
        o = rs.uniform(-1.0, 1.0, (Bn, H * W, 16)).astype(np.float32)
    else:
        o = np.full((Bn, H * W, 16), 0.0 if fill is None else fill, dtype=np.float32)
    o[:, :, :3] = x.reshape(Bn, 3, H * W).transpose(0, 2, 1)
    return o


def l2_reference(out, target, weight, mask, wsum, gscale):
    """loss [B] and d [B,3,H,W] in float64:  loss = sum w m (t - o)^2 / wsum;  d = (gscale / wsum) 2 w m (o - t)"""
    o, t, w = (a.astype(np.float64) for a in (out, target, weight))
    wm = w if mask is None else w * mask.astype(np.float64)
    Bn = o.shape[0]
    ws = wsum.astype(np.float64)
    loss = (wm * (t - o) ** 2).reshape(Bn, -1).sum(1) / ws
    d = (gscale.astype(np.float64) / ws).reshape(Bn, 1, 1, 1) * 2.0 * wm * (o - t)
    return loss, d


# ---- schedules -----------------------------------------------------------------------------------------------------
def constant(lr):
    return [lr]


def cosine(lr, num_steps, final=0.0):
    if num_steps == 1:
        return [lr]
    return [final + (lr - final) * (0.5 + 0.5 * math.cos(math.pi * i / (num_steps - 1))) for i in range(num_steps)]


def projector_ramp(lr, num_steps, rampdown=0.25, rampup=0.05):
    vals = []
    for i in range(num_steps):
        t = i / num_steps
        r = min(1.0, (1.0 - t) / rampdown)
        r = 0.5 - 0.5 * math.cos(math.pi * r)
        r = r * min(1.0, t / rampup)
        vals.append(lr * r)
    return vals


def fp32(values):
    return np.asarray(values, dtype=np.float64).astype(np.float32)


def ulps(a, b):
    """distance of two fp32 numbers of one sign in units in the last place"""
    a, b = (np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    return np.abs(a - b)

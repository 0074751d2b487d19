"""numpy reference of the StyleGAN2 noise regulariser and the per-layer noise normalisation
(DESIGN.md section 11): the pyramid is pooled in fp32 with the association
((a + b) + (c + d)) * 0.25f, everything else is fp64."""
import numpy as np

SMALL = [4, 8, 8, 16, 16, 32, 32, 64, 64, 128, 128]          # 43 664 floats per candidate
FFHQ1024 = [4] + [r for k in range(3, 11) for r in (2 ** k, 2 ** k)]


def total(sizes):
    return sum(s * s for s in sizes)


def n_levels(sizes):
    return sum(len(_sides(s)) for s in sizes)


def _sides(s):
    out = [s]
    while out[-1] > 8:
        out.append(out[-1] // 2)
    return out


def pyramid(m):
    """fp32 levels of one fp32 map, finest first"""
    m = np.asarray(m, dtype=np.float32)
    levels = [m]
    while levels[-1].shape[0] > 8:
        n = levels[-1]
        p = ((n[0::2, 0::2] + n[0::2, 1::2]) + (n[1::2, 0::2] + n[1::2, 1::2])) * np.float32(0.25)
        assert p.dtype == np.float32
        levels.append(p)
    return levels


def regularize(noises, sizes):
    """noises [B, T] fp32 -> R [B] fp64, corr [B, levels, 2] fp64 (ax, ay; layer-major, finest first),
    grad [B, T] fp64 (dR_b / dnoises_b), prod [B, levels, 2] fp64 (the means of |n[y,x] n[y,x-1]| and
    |n[y,x] n[y-1,x]|: the scale of the summation error of ax and ay)"""
    noises = np.asarray(noises, dtype=np.float32)
    B = noises.shape[0]
    assert noises.shape[1] == total(sizes)
    R = np.zeros(B)
    corr = np.zeros((B, n_levels(sizes), 2))
    prod = np.zeros((B, n_levels(sizes), 2))
    grad = np.zeros(noises.shape)
    for b in range(B):
        off, lev = 0, 0
        for s in sizes:
            g0 = np.zeros((s, s))
            for k, n32 in enumerate(pyramid(noises[b, off:off + s * s].reshape(s, s))):
                n = n32.astype(np.float64)
                left, up = np.roll(n, 1, 1), np.roll(n, 1, 0)        # n[y, x-1], n[y-1, x]
                ax, ay = (n * left).mean(), (n * up).mean()
                corr[b, lev] = ax, ay
                prod[b, lev] = np.abs(n * left).mean(), np.abs(n * up).mean()
                R[b] += ax * ax + ay * ay
                sk = n.shape[0]
                g = (2.0 / (sk * sk)) * (ax * (left + np.roll(n, -1, 1)) + ay * (up + np.roll(n, -1, 0)))
                g0 += np.kron(g, np.ones((2 ** k, 2 ** k))) * 4.0 ** (-k)
                lev += 1
            grad[b, off:off + s * s] = g0.reshape(-1)
            off += s * s
    return R, corr, grad, prod


def normalize(noises, sizes):
    """per candidate and layer (n - mean) / std, unbiased std, fp64 (not rounded)"""
    x = np.asarray(noises, dtype=np.float32).astype(np.float64)
    out = np.empty_like(x)
    off = 0
    for s in sizes:
        n = x[:, off:off + s * s]
        mean = n.mean(1, keepdims=True)
        std = np.sqrt(((n - mean) ** 2).sum(1, keepdims=True) / (s * s - 1))
        out[:, off:off + s * s] = (n - mean) / std
        off += s * s
    return out


def white(B, sizes, seed=0):
    return np.random.RandomState(seed).randn(B, total(sizes)).astype(np.float32)


def planted(row, sizes):
    """0.6 n + 0.8 roll(n, 1, x) per layer: horizontally correlated, R = O(1)"""
    out = np.empty_like(row)
    off = 0
    for s in sizes:
        n = row[off:off + s * s].reshape(s, s)
        out[off:off + s * s] = (np.float32(0.6) * n + np.float32(0.8) * np.roll(n, 1, 1)).reshape(-1)
        off += s * s
    return out

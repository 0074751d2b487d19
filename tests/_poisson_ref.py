"""fp64 reference of the Poisson blend contract, independent of the product code:
the sparse system is assembled with scipy.sparse and solved directly (spsolve), and the output is put
together exactly as the contract says, in float64.  Shared by tests/test_poisson_blend.py and
tests/test_poisson_blend_gpu.py, which also take their inputs and masks from here."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def omega_of(mask):
    """interior Omega of a boolean [H, W] mask: the masked pixels off the outermost one-pixel frame"""
    om = np.asarray(mask, dtype=bool).copy()
    om[0, :] = om[-1, :] = False
    om[:, 0] = om[:, -1] = False
    return om


def poisson_system(target, mask, generated):
    """one image, one channel ([H, W] arrays): (omega, A, b) with A the 5-point Laplacian on Omega (csc, fp64) and
    b the sum of target - generated over each unknown's neighbours outside Omega; unknowns in row-major order"""
    t = np.asarray(target, dtype=np.float64)
    g = np.asarray(generated, dtype=np.float64)
    om = omega_of(mask)
    H, W = om.shape
    n = int(om.sum())
    idx = -np.ones((H, W), dtype=np.int64)
    idx[om] = np.arange(n)
    ys, xs = np.nonzero(om)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [np.full(n, 4.0)]
    b = np.zeros(n)
    d = t - g
    for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):
        qy, qx = ys + dy, xs + dx                 # (Omega is off the frame: every neighbour is a pixel)
        inside = om[qy, qx]
        rows.append(np.nonzero(inside)[0])
        cols.append(idx[qy[inside], qx[inside]])
        vals.append(np.full(int(inside.sum()), -1.0))
        b += np.where(inside, 0.0, d[qy, qx])
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    return om, A, b


def blend_channel(target, mask, generated):
    """-> (out [H, W] float64, omega, A, b) for one image and one channel"""
    t = np.asarray(target, dtype=np.float64)
    g = np.asarray(generated, dtype=np.float64)
    om, A, b = poisson_system(t, mask, g)
    out = t.copy()
    if b.size:
        u = spla.spsolve(A, b) if b.size > 1 else b / A.toarray()[0, 0]
        out[om] = np.clip(g[om] + np.atleast_1d(u), -1.0, 1.0)
    return out, om, A, b


def blend(target, mask, generated):
    """target [1|B, C, H, W], mask [1|B, H, W] bool, generated [B, C, H, W] (numpy) -> (out [B, C, H, W] float64,
    systems) with systems[b][c] = (omega, A, b)"""
    target, mask, generated = np.asarray(target), np.asarray(mask), np.asarray(generated)
    B, C = generated.shape[:2]
    out = np.empty(generated.shape, dtype=np.float64)
    systems = []
    for i in range(B):
        row = []
        for c in range(C):
            o, om, A, b = blend_channel(target[i % target.shape[0], c], mask[i % mask.shape[0]], generated[i, c])
            out[i, c] = o
            row.append((om, A, b))
        systems.append(row)
    return out, systems


# ---- inputs of the tests -------------------------------------------------------------------------------------

def images(seed, B, C, H, W):
    """seeded uniform(-1, 1) noise added to a smooth ramp, halved so that the sum lies in the contract's [-1, 1]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing='ij')
    ramp = 0.6 * yy - 0.4 * xx
    return (0.5 * (ramp[None, None] + rng.uniform(-1.0, 1.0, size=(B, C, H, W)))).astype(np.float32)


def disk(H, W, cy, cx, r):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def blob_with_hole(H, W, S):
    """an ellipse-ish blob about 0.42 * S across inside an S x S corner region (offset from the frame), with a hole"""
    r = 0.21 * S
    cy, cx = 2 + 0.5 * S, 3 + 0.5 * S
    yy, xx = np.mgrid[0:H, 0:W]
    m = ((yy - cy) / r) ** 2 + ((xx - cx) / (1.15 * r)) ** 2 <= 1.0
    return m & ~disk(H, W, cy + 0.2 * r, cx - 0.3 * r, 0.3 * r)


def mask_cases(H, W):
    """name -> boolean [H, W] mask; the shapes the issue lists, scaled to the image"""
    S = {40: 24, 72: 48, 96: 64}[H]
    two = disk(H, W, 0.3 * H, 0.25 * W, 0.15 * H) | disk(H, W, 0.7 * H, 0.75 * W, 0.12 * H)
    off = disk(H, W, 2, 3, 0.3 * H)                       # runs off the top and the left border
    single = np.zeros((H, W), dtype=bool)
    single[H // 3, W // 2] = True
    return {'blob_hole': blob_with_hole(H, W, S), 'two_parts': two, 'full': np.ones((H, W), dtype=bool),
            'off_borders': off, 'single': single, 'empty': np.zeros((H, W), dtype=bool)}

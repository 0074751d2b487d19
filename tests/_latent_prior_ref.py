"""numpy fp64 reference of the whitened latent prior, shared by tests/test_latent_prior.py and
tests/test_latent_prior_gpu.py.

    x = 5 w where p_space and w < 0, else w;  d = x - m;  v[b,l,k] = sum_j A[k,j] d[b,l,j]
    P[b] = sum_l a_l (1 / K) sum_k v[b,l,k]^2
    dw[b,l,j] = gloss[b] slope(w[b,l,j]) (2 a_l / K) sum_k A[k,j] v[b,l,k]

and the same expressions with every term replaced by its absolute value (P_abs, G_abs): what an error of the ORDER of
an fp64 sum is measured against."""
import numpy as np


def slope(w, p_space):
    """5 where p_space and w < 0, else 1 (-0.0 and 0: 1)"""
    return np.where(np.logical_and(bool(p_space), w < 0), 5.0, 1.0)


def reference(w, A, m, a=None, p_space=True, gloss=None):
    """w [B, L, D] (or [B, D]) fp32, A [K, D], m [D], a [L] (None: 1 / L), gloss [B] (None: ones) ->
    dict of P [B], dw [B, L, D], v [B, L, K], P_abs [B], G_abs [B, L, D], all fp64"""
    w = np.asarray(w)
    assert w.dtype == np.float32
    if w.ndim == 2:
        w = w[:, None, :]
    B, L, D = w.shape
    A = np.asarray(A, np.float64)
    m = np.asarray(m, np.float64)
    K = A.shape[0]
    a = np.full(L, 1.0 / L) if a is None else np.asarray(a, np.float64)
    g = np.ones(B) if gloss is None else np.asarray(gloss, np.float64)
    s = slope(w, p_space)
    d = w.astype(np.float64) * s - m
    v = d @ A.T
    P = ((v * v).sum(2) / K * a).sum(1)
    c = g[:, None, None] * s * (2.0 * a / K)[None, :, None]
    dw = c * (v @ A)
    v_abs = np.abs(d) @ np.abs(A).T
    P_abs = ((v_abs * v_abs).sum(2) / K * a).sum(1)
    G_abs = np.abs(c) * (v_abs @ np.abs(A))
    return dict(P=P, dw=dw, v=v, P_abs=P_abs, G_abs=G_abs)


def rounding_bound(x, A, m, a=None):
    """how far P can move when every entry of x [N, D] moves by half an fp32 ulp at most (|dx_j| <= 2^-24 |x_j|):
    e_k = 2^-24 sum_j |A_kj| |x_j| bounds the change of v_k, so |dP| <= (1 / K) sum_k (2 |v_k| e_k + e_k^2).
    [N] fp64 (L = 1)"""
    x = np.asarray(x, np.float64)
    A = np.asarray(A, np.float64)
    v = (x - np.asarray(m, np.float64)) @ A.T
    e = 2.0 ** -24 * (np.abs(x) @ np.abs(A).T)
    return (2.0 * np.abs(v) * e + e * e).sum(1) / A.shape[0]


def make_case(B, L, D, K, seed, mean_scale=0.3):
    """random w (with zeros, -0.0 and both signs), a non-orthogonal basis, a mean and non-uniform layer weights"""
    rs = np.random.RandomState(seed)
    w = rs.randn(B, L, D).astype(np.float32)
    flat = w.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    A = rs.randn(K, D) / np.sqrt(D) * np.exp(rs.randn(K, 1))
    m = mean_scale * rs.randn(D)
    a = rs.rand(L) + 0.25
    a /= a.sum()
    return w, A, m, a

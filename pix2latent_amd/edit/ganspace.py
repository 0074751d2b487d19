"""GANSpace components of BigGAN in z-space (reference pix2latent/edit/ganspace.py) and of StyleGAN2 in W.

The reference draws z, materialises feat = gen_z([z, c]) (N x 32768), runs `torch.pca_lowrank` on it and
fits z ~ x u^T with 100 Adam steps.  gen_z is affine and c is the same in every row, so the centred
features are exactly Zc W_z^T (Zc = z - mean(z), W_z the 32768 x 128 z-block of the gen_z weight): the
bias and the class cancel, and everything the procedure needs follows from two 128 x 128 matrices,
S = Zc^T Zc and G = W_z^T W_z.  Both come from one HIP kernel (`p2l_gram_f64`, the
only O(N) work); the rest is 128 x 128 algebra and the reference's Adam loop on the host in float64.
The PCA is the exact one that `pca_lowrank`'s randomized sketch approximates.

StyleGAN2 (the GANSpace paper's own case; the reference has no editor for it): the principal directions of
w = mapping(z) are the eigenvectors of the 512 x 512 covariance of w.  Its Gram and column sums come from
`p2l_gram_f64_wide`, one call per chunk of samples (`w_covariance`); the eigh is host float64
(`components_from_covariance`).
"""
import ctypes as C

import torch
import torch.nn.functional as F

from .. import _native as N

ADAM_STEPS = 100
ADAM_LR = 1.0
LR_DECAY = 0.98


def gram_f64(x, rows, cols, ld, trans=0):
    """(X^T X [cols, cols], column sums [cols]) of the fp32 panel X inside the device tensor `x`, float64
    device tensors (p2l_gram_f64).  trans=0: element (r, j) at x.flatten()[r * ld + j]; trans=1: at
    x.flatten()[j * ld + r]."""
    if x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError('gram_f64 expects a contiguous fp32 device tensor')
    last = (rows - 1) * ld + cols - 1 if trans == 0 else (cols - 1) * ld + rows - 1
    if (trans not in (0, 1) or rows < 1 or not 1 <= cols <= 128 or ld < (cols if trans == 0 else rows)
            or last >= x.numel()):
        raise ValueError('gram_f64: rows %d, cols %d, ld %d, trans %d do not describe a panel of a tensor of '
                         '%d floats' % (rows, cols, ld, trans, x.numel()))
    L = N.lib()
    nbytes = L.p2l_gram_f64_ws_bytes(rows, cols, trans)
    with torch.cuda.device(x.device):
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
        gram = torch.empty(cols, cols, dtype=torch.float64, device=x.device)
        colsum = torch.empty(cols, dtype=torch.float64, device=x.device)
        N.check(L.p2l_gram_f64(x.data_ptr(), rows, cols, ld, trans, gram.data_ptr(), colsum.data_ptr(),
                               ws.data_ptr(), nbytes, N.stream()), 'p2l_gram_f64')
    return gram, colsum


def orient(m):
    """+1 / -1 per column of m: the sign that makes the column's entry of largest magnitude positive,
    the lowest row index on ties"""
    a = m.abs()
    first = (a == a.max(0, keepdim=True).values).to(torch.int8).argmax(0)     # first maximal row
    s = torch.sign(m[first, torch.arange(m.shape[1])])
    s[s == 0] = 1
    return s


def principal_directions(S, G, num_components):
    """(lam, Y, zx) from S = Zc^T Zc and G = W_z^T W_z (float64):

    with G = L L^T (Cholesky) and eigh(L^T S L) = Y diag(lam) Y^T, the top `num_components` eigenpairs
    in descending order.  The principal directions in feature space are v_k = W_z L^-T y_k (unit norm,
    never formed), the principal coordinates x = Zc L Y, so x^T x = diag(lam) and zx = z^T x = S L Y.
    Each direction is oriented so that the entry of largest magnitude of its column of zx is positive."""
    S = torch.as_tensor(S, dtype=torch.float64).cpu()
    G = torch.as_tensor(G, dtype=torch.float64).cpu()
    L = torch.linalg.cholesky(G)
    lam, Y = torch.linalg.eigh(L.t() @ S @ L)
    lam = lam.flip(0)[:num_components]
    Y = Y.flip(1)[:, :num_components]
    zx = S @ L @ Y
    s = orient(zx)
    return lam, Y * s, zx * s


def components_from_grams(S, G, num_samples, u0=None, num_components=32, method='sgd'):
    """the reference's result, [num_components, d] float64 on the CPU, from S and G (principal_directions).

    'sgd': the reference's loop from u0 [d, num_components]: 100 steps of torch's Adam (lr 1, times 0.98
    after each step) on ((z - x u^T) ** 2).mean(), whose gradient is 2 / (N d) (u x^T x - z^T x).
    'lstsq': the closed-form optimum u = z^T x diag(lam)^-1.  Then, as the reference,
    F.normalize(u, dim=1) (each of the d rows of u, across the components), transposed."""
    d = S.shape[0]
    lam, _, zx = principal_directions(S, G, num_components)
    if method == 'lstsq':
        u = zx / lam
    elif method == 'sgd':
        u = torch.nn.Parameter(torch.as_tensor(u0, dtype=torch.float64).cpu().clone())
        opt = torch.optim.Adam([u], lr=ADAM_LR)
        scale = 2.0 / (num_samples * d)
        for _ in range(ADAM_STEPS):
            opt.zero_grad()
            u.grad = scale * (u.detach() * lam - zx)
            opt.step()
            for param_group in opt.param_groups:
                param_group['lr'] = param_group['lr'] * LR_DECAY
        u = u.detach()
    else:
        raise ValueError('method must be sgd or lstsq, got %r' % (method,))
    return F.normalize(u, p=2, dim=1).t().contiguous()


def genz_gram(model):
    """G = W_z^T W_z of a BigGAN from its packed gen_z weight on the device (float64, CPU), cached on the
    model (it does not depend on the truncation)"""
    G = getattr(model, '_ganspace_gram', None)
    if G is None:
        w = model._genz_wt                       # [z_dim + c_dim][16 * 16 * ch]: rows 0 .. z_dim - 1 are W_z^T
        G, _ = gram_f64(w, w.shape[1], model.z_dim, w.shape[1], trans=1)
        G = model._ganspace_gram = G.cpu()
    return G


def biggan_components(model, class_lbl, num_components=32, num_samples=12800,
                      feat_size=128, method='sgd'):
    """
    Args:
        model: BigGAN model instance
        class_lbl: class index (int) or class embedding (tensor); the components do not depend on it
        num_components: number of PCA components (at most feat_size)
        num_samples: number of samples to estimate PCA
        feat_size: feature size of BigGAN (= model.z_dim)
        method: 'sgd' (the reference's Adam fit) or 'lstsq' (its closed-form optimum)

    Returns [num_components, feat_size] float32 on the model's device: u of the fit z ~ x u^T,
    normalised as the reference does (F.normalize(u, dim=1): each of the feat_size rows across the
    components), transposed.

    z and the initial u are drawn on the CPU generator as the reference draws them, so under one
    torch.manual_seed they are the same tensors.  The PCA is exact (eigh of a 128 x 128 matrix) where the
    reference's pca_lowrank is a randomized sketch.  Sign convention (the reference's is arbitrary): each
    principal direction is flipped so that the entry of largest magnitude of z^T x_k is positive, the
    lowest index on ties.

    GANSpace: Erik Härkönen et al., https://arxiv.org/abs/2004.02546
    """
    assert method in ['sgd', 'lstsq']
    if feat_size != model.z_dim:
        raise ValueError('feat_size %d != model.z_dim %d' % (feat_size, model.z_dim))
    if not 1 <= num_components <= feat_size:
        raise ValueError('num_components must be in [1, %d], got %d' % (feat_size, num_components))
    if not (isinstance(class_lbl, int) or torch.is_tensor(class_lbl)):
        raise TypeError('class_lbl must be an int or a tensor')
    if num_samples < 2:
        raise ValueError('num_samples must be at least 2')
    dev = model._dev
    z = torch.randn(num_samples, feat_size)
    u0 = torch.randn(feat_size, num_components) if method == 'sgd' else None
    zz, zsum = gram_f64(z.to(dev), num_samples, feat_size, feat_size)
    G = genz_gram(model)
    zz, zsum = zz.cpu(), zsum.cpu()
    S = zz - torch.outer(zsum, zsum) / num_samples            # Zc^T Zc = Z^T Z - N mean mean^T
    u = components_from_grams(S, G, num_samples, u0, num_components, method)
    return u.float().to(dev)


# ---------------------------------------------------------------------------------------- StyleGAN2, W space
W_DIM = 512


def gram_f64_wide(x, rows, cols, ld):
    """(X^T X [cols, cols], column sums [cols]) of the fp32 panel X of up to 512 columns inside the device
    tensor `x`, float64 device tensors (p2l_gram_f64_wide): element (r, j) at x.flatten()[r * ld + j]."""
    if x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError('gram_f64_wide expects a contiguous fp32 device tensor')
    if rows < 1 or not 1 <= cols <= W_DIM or ld < cols or (rows - 1) * ld + cols - 1 >= x.numel():
        raise ValueError('gram_f64_wide: rows %d, cols %d, ld %d do not describe a panel of a tensor of '
                         '%d floats' % (rows, cols, ld, x.numel()))
    L = N.lib()
    nbytes = L.p2l_gram_f64_wide_ws_bytes(rows, cols)
    with torch.cuda.device(x.device):
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
        gram = torch.empty(cols, cols, dtype=torch.float64, device=x.device)
        colsum = torch.empty(cols, dtype=torch.float64, device=x.device)
        N.check(L.p2l_gram_f64_wide(x.data_ptr(), rows, cols, ld, gram.data_ptr(), colsum.data_ptr(),
                                    ws.data_ptr(), nbytes, N.stream()), 'p2l_gram_f64_wide')
    return gram, colsum


def _mapped_covariance(model, num_samples, chunk_rows, p_space):
    from ..loss_functions import to_p_space
    if num_samples < 2:
        raise ValueError('num_samples must be at least 2')
    if chunk_rows < 1:
        raise ValueError('chunk_rows must be at least 1')
    dev = model._dev
    G = torch.zeros(W_DIM, W_DIM, dtype=torch.float64, device=dev)
    s = torch.zeros(W_DIM, dtype=torch.float64, device=dev)
    with torch.no_grad():
        for start in range(0, num_samples, chunk_rows):
            n = min(chunk_rows, num_samples - start)
            w = model.mapping(torch.randn(n, W_DIM)).contiguous()
            if p_space:
                w = to_p_space(w)                    # fp32: the samples are these rounded values
            g, cs = gram_f64_wide(w, n, W_DIM, W_DIM)
            G += g
            s += cs
            del w
    G, s = G.cpu(), s.cpu()
    C = (G - torch.outer(s, s) / num_samples) / (num_samples - 1)
    return C, s / num_samples


def w_covariance(model, num_samples, chunk_rows=65536):
    """(C [512, 512], mean [512]) of w = model.mapping(z), z ~ N(0, I), float64 on the CPU.

    z is drawn with torch.randn on the CPU generator in chunks of `chunk_rows` rows, so under one
    torch.manual_seed the draws depend on (num_samples, chunk_rows) only.  Each chunk is mapped on the device
    and goes through p2l_gram_f64_wide once; the Grams and column sums are added in float64 on the device in
    chunk order, C = (G - s s^T / N) / (N - 1).  Only one chunk of w exists at a time."""
    return _mapped_covariance(model, num_samples, chunk_rows, False)


def p_covariance(model, num_samples, chunk_rows=65536):
    """(C [512, 512], mean [512]) of x = to_p_space(model.mapping(z)), float64 on the CPU: the statistics of the
    P_N prior (`LF.LatentPrior.stylegan2`).  The chunk loop and the draws of `w_covariance`;
    the slope-5 map is one fp32 torch op on the chunk (the samples ARE its rounded values), each chunk goes through p2l_gram_f64_wide."""
    return _mapped_covariance(model, num_samples, chunk_rows, True)


def components_from_covariance(C, num_components):
    """(V [K, d] unit rows, stdev [K]) float64 on the CPU: the top K eigenpairs of the covariance C [d, d] in
    descending order, stdev = sqrt(max(lambda, 0)).  Each direction is oriented by `orient`: its entry of
    largest magnitude is positive, the lowest index on ties."""
    C = torch.as_tensor(C, dtype=torch.float64).cpu()
    d = C.shape[0]
    if C.dim() != 2 or C.shape[1] != d:
        raise ValueError('C must be square, got %s' % (tuple(C.shape),))
    if not 1 <= num_components <= d:
        raise ValueError('num_components must be in [1, %d], got %d' % (d, num_components))
    lam, Y = torch.linalg.eigh(C)
    lam = lam.flip(0)[:num_components]
    Y = Y.flip(1)[:, :num_components]
    V = (Y * orient(Y)).t().contiguous()
    return V, lam.clamp(min=0.0).sqrt()


def stylegan2_components(model, num_components=32, num_samples=100000):
    """
    Args:
        model: StyleGAN2 model instance
        num_components: number of PCA components (at most 512)
        num_samples: number of z samples to estimate the covariance of w = mapping(z)

    Returns (components [K, 512], stdev [K], mean [512]) float32 on the model's device: the principal
    directions of W (unit rows), the standard deviation of w along each, and the mean w.  Cached on the model
    per (num_components, num_samples).  z is drawn on the CPU generator (w_covariance).

    GANSpace: Erik Härkönen et al., https://arxiv.org/abs/2004.02546
    """
    if not 1 <= num_components <= W_DIM:
        raise ValueError('num_components must be in [1, %d], got %d' % (W_DIM, num_components))
    if num_samples < 2:
        raise ValueError('num_samples must be at least 2')
    cache = getattr(model, '_ganspace_w', None)
    if cache is None:
        cache = model._ganspace_w = {}
    key = (num_components, num_samples)
    if key not in cache:
        C, mean = w_covariance(model, num_samples)
        V, stdev = components_from_covariance(C, num_components)
        cache[key] = tuple(t.float().to(model._dev) for t in (V, stdev, mean))
    return cache[key]

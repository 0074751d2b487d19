"""The harness of the tests that pin a kernel against a float64 reference of its own (tests/test_small_kernels_gpu.py,
tests/test_loss_kernels_gpu.py, tests/test_glue_kernels_gpu.py and the conv families: tests/test_pw_kernels_gpu.py,
tests/test_wino_kernels_gpu.py, tests/test_direct_kernels_gpu.py, tests/test_subpix_kernels_gpu.py,
tests/test_gconv_kernels_gpu.py, tests/test_thin_kernels_gpu.py; the metric and the bars are described in the
first): seeded draws, guard-banded outputs, the pooled error figures and the file they are recorded in.  A test module
imports the fixtures `N` and `_record_file` by name; `_record_file` writes the rows of the module it was imported
into, to the file that module's environment variable names."""
import functools
import os
import zlib

import pytest
import torch

import _small_refs as R

D64 = torch.float64
U = R.U
G = 256                               # guard floats on either side of every output
SENT = 0x4EADBEEF                     # sentinel bit pattern (a finite float, ~1.46e9)
_RECORDS = []
# test module -> the environment variable that names its record file (profiles/*_kernels_err.txt)
_ERR_FILE_ENV = {'test_small_kernels_gpu': 'P2L_SMALL_ERR_FILE', 'test_loss_kernels_gpu': 'P2L_LOSS_ERR_FILE',
                 'test_glue_kernels_gpu': 'P2L_GLUE_ERR_FILE', 'test_pw_kernels_gpu': 'P2L_PW_ERR_FILE',
                 'test_wino_kernels_gpu': 'P2L_WINO_ERR_FILE', 'test_direct_kernels_gpu': 'P2L_DIRECT_ERR_FILE',
                 'test_subpix_kernels_gpu': 'P2L_SUBPIX_ERR_FILE', 'test_gconv_kernels_gpu': 'P2L_GCONV_ERR_FILE',
                 'test_thin_kernels_gpu': 'P2L_THIN_ERR_FILE'}


class _Native(object):
    """pix2latent_amd._native whose ptr() keeps its tensor alive until the test ends: `N.ptr(x.to(dev))` hands the
    kernel the address of a temporary, which the caching allocator would give to the next temporary at once"""

    def __init__(self, native):
        self._native, self.alive = native, []

    def __getattr__(self, name):
        return getattr(self._native, name)

    def ptr(self, t):
        if t is not None:
            self.alive.append(t)
        return self._native.ptr(t)


@pytest.fixture
def N(dev):
    from pix2latent_amd import _native
    _native.lib()
    n = _Native(_native)
    yield n
    torch.cuda.synchronize()
    del n.alive[:]


_HEAD = ('# |got - fp64| / sum|terms| in units of 2^-24, maxima over >= %d draws: kernel, fp32 torch-CPU restatement, bar '
         '= min(k, 4 x fp32) (tests/%s.py)\n')
_FMT = '%-34s | %-40s | %10.3f %10.3f %8.2f %6.1f\n'


@pytest.fixture(scope='module', autouse=True)
def _record_file(request):
    first = len(_RECORDS)                         # the rows behind this one belong to the modules that ran before
    yield
    name = request.module.__name__.rpartition('.')[2]
    path = os.environ.get(_ERR_FILE_ENV[name])
    mine = _RECORDS[first:]
    if not path or not mine:
        return
    rows = {}
    if os.path.exists(path):                      # a partial run (-k) updates its rows and keeps the others
        for line in open(path):
            cols = line.rstrip('\n').split(' | ')
            if len(cols) == 3 and not line.startswith(('#', 'entry point')):
                rows[(cols[0].strip(), cols[1].strip())] = line
    for r in mine:
        rows[(r[0], r[1])] = _FMT % r
    with open(path, 'w') as f:
        f.write(_HEAD % (SEEDS, name))
        f.write('%-34s | %-40s | %10s %10s %8s %6s\n' % ('entry point : output', 'case', 'kernel', 'fp32', 'bar', 'k'))
        for key in sorted(rows):
            f.write(rows[key])


SEEDS, MAX_SEEDS = 5, 64          # draws per case: at least / at most
MIN_ELEMS, SMALL = 64, 65536      # ... until the smallest held output has seen MIN_ELEMS elements, where no held
                                  # output of the case is larger than SMALL elements per draw (the large cases
                                  # take seconds per draw)
_DRAW = {'seed': 0, 'pool': None}


def seeded(fn):
    """run the test body with SEEDS independent draws of its inputs; `hold` pools the figures, judged at the end"""
    @functools.wraps(fn)
    def wrapper(*args, **kw):
        pool = _DRAW['pool'] = {}
        try:
            sd = 0
            while True:
                _DRAW['seed'] = sd
                fn(*args, **kw)
                if 'N' in kw:
                    torch.cuda.synchronize()
                    del kw['N'].alive[:]
                sd += 1
                seen = [v[3] for v in pool.values()]
                # small cases go on until every held output has MIN_ELEMS elements behind its maxima
                if sd >= SEEDS and (not seen or min(seen) >= MIN_ELEMS or max(seen) > sd * SMALL or sd >= MAX_SEEDS):
                    break
        finally:
            _DRAW['seed'], _DRAW['pool'] = 0, None
        bad = []
        for (name, case), (fk, f32, k, _) in pool.items():
            bar = min(float(k), 4.0 * f32)
            _RECORDS.append((name, case, fk, f32, bar, float(k)))
            print('%s [%s]: kernel %.3f fp32 %.3f bar %.2f (k = %.1f) x 2^-24' % (name, case, fk, f32, bar, k))
            if not fk <= bar:
                bad.append('%s [%s]: %.3f > %.2f x 2^-24 (fp32 restatement %.3f, k = %.1f)' % (name, case, fk, bar, f32, k))
        assert not bad, bad
    return wrapper


def draw():
    """the number of the draw a @seeded test body is in"""
    return _DRAW['seed']


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed + (_DRAW['seed'],)).encode()))


def randn(g, *shape):
    return torch.randn(*shape, generator=g)


class Out(object):
    """an output buffer of n floats between two guard bands, everything pre-filled with the sentinel (or, the n
    floats, with `prefill`)."""

    def __init__(self, dev, n, prefill=None):
        self.n = n
        self.full = torch.full((n + 2 * G,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
        self.t = self.full[G:G + n]
        if prefill is not None:
            self.t.copy_(prefill.reshape(-1).to(dev))

    def cpu(self, *shape):
        """guards bit-unchanged -> the payload on the host"""
        torch.cuda.synchronize()
        bits = self.full.view(torch.int32)
        assert bool((bits[:G] == SENT).all()) and bool((bits[G + self.n:] == SENT).all()), 'guard band written'
        return self.t.cpu().view(*shape) if shape else self.t.cpu()


def is_sentinel(t):
    return bool((t.contiguous().view(torch.int32) == SENT).all())


def fig(got, ref64, denom64):
    """max |got - ref| / denom in units of 2^-24; where denom == 0 the result must be exact"""
    err = (got.to(D64) - ref64).abs()
    zero = denom64 == 0
    assert bool((err[zero] == 0).all()), 'non-zero result where every term is zero'
    return float((err[~zero] / denom64[~zero]).max().item() / U) if bool((~zero).any()) else 0.0


def hold(name, case, got, ref64, denom64, got32, k):
    """pool this draw's figures of the kernel and of the fp32 restatement (judged by `seeded` over all draws)"""
    fk, f32 = fig(got, ref64, denom64), fig(got32, ref64, denom64)
    pool = _DRAW['pool']
    assert pool is not None, 'hold() outside a @seeded test'
    old = pool.get((name, case), (0.0, 0.0, k, 0))
    pool[(name, case)] = (max(old[0], fk), max(old[1], f32), k, old[3] + got.numel())


def hold_k(name, case, got, ref64, denom64, k):
    """pool a figure that is held to its counted k alone -- no restatement stands behind it (recorded with fp32 = inf)"""
    f = fig(got, ref64, denom64)
    pool = _DRAW['pool']
    assert pool is not None, 'hold_k() outside a @seeded test'
    old = pool.get((name, case), (0.0, float('inf'), k, 0))
    pool[(name, case)] = (max(old[0], f), float('inf'), k, old[3] + got.numel())


def note(name, case, got, ref64, denom64):
    """pool a figure that is recorded and not judged (bar and k = inf)"""
    hold_k(name, case, got, ref64, denom64, float('inf'))


def d64(*ts):
    return [None if t is None else t.to(D64) for t in ts]

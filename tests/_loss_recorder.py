"""A recording stand-in for libp2l_hip behind pix2latent_amd/loss_functions.py: the native image losses run on CPU
tensors, nothing is launched, and every library call is kept as one line of text.  Shared by
tests/test_loss_forms.py and tools/loss_trace.py; it hooks the LIBRARY (`_native._lib`), not the autograd
Functions, so it says the same about any host-side arrangement of the same calls.

    with recording() as rec:
        loss_fn = LF.ProjectionLoss(lpips_net='vgg')      # (the LPIPS parameter object is a stub)
        rec.watch(loss_fn._engine, output=out, target=target)
        loss_fn(out, target, weight).sum().backward()
    rec.calls        # [Call(name, args, text)]

Pure size queries (`*_ws_bytes`, `*_cache_floats`, `p2l_l1_loss_nblk`, `p2l_l2_loss_nblk`) go through to the real
library; everything else is recorded with its scalar arguments and answers 0.  A pointer is printed as the ROLE of
the buffer it points into -- a lane's scratch (`lane0.img16`), a cache slot (`slot1.wsum`), a pooled entry
(`pooled1.target`), a tensor the caller named with `watch`, the bound copy the engine keeps of one (`bound.weight`)
-- slots, pooled entries and unnamed buffers (`t3`) numbered by first appearance; NULL as NULL.  Unnamed buffers are
the per-call temporaries (loss, l1, lp, the gradient): every tensor `torch.empty` / `empty_like` makes is kept alive
until `step_end()`, so that no two of one step share an address, and `step_end()` forgets their addresses.
`_CacheSlot.used()` -- the reader event a second lane leaves on a slot, no library call -- is kept in the same list
as `slot.used(slotN)`."""
import collections
import contextlib
import ctypes as C
import types

import torch

import pix2latent_amd.loss_functions as LF
from pix2latent_amd import _native as N

STREAM = 0x57524d00           # what the stubbed N.stream() hands out
PASS_THROUGH = ('_ws_bytes', '_cache_floats', 'p2l_l1_loss_nblk', 'p2l_l2_loss_nblk', 'p2l_version', 'p2l_strerror',
                'p2l_last_hip_error')
LANE_FIELDS = ('ws', 'img16', 'dimg16', 'full16', 'dfull16', 'l1_part', 'pix_part')
Call = collections.namedtuple('Call', 'name args text')


def _span(t):
    return t.data_ptr(), t.data_ptr() + max(1, t.numel() * t.element_size())


class Recorder(object):
    def __init__(self, real):
        self.real, self.calls = real, []
        self._fns, self._keep = {}, []
        self._engines, self._named = [], {}
        self._ids = {}               # ('slot' | 'pooled' | 't', key) -> number, by first appearance
        self._temps = {}

    # ---- the library's face ----
    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        if name.endswith(PASS_THROUGH[:2]) or name in PASS_THROUGH:
            return getattr(self.real, name)
        if name not in self._fns:
            if not hasattr(self.real, name):
                raise AttributeError(name)

            def fn(*args, _name=name):
                shown = [self.show(a) for a in args]
                self.calls.append(Call(_name, args, '%s(%s)' % (_name, ', '.join(shown))))
                return 0
            self._fns[name] = fn
        return self._fns[name]

    # ---- naming ----
    def watch(self, engine=None, **tensors):
        """name the tensors a case hands in, and the engine whose scratch, slots and memos give the other roles"""
        if engine is not None and all(e is not engine for e in self._engines):
            self._engines.append(engine)
        self._named.update({k: v for k, v in tensors.items() if v is not None})

    def step_end(self):
        self._keep, self._temps = [], {}

    def reset(self):
        """a new case: calls, names and numbering start again"""
        self.step_end()
        self.calls, self._engines, self._named, self._ids = [], [], {}, {}

    def _number(self, kind, key):
        n = self._ids.get((kind, key))
        if n is None:
            n = self._ids[(kind, key)] = 1 + sum(1 for k in self._ids if k[0] == kind)
        return '%s%d' % (kind, n)

    def _regions(self):
        for name, t in self._named.items():
            yield _span(t), name
        for eng in self._engines:
            for k in sorted(eng._scratch.lanes):
                s = eng._scratch.lanes[k]
                for f in LANE_FIELDS:
                    if getattr(s, f, None) is not None:
                        yield _span(getattr(s, f)), 'lane%d.%s' % (k, f)
            for slot in eng.slots.values():
                tag = self._number('slot', id(slot))
                a = C.addressof(slot.desc)
                yield (a, a + C.sizeof(slot.desc)), tag + '.desc'
                yield (slot.desc.wsum, slot.desc.wsum + 4 * slot.B), tag + '.wsum'
                yield _span(slot.buf), tag + '.buf'
            for ent in eng._pooled.values():
                tag = self._number('pooled', id(ent))
                for f in ('target', 'weight', 'wsum'):
                    if getattr(ent, f) is not None:
                        yield _span(getattr(ent, f)), '%s.%s' % (tag, f)
            for name, memo in eng._memo.items():
                yield _span(memo[1]), 'bound.' + name
            if getattr(eng.vgg, 'desc', None) is not None:
                a = C.addressof(eng.vgg.desc)
                yield (a, a + C.sizeof(eng.vgg.desc)), 'net'

    def role(self, addr):
        if not addr:
            return 'NULL'
        if addr == STREAM:
            return 'stream'
        for (lo, hi), name in self._regions():
            if lo <= addr < hi:
                return name if addr == lo else '%s+%d' % (name, addr - lo)
        if addr not in self._temps:
            self._temps[addr] = self._number('t', object())
        return self._temps[addr]

    def show(self, a):
        if a is None:
            return 'NULL'
        if isinstance(a, C.c_void_p):
            return self.role(a.value)
        if isinstance(a, C.c_float):
            return '%.9g' % a.value
        if isinstance(a, (C.c_size_t, C.c_int, C.c_int64)):
            return str(a.value)
        if isinstance(a, (int, float)):
            return repr(a)
        if hasattr(a, '_obj'):                          # C.byref(struct)
            return self.role(C.addressof(a._obj))
        return type(a).__name__

    # ---- reading a trace ----
    def names(self, since=0):
        return [c.name for c in self.calls[since:]]

    def scalar(self, call, index):
        a = call.args[index]
        return getattr(a, 'value', a)


def _stub_params(net, weights=None, device=None):
    net = 'vgg' if net in ('vgg16',) else net
    cls = LF._LPIPS_NETS[net][0]
    return types.SimpleNamespace(prefix=cls.prefix, desc=cls.desc_cls())


@contextlib.contextmanager
def recording():
    """-> Recorder, installed as THE library until the block ends.  Inside: `N.stream()` is a constant, the LPIPS
    parameter object is `prefix` + a zeroed descriptor, the losses take CPU tensors on their native routes, and
    torch.cuda reports no device (no stream, no event: the same trace on a machine with a GPU)."""
    rec = Recorder(N.lib())
    saved = (N._lib, N.stream, LF._vgg_params, LF._native_ok, torch.cuda.is_available, torch.empty, torch.empty_like,
             LF._CacheSlot.used)

    def used(slot):
        rec.calls.append(Call('slot.used', (), 'slot.used(%s)' % rec._number('slot', id(slot))))
        return saved[7](slot)

    def kept(make):
        def f(*a, **kw):
            t = make(*a, **kw)
            rec._keep.append(t)
            return t
        return f
    try:
        N._lib = rec
        N.stream = lambda: C.c_void_p(STREAM)
        LF._vgg_params = _stub_params
        LF._native_ok = lambda output, target, weight: (output.dim() == 4 and output.size(1) == 3 and
                                                         target is not None)
        torch.cuda.is_available = lambda: False
        torch.empty, torch.empty_like = kept(saved[5]), kept(saved[6])
        LF._CacheSlot.used = used
        yield rec
    finally:
        (N._lib, N.stream, LF._vgg_params, LF._native_ok, torch.cuda.is_available, torch.empty,
         torch.empty_like, LF._CacheSlot.used) = saved

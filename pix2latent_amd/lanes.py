"""Execution lanes: the reference chunks of one step on separate HIP streams.

The reference evaluates a population chunk by chunk (`max_batch_size` = 9 of 18; reference
pix2latent/optimizer/closure.py:23-27), each chunk forward -> loss -> backward -> Adam on its own rows:
the chunks are independent.  On an MI355X one chunk of 9 leaves the 4^2 ... 16^2 layers of the generator
and the loss network latency-bound (a few dozen blocks on 256 CUs), and so does one pass of 18; two chunks
in flight on two streams fill each other's gaps: 16.4 -> 15.2 ms per step of 18 (tools/two_stream_probe.py).
Such a step is replayed as ONE HIP graph with two branches by default (optimizer/base_optimizer.py): 2 launches
instead of 520 per step on the host.
Results are the same bits as one stream (a candidate's arithmetic does not depend on what runs beside it).

A lane = a stream + its own workspaces in every object that keeps device scratch (the generator's arena
and image staging, the loss's arena); objects advertise `lanes_ok = True` and keep that scratch in a
`Scratch` (`_scratch`).  Lane 0 on the caller's stream is the only one unless closure.step opens more.
"""
import os
import threading

import torch

_tls = threading.local()         # the current lane is per host thread: two threads may each drive an optimizer
_side = {}


def current():
    return getattr(_tls, 'lane', 0)


class use(object):
    """`with use(k):` -- workspaces of lane k for this thread (no stream switch: closure._LaneCtx pairs it with
    `torch.cuda.stream`).  autograd runs a backward on its own thread: the Functions remember the forward's
    lane and re-enter it there (model/biggan.py `_BigGANFn.backward`)."""

    def __init__(self, lane):
        self.lane = lane

    def __enter__(self):
        self.prev = current()
        _tls.lane = self.lane
        return self

    def __exit__(self, *a):
        _tls.lane = self.prev


class LaneScratch(object):
    """the device scratch of one execution lane: arena, image staging, forward ticket"""

    def __init__(self):
        self.ws, self.ws_bytes, self.cap = None, 0, -1
        self.img16 = self.dimg16 = None
        self.ticket, self.last_B = 0, 0
        # a loss with `lpips_size`: its arena and staging above are at the pooled size, the L1 term's are here
        self.full16 = self.dfull16 = self.l1_part = None
        self.full_cap, self.full_res = -1, None
        # the block partial sums of an L2 pixel term beside a full-resolution LPIPS term
        self.pix_part = None


class Scratch(object):
    """The per-lane device scratch of ONE object (a generator, a loss engine): `lanes` (lane -> LaneScratch)
    and `generation`.  The rule it keeps: whatever frees or moves a lane's buffers bumps `generation` --
    captured HIP graphs hold the old pointers, and the graph cache keys on it (base_optimizer._graph_key)."""

    def __init__(self):
        self.lanes, self.generation = {}, 0

    def here(self):
        """the record of the current lane"""
        k = current()
        s = self.lanes.get(k)
        if s is None:
            s = self.lanes[k] = LaneScratch()
        return s

    def grow(self, B, H, W, sizing, device):
        """the current lane's record with room for B images of H x W: arena of `sizing(B, H, W)` bytes and the two
        16-channel staging tensors, re-allocated only when B exceeds what the lane holds (sized for the LARGEST
        batch seen: a ragged last chunk must not re-allocate GBs twice per step).  A failed sizing or
        allocation leaves the record as it was."""
        s = self.here()
        if B > s.cap:
            nbytes = sizing(B, H, W)
            ws = torch.empty(nbytes // 4, device=device, dtype=torch.float32)
            img16 = torch.empty(B, H, W, 16, device=device, dtype=torch.float32)
            dimg16 = torch.empty(B, H, W, 16, device=device, dtype=torch.float32)
            s.ws, s.ws_bytes, s.cap, s.img16, s.dimg16 = ws, nbytes, B, img16, dimg16
            self.generation += 1
        return s

    def grow_full(self, B, H, W, n_part, device):
        """the current lane's record with the full-resolution staging of a pooled loss for B images of H x W (the
        two 16-channel tensors and B * n_part floats of L1 partial sums), kept in the SAME record as the pooled-size
        scratch: `drop_side` and `clear` free both, and a re-allocation bumps the one `generation`"""
        s = self.here()
        if B > s.full_cap or s.full_res != (H, W):
            full16 = torch.empty(B, H, W, 16, device=device, dtype=torch.float32)
            dfull16 = torch.empty(B, H, W, 16, device=device, dtype=torch.float32)
            part = torch.empty(B * n_part, device=device, dtype=torch.float32)
            s.full16, s.dfull16, s.l1_part, s.full_cap, s.full_res = full16, dfull16, part, B, (H, W)
            self.generation += 1
        return s

    def grow_part(self, n_floats, device):
        """the current lane's record with `pix_part` of at least n_floats (the block partial sums of the L2 pixel
        term); a re-allocation bumps `generation`"""
        s = self.here()
        if s.pix_part is None or s.pix_part.numel() < n_floats:
            s.pix_part = torch.empty(n_floats, device=device, dtype=torch.float32)
            self.generation += 1
        return s

    def drop_side(self):
        """free what lanes > 0 hold"""
        for k in [k for k in self.lanes if k != 0]:
            del self.lanes[k]
        self.generation += 1

    def clear(self):
        """free every lane (the loss engine at a new resolution)"""
        self.lanes.clear()
        self.generation += 1

    def stamp(self):
        """called by a forward that has filled the current lane: -> (lane, ticket) for its backward"""
        s = self.here()
        s.ticket += 1
        return current(), s.ticket

    def stale(self, stamp):
        """has a later forward (or a drop) taken the scratch of the stamp's lane since?"""
        s = self.lanes.get(stamp[0])
        return s is None or s.ticket != stamp[1]


def env_int(name, default):
    """$name as an integer; unset, empty or not a number = default"""
    try:
        return int(os.environ.get(name, '') or default)
    except ValueError:
        return default


_gave_up = []


def give_up(reason):
    """no more lanes in this process (the second set of workspaces did not fit: closure._step_fused)"""
    if not _gave_up:
        import warnings
        warnings.warn('execution lanes switched off for this process: %s' % reason)
    _gave_up.append(reason)


def drop_side_scratch(*objs):
    """free what lanes > 0 allocated in the objects that keep per-lane scratch (retires their captured graphs)"""
    for o in objs:
        if isinstance(getattr(o, '_scratch', None), Scratch):
            o._scratch.drop_side()


def wanted(n_chunks, *objs):
    """number of lanes for a step of n_chunks reference chunks over objs (model, loss): $P2L_STREAMS
    (default 2; 1 = off) when every object has per-lane workspaces.  Also while a HIP graph is being captured:
    the side streams fork from the capturing stream and join it again, the graph gets two branches and the
    replay runs them side by side (measured: 15.3 ms replayed, 15.5 eager, 19.6 replayed on one stream)"""
    want = env_int('P2L_STREAMS', 2)
    if n_chunks < 2 or want < 2 or _gave_up or not torch.cuda.is_available():
        return 1
    if not all(getattr(o, 'lanes_ok', False) for o in objs):
        return 1
    return min(want, n_chunks)


SUB_MIN = 7


def sub_wanted(n, *objs):
    """a step that is ONE chunk of n candidates -- a rank of a 2-GPU run holds 9, the GradientOptimizer example
    8 -- cut in two for two lanes.  The gradient factor stays the one of the whole chunk (closure._step_fused
    passes it explicitly), so the bits do not change (tests/test_sublanes_gpu.py).  Measured
    (profiles/round5_sublanes.txt): 9 candidates 9.92 -> 9.27 ms eager, 9.07 replayed as one graph; 5: 6.57 ->
    6.41; 3 and 2: 2 % SLOWER (there the step is one chain of tiny dependent launches, and two chains side by
    side are as long as one) -- hence from SUB_MIN candidates up.  $P2L_SUBLANES: 0 = never, 1 = from 2 up."""
    mode = os.environ.get('P2L_SUBLANES', '')
    if mode == '0' or n < 2 or (mode != '1' and n < SUB_MIN):
        return False
    return wanted(2, *objs) == 2


def side_streams(device, n):
    """n streams of `device`, made once per process"""
    key = str(device)
    have = _side.setdefault(key, [])
    while len(have) < n:
        have.append(torch.cuda.Stream(device=device))
    return have[:n]

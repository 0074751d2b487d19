"""Host logic of the execution lanes (pix2latent_amd/lanes.py): which lane a thread is in, when a step may
open a second one.  (The device side -- same bits on two streams -- is tests/test_lanes_gpu.py.)"""
import threading

from pix2latent_amd import lanes


class _Ok(object):
    lanes_ok = True


def test_lane_is_per_thread_and_nests():
    assert lanes.current() == 0
    seen = {}

    def other():
        seen['start'] = lanes.current()
        with lanes.use(1):
            seen['inside'] = lanes.current()
        seen['after'] = lanes.current()

    with lanes.use(1):
        assert lanes.current() == 1
        with lanes.use(0):
            assert lanes.current() == 0
        assert lanes.current() == 1
        t = threading.Thread(target=other)
        t.start()
        t.join()
    assert lanes.current() == 0
    assert seen == {'start': 0, 'inside': 1, 'after': 0}


def test_no_second_lane_without_a_device_or_per_lane_scratch(monkeypatch):
    import torch
    monkeypatch.delenv('P2L_STREAMS', raising=False)
    monkeypatch.delenv('P2L_SUBLANES', raising=False)
    if not torch.cuda.is_available():
        assert lanes.wanted(2, _Ok(), _Ok()) == 1          # (CPU tensors: the reference's own sequence)
        assert not lanes.sub_wanted(9, _Ok(), _Ok())
    assert lanes.wanted(2, _Ok(), object()) == 1
    assert lanes.wanted(1, _Ok(), _Ok()) == 1
    monkeypatch.setenv('P2L_STREAMS', '1')
    assert lanes.wanted(4, _Ok(), _Ok()) == 1
    monkeypatch.setenv('P2L_STREAMS', 'not a number')
    assert lanes.wanted(1, _Ok()) == 1


def test_graph_default_follows_the_lanes(monkeypatch):
    """which steps are replayed as a HIP graph unless told otherwise (base_optimizer._graph_default): <= 6 local
    candidates; two reference chunks or more on lanes; one chunk of 7 ... max_batch_size candidates in two
    sub-lanes; NOT an execution pass above the reference chunk, not when P2L_STREAMS=1 leaves one stream."""
    import torch
    from pix2latent_amd.optimizer.base_optimizer import _BaseOptimizer

    class Shard(object):
        enabled = False

    class Stub(object):
        _graph_default = _BaseOptimizer._graph_default
        max_batch_size, exec_batch_size, shard = 9, None, Shard()
        model, loss_fn = _Ok(), type('L', (), {'_engine': _Ok()})()

    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.delenv('P2L_STREAMS', raising=False)
    monkeypatch.delenv('P2L_SUBLANES', raising=False)
    o = Stub()
    assert o._graph_default(3) and o._graph_default(6)
    assert o._graph_default(18)                       # 9 + 9 on two lanes
    assert o._graph_default(9) and o._graph_default(8) and o._graph_default(7)      # one chunk, two sub-lanes
    o.exec_batch_size = 'all'
    assert not o._graph_default(18)                   # one pass of 18 on one stream: eager, as before
    o.exec_batch_size = 18
    assert not o._graph_default(18)
    o.exec_batch_size = None
    monkeypatch.setenv('P2L_STREAMS', '1')
    assert not o._graph_default(18) and not o._graph_default(9) and o._graph_default(6)
    monkeypatch.delenv('P2L_STREAMS')
    o.model = object()                                # no per-lane scratch: no lanes, no graph above 6
    assert not o._graph_default(18) and not o._graph_default(9)
    o.model = _Ok()
    o.shard = type('S', (), {'enabled': True})()
    assert o._graph_default(9)                        # a rank's block of 9: sub-lanes, one graph
    assert not o._graph_default(16)                   # a rank's block of two chunks: lanes, eager


# -- lanes.Scratch: the per-lane device scratch of one object, on CPU tensors ------------------------------------
def _sizing(B, H, W):
    return 64 * B * H * W


def _grow(sc, B, sizing=_sizing):
    return sc.grow(B, 4, 5, sizing, 'cpu')


def test_scratch_lanes_are_separate_and_grow_only():
    sc = lanes.Scratch()
    assert sc.lanes == {} and sc.generation == 0
    a = _grow(sc, 3)
    assert sorted(sc.lanes) == [0] and sc.here() is a and sc.generation == 1
    assert (a.cap, a.ws_bytes, a.ws.numel()) == (3, _sizing(3, 4, 5), _sizing(3, 4, 5) // 4)
    assert a.img16.shape == a.dimg16.shape == (3, 4, 5, 16) and a.img16.data_ptr() != a.dimg16.data_ptr()
    held = (a.ws, a.img16, a.dimg16)
    ptr = a.ws.data_ptr()
    assert _grow(sc, 2) is a and _grow(sc, 3) is a          # a smaller or equal request: nothing moves
    assert a.ws.data_ptr() == ptr and a.cap == 3 and sc.generation == 1
    with lanes.use(1):
        b = _grow(sc, 2)
        assert b is not a and sc.here() is b and sc.generation == 2
        _grow(sc, 5)                                        # lane 1 grows: once per allocation, lane 0 untouched
        assert b.cap == 5 and b.img16.shape == (5, 4, 5, 16) and sc.generation == 3
        seen = []
        t = threading.Thread(target=lambda: seen.append(sc.here()))     # (another thread is in lane 0)
        t.start()
        t.join()
        assert seen == [a]
    assert sorted(sc.lanes) == [0, 1] and sc.here() is a
    assert all(x is y for x, y in zip((a.ws, a.img16, a.dimg16), held))
    assert a.ws.data_ptr() == ptr and a.cap == 3
    _grow(sc, 4)
    assert a.cap == 4 and a.ws.numel() == _sizing(4, 4, 5) // 4 and sc.generation == 4


def test_scratch_failed_allocation_does_not_bump(monkeypatch):
    import pytest
    import torch
    sc = lanes.Scratch()
    a = _grow(sc, 3)
    before = (a.ws, a.ws_bytes, a.cap, a.img16, a.dimg16, a.ticket, sc.generation)

    def rejecting(B, H, W):
        raise RuntimeError('sizing rejected batch %d' % B)
    with pytest.raises(RuntimeError, match='sizing rejected batch 4'):
        _grow(sc, 4, rejecting)
    real, calls = torch.empty, []

    def third_allocation_fails(*a_, **kw):
        calls.append(a_)
        if len(calls) == 3:
            raise MemoryError('injected')
        return real(*a_, **kw)
    monkeypatch.setattr(torch, 'empty', third_allocation_fails)
    with pytest.raises(MemoryError):
        _grow(sc, 4)
    monkeypatch.undo()
    assert len(calls) == 3                                   # arena, img16, then dimg16 failed
    after = (a.ws, a.ws_bytes, a.cap, a.img16, a.dimg16, a.ticket, sc.generation)
    assert all(x is y for x, y in zip(before, after)) and sc.here() is a
    with lanes.use(1):                                       # a lane whose first allocation fails holds nothing
        with pytest.raises(RuntimeError):
            _grow(sc, 2, rejecting)
        assert sc.here().ws is None and sc.here().cap == -1
    assert sc.generation == before[-1]


def test_scratch_drop_and_clear_bump():
    sc = lanes.Scratch()
    a = _grow(sc, 3)
    for k in (1, 2):
        with lanes.use(k):
            _grow(sc, 3)
    g = sc.generation
    sc.drop_side()
    assert sorted(sc.lanes) == [0] and sc.lanes[0] is a and a.cap == 3 and sc.generation == g + 1
    sc.drop_side()                                           # nothing to drop: lane 0 unchanged, still a bump
    assert sorted(sc.lanes) == [0] and sc.lanes[0] is a and sc.generation == g + 2
    held = sc.lanes                                          # (what `owner._lanes` hands out stays the owner's dict)
    sc.clear()
    assert sc.lanes == {} and sc.lanes is held and sc.generation == g + 3
    assert _grow(sc, 1) is not a and sc.generation == g + 4


def test_drop_side_scratch_walks_the_owners():
    class Holder(object):
        def __init__(self):
            self._scratch = lanes.Scratch()
    m, e = Holder(), Holder()
    for h in (m, e):
        _grow(h._scratch, 2)
        with lanes.use(1):
            _grow(h._scratch, 2)
    gm, ge = m._scratch.generation, e._scratch.generation
    lanes.drop_side_scratch(m, None, object(), e)            # (a loss without an engine, a model without scratch)
    assert sorted(m._scratch.lanes) == [0] and sorted(e._scratch.lanes) == [0]
    assert m._scratch.generation == gm + 1 and e._scratch.generation == ge + 1


def test_scratch_ticket_stamps_are_per_lane():
    sc = lanes.Scratch()
    s0 = sc.stamp()
    with lanes.use(1):
        s1 = sc.stamp()
    assert s0[0] == 0 and s1[0] == 1
    assert not sc.stale(s0) and not sc.stale(s1)             # a forward in lane 1 leaves lane 0's stamp good
    with lanes.use(1):
        assert not sc.stale(s0)                              # (checked from whatever lane: the stamp names its own)
        s1b = sc.stamp()
    assert sc.stale(s1) and not sc.stale(s1b) and not sc.stale(s0)
    s0b = sc.stamp()
    assert sc.stale(s0) and not sc.stale(s0b) and not sc.stale(s1b)
    sc.drop_side()
    assert sc.stale(s1b) and not sc.stale(s0b)               # a dropped lane's saved activations are gone


def test_graph_key_follows_the_generation():
    """base_optimizer._graph_key: a drop on the model's or the engine's owner changes the key a captured graph is
    found under (closure._step_fused frees lane 1's arenas through lanes.drop_side_scratch: a graph captured on
    two lanes points into them), nothing happening leaves it equal."""
    from pix2latent_amd.optimizer.base_optimizer import _BaseOptimizer

    class Holder(object):
        lanes_ok = True

        def __init__(self):
            self._scratch = lanes.Scratch()

    class Stub(object):
        _graph_key = _BaseOptimizer._graph_key
        max_batch_size, exec_batch_size = 9, None

    class Vars(object):
        num_samples, input, output = 18, {}, {}
        opt = type('Adam', (), {'state_key': lambda self: 7})()

    o = Stub()
    o.model, o.loss_fn = Holder(), type('L', (), {'_engine': Holder()})()
    for h in (o.model, o.loss_fn._engine):
        _grow(h._scratch, 9)
        with lanes.use(1):
            _grow(h._scratch, 9)
    k0 = o._graph_key(Vars(), 0, 18)
    assert o._graph_key(Vars(), 0, 18) == k0 and hash(k0) == hash(o._graph_key(Vars(), 0, 18))
    lanes.drop_side_scratch(o.model)
    k1 = o._graph_key(Vars(), 0, 18)
    assert k1 != k0
    lanes.drop_side_scratch(o.loss_fn._engine)
    k2 = o._graph_key(Vars(), 0, 18)
    assert k2 != k1 and k2 != k0
    assert o._graph_key(Vars(), 0, 18) == k2
    assert o._graph_key(Vars(), 0, 9) != k2
    o.model, o.loss_fn = object(), object()                  # objects without scratch: generation 0
    assert o._graph_key(Vars(), 0, 18)[6:8] == (0, 0)


def test_lane_split_parse(monkeypatch):
    monkeypatch.delenv('P2L_STREAMS', raising=False)
    monkeypatch.setenv('P2L_LANE_SPLIT', 'x')
    assert lanes.env_int('P2L_LANE_SPLIT', 1) == 1           # not a number: off, as P2L_STREAMS falls back to 2
    assert lanes.env_int('P2L_STREAMS', 2) == 2
    monkeypatch.setenv('P2L_LANE_SPLIT', '')
    assert lanes.env_int('P2L_LANE_SPLIT', 1) == 1
    monkeypatch.setenv('P2L_LANE_SPLIT', ' 3 ')
    assert lanes.env_int('P2L_LANE_SPLIT', 1) == 3
    monkeypatch.delenv('P2L_LANE_SPLIT')
    assert lanes.env_int('P2L_LANE_SPLIT', 1) == 1

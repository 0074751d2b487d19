"""The BigGAN and StyleGAN2 plans keep no state between calls: a run context on the stack of the entry point
carries the weight format, and every layout is told the format it lays out for.  Host checks, no GPU: every
workspace size and test-hook lookup equals what the plans laid out while the format still travelled in
per-thread globals (tests/golden/plan_layout.json, written by tools/make_plan_layout_golden.py from that
build), in whatever order the queries come."""
import ctypes as C
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(ROOT, 'pix2latent_amd', 'libp2l_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from pix2latent_amd import _native as N
    return N.lib()


@pytest.fixture(scope='module')
def tool():
    spec = importlib.util.spec_from_file_location('make_plan_layout_golden',
                                                  os.path.join(ROOT, 'tools', 'make_plan_layout_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                       # (the calls that wrote the file, so both read alike)
    return mod


@pytest.fixture(scope='module')
def gold():
    with open(os.path.join(ROOT, 'tests', 'golden', 'plan_layout.json')) as f:
        return json.load(f)


def test_the_file_holds_the_cases_it_was_asked_for(tool, gold):
    qs = tool.queries()
    assert {c for c, _, _ in qs} == set(gold) and sum(len(v) for v in gold.values()) == len(qs)
    assert len([c for c in gold if c.startswith('biggan')]) == 21
    assert len([c for c in gold if c.startswith('sg2')]) == 24
    # the formats are told apart: kernel choice, hence split-K workspace and partial rows, follows the format
    at3 = [gold['biggan B=3 wfmt=0x%x' % f]['ws_bytes'] for f in (0x0, 0x1, 0x2, 0x42)]
    assert at3 == [1152995584, 1144002048, 1155601920, 1164595456]
    for case, rec in gold.items():
        assert rec['ws_bytes'] > 0, case
        refused = [k for k, v in rec.items() if k != 'ws_bytes' and v[0] != 0]
        assert refused and all(rec[k] == [-1, 0, [0, 0, 0, 0]] for k in refused), case
        assert len(refused) < len(rec) - 1, case


@pytest.mark.parametrize('order', ['as recorded', 'reversed'])
def test_layout_equals_the_recorded_one(lib, tool, gold, order):
    qs = tool.queries()
    got = tool.record(lib, qs if order == 'as recorded' else qs[::-1])
    for case in gold:
        assert got[case] == gold[case], case
    assert set(got) == set(gold)


def test_loss_lookup_does_not_depend_on_the_plan_query_before_it(lib, tool):
    """p2l_projloss_ws_lookup has no descriptor; it used to lay the arena out for the format the last plan call
    on the thread had left behind"""
    loss = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'loss_layout.json')))['vgg']['3x64x64']['lookup']
    assert len(loss) == 13

    def lookups():
        out = []
        for idx in range(13):
            off, shape = C.c_size_t(0), (C.c_int32 * 4)()
            rc = lib.p2l_projloss_ws_lookup(3, 64, 64, idx, C.byref(off), shape)
            out.append([rc, off.value, list(shape)])
        return out

    d12, d0, sg = tool.biggan_desc(0x12), tool.biggan_desc(0x0), tool.sg2_desc('64', 2)
    assert lib.p2l_biggan_ws_bytes(C.byref(d12), 3) > 0
    assert lookups() == loss
    assert lib.p2l_biggan_ws_bytes(C.byref(d0), 3) > 0
    assert lookups() == loss
    assert lib.p2l_sg2_ws_bytes(C.byref(sg), 3) > 0
    assert lookups() == loss

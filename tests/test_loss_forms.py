"""Which library calls each form of the native image losses makes (pix2latent_amd/loss_functions.py `_ImageLossFn`),
on the host: the losses run on CPU tensors against the recording stand-in of tests/_loss_recorder.py, nothing is
launched.  The call-name sequences below are literals; tools/loss_trace.py prints the same runs with every argument."""
import ctypes as C

import pytest
import torch

import _loss_recorder as R
import pix2latent_amd.loss_functions as LF
from pix2latent_amd import _native as N, lanes

B = 3
STEMS = {'vgg': 'p2l_projloss', 'alex': 'p2l_alexloss', 'squeeze': 'p2l_sqzloss'}
PACK, UNPACK = 'p2l_nchw3_to_nhwc16', 'p2l_nhwc16_to_nchw3'
POOLPACK, UNPOOL = 'p2l_area_pool3_to_nhwc16', 'p2l_area_unpool16_add_nchw3'
COMBINE = ['p2l_vec_scale_div', 'p2l_reduce_rows']
# plan forward: net, img16, target, weight, loss_mask, slot, beta, use_lpips, B, H, W, ws, ws_bytes, loss, l1, lp, stream
NET, BETA, USE, FWD_L1, FWD_LP = 0, 6, 7, 14, 15
# pixel forward: img, target, weight, loss_mask, wsum, out, part, ...; backward: ..., wsum, g, d, B, H, W, accumulate
PIX_WSUM, PIX_OUT, PIX_PART, PIX_ACC = 4, 5, 6, 10


def plan_form(stem):
    """the plan alone: forward, backward; then what a first call adds in front"""
    return ([PACK, stem + '_fwd'], [stem + '_bwd', UNPACK], [stem + '_prepare'])


def l2_alone(stem):
    return ([PACK, 'p2l_l2_loss_fwd'], ['p2l_l2_loss_bwd', UNPACK], ['p2l_weight_sum'])


def l2_beside(stem):
    return ([PACK, stem + '_fwd', 'p2l_l2_loss_fwd'] + COMBINE, [stem + '_bwd', 'p2l_l2_loss_bwd', UNPACK],
            [stem + '_prepare'])


def pooled_pixel(pixel):
    def form(stem):
        return ([POOLPACK, stem + '_fwd', PACK, 'p2l_%s_loss_fwd' % pixel] + COMBINE,
                [stem + '_bwd', 'p2l_%s_loss_bwd' % pixel, UNPOOL],
                ['p2l_weight_sum', 'p2l_area_pool_nchw', 'p2l_area_pool_nchw', stem + '_prepare'])
    return form


def pooled_lpips(stem):
    return ([POOLPACK, stem + '_fwd'], [stem + '_bwd', UNPOOL],
            ['p2l_area_pool_nchw', 'p2l_area_pool_nchw', stem + '_prepare'])


# name -> (class, constructor arguments, pooled?, the form's sequences, where slot.used() sits in a second lane's
#          backward: behind this many of its calls (None: the form has no slot))
FORMS = {
    'proj l1': ('ProjectionLoss', {}, False, plan_form, 1),
    'proj l1 a=0.37': ('ProjectionLoss', dict(pixel_weight=0.37), False, plan_form, 1),
    'proj a=0': ('ProjectionLoss', dict(pixel_weight=0.0), False, plan_form, 1),
    'perceptual': ('PerceptualLoss', {}, False, plan_form, 1),
    'recon l1': ('ReconstructionLoss', dict(loss_type='l1'), False, plan_form, 1),
    'recon l2': ('ReconstructionLoss', dict(loss_type='l2'), False, l2_alone, None),
    'proj l2': ('ProjectionLoss', dict(pixel_loss='l2', pixel_weight=0.37), False, l2_beside, 2),
    'proj l2 a=0': ('ProjectionLoss', dict(pixel_loss='l2', pixel_weight=0.0), False, l2_beside, 2),
    'pooled l1': ('ProjectionLoss', {}, True, pooled_pixel('l1'), 1),
    'pooled l1 a=0.37': ('ProjectionLoss', dict(pixel_weight=0.37), True, pooled_pixel('l1'), 1),
    'pooled l2': ('ProjectionLoss', dict(pixel_loss='l2', pixel_weight=0.37), True, pooled_pixel('l2'), 1),
    'pooled a=0': ('ProjectionLoss', dict(pixel_weight=0.0), True, pooled_lpips, 1),
    'pooled perceptual': ('PerceptualLoss', {}, True, pooled_lpips, 1),
}


class Run(object):
    """one loss object under the recorder: `step()` = forward + backward, -> the names of its calls"""

    def __init__(self, rec, form, net='vgg', weight='w3', mask=False, beta=None):
        cls, kw, pooled, _, _ = FORMS[form]
        size = 128 if pooled else 64
        kw = dict(kw, **({'lpips_size': 64} if pooled else {}))
        if cls != 'ReconstructionLoss':
            kw['net' if cls == 'PerceptualLoss' else 'lpips_net'] = net
        if beta is not None:
            kw['beta'] = beta
        self.fn = getattr(LF, cls)(**kw)
        if self.fn._engine is None:
            self.fn._engine = LF._LossEngine(None)
        self.rec, self.eng = rec, self.fn._engine
        g = torch.Generator().manual_seed(1)
        r = lambda c: torch.rand(B, c, size, size, generator=g)
        self.t = dict(output=(r(3) * 2 - 1).requires_grad_(True), target=r(3) * 2 - 1,
                      weight={'w3': r(3) + 0.5, 'w1': r(1) + 0.5, 'none': None}[weight],
                      loss_mask=(r(1) > 0.3).float() if mask else None)
        rec.reset()
        rec.watch(self.eng, **self.t)

    def forward(self, n=B, lane=0):
        t = self.t
        with lanes.use(lane):
            return self.fn(*(None if v is None else v[:n] for v in (t['output'], t['target'], t['weight'],
                                                                    t['loss_mask'])))

    def step(self, n=B, lane=0):
        self.mark = len(self.rec.calls)
        self.forward(n, lane).sum().backward()
        names = self.rec.names(self.mark)
        self.rec.step_end()
        return names

    def call(self, name):
        """the one call of that name in the last step"""
        found = [c for c in self.rec.calls[self.mark:] if c.name.endswith(name)]
        assert len(found) == 1, (name, self.rec.names(self.mark))
        return found[0]

    def role(self, call, index):
        return self.rec.show(call.args[index])


@pytest.fixture
def rec():
    with R.recording() as r:
        yield r


@pytest.mark.parametrize('form', sorted(FORMS))
def test_call_sequences(rec, form):
    """first call, second call on the same tensors (nothing prepared again), the same under a second lane (the
    slot's reader events behind the forward and behind the last launch of the backward that reads the slot)"""
    for net in (('vgg',) if FORMS[form][0] == 'ReconstructionLoss' else STEMS):
        fwd, bwd, once = FORMS[form][3](STEMS[net])
        used = FORMS[form][4]
        run = Run(rec, form, net)
        first = run.step()
        assert first == once + fwd + bwd, (net, first)
        assert run.step() == fwd + bwd
        lane1 = run.step(lane=1)
        if used is None:
            assert lane1 == fwd + bwd
        else:
            assert lane1 == fwd + ['slot.used'] + bwd[:used] + ['slot.used'] + bwd[used:], (net, lane1)


@pytest.mark.parametrize('form', sorted(FORMS))
def test_what_a_form_holds(rec, form):
    """full-size staging only where a pixel term runs off the plan's buffer; `pix_part` only for L2 beside a
    full-size plan; no arena and no cache slot for L2 alone; B = 3, 2, 3 re-allocates nothing"""
    run = Run(rec, form)
    run.step()
    s = run.eng._scratch.lanes[0]
    side = form in ('recon l2', 'pooled l1', 'pooled l1 a=0.37', 'pooled l2')
    assert (s.full16 is not None) == side and (s.dfull16 is not None) == side and (s.l1_part is not None) == side
    assert (s.pix_part is not None) == form.startswith('proj l2')
    assert (s.ws is not None) == (form != 'recon l2')
    assert len(run.eng.slots) == (0 if form == 'recon l2' else 1)
    generation = run.eng._scratch.generation
    run.step(2)
    run.step(3)
    assert run.eng._scratch.generation == generation
    assert len(set(map(id, run.eng.slots.values()))) == (0 if form == 'recon l2' else 2)


@pytest.mark.parametrize('form,fwd,bwd', [
    ('proj l1', 1, 1), ('proj l1 a=0.37', 1, 1), ('recon l1', 0, 0), ('proj a=0', 1, 2), ('perceptual', 1, 2),
    ('proj l2', 1, 2), ('proj l2 a=0', 1, 2), ('pooled l1', 1, 2), ('pooled l1 a=0.37', 1, 2), ('pooled l2', 1, 2),
    ('pooled a=0', 1, 2), ('pooled perceptual', 1, 2)])
def test_use_lpips_and_network(rec, form, fwd, bwd):
    run = Run(rec, form)
    run.step()
    f, b = run.call('projloss_fwd'), run.call('projloss_bwd')
    assert (rec.scalar(f, USE), rec.scalar(b, USE)) == (fwd, bwd)
    # use_lpips = 0 passes a NULL network, forward and backward
    assert (f.args[NET] is None) == (fwd == 0) and (b.args[NET] is None) == (bwd == 0)
    if fwd:
        assert run.role(f, NET) == 'net'


def f32(v):
    return C.c_float(v).value


@pytest.mark.parametrize('weight,k', [('w3', 1.0), ('w1', 3.0), ('none', 1.0)])
def test_betas_scales_and_the_factor_three(rec, weight, k):
    """where each form puts beta, pixel_weight and the factor 3 of a one-channel weight"""
    def scalars(form):
        run = Run(rec, form, weight=weight, beta=10)
        run.step()
        scale = rec.scalar(run.call('vec_scale_div'), 4) if 'l2' in form or 'pooled l1' in form else None
        return (rec.scalar(run.call('projloss_fwd'), BETA), rec.scalar(run.call('projloss_bwd'), BETA), scale)
    # the plan's own L1: beta / k inside, k outside the Function; pixel_weight by the rescaling route
    assert scalars('proj l1') == (f32(10 / k), f32(10 / k), None)
    assert scalars('proj l1 a=0.37') == (f32(10 / 0.37 / k), f32(10 / 0.37 / k), None)
    # a pixel term beside the plan: the plan forward with beta = 1, a * k inside the Function
    assert scalars('proj l2') == (1.0, 10.0, f32(0.37 * k))
    assert scalars('pooled l1') == (1.0, 10.0, f32(k))
    assert scalars('pooled l1 a=0.37') == (1.0, f32(10 / 0.37), f32(k))
    assert scalars('pooled l2') == (1.0, 10.0, f32(0.37 * k))
    # LPIPS alone: beta outside
    assert scalars('proj a=0')[:2] == (1.0, 1.0) and scalars('pooled a=0')[:2] == (1.0, 1.0)


def test_pixel_term_buffers_and_accumulate(rec):
    """L2 beside a full-size plan: on the plan's image, partials in pix_part, the slot's weight sum, its gradient
    ADDED into dimg16; everywhere else: own staging, l1_part, the memoised weight sum, accumulate = 0"""
    run = Run(rec, 'proj l2')
    run.step()
    f, b = run.call('l2_loss_fwd'), run.call('l2_loss_bwd')
    assert [run.role(f, i) for i in (0, PIX_WSUM, PIX_PART)] == ['lane0.img16', 'slot1.wsum', 'lane0.pix_part']
    assert [run.role(b, i) for i in (0, PIX_WSUM, 6)] == ['lane0.img16', 'slot1.wsum', 'lane0.dimg16']
    assert rec.scalar(b, PIX_ACC) == 1
    assert run.role(run.call(UNPACK), 0) == 'lane0.dimg16'
    for form, pixel in (('recon l2', 'l2'), ('pooled l1', 'l1'), ('pooled l2', 'l2')):
        run = Run(rec, form)
        run.step()
        f, b = run.call(pixel + '_loss_fwd'), run.call(pixel + '_loss_bwd')
        assert [run.role(f, i) for i in (0, PIX_WSUM, PIX_PART)] == ['lane0.full16', 'pooled1.wsum', 'lane0.l1_part']
        assert [run.role(b, i) for i in (0, PIX_WSUM, 6)] == ['lane0.full16', 'pooled1.wsum', 'lane0.dfull16']
        assert rec.scalar(b, PIX_ACC) == 0
        last = run.call(UNPOOL if 'pooled' in form else UNPACK)
        assert run.role(last, 1 if 'pooled' in form else 0) == 'lane0.dfull16'
    # LPIPS alone, pooled: a NULL full-size gradient
    run = Run(rec, 'pooled a=0')
    run.step()
    assert run.call(UNPOOL).args[1].value is None


@pytest.mark.parametrize('form', sorted(FORMS))
def test_last_l1_and_last_lpips(rec, form):
    """after a forward `eng.last_l1` is the tensor the pixel term was written to (the plan's by-product where no
    pixel term runs), `eng.last_lpips` the one the plan wrote the LPIPS term to"""
    run = Run(rec, form)
    run.mark = len(rec.calls)
    loss = run.forward()
    pixel = [c for c in rec.calls if c.name in ('p2l_l1_loss_fwd', 'p2l_l2_loss_fwd')]
    plan = [c for c in rec.calls if c.name.endswith('loss_fwd') and c not in pixel]
    assert len(pixel) == (1 if 'l2' in form or 'pooled l1' in form else 0) and len(plan) == (form != 'recon l2')
    want = pixel[0].args[PIX_OUT].value if pixel else plan[0].args[FWD_L1].value
    assert run.eng.last_l1.data_ptr() == want
    if plan:
        assert run.eng.last_lpips.data_ptr() == plan[0].args[FWD_LP].value
    # what comes back: the LPIPS term itself where it runs alone
    if form in ('perceptual', 'pooled perceptual'):
        assert loss.data_ptr() == run.eng.last_lpips.data_ptr()
    if form == 'recon l2':
        assert loss.data_ptr() == run.eng.last_l1.data_ptr()


@pytest.mark.parametrize('form', sorted(FORMS))
def test_a_backward_behind_a_later_forward_raises_and_launches_nothing(rec, form):
    run = Run(rec, form)
    early = run.forward()
    run.forward()
    mark = len(rec.calls)
    with pytest.raises(N.NativeError, match='loss workspace was reused by a later forward before backward'):
        early.sum().backward()
    assert rec.calls[mark:] == []
    # ... while another lane's forward leaves this lane's backward alone
    early = run.forward()
    run.forward(lane=1)
    early.sum().backward()
    assert len(rec.calls) > mark

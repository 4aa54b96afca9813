"""CPU: the shared pieces of the evaluation drivers -- util.host_scores against the scoring sequence of test.evaluate written out here (the arithmetic order is the
contract: `==` on every float), imgio.decode_ahead (order, the bound on what waits, the clamp of the thread count, where an exception surfaces), the tail that
BaseModel.test() and test_x8() share, and the ground-truth accessor behind current_metrics."""
import threading

import numpy as np
import pytest
import torch


def _written_out(sr_img, gt_img, c):
    """the host branch of test.evaluate as it stood before util.host_scores, line by line.  The slices are written c:n - c (the same elements as c:-c for every
    c > 0, and the whole image at c = 0, where -0 would select nothing); an HW image has no third axis and no Y form."""
    from dasr_amd import util
    h, w = sr_img.shape[:2]
    gt_img = gt_img / 255.
    sr_img = sr_img / 255.
    csr, cgt = sr_img[c:h - c, c:w - c], gt_img[c:h - c, c:w - c]
    out = [util.calculate_psnr(csr * 255, cgt * 255), util.calculate_ssim(csr * 255, cgt * 255)]
    if sr_img.ndim == 3 and sr_img.shape[2] == 3:
        sr_y, gt_y = util.bgr2ycbcr(sr_img, only_y=True), util.bgr2ycbcr(gt_img, only_y=True)
        out.append(util.calculate_psnr(sr_y[c:h - c, c:w - c] * 255, gt_y[c:h - c, c:w - c] * 255))
        out.append(util.calculate_ssim(sr_y[c:h - c, c:w - c] * 255, gt_y[c:h - c, c:w - c] * 255))
    return out


@pytest.mark.parametrize('shape', [(12, 13, 3), (12, 13)], ids=['hwc', 'hw'])
@pytest.mark.parametrize('crop', [0, 1])
def test_host_scores_is_the_written_out_sequence_float_for_float(shape, crop):
    """crop 0 scores 12 x 13; crop 1 leaves 10 x 11, under the 11-pixel window: numpy's ValueError comes out of both unchanged, and PSNR alone (what train.validate
    asks for) still equals validate's expression"""
    from dasr_amd import util
    r = np.random.RandomState(5 + len(shape))
    sr, gt = r.randint(0, 256, size=shape).astype(np.uint8), r.randint(0, 256, size=shape).astype(np.uint8)
    if crop == 0:
        want = _written_out(sr, gt, crop)
        got = util.host_scores(sr, gt, crop)
        assert list(got) == ['psnr', 'ssim', 'psnr_y', 'ssim_y'][:len(want)]
        assert list(got.values()) == want and all(np.isfinite(v) for v in want)
    else:
        with pytest.raises(ValueError) as want:
            _written_out(sr, gt, crop)
        with pytest.raises(ValueError) as got:
            util.host_scores(sr, gt, crop)
        assert str(got.value) == str(want.value) and 'window shape' in str(want.value)
    c = crop or 2   # (validate's slices are c:-c)
    psnr_only = util.host_scores(sr, gt, c, ssim=False, y=False)
    assert psnr_only == {'psnr': util.calculate_psnr((sr / 255.)[c:-c, c:-c] * 255, (gt / 255.)[c:-c, c:-c] * 255)}
    if len(shape) == 3:
        assert list(util.host_scores(sr, gt, c, ssim=False)) == ['psnr', 'psnr_y']


@pytest.mark.parametrize('threads,eff', [(2, 2), (0, 1), (99, None)], ids=['2', '0->1', '99->max'])
def test_decode_ahead_keeps_order_and_bounds_what_waits(threads, eff):
    """job lists of 0, 1, 5 and 2 x threads + 1 items: results in job order.  Outstanding = submitted and not yet with the consumer.  When a job is drawn for
    submission at most 2 x (clamped) threads earlier ones are outstanding (counted where the generator draws it), so a load that starts finds at most that many
    beside itself (counted under a lock inside `load`: one of them is the result the generator has taken from the queue for the consumer, 2 x threads wait).
    Counting the starting load too, that is 2 x threads + 1 outstanding, one above the literal '2 x threads': decode_ahead keeps the order of the loops it
    replaces (take one result, submit one job, hand the result over), whose queue held 2 x threads next to the result in hand.  A thread count of 0 runs on 1
    thread, one of 99 on MAX_DECODE_THREADS."""
    from dasr_amd import imgio
    eff = imgio.MAX_DECODE_THREADS if eff is None else eff
    for n in (0, 1, 5, 2 * eff + 1):
        lock, state = threading.Lock(), {'started': 0, 'taken': 0, 'beside': 0, 'at_draw': 0, 'workers': set()}

        def jobs():
            for i in range(n):
                with lock:
                    state['at_draw'] = max(state['at_draw'], i - state['taken'])
                yield i, 'j%d' % i

        def load(i, tag):
            with lock:
                state['started'] += 1
                state['beside'] = max(state['beside'], state['started'] - state['taken'] - 1)
                state['workers'].add(threading.get_ident())
            return i, tag
        got = []
        for item in imgio.decode_ahead(load, jobs(), threads):
            with lock:
                state['taken'] += 1
            got.append(item)
        assert got == [(i, 'j%d' % i) for i in range(n)]
        assert state['started'] == n and len(state['workers']) <= eff
        assert state['at_draw'] == min(max(n - 1, 0), 2 * eff) and state['beside'] <= 2 * eff


def test_decode_ahead_raises_at_the_item_whose_load_failed():
    from dasr_amd import imgio

    def load(i):
        if i == 3:
            raise KeyError('job %d' % i)
        return i
    got = []
    with pytest.raises(KeyError, match='job 3'):
        for v in imgio.decode_ahead(load, [(i,) for i in range(6)], 1):
            got.append(v)
    assert got == [0, 1, 2]


def _stub_model(opt, ground_truth=None):
    """BaseModel without a device: the generator, the back-projection and LPIPS only record that they ran"""
    from dasr_amd.models import BaseModel

    class Stub(BaseModel):
        def __init__(self):
            self.opt, self.calls, self.var_L, self.fake_H = opt, [], torch.zeros(1, 3, 4, 5), None
            self.ground_truth = ground_truth

        def _generate(self, x):
            self.calls.append('generate%d' % x.shape[0])
            return x

        def _back_project(self):
            self.calls.append('back_project')

        def _eval_lpips(self):
            self.calls.append('lpips')
    return Stub()


@pytest.mark.parametrize('val_lpips', [False, True])
def test_test_and_test_x8_end_in_one_tail(monkeypatch, val_lpips):
    """generator, then back-projection (which decides for itself whether the option is on), then LPIPS under `val_lpips` only; test(tsamples=True) stops behind the
    generator; test_x8 runs the generator on its two batches of 4 first"""
    from dasr_amd import util
    monkeypatch.setattr(util, 'dihedral8', lambda x: (x[None].expand(4, -1, -1, -1), x[None].expand(4, -1, -1, -1).transpose(2, 3)))
    monkeypatch.setattr(util, 'dihedral8_mean', lambda a, b: a[:1])
    tail = ['back_project'] + (['lpips'] if val_lpips else [])
    m = _stub_model({'val_lpips': val_lpips})
    m.test()
    assert m.calls == ['generate1'] + tail and m.fake_H is m.var_L
    m.calls.clear()
    m.test_x8()
    assert m.calls == ['generate4', 'generate4'] + tail and tuple(m.fake_H.shape) == (1, 3, 4, 5)
    m.calls.clear()
    m.test(tsamples=True)
    assert m.calls == ['generate1']


def test_current_metrics_reads_the_ground_truth_through_the_accessor():
    """no HR fed: the RuntimeError texts of current_metrics as they were; SRModel answers with real_H, DASR_Model with var_H unless the last feed_data carried no HR"""
    from dasr_amd.dasr_model import DASR_Model
    from dasr_amd.models import BaseModel, SRModel
    m = _stub_model({})
    m.fake_H = torch.zeros(1, 3, 16, 20)
    with pytest.raises(RuntimeError) as e:
        m.current_metrics(4)
    assert str(e.value) == 'current_metrics needs test() on a batch that carried an HR image (feed_data was given no HR)'
    m.ground_truth = torch.zeros(1, 3, 8, 8)   # (a stale HR batch)
    with pytest.raises(RuntimeError) as e:
        m.current_metrics(4)
    assert str(e.value) == 'current_metrics: HR (1, 3, 8, 8) does not belong to SR (1, 3, 16, 20) (the last feed_data carried no HR?)'
    assert BaseModel.ground_truth is None
    sr, dasr, t = SRModel.__new__(SRModel), DASR_Model.__new__(DASR_Model), torch.zeros(1)
    assert sr.ground_truth is None and dasr.ground_truth is None
    sr.real_H = dasr.var_H = t
    assert sr.ground_truth is t and dasr.ground_truth is t     # (a training batch sets no needHR)
    dasr.needHR = False
    assert dasr.ground_truth is None
    dasr.needHR = True
    assert dasr.ground_truth is t

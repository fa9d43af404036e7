"""SparseFlowAugmentor on the device against the reference's own run (tests/golden/sparse_augment_golden.npz) -- EXACT equality by
value, no tolerance: uint8 crops bit for bit, the flow after the reference's float64 is narrowed to float32, `valid` after the
reference's int32 is widened to float32.

Beyond the fixture's cases the yardstick is `make_sparse_augment_golden.sparse_numpy_chain`: the reference's chain step by step on
the stand-in cv2 / albumentations, its flow resize the reference's SCATTER in NumPy, which tests/test_sparse_augment.py pins to the
reference itself (the reference tree does not exist on the GPU box).
"""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, report

sys.path.insert(0, GOLDEN)
import make_augment_golden as mk                                   # noqa: E402
import make_sparse_augment_golden as ms                            # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ms.NAMES


def _np(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy()


def _aug(seed=0, crop=ms.CROP, do_flip=False):
    from tf_raft_amd.augment import SparseFlowAugmentor
    return SparseFlowAugmentor(crop, do_flip=do_flip, rng=np.random.RandomState(seed), photo_rng=np.random.RandomState(seed + mk.PHOTO_SEED_OFFSET))


def _compare(got, want, what):
    """Exact, with the figures printed first: number of differing elements and the largest difference per output."""
    bad = {}
    for name, g in zip(NAMES, got):
        g, w = _np(g), np.asarray(want[name])
        if name in ('flow', 'valid'):
            w = w.astype(np.float32)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        diff = ~((g == w) | (np.isnan(g) & np.isnan(w)))
        if diff.any():
            bad[name] = (int(diff.sum()), float(np.nanmax(np.abs(g.astype(np.float64) - w.astype(np.float64))[diff])))
    report(what, **{f'{k}_differ': v[0] for k, v in bad.items()}, **{f'{k}_maxdiff': v[1] for k, v in bad.items()}, exact=not bad)
    assert not bad, (what, bad)


def _record(H, W, f, crop, y0=0, x0=0, flip_h=False, resize=True):
    """A hand-made record: no colour change, no rectangle."""
    H1, W1 = (int(round(H * np.float64(f))), int(round(W * np.float64(f)))) if resize else (H, W)
    assert 0 <= y0 <= H1 - crop[0] and 0 <= x0 <= W1 - crop[1]
    none = {'bc': None, 'hsv': None}
    return {'photo': (none, none), 'rects': [], 'scale_x': float(f), 'scale_y': float(f), 'clipped': False, 'resize': resize, 'size': (H1, W1),
            'flip_h': flip_h, 'flip_v': False, 'y0': y0, 'x0': x0, 'y0_drawn': y0, 'x0_drawn': x0, 'source': (H, W)}


def test_apply_with_the_recorded_parameters_equals_the_fixture():
    for H, W, seed, do_flip, rec, outs, _ in ms.load_fixture():
        inputs = ms.sparse_case_inputs(seed, H, W)
        got = _aug(do_flip=do_flip).apply([rec], *inputs)
        assert len(got) == 4 and all(g.is_cuda for g in got)
        assert [g.dtype for g in got] == [torch.uint8, torch.uint8, torch.float32, torch.float32]
        _compare(got, outs, f'sparse augment fixture {H}x{W} seed {seed}')


def test_drawn_cases_equal_the_numpy_chain():
    """Cases the fixture has no room for: 40 draws on each of its two source sizes and a few KITTI-sized frames at the reference's
    KITTI crop, each against the chain (whose flow resize is the scatter) on the stand-ins."""
    for (H, W), crop, seeds in ((ms.SIZES[0], ms.CROP, range(300, 340)), (ms.SIZES[1], ms.CROP, range(300, 340)),
                                ((375, 1242), (288, 960), range(400, 404))):
        for seed in seeds:
            aug = _aug(seed, crop, do_flip=bool(seed % 2))
            rec = aug.draw(H, W)[0]
            inputs = ms.sparse_case_inputs(seed, H, W)
            _compare(aug.apply([rec], *inputs), ms.sparse_numpy_chain(rec, *inputs, crop), f'sparse augment chain {H}x{W} seed {seed}')


@pytest.mark.parametrize('f', (0.5, 1.5, 1.0 / 3, 0.125, 2.0))
def test_hand_made_factors_cover_the_halves_to_even(f):
    """x * 0.5 and x * 1.5 are exact halves for odd x, 1 / 3 puts three sources on a target, 1 / 8 is the smallest factor taken."""
    H, W = 144, 200
    H1, W1 = int(round(H * np.float64(f))), int(round(W * np.float64(f)))
    crop = (min(H1, 40), min(W1, 56))
    inputs = ms.sparse_case_inputs(11, H, W)
    for flip_h in (False, True):
        for y0, x0 in ((0, 0), (H1 - crop[0], W1 - crop[1])):
            rec = _record(H, W, f, crop, y0, x0, flip_h)
            _compare(_aug(crop=crop).apply([rec], *inputs), ms.sparse_numpy_chain(rec, *inputs, crop), f'sparse f={f:.4f} flip={flip_h} origin {y0},{x0}')


def test_nothing_of_an_invalid_source_reaches_a_resized_output():
    H, W = 120, 160
    img1, img2, flow, valid = ms.sparse_case_inputs(21, H, W)
    flow[valid == 0] = np.nan
    for f in (0.75, 1.3):
        rec = _record(H, W, f, ms.CROP, 3, 5)
        got = _aug().apply([rec], img1, img2, flow, valid)
        assert not torch.isnan(got[2]).any()
        _compare(got, ms.sparse_numpy_chain(rec, img1, img2, flow, valid), f'sparse NaN at invalid, f={f}')
    # not resized: flow is copied where invalid too, NaN included
    rec = _record(H, W, 1.0, ms.CROP, 3, 5, resize=False)
    got = _aug().apply([rec], img1, img2, flow, valid)
    assert torch.isnan(got[2]).any()
    _compare(got, ms.sparse_numpy_chain(rec, img1, img2, flow, valid), 'sparse NaN at invalid, not resized')


def test_validity_values_pass_through_without_resize_and_are_thresholded_at_one_with_it():
    H, W = 120, 160
    img1, img2, flow, _ = ms.sparse_case_inputs(22, H, W)
    valid = np.random.RandomState(5).choice(np.array([0, 0.5, 1, 2], np.float32), size=(H, W))
    for flip_h in (False, True):
        rec = _record(H, W, 1.0, ms.CROP, 7, 9, flip_h, resize=False)
        got = _aug().apply([rec], img1, img2, flow, valid)
        assert set(np.unique(_np(got[3])).tolist()) == {0.0, 0.5, 1.0, 2.0}
        _compare(got, ms.sparse_numpy_chain(rec, img1, img2, flow, valid), f'sparse validity values, not resized, flip={flip_h}')
        for f in (0.8, 1.25):
            rec = _record(H, W, f, ms.CROP, 7, 9, flip_h)
            got = _aug().apply([rec], img1, img2, flow, valid)
            assert set(np.unique(_np(got[3])).tolist()) == {0.0, 1.0}
            _compare(got, ms.sparse_numpy_chain(rec, img1, img2, flow, valid), f'sparse validity values, f={f}, flip={flip_h}')


def _batch_inputs(seeds, H, W):
    samples = [ms.sparse_case_inputs(s, H, W) for s in seeds]
    return tuple(np.stack([s[k] for s in samples]) for k in range(4))


def test_a_batch_call_equals_the_per_sample_calls():
    H, W = 120, 160
    aug = _aug(7, do_flip=True)
    recs, tries = [], 0
    while sorted(len(r['rects']) for r in recs[:3]) != [0, 1, 2] or all(r['resize'] for r in recs) or not any(r['resize'] for r in recs):
        recs = aug.draw(H, W, 5)                                          # 0, 1 and 2 rectangles, resized and not, in one batch
        tries += 1
        assert tries < 500
    inputs = _batch_inputs(range(50, 55), H, W)
    got = aug.apply(recs, *inputs)
    assert tuple(got[0].shape) == (5, *ms.CROP, 3) and tuple(got[2].shape) == (5, *ms.CROP, 2) and tuple(got[3].shape) == (5, *ms.CROP)
    for k, rec in enumerate(recs):
        sample = tuple(a[k] for a in inputs)
        single = aug.apply([rec], *sample)
        assert tuple(single[0].shape) == (*ms.CROP, 3) and tuple(single[3].shape) == ms.CROP
        for name, b, s in zip(NAMES, got, single):
            np.testing.assert_array_equal(_np(b)[k], _np(s), err_msg=f'{name} of sample {k}')
        _compare(single, ms.sparse_numpy_chain(rec, *sample), f'sparse augment batch sample {k} ({len(rec["rects"])} rectangles)')


def test_host_and_device_inputs_agree_numpy_and_torch_on_a_side_stream_and_twice():
    H, W = 120, 160
    aug = _aug(11, do_flip=True)
    recs = aug.draw(H, W, 2)
    inputs = _batch_inputs((60, 61), H, W)
    want = [_np(o) for o in aug.apply(recs, *inputs)]
    again = [_np(o) for o in aug.apply(recs, *inputs)]                   # two runs are identical
    for name, g, w in zip(NAMES, again, want):
        assert g.tobytes() == w.tobytes(), name
    for conv in (torch.from_numpy, lambda a: torch.from_numpy(a).cuda()):
        got = aug.apply(recs, *(conv(a) for a in inputs))
        for name, g, w in zip(NAMES, got, want):
            np.testing.assert_array_equal(_np(g), w, err_msg=name)
    # a side stream is honoured: the call enqueues on the current stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = aug.apply(recs, *inputs)
    side.synchronize()
    for name, g, w in zip(NAMES, got, want):
        np.testing.assert_array_equal(_np(g), w, err_msg=name)


def test_call_and_batch_draw_like_the_reference_would():
    """`aug(...)` = `batch(...)` = draw + apply: the same generator state gives the same four outputs."""
    H, W = 120, 160
    inputs = _batch_inputs((70, 71, 72), H, W)
    a, b, c = _aug(3, do_flip=True), _aug(3, do_flip=True), _aug(3, do_flip=True)
    out, four = a(*inputs), c.batch(*inputs)
    want = b.apply(b.draw(H, W, 3), *inputs)
    assert len(out) == 4 and len(four) == 4
    for g, g4, w in zip(out, four, want):
        np.testing.assert_array_equal(_np(g), _np(w))
        np.testing.assert_array_equal(_np(g4), _np(w))
    np.testing.assert_array_equal(a.rng.get_state()[1], b.rng.get_state()[1])


def test_batch_feeds_one_train_step():
    import tf_raft_amd
    from tf_raft_amd import losses, training, weights as wm
    H, W, crop = 120, 160, (64, 96)
    data = _aug(5, crop).batch(*_batch_inputs((80, 81), H, W))
    model = tf_raft_amd.SmallRAFT(weights=wm.init_weights('small', seed=0), iters=2, iters_pred=2)
    model.compile(optimizer=training.AdamW(1e-4, 1e-3), clip_norm=1.0, loss=losses.sequence_loss, epe=losses.end_point_error)
    info = model.train_step(data)
    loss = float(info['loss'])
    report('sparse augment -> train_step', loss=loss)
    assert np.isfinite(loss) and loss > 0

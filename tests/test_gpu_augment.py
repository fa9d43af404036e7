"""FlowAugmentor on the device against the reference's own run (tests/golden/augment_golden.npz) -- EXACT equality, no tolerance:
uint8 crops and `valid` bit for bit, the flow bit for bit after the reference's float64 is narrowed to float32.

Beyond the fixture's cases the yardstick is `make_augment_golden.numpy_chain`: the reference's chain step by step on the stand-in
cv2 / albumentations, which tests/test_augment.py pins to the reference itself (the reference tree does not exist on the GPU box).
"""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, report

sys.path.insert(0, GOLDEN)
import make_augment_golden as mk                                   # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ('image1', 'image2', 'flow', 'valid')


def _np(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy()


def _aug(seed=0, crop=mk.CROP):
    from tf_raft_amd.augment import FlowAugmentor
    return FlowAugmentor(crop, rng=np.random.RandomState(seed), photo_rng=np.random.RandomState(seed + mk.PHOTO_SEED_OFFSET))


def _compare(got, want, what):
    """Exact, with the figures printed first: number of differing elements and the largest difference per output."""
    bad = {}
    for name, g in zip(NAMES, got):
        g, w = _np(g), np.asarray(want[name])
        if name == 'flow':
            w = w.astype(np.float32)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        diff = g != w
        if diff.any():
            bad[name] = (int(diff.sum()), float(np.abs(g.astype(np.float64) - w.astype(np.float64)).max()))
    report(what, **{f'{k}_differ': v[0] for k, v in bad.items()}, **{f'{k}_maxdiff': v[1] for k, v in bad.items()}, exact=not bad)
    assert not bad, (what, bad)


def test_apply_with_the_recorded_parameters_equals_the_fixture():
    for H, W, seed, rec, outs, _ in mk.load_fixture():
        img1, img2, flow = mk.case_inputs(seed, H, W)
        got = _aug().apply([rec], img1, img2, flow)
        assert all(g.is_cuda for g in got) and got[0].dtype == torch.uint8 and got[2].dtype == torch.float32 and got[3].dtype == torch.float32
        _compare(got, outs, f'augment fixture {H}x{W} seed {seed}')


def test_drawn_cases_equal_the_numpy_chain():
    """Cases the fixture has no room for: 40 draws on each of its two source sizes, and Sintel / Chairs sized frames at the
    training crop, each against the chain on the stand-ins."""
    for (H, W), crop, seeds in (((120, 160), mk.CROP, range(300, 340)), ((96, 128), mk.CROP, range(300, 340)),
                                ((436, 1024), (368, 496), range(400, 403)), ((384, 512), (368, 496), range(410, 412))):
        for seed in seeds:
            aug = _aug(seed, crop)
            rec = aug.draw(H, W)[0]
            img1, img2, flow = mk.case_inputs(seed, H, W)
            _compare(aug.apply([rec], img1, img2, flow), mk.numpy_chain(rec, img1, img2, flow, crop), f'augment chain {H}x{W} seed {seed}')


def _batch_inputs(seeds, H, W):
    samples = [mk.case_inputs(s, H, W) for s in seeds]
    return tuple(np.stack([s[k] for s in samples]) for k in range(3))


def test_a_batch_call_equals_the_per_sample_calls_and_the_means_buffer_serves_0_1_2_rectangles():
    H, W = 120, 160
    aug = _aug(7)
    recs, seed = [], 0
    while sorted(len(r['rects']) for r in recs[:3]) != [0, 1, 2]:      # a batch with 0, 1 and 2 rectangles, in any order
        recs = aug.draw(H, W, 3)
        seed += 1
        assert seed < 500
    recs += aug.draw(H, W, 2)
    i1, i2, fl = _batch_inputs(range(50, 55), H, W)
    got = aug.apply(recs, i1, i2, fl)
    assert tuple(got[0].shape) == (5, *mk.CROP, 3) and tuple(got[3].shape) == (5, *mk.CROP)
    for k, rec in enumerate(recs):
        single = aug.apply([rec], i1[k], i2[k], fl[k])
        assert tuple(single[0].shape) == (*mk.CROP, 3) and tuple(single[3].shape) == mk.CROP
        for name, b, s in zip(NAMES, got, single):
            np.testing.assert_array_equal(_np(b)[k], _np(s), err_msg=f'{name} of sample {k}')
        _compare(single, mk.numpy_chain(rec, i1[k], i2[k], fl[k]), f'augment batch sample {k} ({len(rec["rects"])} rectangles)')


def test_host_and_device_inputs_agree_numpy_and_torch():
    H, W = 120, 160
    aug = _aug(11)
    recs = aug.draw(H, W, 2)
    i1, i2, fl = _batch_inputs((60, 61), H, W)
    want = [_np(o) for o in aug.apply(recs, i1, i2, fl)]
    for conv in (torch.from_numpy, lambda a: torch.from_numpy(a).cuda()):
        got = aug.apply(recs, conv(i1), conv(i2), conv(fl))
        for name, g, w in zip(NAMES, got, want):
            np.testing.assert_array_equal(_np(g), w, err_msg=name)
    # a side stream is honoured: the call enqueues on the current stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = aug.apply(recs, i1, i2, fl)
    side.synchronize()
    for name, g, w in zip(NAMES, got, want):
        np.testing.assert_array_equal(_np(g), w, err_msg=name)


def test_call_and_batch_draw_like_the_reference_would():
    """`aug(...)` = draw + apply: the same generator state gives the same result as draw followed by apply, three outputs."""
    H, W = 120, 160
    i1, i2, fl = _batch_inputs((70, 71, 72), H, W)
    a, b = _aug(3), _aug(3)
    out = a(i1, i2, fl)
    assert len(out) == 3
    want = b.apply(b.draw(H, W, 3), i1, i2, fl)
    for g, w in zip(out, want):
        np.testing.assert_array_equal(_np(g), _np(w))
    np.testing.assert_array_equal(a.rng.get_state()[1], b.rng.get_state()[1])
    four = _aug(3).batch(i1, i2, fl)
    assert len(four) == 4
    np.testing.assert_array_equal(_np(four[3]), _np(want[3]))


def test_batch_feeds_one_train_step():
    import tf_raft_amd
    from tf_raft_amd import losses, training, weights as wm
    H, W, crop = 120, 160, (64, 96)
    i1, i2, fl = _batch_inputs((80, 81), H, W)
    data = _aug(5, crop).batch(i1, i2, fl)
    model = tf_raft_amd.SmallRAFT(weights=wm.init_weights('small', seed=0), iters=2, iters_pred=2)
    model.compile(optimizer=training.AdamW(1e-4, 1e-3), clip_norm=1.0, loss=losses.sequence_loss, epe=losses.end_point_error)
    info = model.train_step(data)
    loss = float(info['loss'])
    report('augment -> train_step', loss=loss)
    assert np.isfinite(loss) and loss > 0

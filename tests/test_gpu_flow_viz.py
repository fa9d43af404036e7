"""Flow colour coding on the GPU: ``raft_flow_rad_max_f32`` / ``raft_flow_to_image_u8`` (tf_raft_amd/csrc/flow_viz.hip) behind
``image_ops.flow_to_image``, ``RAFT.predict(output='image')`` and ``VisFlowCallback(colour_on_device=True)``.

The yardstick is the reference's own flow_viz.py, recorded in tests/golden/flow_viz_device_golden.npz (its generator lists what
each case is there for; tests/test_flow_viz_device.py pins the file on the CPU).  Pictures are held to the parity condition of
DESIGN.md section 13 (``assert_parity``: within one level, at most max(2, 1e-5 * values) values differing -- the rounding of
atan2 is the one source of difference), the radius to equality, and everything that compares two device computations to equality.
"""
import os

import numpy as np
import pytest
import torch

from test_any_size import _decode_png
from test_flow_viz_device import assert_parity, load_golden

pytestmark = pytest.mark.gpu

CHECKS, ARRAYS = load_golden()
BY_NAME = {c['name']: c for c in CHECKS}


def _np(t):
    return t.detach().cpu().numpy()


def _kw(c):
    return dict(size=c['size'], clip_flow=c['clip'], convert_to_bgr=c['bgr'], rad_max=c['rad_max'])


@pytest.mark.parametrize('name', [c['name'] for c in CHECKS])
def test_fixture(name):
    from tf_raft_amd import image_ops
    c = BY_NAME[name]
    flow = ARRAYS['flow/' + c['flow']]
    got = image_ops.flow_to_image(flow, **_kw(c))
    want = ARRAYS['img/' + name]
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    if c['rad_max'] is None:
        rad = _np(image_ops.flow_rad_max(flow, size=c['size'], clip_flow=c['clip']))
        assert rad.dtype == np.float32
        np.testing.assert_array_equal(rad, ARRAYS['rad/' + name], err_msg=name)       # a maximum is exact in any order
    assert_parity(_np(got), want, name)


def test_stream_out_reuse_repeat_and_rank():
    from tf_raft_amd import image_ops
    dev = torch.device('cuda')
    flow = torch.from_numpy(ARRAYS['flow/batch3']).to(dev)
    first = image_ops.flow_to_image(flow)
    again = image_ops.flow_to_image(flow)
    assert torch.equal(first, again)                                              # two runs
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = image_ops.flow_to_image(flow, clip_flow=2.0)
    side.synchronize()
    assert_parity(_np(on_side), ARRAYS['img/batch3_clip'], 'batch3_clip on a side stream')
    assert torch.equal(on_side, image_ops.flow_to_image(flow, clip_flow=2.0))
    # out=: the same buffer twice, and a base that is no multiple of 4 (the byte-wise head of every image)
    out = torch.full(tuple(first.shape), 7, dtype=torch.uint8, device=dev)
    res = image_ops.flow_to_image(flow, out=out)
    assert res.data_ptr() == out.data_ptr() and torch.equal(out, first)
    image_ops.flow_to_image(flow, clip_flow=2.0, out=out)
    assert torch.equal(out, on_side)
    for offset in (1, 2, 3):
        buf = torch.full((first.numel() + 8,), 7, dtype=torch.uint8, device=dev)
        view = buf[offset:offset + first.numel()].view(first.shape)
        image_ops.flow_to_image(flow, out=view)
        assert torch.equal(view, first), offset
        assert (buf[:offset] == 7).all() and (buf[offset + first.numel():] == 7).all(), offset      # nothing beyond the picture
    with pytest.raises(ValueError, match='out'):
        image_ops.flow_to_image(flow, out=out[:2])
    # (H, W, 2) and (N, H, W, 2); host and device input
    for n in range(3):
        one = image_ops.flow_to_image(ARRAYS['flow/batch3'][n])
        assert tuple(one.shape) == tuple(first.shape[1:]) and torch.equal(one, first[n]), n
    fixed = image_ops.flow_to_image(flow[1], rad_max=3.0)
    assert_parity(_np(fixed), ARRAYS['img/batch3_fixed'][1], 'batch3_fixed[1] alone')
    for bad in (flow[..., :1], flow[0, 0], flow.to(torch.int32)):
        with pytest.raises((ValueError, TypeError)):
            image_ops.flow_to_image(bad)


@pytest.mark.parametrize('size', [(61, 67), (70, 80), (70, 60), (64, 72), (1, 1), (3, 200)])
def test_size_is_crop_or_pad_then_colour(size):
    from tf_raft_amd import image_ops
    flow = torch.from_numpy(ARRAYS['flow/window']).cuda()
    for kw in ({}, {'clip_flow': 2.0, 'convert_to_bgr': True}, {'rad_max': 1.5}):
        fused = image_ops.flow_to_image(flow, size=size, **kw)
        two = image_ops.flow_to_image(image_ops.resize_with_crop_or_pad(flow, *size), **kw)
        assert tuple(fused.shape) == (2,) + size + (3,) and torch.equal(fused, two), (size, kw)
    clip = image_ops.flow_rad_max(flow, size=size, clip_flow=2.0)
    assert torch.equal(clip, image_ops.flow_rad_max(image_ops.resize_with_crop_or_pad(flow, *size), clip_flow=2.0))


def _frames(seed, B, H, W):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8) for _ in range(2))


@pytest.mark.parametrize('options', [{}, {'target_size': (64, 64)}, {'target_size': (64, 64), 'fit': 'resize'}],
                         ids=['plain', 'target_size', 'resize'])
def test_predict_returns_pictures(options):
    import tf_raft_amd
    from tf_raft_amd import image_ops
    from tf_raft_amd import weights as wm
    model = tf_raft_amd.RAFT(weights=wm.init_weights('raft', seed=2, perturb=True), iters_pred=2, **options)
    a, b = _frames(70, 3, 64, 72)
    flow = model.predict([a, b], batch_size=2)                                   # a ragged last batch
    assert flow.shape == (3, 64, 72, 2) and flow.dtype == np.float32
    for kw in ({}, {'clip_flow': 1.0, 'convert_to_bgr': True, 'rad_max': 0.5}):
        image = model.predict([a, b], batch_size=2, output='image', **kw)
        assert isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.shape == (3, 64, 72, 3)
        np.testing.assert_array_equal(image, _np(image_ops.flow_to_image(flow, **kw)))
    np.testing.assert_array_equal(model.predict([a, b], batch_size=2, output='flow'), flow)
    with pytest.raises(ValueError, match='output'):
        model.predict([a, b], batch_size=2, output='bogus')


def test_vis_flow_callback_colours_on_the_device(tmp_path):
    import tf_raft_amd
    from tf_raft.training import VisFlowCallback
    from tf_raft_amd import weights as wm
    model = tf_raft_amd.RAFT(weights=wm.init_weights('raft', seed=2, perturb=True), iters_pred=2)
    a, b = _frames(71, 1, 50, 70)
    dataset = [(a[0], b[0], None, None)]
    pictures = []
    for on_device in (False, True):
        cb = VisFlowCallback(dataset, target_size=(64, 72), logdir=str(tmp_path / f'device_{on_device}'), colour_on_device=on_device)
        cb.set_model(model)
        cb.on_epoch_end(0)
        pictures.append(_decode_png(os.path.join(cb.logdir, 'epoch001_001.png')))
    host, device = pictures
    assert host.shape == device.shape == (150, 70, 3)
    np.testing.assert_array_equal(device[:100], host[:100])                      # the two frames
    np.testing.assert_array_equal(device[:50], a[0])
    assert_parity(device[100:], host[100:], 'VisFlowCallback')

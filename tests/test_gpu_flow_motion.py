"""The camera's motion from a flow on the GPU: ``raft_flow_fit_motion_f32`` against the float64 NumPy
restatement of tests/test_flow_motion.py at every shared input, model, iteration count and mask polarity; ``raft_flow_residual_f32``
and ``raft_motion_flow_f32`` against theirs BIT FOR BIT; the public functions against the launch forms; and the model's
``camera_motion_step`` / ``stabilize_video`` against their compositions, bit for bit.

The bounds of the fit are derived, not measured.  Kernel and restatement are both float64 and differ only in the order in which a
solve's sums are added; tests/test_flow_motion.py shows that on these inputs three such orders agree within 2^-30 of every result,
a million times below a float32 ulp.  So only the one final rounding to float32 can differ, and by one ulp at most where the
float64 value happens to lie next to a rounding boundary: the linear entries (below 2 in size) within 2^-22, the translation within
2 ulps of max(1, |expected|), the inlier share and the RMS residual within 4 * 2^-24 relative; the status and the used share (a
count of at most 2^24 divided by H W) are equal.
"""
import numpy as np
import pytest
import torch

from conftest import report
from test_flow_motion import (IDS, MASKS, SHAPES, bits, expected_fit, inverted, motion_case, np_fit_motion, np_motion_flow, np_residual)

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xAB
MODELS = ('translation', 'similarity', 'affine')


def _np(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy()


def _dev():
    from tf_raft_amd import _dev as d
    return d.require_gpu()


def _guarded(n, dtype, device):
    """A buffer of ``n`` elements between two guard bands, every byte FILL: (whole buffer, the view a launch writes)."""
    size = torch.empty((), dtype=dtype).element_size()
    buf = torch.full(((2 * GUARD + n) * size,), FILL, dtype=torch.uint8, device=device)
    return buf, buf[GUARD * size:(GUARD + n) * size].view(dtype)


def _intact(buf, n_bytes):
    b = buf.cpu().numpy()
    band = (len(b) - n_bytes) // 2
    return bool((b[:band] == FILL).all() and (b[-band:] == FILL).all())


def _fit(flow, mask, invert, model, iterations, scale=1.0, dirty=False):
    """raft_flow_fit_motion_f32 through the library itself on device tensors, into guarded outputs and a workspace of exactly the
    size the library asks for (``dirty``: every double a NaN beforehand): (motion (N, 2, 3), stats (N, 4)) as host arrays."""
    from tf_raft_amd import _dev as d
    from tf_raft_amd._ffi import check
    N, H, W, _ = flow.shape
    lib = d.lib()
    doubles = int(lib.raft_flow_motion_workspace_doubles(N, H, W))
    assert doubles > 0
    buf_w, ws = _guarded(doubles, torch.float64, flow.device)
    if dirty:
        ws.fill_(float('nan'))
    buf_m, motion = _guarded(N * 6, torch.float32, flow.device)
    buf_s, stats = _guarded(N * 4, torch.float32, flow.device)
    check(lib.raft_flow_fit_motion_f32(d.ptr(flow), d.ptr(mask) if mask is not None else None, int(invert), d.ptr(motion), d.ptr(stats), N, H,
                                       W, model, iterations, scale, d.ptr(ws), d.stream_ptr()), 'fit_motion')
    torch.cuda.synchronize()
    assert _intact(buf_w, doubles * 8) and _intact(buf_m, N * 24) and _intact(buf_s, N * 16)
    return motion.cpu().numpy().reshape(N, 2, 3), stats.cpu().numpy().reshape(N, 4)


def _ulp(x):
    return np.spacing(np.maximum(np.float32(1), np.abs(x)).astype(np.float32)).astype(np.float64)


def assert_fit(got, want, what):
    """The derived bounds of the module's docstring."""
    motion, stats = got
    assert motion.dtype == np.float32 and stats.dtype == np.float32
    np.testing.assert_array_equal(stats[:, 3], want['stats'][:, 3], err_msg=f'{what}: status')
    np.testing.assert_array_equal(bits(stats[:, 0]), bits(want['stats'][:, 0]), err_msg=f'{what}: used share')
    lin = np.abs(motion[:, :, :2].astype(np.float64) - want['motion'][:, :, :2])
    tr = np.abs(motion[:, :, 2].astype(np.float64) - want['motion'][:, :, 2]) / _ulp(want['motion'][:, :, 2])
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.abs(stats[:, 1:3].astype(np.float64) - want['stats'][:, 1:3]) / np.abs(want['stats'][:, 1:3].astype(np.float64))
    rel = np.where(want['stats'][:, 1:3] == 0, np.where(stats[:, 1:3] == 0, 0.0, np.inf), rel)
    assert lin.max() <= 2.0 ** -22, (what, 'linear', lin.max())
    assert tr.max() <= 2.0, (what, 'translation in ulps', tr.max())
    assert rel.max() <= 4 * 2.0 ** -24, (what, 'inlier share and RMS, relative', rel.max())
    return lin.max(), tr.max(), rel.max()


def _on(a, dev):
    return None if a is None else torch.from_numpy(a.copy()).to(dev)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_the_fit_is_the_restatement_within_the_final_rounding(shape):
    dev = _dev()
    worst = np.zeros(3)
    for kind in MASKS:
        flow, mask = motion_case(shape, kind)
        f, m = _on(flow, dev), _on(mask, dev)
        mi = _on(None if mask is None else inverted(mask), dev)
        for model in range(3):
            for iterations in (1, 5):
                want = expected_fit(shape, kind, model, iterations)
                got = _fit(f, m, 0, model, iterations)
                worst = np.maximum(worst, assert_fit(got, want, (shape, kind, model, iterations)))
                if mask is not None:                                    # the other polarity says the same: the same bits
                    other = _fit(f, mi, 1, model, iterations)
                    assert_fit(other, want, (shape, kind, model, iterations, 'inverted'))
                    np.testing.assert_array_equal(bits(other[0]), bits(got[0]))
                    np.testing.assert_array_equal(bits(other[1]), bits(got[1]))
    report(f'fit_motion {shape}', linear=float(worst[0]), translation_ulps=float(worst[1]), stats_relative=float(worst[2]))


@pytest.mark.parametrize('shape', [SHAPES[3], SHAPES[4], SHAPES[6], SHAPES[7]], ids=[IDS[3], IDS[4], IDS[6], IDS[7]])
def test_the_fit_repeats_ignores_its_workspace_and_keeps_slices_apart(shape):
    dev = _dev()
    N, H, W = shape
    for kind in ('none', 'random'):
        flow, mask = motion_case(shape, kind)
        f, m = _on(flow, dev), _on(mask, dev)
        first = _fit(f, m, 0, 2, 5)
        for dirty in (False, True):                                     # twice the same bits; a workspace full of NaN changes nothing
            again = _fit(f, m, 0, 2, 5, dirty=dirty)
            np.testing.assert_array_equal(bits(again[0]), bits(first[0]))
            np.testing.assert_array_equal(bits(again[1]), bits(first[1]))
        # a slice on its own, and among other slices: the same bits
        for n in range(N):
            alone = _fit(f[n:n + 1].contiguous(), None if m is None else m[n:n + 1].contiguous(), 0, 2, 5)
            np.testing.assert_array_equal(bits(alone[0]), bits(first[0][n:n + 1]))
            np.testing.assert_array_equal(bits(alone[1]), bits(first[1][n:n + 1]))
        junk = torch.full_like(f, float('nan'))
        mixed = torch.cat([junk[:1], f, junk[:1] * 0 + 1e30], dim=0)
        mm = None if m is None else torch.cat([m[:1], m, m[:1]], dim=0)
        among = _fit(mixed, mm, 0, 2, 5)
        np.testing.assert_array_equal(bits(among[0][1:-1]), bits(first[0]))
        np.testing.assert_array_equal(bits(among[1][1:-1]), bits(first[1]))
        assert among[1][0, 3] == 2 and among[1][0, 0] == 0              # (a slice of NaN: nothing to fit, the identity)
        np.testing.assert_array_equal(among[0][0], np.array([[1, 0, 0], [0, 1, 0]], np.float32))


def test_the_load_paths_other_alignments_and_the_scale():
    """An even slice whose flow is only 8-byte aligned, or whose mask starts at an odd address, takes one pixel per trip instead of
    two: other partial sums, the same bounds."""
    dev = _dev()
    for shape in (SHAPES[5], SHAPES[6]):
        N, H, W = shape
        flow, mask = motion_case(shape, 'random')
        want = expected_fit(shape, 'random', 2, 5)
        base = torch.empty((N * H * W * 2 + 2,), device=dev)
        shifted = base[2:].view(N, H, W, 2)
        shifted.copy_(_on(flow, dev))
        assert shifted.data_ptr() % 16 == 8
        assert_fit(_fit(shifted, _on(mask, dev), 0, 2, 5), want, (shape, 'flow at 8 mod 16'))
        mbase = torch.empty((N * H * W + 1,), device=dev, dtype=torch.uint8)
        odd = mbase[1:].view(N, H, W)
        odd.copy_(_on(mask, dev))
        assert odd.data_ptr() % 2 == 1
        assert_fit(_fit(_on(flow, dev), odd, 0, 2, 5), want, (shape, 'mask at an odd address'))
    # the scale reaches the kernel
    flow, mask = motion_case(SHAPES[4], 'none')
    for scale in (0.25, 4.0):
        want = np_fit_motion(flow, None, 0, 1, 5, scale)
        got = _fit(_on(flow, dev), None, 0, 1, 5, scale)
        assert_fit(got, want, ('scale', scale))
        assert not np.array_equal(bits(got[0]), bits(expected_fit(SHAPES[4], 'none', 1, 5)['motion']))


def _residual(flow, motion, threshold, want_residual=True, want_moving=True):
    from tf_raft_amd import _dev as d
    from tf_raft_amd._ffi import check
    N, H, W, _ = flow.shape
    buf_r, residual = _guarded(N * H * W * 2, torch.float32, flow.device)
    buf_m, moving = _guarded(N * H * W, torch.uint8, flow.device)
    check(d.lib().raft_flow_residual_f32(d.ptr(flow), d.ptr(motion), d.ptr(residual) if want_residual else None,
                                         d.ptr(moving) if want_moving else None, N, H, W, threshold, d.stream_ptr()), 'residual')
    torch.cuda.synchronize()
    assert _intact(buf_r, N * H * W * 8) and _intact(buf_m, N * H * W)
    untouched = lambda t: bool((t.view(torch.uint8) == FILL).all())      # noqa: E731
    assert want_residual or untouched(residual)
    assert want_moving or untouched(moving)
    return residual.cpu().numpy().reshape(N, H, W, 2), moving.cpu().numpy().reshape(N, H, W)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_the_residual_and_the_dense_flow_are_their_restatements_bit_for_bit(shape):
    from tf_raft_amd import image_ops
    dev = _dev()
    N, H, W = shape
    flow, _ = motion_case(shape, 'none')
    rng = np.random.default_rng(11)
    motions = [expected_fit(shape, 'none', 2, 5)['motion'].copy(),
               (np.array([[1, 0, 0], [0, 1, 0]]) + rng.normal(0, 0.1, (N, 2, 3)) * np.array([1, 1, 30])).astype(np.float32)]
    f = _on(flow, dev)
    for motion in motions:
        m = _on(motion, dev)
        for threshold in (1.0, 0.0, 7.5):
            want_r, want_m = np_residual(flow, motion, threshold)
            got_r, got_m = _residual(f, m, threshold)
            np.testing.assert_array_equal(bits(got_r), bits(want_r))
            np.testing.assert_array_equal(got_m, want_m)
        only_r, _ = _residual(f, m, 1.0, want_moving=False)
        _, only_m = _residual(f, m, 1.0, want_residual=False)
        want_r, want_m = np_residual(flow, motion, 1.0)
        np.testing.assert_array_equal(bits(only_r), bits(want_r))
        np.testing.assert_array_equal(only_m, want_m)
        dense = image_ops.motion_flow_launch(m, H, W)
        np.testing.assert_array_equal(bits(_np(dense)), bits(np_motion_flow(motion, H, W).astype(np.float32)))
    # the identity has no flow, and zero flow fits the identity exactly
    eye = torch.tensor([[[1.0, 0, 0], [0, 1, 0]]], device=dev).repeat(N, 1, 1)
    assert not _np(image_ops.motion_flow_launch(eye, H, W)).any()
    got = _fit(torch.zeros_like(f), None, 0, 2, 5)
    np.testing.assert_array_equal(got[0], _np(eye))


@pytest.mark.parametrize('shape', [SHAPES[4], SHAPES[5]], ids=[IDS[4], IDS[5]])
def test_the_public_functions(shape):
    from tf_raft_amd import image_ops
    dev = _dev()
    N, H, W = shape
    flow, mask = (a.copy() for a in motion_case(shape, 'random'))          # (writable: torch.from_numpy asks for it)
    f, m = _on(flow, dev), _on(mask, dev)
    for model in MODELS:
        want = image_ops.fit_motion_launch(f, m, False, model, 5, 1.0)
        assert tuple(want[0].shape) == (N, 2, 3) and tuple(want[1].shape) == (N, 4) and type(want[0]) is torch.Tensor
        assert_fit((_np(want[0]), _np(want[1])), expected_fit(shape, 'random', MODELS.index(model), 5), ('launch form', model))
        # host arrays in, device tensors out; float64 narrows; bool masks; the other polarity
        got = image_ops.fit_motion(flow.astype(np.float64), mask=mask != 0, model=model, return_stats=True)
        assert got[0].is_cuda and got[0].dtype == torch.float32 and tuple(got[0].shape) == (N, 2, 3) and tuple(got[1].shape) == (N, 4)
        np.testing.assert_array_equal(bits(_np(got[0])), bits(_np(want[0])))
        np.testing.assert_array_equal(bits(_np(got[1])), bits(_np(want[1])))
        occ = image_ops.fit_motion(f, occluded=torch.from_numpy(inverted(mask)).to(dev), model=model)
        np.testing.assert_array_equal(bits(_np(occ)), bits(_np(want[0])))
    # leading axes: none, and two
    one = image_ops.fit_motion(flow[0], mask=mask[0], return_stats=True)
    assert tuple(one[0].shape) == (2, 3) and tuple(one[1].shape) == (4,)
    want = image_ops.fit_motion_launch(f[:1], m[:1])
    np.testing.assert_array_equal(bits(_np(one[0])), bits(_np(want[0])[0]))
    np.testing.assert_array_equal(bits(_np(one[1])), bits(_np(want[1])[0]))
    two = image_ops.fit_motion(flow[None], iterations=1, scale=2.0, model='similarity')
    assert tuple(two.shape) == (1, N, 2, 3)
    np.testing.assert_array_equal(bits(_np(two)[0]), bits(_np(image_ops.fit_motion_launch(f, None, False, 'similarity', 1, 2.0)[0])))
    # the residual and the dense flow
    motion = image_ops.fit_motion(f, mask=m)
    r_launch, m_launch = image_ops.residual_flow_launch(f, motion.as_subclass(torch.Tensor), 1.0)
    want_r, want_m = np_residual(flow, _np(motion), 1.0)
    np.testing.assert_array_equal(bits(_np(r_launch)), bits(want_r))
    np.testing.assert_array_equal(_np(m_launch), want_m)
    only = image_ops.residual_flow(flow, _np(motion))
    assert isinstance(only, torch.Tensor) and tuple(only.shape) == (N, H, W, 2)
    np.testing.assert_array_equal(bits(_np(only)), bits(want_r))
    r, mv = image_ops.residual_flow(flow[-1], _np(motion)[-1], threshold=1.0)
    assert tuple(r.shape) == (H, W, 2) and tuple(mv.shape) == (H, W) and mv.dtype == torch.uint8
    np.testing.assert_array_equal(bits(_np(r)), bits(want_r[-1]))
    np.testing.assert_array_equal(_np(mv), want_m[-1])
    none_r, mask_only = image_ops.residual_flow_launch(f, motion.as_subclass(torch.Tensor), 1.0, want_residual=False)
    assert none_r is None
    np.testing.assert_array_equal(_np(mask_only), want_m)
    dense = image_ops.motion_flow(_np(motion)[None], H, W)
    assert tuple(dense.shape) == (1, N, H, W, 2)
    np.testing.assert_array_equal(bits(_np(dense)[0]), bits(np_motion_flow(_np(motion), H, W).astype(np.float32)))
    assert tuple(image_ops.motion_flow(motion[0], H, W).shape) == (H, W, 2)


# ------------------------------------------------------------------ the model
def _plain(t):
    return t.detach().as_subclass(torch.Tensor)


def _model(route):
    import tf_raft_amd
    from tf_raft_amd import weights as wm
    wts = wm.init_weights('small', seed=6, perturb=True)
    if route == 'plain':
        return tf_raft_amd.SmallRAFT(weights=wts, iters_pred=3), (64, 96)
    return tf_raft_amd.SmallRAFT(weights=wts, iters_pred=3, target_size=(64, 96), fit='resize'), (100, 150)


def _footage(H, W, T=5, seed=70, dtype=np.uint8):
    """One video of T frames: a texture that shifts by a pixel or two per frame, plus noise."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0, 255, (H + 16, W + 16, 3))
    video = np.stack([base[8 + t:8 + t + H, 8 - t:8 - t + W] for t in range(T)])
    video = (video + rng.normal(0, 4, video.shape)).clip(0, 255)
    return np.round(video).astype(np.uint8) if dtype == np.uint8 else video.astype(np.float32)


@pytest.mark.parametrize('route', ['plain', 'resize'])
def test_camera_motion_step_is_its_composition(route):
    from tf_raft_amd import image_ops
    from tf_raft_amd.model import CameraMotion
    model, (H, W) = _model(route)
    video = _footage(H, W, dtype=np.float32)
    pair = (video[:2], video[1:3])
    for kw in ({}, {'model': 'similarity', 'occlusion_test': 'range', 'iterations': 2, 'scale': 0.5, 'threshold': 0.25}):
        got = model.camera_motion_step(pair, **kw)
        assert isinstance(got, CameraMotion) and all(t.is_cuda for t in got)
        assert tuple(got.motion.shape) == (2, 2, 3) and tuple(got.stats.shape) == (2, 4) and tuple(got.residual.shape) == (2, H, W, 2)
        assert tuple(got.moving.shape) == (2, H, W) and got.moving.dtype == torch.uint8
        res = model.predict_step_bidirectional(pair, occlusion_test=kw.get('occlusion_test', 'consistency'))
        np.testing.assert_array_equal(bits(_np(got.forward)), bits(_np(res.forward)))
        np.testing.assert_array_equal(_np(got.occluded_forward), _np(res.occluded_forward))
        motion, stats = image_ops.fit_motion_launch(_plain(res.forward), _plain(res.occluded_forward), True, kw.get('model', 'affine'),
                                                    kw.get('iterations', 5), kw.get('scale', 1.0))
        residual, moving = image_ops.residual_flow_launch(_plain(res.forward), motion, kw.get('threshold', 1.0))
        np.testing.assert_array_equal(bits(_np(got.motion)), bits(_np(motion)))
        np.testing.assert_array_equal(bits(_np(got.stats)), bits(_np(stats)))
        np.testing.assert_array_equal(bits(_np(got.residual)), bits(_np(residual)))
        np.testing.assert_array_equal(_np(got.moving), _np(moving))
    report(f'camera_motion_step ({route})', used=float(_np(got.stats)[0, 0]), inliers=float(_np(got.stats)[0, 1]),
           rms=float(_np(got.stats)[0, 2]), status=float(_np(got.stats)[0, 3]), moving=float(_np(got.moving).mean()))


@pytest.mark.parametrize('route', ['plain', 'resize'])
def test_stabilize_video_is_its_composition_and_a_window_of_one_frame_returns_the_frames(route):
    from tf_raft_amd import image_ops
    from tf_raft_amd.video import smooth_trajectory
    model, (H, W) = _model(route)
    dev = _dev()
    for dtype in (np.uint8, np.float32):
        video = _footage(H, W, dtype=dtype)
        T = video.shape[0]
        same = model.stabilize_video(video, radius=0)
        assert isinstance(same, np.ndarray) and same.dtype == dtype and same.shape == video.shape
        np.testing.assert_array_equal(same, video)                           # exactly, float32 too: the identity samples the taps
        got, motions, corrections = model.stabilize_video(torch.from_numpy(video), radius=2, batch_size=3, return_motion=True)
        assert got.dtype == dtype and got.shape == video.shape and motions.shape == (T - 1, 2, 3) and motions.dtype == np.float32
        assert corrections.shape == (T, 2, 3) and corrections.dtype == np.float64
        # the composition: the pairs' forward flows fitted with their occlusion masks, smoothed, every frame resampled
        res = model.predict_bidirectional([video[:-1], video[1:]], batch_size=3)
        fit, _ = image_ops.fit_motion_launch(torch.from_numpy(res.forward).to(dev), torch.from_numpy(res.occluded_forward).to(dev), True,
                                             'similarity', 5, 1.0)
        np.testing.assert_array_equal(bits(motions), bits(_np(fit)))
        want_c = smooth_trajectory(_np(fit), 2)
        np.testing.assert_array_equal(corrections, want_c)
        records = image_ops.view_records(image_ops.MotionViews(want_c), T, dev)
        seen = image_ops.view_frames_launch(torch.from_numpy(video).to(dev).to(torch.float32), records, (H, W))
        want = _np(seen.round().clamp(0, 255).to(torch.uint8)) if dtype == np.uint8 else _np(seen)
        np.testing.assert_array_equal(got, want)
        assert not np.array_equal(got, video)
        # one pair per call chains the flows of one pair per call
        _, motions1, _ = model.stabilize_video(video, radius=2, batch_size=1, return_motion=True)
        res = model.predict_bidirectional([video[:-1], video[1:]], batch_size=1)
        fit, _ = image_ops.fit_motion_launch(torch.from_numpy(res.forward).to(dev), torch.from_numpy(res.occluded_forward).to(dev), True,
                                             'similarity', 5, 1.0)
        np.testing.assert_array_equal(bits(motions1), bits(_np(fit)))
    report(f'stabilize_video ({route})', shift=float(np.abs(motions[:, :, 2]).max()), correction=float(np.abs(corrections[:, :, 2]).max()))

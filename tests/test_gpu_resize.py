"""Frames of any size by interpolation, on the GPU: the table-driven resize kernel against the float64 restatement of
tests/test_resize.py, the public ops, and ``fit='resize'`` on RAFT / SmallRAFT through every inference entry point.

The kernel's bound.  An output is ``factor * sum_b wx[b] * sum_a wy[a] * x[a, b]`` in float32 with ``ty x tx`` taps at most.  The
weights are non-negative, sum to 1 per axis in float64 and are each rounded ONCE to float32 (relative error <= u = 2^-24), the
sources are exact (uint8, or the float32 values themselves).  To first order in u every term ``wx wy x`` carries the two weight
roundings, its two products and the additions it passes through -- at most ``ty + tx + 2`` roundings, fewer than ``ty * tx + 2``
whenever there is more than one tap -- so the sum of products is within ``(ty * tx + 2) u max|x|`` of the exact one (the weights
summing to 1 turn the sum of |terms| into at most ``max|x|``); the channel factor, itself rounded once, adds two more roundings of
the scaled value:

    |got - want| <= (ty * tx + 4) * 2^-24 * max|x| * max(1, |factor|)

which is 9e-5 .. 8.4e-4 for 0..255 data at the shapes below (an fp32 emulation of the sum stays under 4.1e-5).  The model's route
is compared bit for bit: it runs the same kernels on the same bytes.
"""
import functools

import numpy as np
import pytest
import torch

from test_resize import SHAPES, np_axis_matrix, np_max_taps, np_resize

pytestmark = pytest.mark.gpu

U = 2.0 ** -24

# (Hs, Ws) -> (Ht, Wt)                what it exercises
# (37, 53)   -> (64, 72)              up both axes, clamped single-tap borders
# (150, 201) -> (64, 88)              down both axes, 5 x 5 taps, 603-byte uint8 rows
# (45, 200)  -> (64, 96)              up one axis, down the other
# (131, 67)  -> (64, 64)
# (1, 5)     -> (64, 64)              one source row
# (3, 5)     -> (1, 1)                everything into one pixel
# (530, 70)  -> (64, 64)              17 taps
# (9, 1242)  -> (8, 1248)             KITTI-wide rows
# (64, 96)   -> (45, 200)             the flow direction
# (64, 88)   -> (150, 201)            the flow direction
assert len(SHAPES) == 10


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _matrix(n_in, n_out, antialias):
    return np_axis_matrix(n_in, n_out, antialias)


def _want(x, ht, wt, antialias, factors=None):
    """np_resize with the axis matrices shared between the cases."""
    x = np.asarray(x, np.float64)
    out = np.einsum('yh,...hwc->...ywc', _matrix(x.shape[-3], ht, antialias), x)
    out = np.einsum('xw,...ywc->...yxc', _matrix(x.shape[-2], wt, antialias), out)
    return out if factors is None else out * np.asarray(factors, np.float64)


_max_taps = functools.lru_cache(maxsize=None)(np_max_taps)


def _bound(src, dst, antialias, maxabs, factor=1.0):
    ty, tx = _max_taps(src[0], dst[0], antialias), _max_taps(src[1], dst[1], antialias)
    return (ty * tx + 4) * U * maxabs * max(1.0, abs(factor))


def _data(rng, shape, kind):
    if kind == 'u8':
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    return rng.uniform(0, 255, size=shape).astype(np.float32)


def _skewed(x, skew):
    """``x`` on the device, ``skew`` elements past a 16-byte boundary, with NaN (0xAB for bytes) around it."""
    t = torch.as_tensor(x)
    slab = torch.full((t.numel() + 64,), float('nan') if t.dtype == torch.float32 else 0xAB, dtype=t.dtype, device='cuda')
    slab[32 + skew:32 + skew + t.numel()] = t.reshape(-1).cuda()
    return slab[32 + skew:32 + skew + t.numel()].view(t.shape)


def _run(op, x, ht, wt, antialias, src_skew=0, dst_skew=0):
    """One launch into a NaN slab: the result, after checking that the guard bands on both sides are still NaN."""
    shape = tuple(x.shape[:-3]) + (ht, wt, x.shape[-1])
    n = int(np.prod(shape))
    slab = torch.full((n + 64,), float('nan'), device='cuda')
    out = slab[32 + dst_skew:32 + dst_skew + n].view(shape)
    src = _skewed(x, src_skew)
    assert src.data_ptr() % 16 == (src_skew * src.element_size()) % 16 and out.data_ptr() % 16 == (4 * dst_skew) % 16
    got = op(src, ht, wt, antialias=antialias, out=out)
    assert got.data_ptr() == out.data_ptr() and got.dtype == torch.float32 and tuple(got.shape) == shape
    assert torch.isnan(slab[:32 + dst_skew]).all() and torch.isnan(slab[32 + dst_skew + n:]).all(), 'written outside the destination'
    res = _np(out)
    assert not np.isnan(res).any(), 'an element of the destination was left unwritten'
    return res


@pytest.mark.parametrize('src,dst', SHAPES, ids=[f'{s[0]}x{s[1]}to{t[0]}x{t[1]}' for s, t in SHAPES])
def test_resize_kernel_is_the_float64_rule(src, dst):
    """The bound of the module's docstring, at every shape, both modes, 1 / 2 / 3 channels, one and three images, both source
    types; with two channels also as a flow (channel factors); and with source and destination 1 and 3 elements off 16 bytes."""
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(5)
    (hs, ws), (ht, wt) = src, dst
    worst = 0.0
    for antialias in (False, True):
        for C_ in (1, 2, 3):
            for N in (1, 3):
                for kind in ('u8', 'f32'):
                    x = _data(rng, (N, hs, ws, C_), kind)
                    want = _want(x, ht, wt, antialias)
                    bound = _bound(src, dst, antialias, float(x.max()))
                    runs = [(0, 0)] + ([(1, 1), (3, 3), (0, 1), (3, 0)] if N == 1 else [])
                    for src_skew, dst_skew in runs:
                        err = np.abs(_run(image_ops.resize, x, ht, wt, antialias, src_skew, dst_skew) - want).max()
                        worst = max(worst, err / bound)
                        assert err <= bound, (kind, (N, hs, ws, C_), (ht, wt), antialias, src_skew, dst_skew, err, bound)
                    # the public op from the host, (N, H, W, C) and (H, W, C)
                    assert np.abs(_np(image_ops.resize(x[0], ht, wt, antialias=antialias)) - want[0]).max() <= bound
                if C_ == 2:
                    f = (rng.normal(size=(2, 3, hs, ws, 2)) * 40).astype(np.float32)             # any leading axes
                    factors = (wt / ws, ht / hs)
                    want = _want(f, ht, wt, antialias, factors)
                    bound = _bound(src, dst, antialias, float(np.abs(f).max()), max(factors))
                    for skew in (0, 1):
                        err = np.abs(_run(image_ops.resize_flow, f, ht, wt, antialias, skew, skew) - want).max()
                        worst = max(worst, err / bound)
                        assert err <= bound, ('flow', (hs, ws), (ht, wt), antialias, skew, err, bound)
    print(f'[resize] {src} -> {dst}: worst error / bound = {worst:.3f}')


def test_a_shrink_ratio_of_sixteen_and_the_refusal_beyond_the_kernel():
    """34 taps per axis work; what the kernel cannot take is a ValueError before any launch, never another result."""
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(6)
    src, dst = (1040, 130), (64, 8)                                      # ratios 16.25 and 16.25
    assert np_max_taps(1040, 64, True) >= 33 and np_max_taps(130, 8, True) >= 33
    for kind in ('u8', 'f32'):
        x = _data(rng, (2,) + src + (3,), kind)
        err = np.abs(_run(image_ops.resize, x, *dst, True) - _want(x, *dst, True)).max()
        assert err <= _bound(src, dst, True, float(x.max())), (kind, err)
    out = torch.full((1, 4, 4, 3), float('nan'), device='cuda')
    x = torch.zeros((1, 4, 400, 3), device='cuda')
    with pytest.raises(ValueError, match='taps'):
        image_ops.resize(x, 4, 4, antialias=True, out=out)                # 100 : 1 with the widened triangle: 201 taps
    assert torch.isnan(out).all()
    assert tuple(image_ops.resize(x, 4, 4, antialias=False).shape) == (1, 4, 4, 3)       # two taps whatever the ratio
    with pytest.raises(ValueError, match='taps'):
        image_ops.resize(torch.zeros((1, 70, 70, 200), device='cuda'), 8, 8, antialias=True)   # 19 taps of 200 channels


def test_a_sample_of_a_batch_is_bitwise_the_sample_alone_and_calls_repeat():
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(8)
    for (hs, ws), (ht, wt), C_, kind in (((150, 201), (64, 88), 3, 'u8'), ((64, 96), (45, 200), 2, 'f32'), ((37, 53), (64, 72), 1, 'f32')):
        x = torch.as_tensor(_data(rng, (4, hs, ws, C_), kind)).cuda()
        for antialias in (False, True):
            whole = _np(image_ops.resize(x, ht, wt, antialias=antialias))
            np.testing.assert_array_equal(_np(image_ops.resize(x, ht, wt, antialias=antialias)), whole)
            for n in range(4):
                np.testing.assert_array_equal(_np(image_ops.resize(x[n:n + 1], ht, wt, antialias=antialias))[0], whole[n])
                np.testing.assert_array_equal(_np(image_ops.resize(x[n], ht, wt, antialias=antialias)), whole[n])


def test_element_offsets_beyond_two_to_the_31():
    """1025 predictions of 1024 x 1024 x 2 are 2^31 + 2^21 elements: the last one, whose offsets do not fit 32 bits, is bitwise
    the same prediction resized alone, and nothing is written behind it."""
    from tf_raft_amd import image_ops
    n, side = 1025, 1024
    src = torch.as_tensor(np.random.default_rng(9).normal(size=(n, 8, 8, 2)).astype(np.float32)).cuda()
    per = side * side * 2
    assert n * per > 2 ** 31
    slab = torch.empty((n * per + 64,), device='cuda')
    slab[-64:] = float('nan')
    slab[(n - 1) * per:n * per] = float('nan')
    out = slab[:n * per].view(n, side, side, 2)
    image_ops.resize_flow(src, side, side, out=out)
    for k in (0, 511, n - 1):
        assert torch.equal(out[k], image_ops.resize_flow(src[k], side, side).as_subclass(torch.Tensor)), k
    assert torch.isnan(slab[-64:]).all()


def test_resize_flow_scales_u_by_the_width_ratio_and_v_by_the_height_ratio():
    from tf_raft_amd import image_ops
    flow = np.empty((2, 64, 96, 2), np.float32)
    flow[..., 0], flow[..., 1] = 1.0, 2.0
    for antialias in (False, True):
        got = _np(image_ops.resize_flow(flow, 32, 192, antialias=antialias))
        assert got.shape == (2, 32, 192, 2)
        bound = _bound((64, 96), (32, 192), antialias, 2.0, 2.0)
        assert np.abs(got[..., 0] - 2.0).max() <= bound and np.abs(got[..., 1] - 1.0).max() <= bound


def test_equal_sizes_launch_nothing():
    from tf_raft_amd import image_ops
    x = torch.rand((2, 30, 40, 3), device='cuda')
    assert image_ops.resize(x, 30, 40).data_ptr() == x.data_ptr()
    assert image_ops.resize(x[0], 30, 40, antialias=True).data_ptr() == x[0].data_ptr()
    f = torch.rand((3, 2, 30, 40, 2), device='cuda')
    assert image_ops.resize_flow(f, 30, 40).data_ptr() == f.data_ptr()
    u = torch.randint(0, 256, (2, 30, 40, 3), dtype=torch.uint8, device='cuda')
    same = image_ops.resize(u, 30, 40)
    assert same.dtype == torch.float32 and torch.equal(same.as_subclass(torch.Tensor), u.to(torch.float32))
    assert image_ops.resize(np.zeros((30, 40, 1), np.float64), 30, 40).dtype == torch.float32


def test_resize_follows_the_current_stream_and_rejects_what_it_cannot_take():
    from tf_raft_amd import image_ops
    side = torch.cuda.Stream()
    x = torch.arange(2 * 30 * 40 * 2, dtype=torch.float32, device='cuda').view(2, 30, 40, 2) % 251 + 1
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        y = x * 2                                                       # produced on `side`: only stream order makes the resize see it
        z = image_ops.resize(y, 33, 47)                                 # (tables of sizes no other test uses: uploaded on `side`)
        zf = image_ops.resize_flow(y, 33, 47)
    side.synchronize()
    want = _want(_np(x) * 2, 33, 47, False)
    assert np.abs(_np(z) - want).max() <= _bound((30, 40), (33, 47), False, 502.0)
    assert np.abs(_np(zf) - want * (47 / 40, 33 / 30)).max() <= _bound((30, 40), (33, 47), False, 502.0, 47 / 40)
    z2 = image_ops.resize(y, 33, 47)                                    # the cached tables, now from another stream than their own
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(z2), _np(z))
    with pytest.raises(TypeError):
        image_ops.resize(torch.zeros((1, 4, 4, 1), dtype=torch.int32), 8, 8)
    with pytest.raises(TypeError):
        image_ops.resize(torch.zeros((1, 4, 4, 1), dtype=torch.float16, device='cuda'), 8, 8)
    with pytest.raises(TypeError):
        image_ops.resize_flow(torch.zeros((1, 4, 4, 2), dtype=torch.uint8), 8, 8)
    with pytest.raises(ValueError):
        image_ops.resize(x[0, 0], 8, 8)
    with pytest.raises(ValueError):
        image_ops.resize(x, 0, 8)
    with pytest.raises(ValueError):
        image_ops.resize(torch.zeros((0, 4, 4, 3)), 8, 8)
    with pytest.raises(ValueError):
        image_ops.resize_flow(torch.zeros((1, 4, 4, 3)), 8, 8)           # a flow has two channels
    with pytest.raises(ValueError):
        image_ops.resize(x, 32, 48, out=torch.empty((2, 32, 48, 1), device='cuda'))
    with pytest.raises(ValueError):
        image_ops.resize(x, 32, 48, out=torch.empty((2, 32, 48, 4), device='cuda')[..., :2])      # not contiguous
    with pytest.raises(ValueError):
        image_ops.resize(x, 32, 48, out=torch.empty((2, 32, 48, 2), device='cuda', dtype=torch.float64))


# ------------------------------------------------------------------ the model option
def _cls(variant):
    import tf_raft_amd
    return tf_raft_amd.RAFT if variant == 'raft' else tf_raft_amd.SmallRAFT


def _frames(seed, B, H, W, dtype):
    rng = np.random.default_rng(seed)
    return tuple(_data(rng, (B, H, W, 3), 'u8' if dtype == np.uint8 else 'f32') for _ in range(2))


def _route(plain, i1, i2, size, antialias=True, entry='call'):
    """image_ops.resize -> a model WITHOUT the option -> image_ops.resize_flow back: every prediction (or the last one)."""
    from tf_raft_amd import image_ops
    H, W = i1.shape[1:3]
    r1, r2 = (image_ops.resize(x, *size, antialias=antialias) for x in (i1, i2))
    if entry == 'call':
        preds = torch.stack([p.as_subclass(torch.Tensor) for p in plain([r1, r2])])
        return [_np(p) for p in image_ops.resize_flow(preds, H, W, antialias=antialias)]
    return _np(image_ops.resize_flow(plain.predict_step((r1, r2)), H, W, antialias=antialias))


CASES = [(np.uint8, (2, 45, 200)), (np.float32, (2, 150, 201))]


@pytest.mark.parametrize('pipeline', [False, True], ids=['serial', 'pipelined'])
@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_fit_resize_is_bitwise_resize_model_resize_flow(variant, pipeline):
    """__call__, predict_step and predict(batch_size=1) with ``target_size=(64, 96), fit='resize'`` on uint8 and float frames."""
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=4, perturb=True)
    model = _cls(variant)(weights=wts, iters_pred=3, target_size=(64, 96), fit='resize', pipeline=pipeline)
    assert model.fit == 'resize' and model.antialias is True
    plain = _cls(variant)(weights=wts, iters_pred=3, pipeline=False, loop_concurrency=model.lanes if pipeline else None)
    for seed, (dtype, (B, H, W)) in enumerate(CASES):
        i1, i2 = _frames(20 + seed, B, H, W, dtype)
        want = _route(plain, i1, i2, (64, 96))
        got = model([i1, i2])
        assert len(got) == 3
        if pipeline:
            assert all(g.__dict__.get('_pending') is not None for g in got)      # the caller's stream did not wait for the loop
        base = got[0].data_ptr()
        for k, (g, w_) in enumerate(zip(got, want)):
            assert tuple(g.shape) == (B, H, W, 2) and g.is_contiguous() and g.data_ptr() == base + 4 * k * B * H * W * 2
            np.testing.assert_array_equal(_np(g), w_)
        assert np.abs(want[-1]).max() > 0
        np.testing.assert_array_equal(_np(model.predict_step((i1, i2))), want[-1])
        np.testing.assert_array_equal(_np(model.predict_step((torch.as_tensor(i1).cuda(), torch.as_tensor(i2).cuda()))), want[-1])
        single = np.concatenate([_route(plain, i1[k:k + 1], i2[k:k + 1], (64, 96), entry='predict_step') for k in range(B)])
        pred = model.predict([i1, i2], batch_size=1)
        assert isinstance(pred, np.ndarray) and pred.shape == (B, H, W, 2)
        np.testing.assert_array_equal(pred, single)
        with pytest.raises(ValueError):
            model([i1, i2], training=True)                                # training-mode calls keep their check


@pytest.mark.parametrize('pipeline', [False, True], ids=['serial', 'pipelined'])
@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_test_step_with_fit_resize_scores_at_the_frames_own_size(variant, pipeline):
    """Ground truth of the frames' own size against the resized-back last prediction.  Both sides reduce the same float values
    with the same kernel; the mean comes back as float32, so one float32 ulp (1.2e-7 relative) is allowed, as in
    tests/test_gpu_any_size.py::test_test_step_on_raw_frames_equals_the_reference_route."""
    from tf_raft_amd import losses
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=9, perturb=True)
    model = _cls(variant)(weights=wts, iters_pred=3, target_size=(64, 96), fit='resize', pipeline=pipeline)
    model.compile(optimizer=None)
    plain = _cls(variant)(weights=wts, iters_pred=3, pipeline=False, loop_concurrency=model.lanes if pipeline else None)
    rng = np.random.default_rng(31)
    for seed, (dtype, (B, H, W)) in enumerate(CASES):
        model.reset_metrics()
        i1, i2 = _frames(50 + seed, B, H, W, dtype)
        flow = (rng.normal(size=(B, H, W, 2)) * 2).astype(np.float32)
        valid = rng.uniform(size=(B, H, W)) < 0.9
        got = {k: float(v) for k, v in model.test_step((i1, i2, flow, valid)).items()}
        last = torch.as_tensor(_route(plain, i1, i2, (64, 96), entry='predict_step')).cuda()
        want = {k: float(v) for k, v in losses.end_point_error([flow, valid], last).items()}
        for k in ('u1', 'u3', 'u5'):
            assert abs(got[k] - want[k]) <= 1.2e-7 * abs(want[k]), (k, got[k], want[k])
        assert want['epe'] > 0 and abs(got['epe'] - want['epe']) <= 1.2e-7 * abs(want['epe']), (got['epe'], want['epe'])


@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_auto_target_sizes_equal_sizes_and_the_default(variant):
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=5, perturb=True)
    plain = _cls(variant)(weights=wts, iters_pred=3)
    auto = _cls(variant)(weights=wts, iters_pred=3, target_size='auto', fit='resize', antialias=False)
    assert auto._model_size(61, 100) == (64, 104)
    i1, i2 = _frames(2, 1, 61, 100, np.float32)
    got = auto([i1, i2])
    want = _route(plain, i1, i2, (64, 104), antialias=False)
    for g, w_ in zip(got, want):
        assert tuple(g.shape) == (1, 61, 100, 2)
        np.testing.assert_array_equal(_np(g), w_)
    # frames that already have the model's size: the model without the option, on the buffers that came in
    fixed = _cls(variant)(weights=wts, iters_pred=3, target_size=(64, 96), fit='resize')
    a, b = (torch.as_tensor(x).cuda() for x in _frames(7, 2, 64, 96, np.float32))
    for g, w_ in zip(fixed([a, b]), plain([a, b])):
        np.testing.assert_array_equal(_np(g), _np(w_))
    fa, fb, window = fixed._fit_frames(a, b)
    assert window is None and fa.data_ptr() == a.data_ptr() and fb.data_ptr() == b.data_ptr()
    # fit not given = 'crop_or_pad' = the behaviour before the option existed
    default = _cls(variant)(weights=wts, iters_pred=3, target_size='auto')
    named = _cls(variant)(weights=wts, iters_pred=3, target_size='auto', fit='crop_or_pad', antialias=False)
    assert default.fit == 'crop_or_pad'
    u1, u2 = _frames(3, 2, 60, 90, np.uint8)
    for g, w_ in zip(default([u1, u2]), named([u1, u2])):
        np.testing.assert_array_equal(_np(g), _np(w_))
    np.testing.assert_array_equal(_np(default.predict_step((u1, u2))), _np(named.predict_step((u1, u2))))

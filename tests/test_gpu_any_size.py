"""Frames of any size on the GPU: the window-copy kernel, CropOrPadder, ``target_size`` on RAFT / SmallRAFT through every
inference entry point, VisFlowCallback.  A copy has no rounding: everything is compared exactly, except against the CPU oracle
(the project's 1e-3 max-EPE bound where tests/golden/conditioning_any_size.json shows the oracle well conditioned) and the
mean EPE of ``test_step`` (one float32 ulp: see the test).

The yardstick of the crop-or-pad rule is the NumPy restatement of tests/test_any_size.py.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, report
from test_any_size import _decode_png, np_crop_or_pad

pytestmark = pytest.mark.gpu

TOL = 1e-3            # tests/test_gpu_model.py TOL: max EPE against the oracle


def _np(t):
    return t.detach().cpu().numpy()


def _frames(seed, B, H, W, dtype=np.float32):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return tuple(rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8) for _ in range(2))
    return tuple(rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32) for _ in range(2))


def _cls(variant):
    import tf_raft_amd
    return tf_raft_amd.RAFT if variant == 'raft' else tf_raft_amd.SmallRAFT


def _via_numpy(model, i1, i2, th, tw):
    """NumPy-pad -> a model WITHOUT the option -> NumPy-crop: every prediction of __call__."""
    H, W = i1.shape[1:3]
    p1, p2 = (np_crop_or_pad(np.asarray(x, np.float32), th, tw) for x in (i1, i2))
    return [np_crop_or_pad(_np(o), H, W) for o in model([p1, p2])]


# ------------------------------------------------------------------ the kernel
# (Hs, Ws) -> (Ht, Wt): pad, crop, one axis each way, equal, odd surpluses, 1 x 1 windows, rows that are not whole 16-byte chunks
SIZES = [((7, 10), (12, 16)), ((12, 16), (7, 10)), ((9, 20), (12, 16)), ((12, 9), (8, 16)), ((8, 16), (8, 16)), ((5, 5), (8, 8)),
         ((7, 7), (4, 4)), ((1, 1), (4, 8)), ((3, 5), (1, 1)), ((1, 1), (1, 1)), ((6, 13), (9, 7)), ((4, 414), (8, 416))]


@pytest.mark.parametrize('pair', ['f32', 'u8_f32', 'u8', 'bool'])
def test_window_copy_kernel_is_the_numpy_rule(pair):
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(7)
    want_dtype = torch.float32 if pair == 'u8_f32' else None
    launches = 0
    for (hs, ws), (ht, wt) in SIZES:
        for C_ in (1, 2, 3):
            for N in (1, 5):
                if pair == 'f32':
                    x = rng.normal(size=(N, hs, ws, C_)).astype(np.float32)
                    x[x == 0] = 1.0
                elif pair == 'bool':
                    x = rng.uniform(size=(N, hs, ws, C_)) < 0.7
                else:
                    x = rng.integers(1, 256, size=(N, hs, ws, C_), dtype=np.uint8)
                want = np_crop_or_pad(x, ht, wt)
                if pair == 'u8_f32':
                    want = want.astype(np.float32)
                t = torch.as_tensor(x).cuda()
                # a destination pre-filled with NaN (0xAB bytes): an element the kernel leaves unwritten shows
                out_dtype = torch.float32 if pair in ('f32', 'u8_f32') else torch.uint8
                out = torch.full((N, ht, wt, C_), float('nan') if out_dtype == torch.float32 else 0xAB, dtype=out_dtype, device='cuda')
                got = image_ops.window_copy(t, ht, wt, want_dtype, out=out)
                launches += 1
                assert got.data_ptr() == out.data_ptr() and got.is_contiguous()
                np.testing.assert_array_equal(_np(got), want, err_msg=f'{pair} {(N, hs, ws, C_)} -> {(ht, wt)}')
                # the public op: (N, H, W, C) and (H, W, C), from the host as well
                pub = image_ops.resize_with_crop_or_pad(x if N == 1 else t, ht, wt, dtype=want_dtype)
                assert pub.is_contiguous() and pub.is_cuda and _np(pub).dtype == want.dtype
                np.testing.assert_array_equal(_np(pub), want)
                np.testing.assert_array_equal(_np(image_ops.resize_with_crop_or_pad(x[0], ht, wt, dtype=want_dtype)), want[0])
    assert launches == len(SIZES) * 6
    same = torch.as_tensor(x).cuda()                                    # equal sizes: the input itself comes back, nothing is launched
    assert image_ops.resize_with_crop_or_pad(same, *same.shape[1:3]).data_ptr() == same.data_ptr()


@pytest.mark.parametrize('src_shape,target', [((1, 375, 1242, 3), (376, 1248)), ((2, 436, 1024, 3), (448, 1024)), ((1, 1242, 375, 3), (64, 96)),
                                              ((2, 61, 1001, 1), (64, 1008))])
def test_window_copy_kernel_on_frame_sized_inputs(src_shape, target):
    """KITTI's 375 x 1242 (source rows of 1242 x 3 bytes: most are not 4-byte aligned), Sintel's 436 x 1024, a crop of both
    axes -- uint8 -> float, uint8 -> uint8 and float -> float; and a destination that does not start on 16 bytes."""
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(3)
    u = rng.integers(1, 256, size=src_shape, dtype=np.uint8)
    f = u.astype(np.float32) + 0.25
    th, tw = target
    tu, tf_ = torch.as_tensor(u).cuda(), torch.as_tensor(f).cuda()
    np.testing.assert_array_equal(_np(image_ops.window_copy(tu, th, tw, torch.float32)), np_crop_or_pad(u, th, tw).astype(np.float32))
    np.testing.assert_array_equal(_np(image_ops.window_copy(tu, th, tw)), np_crop_or_pad(u, th, tw))
    np.testing.assert_array_equal(_np(image_ops.window_copy(tf_, th, tw)), np_crop_or_pad(f, th, tw))
    n = src_shape[0] * th * tw * src_shape[3]
    for skew in (1, 3):
        slab = torch.full((n + 8,), float('nan'), device='cuda')
        out = slab[skew:skew + n].view(src_shape[0], th, tw, src_shape[3])
        src = torch.full((tf_.numel() + 8,), float('nan'), device='cuda')
        src[skew:skew + tf_.numel()] = tf_.reshape(-1)
        image_ops.window_copy(src[skew:skew + tf_.numel()].view(src_shape), th, tw, out=out)
        np.testing.assert_array_equal(_np(out), np_crop_or_pad(f, th, tw))
        assert torch.isnan(slab[:skew]).all() and torch.isnan(slab[skew + n:]).all()      # nothing written outside the destination


def test_window_copy_follows_the_current_stream_and_rejects_what_it_cannot_take():
    from tf_raft_amd import image_ops
    side = torch.cuda.Stream()
    x = torch.arange(2 * 30 * 40 * 2, dtype=torch.float32, device='cuda').view(2, 30, 40, 2) + 1
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        y = x * 2                                                       # produced on `side`: only stream order makes the copy see it
        z = image_ops.resize_with_crop_or_pad(y, 32, 48)
    side.synchronize()
    np.testing.assert_array_equal(_np(z), np_crop_or_pad(_np(x) * 2, 32, 48))
    with pytest.raises(TypeError):
        image_ops.resize_with_crop_or_pad(torch.zeros((1, 4, 4, 1), dtype=torch.int32), 8, 8)
    with pytest.raises(TypeError):
        image_ops.resize_with_crop_or_pad(x, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError):
        image_ops.resize_with_crop_or_pad(x[0, 0], 8, 8)
    with pytest.raises(ValueError):
        image_ops.resize_with_crop_or_pad(x, 0, 8)
    with pytest.raises(ValueError):
        image_ops.window_copy(x, 32, 48, out=torch.empty((2, 32, 48, 1), device='cuda'))


def test_crop_or_padder_on_a_sintel_sample():
    """reference dataset.py:323-334 on one validation batch: uint8 frames, float flow, bool valid without a channel axis."""
    from tf_raft.datasets import CropOrPadder, ShapeSetter
    rng = np.random.default_rng(11)
    i1, i2 = _frames(11, 1, 436, 1024, np.uint8)
    flow = rng.normal(size=(1, 436, 1024, 2)).astype(np.float32)
    valid = rng.uniform(size=(1, 436, 1024)) < 0.9
    out = CropOrPadder(target_size=(448, 1024))(i1, i2, flow, valid)
    ShapeSetter(1, (448, 1024))(*out)
    for got, src in zip(out[:3], (i1, i2, flow)):
        assert got.is_cuda and got.is_contiguous() and _np(got).dtype == src.dtype
        np.testing.assert_array_equal(_np(got), np_crop_or_pad(src, 448, 1024))
    assert tuple(out[3].shape) == (1, 448, 1024) and out[3].dtype == torch.bool
    np.testing.assert_array_equal(_np(out[3]), np_crop_or_pad(valid[..., None], 448, 1024)[..., 0])
    with pytest.raises(ValueError):
        ShapeSetter(1, (436, 1024))(*out)
    back = CropOrPadder((436, 1024))(*out)                               # padding then cropping back is the identity
    for got, src in zip(back, (i1, i2, flow, valid)):
        np.testing.assert_array_equal(_np(got), src)


# ------------------------------------------------------------------ the model option
@pytest.mark.parametrize('variant,iters', [('raft', 3), ('small', 4)])
def test_auto_target_is_bitwise_pad_model_crop(variant, iters):
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=4, perturb=True)
    plain = _cls(variant)(weights=wts, iters_pred=iters)
    auto = _cls(variant)(weights=wts, iters_pred=iters, target_size='auto')
    for seed, (B, H, W), (th, tw) in ((1, (2, 60, 90), (64, 96)), (2, (1, 59, 155), (64, 160)), (3, (1, 40, 90), (64, 96))):
        assert auto._model_size(H, W) == (th, tw)
        i1, i2 = _frames(seed, B, H, W)
        want = _via_numpy(plain, i1, i2, th, tw)
        got = auto([i1, i2])
        assert len(got) == iters
        base = got[0].data_ptr()
        for k, (g, w_) in enumerate(zip(got, want)):
            assert tuple(g.shape) == (B, H, W, 2) and g.is_contiguous()
            assert g.data_ptr() == base + 4 * k * B * H * W * 2          # views of ONE allocation, as without the option
            np.testing.assert_array_equal(_np(g), w_)
        last = auto.predict_step((i1, i2))
        assert tuple(last.shape) == (B, H, W, 2) and last.is_contiguous()
        np.testing.assert_array_equal(_np(last), want[-1])
        np.testing.assert_array_equal(_np(auto.predict_step((torch.as_tensor(i1).cuda(), torch.as_tensor(i2).cuda()))), want[-1])
        with pytest.raises(ValueError):
            plain([i1, i2])                                              # without the option nothing changed
        with pytest.raises(ValueError):
            auto([i1, i2], training=True)                                # training-mode calls keep their check
    with pytest.raises(ValueError):
        auto([i1, i2[:, :30]])


@pytest.mark.parametrize('variant,iters', [('raft', 3), ('small', 4)])
def test_predict_with_auto_target_on_uint8_and_float_host_frames(variant, iters):
    """``predict`` with a ragged last batch: uint8 frames go through the uint8 -> float window copy, float frames through the
    float one; both equal predict() of a model without the option on the NumPy-padded frames, cropped."""
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=6, perturb=True)
    plain = _cls(variant)(weights=wts, iters_pred=iters)
    auto = _cls(variant)(weights=wts, iters_pred=iters, target_size='auto')
    for (n, H, W), (th, tw), bs in (((5, 60, 90), (64, 96), 2), ((3, 59, 155), (64, 160), 2)):
        u1, u2 = _frames(21, n, H, W, np.uint8)
        f1, f2 = u1.astype(np.float32), u2.astype(np.float32)
        want = np_crop_or_pad(plain.predict([np_crop_or_pad(f1, th, tw), np_crop_or_pad(f2, th, tw)], batch_size=bs), H, W)
        for a, b in ((u1, u2), (f1, f2)):
            got = auto.predict([a, b], batch_size=bs)
            assert isinstance(got, np.ndarray) and got.shape == (n, H, W, 2)
            np.testing.assert_array_equal(got, want)
        dataset = [(u1[i:i + bs], u2[i:i + bs], None) for i in range(0, n, bs)]
        np.testing.assert_array_equal(auto.predict(dataset), want)


@pytest.mark.parametrize('variant,iters', [('raft', 3), ('small', 4)])
def test_fixed_target_crops_in_and_pads_the_flow_out(variant, iters):
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=8, perturb=True)
    plain = _cls(variant)(weights=wts, iters_pred=iters)
    fixed = _cls(variant)(weights=wts, iters_pred=iters, target_size=(64, 96))
    i1, i2 = _frames(5, 1, 70, 100)
    want = _via_numpy(plain, i1, i2, 64, 96)
    assert not want[-1][:, :3].any() and not want[-1][:, :, :2].any() and want[-1][:, 3:67, 2:98].any()      # a zero frame around the flow
    for g, w_ in zip(fixed([i1, i2]), want):
        assert tuple(g.shape) == (1, 70, 100, 2)
        np.testing.assert_array_equal(_np(g), w_)
    np.testing.assert_array_equal(_np(fixed.predict_step((i1, i2))), want[-1])
    # one axis each way, uint8 frames
    u1, u2 = _frames(6, 2, 50, 120, np.uint8)
    want = _via_numpy(plain, u1, u2, 64, 96)
    for g, w_ in zip(fixed([u1, u2]), want):
        np.testing.assert_array_equal(_np(g), w_)
    # frames that already have the target size: bit for bit the model without the option, on the buffers that came in
    a, b = (torch.as_tensor(x).cuda() for x in _frames(7, 2, 64, 96))
    for g, w_ in zip(fixed([a, b]), plain([a, b])):
        np.testing.assert_array_equal(_np(g), _np(w_))
    fa, fb, window = fixed._fit_frames(a, b)
    assert window is None and fa.data_ptr() == a.data_ptr() and fb.data_ptr() == b.data_ptr()


@pytest.mark.parametrize('variant,kw,iters', [('raft', {}, 4), ('raft', {'lanes': 2}, 3), ('small', {'lanes': 2}, 4)])
def test_pipelined_calls_with_auto_target_are_bitwise_the_serial_calls(variant, kw, iters):
    """Six consecutive calls in flight (the pattern of test_pipelined_calls_are_bitwise_the_serial_calls): the window copy of the
    predictions runs on the loop's stream in front of the `done` event, so the results still carry their pending join and the
    caller's stream was never made to wait for a loop."""
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=3, perturb=True)
    pipe = _cls(variant)(weights=wts, iters_pred=iters, pipeline=True, target_size='auto', **kw)
    serial = _cls(variant)(weights=wts, iters_pred=iters, pipeline=False, loop_concurrency=pipe.lanes, target_size='auto')
    plain = _cls(variant)(weights=wts, iters_pred=iters, pipeline=False, loop_concurrency=pipe.lanes)
    B, H, W = 2, 60, 90
    inputs = [tuple(torch.as_tensor(a).cuda() for a in _frames(40 + k, B, H, W, np.uint8 if k % 2 else np.float32)) for k in range(6)]
    torch.cuda.synchronize()
    outs = [pipe([a, b]) for a, b in inputs]                             # nothing touches the results: six calls in flight
    for o in outs:
        for g in o:
            p = g.__dict__.get('_pending')
            assert p is not None and not p._joined                      # nobody waited for the loop yet
            assert tuple(g.shape) == (B, H, W, 2) and not p._joined      # (metadata: no join)
    assert len({id(o[0].__dict__['_pending']) for o in outs}) == 6
    junk = [torch.full((1 << 22,), float('nan'), device='cuda') for _ in range(4)]     # allocator traffic on the caller's stream
    order = [3, 0, 5, 4, 1, 2]
    got = {k: [_np(o) for o in outs[k]] for k in order}
    del outs, junk
    for k, (a, b) in enumerate(inputs):
        want = serial([a, b])
        via = _via_numpy(plain, _np(a), _np(b), 64, 96)
        for g, w_, v in zip(got[k], want, via):
            np.testing.assert_array_equal(g, _np(w_))
            np.testing.assert_array_equal(g, v)
    # results dropped at once while their loops run; the allocator must not hand their memory out early
    last = None
    for k in range(6):
        last = pipe([inputs[k][0], inputs[k][1]])
        if k < 5:
            del last
            torch.empty((iters, B, 64, 96, 2), device='cuda').fill_(float('nan'))
    np.testing.assert_array_equal(_np(last[-1]), got[5][-1])
    ps = [pipe.predict_step(inputs[k]) for k in range(3)]                # the final-only loop through the same lanes
    assert all(p.__dict__.get('_pending') is not None and not p.__dict__['_pending']._joined for p in ps)
    for k in range(3):
        np.testing.assert_array_equal(_np(ps[k]), got[k][-1])


# ------------------------------------------------------------------ the route object
@pytest.mark.parametrize('fit,antialias', [('crop_or_pad', True), ('resize', False), ('resize', True), ('tile', True)])
def test_route_object_is_bitwise_the_public_functions(fit, antialias):
    """The one object ``_fit_frames`` builds per call, asked directly: frames in, result size, flow back (fresh and into a
    caller's tensor) and tables, bit for bit the public functions, which have kernel tests of their own.  Tiles of 64 x 96 at
    overlap 16: the 100 x 150 frames take 2 x 2 tiles, the 60 x 200 frame one padded row of 3."""
    from tf_raft_amd import image_ops
    th, tw, ov = 64, 96, 16
    overlap = _cls('raft')._check_tile_overlap(fit, ov if fit == 'tile' else None, (th, tw))        # as the constructor keeps it
    rng = np.random.default_rng(23)
    for x, K in ((rng.integers(0, 256, size=(2, 100, 150, 3), dtype=np.uint8), 4), (rng.uniform(0, 255, (1, 60, 200, 3)).astype(np.float32), 3)):
        t = torch.as_tensor(x).cuda()
        N, H, W, _ = t.shape
        route = image_ops.fit_route(fit, t.device, H, W, th, tw, antialias, overlap)
        want_in = {'crop_or_pad': lambda: image_ops.resize_with_crop_or_pad(t, th, tw, torch.float32),
                   'resize': lambda: image_ops.resize(t, th, tw, antialias), 'tile': lambda: image_ops.tile_gather(t, th, tw, ov)}[fit]()
        got_in = route.frames_in(t)
        B = N * K if fit == 'tile' else N
        assert got_in.dtype == torch.float32 and tuple(got_in.shape) == (B, th, tw, 3)
        np.testing.assert_array_equal(_np(got_in), _np(want_in))
        pred = torch.as_tensor(rng.normal(size=(3, B, th, tw, 2)).astype(np.float32) * 4).cuda()
        want = {'crop_or_pad': lambda: torch.stack([image_ops.resize_with_crop_or_pad(p, H, W) for p in pred]),
                'resize': lambda: image_ops.resize_flow(pred, H, W, antialias), 'tile': lambda: image_ops.tile_blend(pred, H, W, ov)}[fit]()
        assert tuple(want.shape) == (3, N, H, W, 2) and route.result_size(B) == tuple(want.shape[1:4])
        fresh = route.flow_back(pred)
        assert tuple(fresh.shape) == (3, N, H, W, 2) and fresh.is_contiguous()
        np.testing.assert_array_equal(_np(fresh), _np(want))
        into = torch.full((3, N, H, W, 2), float('nan'), device='cuda')
        assert route.flow_back(pred, into=into) is into
        np.testing.assert_array_equal(_np(into), _np(want))
        tables = route.tensors()
        assert isinstance(tables, list) and all(isinstance(v, torch.Tensor) and v.is_cuda for v in tables)
        assert (len(tables) == 0) == (fit == 'crop_or_pad')


# ------------------------------------------------------------------ against the CPU oracle
def _conditioned(variant, H, W, seed):
    sys.path.insert(0, GOLDEN)
    from make_conditioning import case_inputs
    return case_inputs(variant, H, W, seed, 'conditioned')


def _assert_oracle_is_well_conditioned(key):
    with open(os.path.join(GOLDEN, 'conditioning_any_size.json')) as f:
        cond = json.load(f)[key]
    assert max(cond['epe32v64']) <= 2e-4, 'fixture: the oracle itself is ill conditioned on this case'
    return cond


@pytest.mark.parametrize('variant,frame,target,iters,seed', [('raft', (436, 1024), (448, 1024), 24, 0), ('small', (60, 90), (64, 96), 12, 0),
                                                             ('raft', (70, 100), (64, 96), 12, 0)])
def test_target_size_against_the_oracle(variant, frame, target, iters, seed):
    """The reference's own validation shape (MPI-Sintel frames at target 448 x 1024, train_sintel.py:72-75), free-running, all 24
    predictions within the project's bound of crop(oracle(pad(frames))); SmallRAFT and a cropping target on small cases."""
    import oracle
    from oracle.losses import max_epe
    H, W = frame
    cond = _assert_oracle_is_well_conditioned(f'{variant}_{H}x{W}_to_{target[0]}x{target[1]}_seed{seed}_it{iters}_conditioned')
    i1, i2, wts = _conditioned(variant, H, W, seed)
    ocls = oracle.RAFT if variant == 'raft' else oracle.SmallRAFT
    want = [np_crop_or_pad(np.asarray(o), H, W) for o in ocls(wts, iters_pred=iters)([np_crop_or_pad(i1, *target), np_crop_or_pad(i2, *target)])]
    model = _cls(variant)(weights=wts, iters_pred=iters, target_size=target)
    got = model([i1, i2])
    errs = [max_epe(_np(g), w_) for g, w_ in zip(got, want)]
    report(f'any-size {variant} {H}x{W} -> {target[0]}x{target[1]}', final_epe=errs[-1], worst_epe=max(errs), oracle32_vs_64_worst=max(cond['epe32v64']))
    print('[parity] per-iteration max EPE hip-vs-oracle32 :', ' '.join(f'{e:.2e}' for e in errs))
    assert len(got) == iters and all(tuple(g.shape) == (1, H, W, 2) for g in got)
    assert max(errs) <= TOL, errs
    assert max_epe(_np(model.predict_step((i1, i2))), want[-1]) <= TOL


def test_test_step_on_raw_frames_equals_the_reference_route():
    """``test_step`` with the option on 436 x 1024 frames and ground truth of the frames' own size, against the reference's route
    (train_sintel.py:72-75: CropOrPadder on all four, a model without the option).  u1 / u3 / u5 are counts over the same
    pixels: equal.  epe: both routes reduce the same float values in double precision over arrays of different shape, so
    partial sums group differently (about n x 2^-53), and raft_flow_metrics_f32 hands the mean back as float32, which can turn
    that into one float32 ulp = 1.2e-7 relative."""
    from tf_raft.datasets import CropOrPadder
    from tf_raft_amd import weights as wm
    wts = wm.init_weights('raft', seed=9, perturb=True)
    rng = np.random.default_rng(31)
    with_option = _cls('raft')(weights=wts, iters_pred=3, target_size=(448, 1024))
    reference_route = _cls('raft')(weights=wts, iters_pred=3)
    for m in (with_option, reference_route):
        m.compile(optimizer=None)
    padder = CropOrPadder((448, 1024))
    for step in range(2):
        i1, i2 = _frames(50 + step, 1, 436, 1024, np.uint8)
        flow = (rng.normal(size=(1, 436, 1024, 2)) * 2).astype(np.float32)
        valid = rng.uniform(size=(1, 436, 1024)) < 0.9
        got = with_option.test_step((i1, i2, flow, valid))
        want = reference_route.test_step(padder(i1, i2, flow, valid))
        got, want = ({k: float(v) for k, v in d.items()} for d in (got, want))
        report(f'test_step raw frames, step {step}', **{f'{k}_{n}': d[k] for k in ('epe', 'u1', 'u3', 'u5') for n, d in (('option', got), ('route', want))})
        for k in ('u1', 'u3', 'u5'):
            assert got[k] == want[k], (k, got[k], want[k])
        assert want['epe'] > 0 and abs(got['epe'] - want['epe']) <= 1.2e-7 * abs(want['epe']), (got['epe'], want['epe'])


def test_vis_flow_callback_writes_frames_over_the_flow_image(tmp_path):
    """reference training.py:55-88 on a two-sample list data set of Sintel-sized frames."""
    from tf_raft.training import VisFlowCallback
    from tf_raft_amd import io
    from tf_raft_amd import weights as wm
    wts = wm.init_weights('raft', seed=2, perturb=True)
    model = _cls('raft')(weights=wts, iters_pred=3)
    dataset = []
    for k in range(2):
        a, b = _frames(60 + k, 1, 436, 1024, np.uint8)
        dataset.append((a[0], b[0], None, None))
    cb = VisFlowCallback(dataset, target_size=(448, 1024), num_visualize=2, logdir=str(tmp_path / 'predicted_flows'))
    cb.set_model(model)
    cb.on_epoch_end(4)
    assert sorted(os.listdir(cb.logdir)) == ['epoch005_001.png', 'epoch005_002.png']
    for k, (a, b, *_rest) in enumerate(dataset):
        image = _decode_png(os.path.join(cb.logdir, f'epoch005_{k + 1:03d}.png'))
        assert image.shape == (3 * 436, 1024, 3)
        np.testing.assert_array_equal(image[:436], a)
        np.testing.assert_array_equal(image[436:872], b)
        flow = model([np_crop_or_pad(a[None].astype(np.float32), 448, 1024), np_crop_or_pad(b[None].astype(np.float32), 448, 1024)])[-1]
        np.testing.assert_array_equal(image[872:], io.flow_to_image(np_crop_or_pad(_np(flow), 436, 1024)[0]))
    # a model that carries the option itself gives the same picture
    cb2 = VisFlowCallback(dataset, target_size=(448, 1024), num_visualize=1, logdir=str(tmp_path / 'again'))
    cb2.set_model(_cls('raft')(weights=wts, iters_pred=3, target_size=(448, 1024)))
    cb2.on_epoch_end(4)
    np.testing.assert_array_equal(_decode_png(os.path.join(cb2.logdir, 'epoch005_001.png')),
                                  _decode_png(os.path.join(cb.logdir, 'epoch005_001.png')))

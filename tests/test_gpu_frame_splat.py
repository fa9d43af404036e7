"""The forward splat of frames and the frame in between on the GPU: the five entries against the NumPy
restatement of tests/test_frame_splat.py BIT FOR BIT (integer sums and one float64 division: no tolerance), with and without
masks, guard bands around every output, a workspace full of garbage, repeats; the public functions; and the model's
``interpolate_step`` / ``predict_interpolated`` / ``interpolate_video`` against ``image_ops.interpolate`` on the flows the
predictor returns.
"""
import numpy as np
import pytest
import torch

from conftest import report
from test_frame_splat import (SHAPES, TIMES, classes, np_frame_splat_acc, np_interpolate, np_splat, splat_flows, splat_frames,
                              splat_masks)

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xAB
IDS = ['x'.join(map(str, s)) for s in SHAPES]
KINDS = {'f32': ('f32', np.float32), 'u8_f32': ('u8', np.float32), 'u8': ('u8', np.uint8)}      # entry suffix: frames, result


def _np(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy()


def _guarded(n, dtype, device):
    """A buffer of ``n`` elements between two guard bands, every byte FILL: (whole buffer, the view a launch writes)."""
    size = torch.empty((), dtype=dtype).element_size()
    buf = torch.full(((2 * GUARD + n) * size,), FILL, dtype=torch.uint8, device=device)
    return buf, buf[GUARD * size:(GUARD + n) * size]


def _intact(buf, n_bytes):
    b = buf.cpu().numpy()
    band = (len(b) - n_bytes) // 2
    return bool((b[:band] == FILL).all() and (b[-band:] == FILL).all())


def _sums(lib, slices, H, W, Cn, device):
    """The workspace of the sums, full of garbage: the entry has to zero it itself."""
    nbytes = int(lib.raft_frame_splat_workspace_bytes(slices, H, W, Cn))
    assert nbytes == slices * H * W * (Cn + 1) * 8
    return torch.full((nbytes // 8,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=device)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _splat(frames, flow, mask, t, want_weight=True):
    """raft_splat_frames_* through the library itself: (dst, weight, guard bytes intact)."""
    from tf_raft_amd import _dev
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    N, H, W, Cn = frames.shape
    fn = lib.raft_splat_frames_f32 if frames.dtype == torch.float32 else lib.raft_splat_frames_u8_f32
    buf_d, dst = _guarded(N * H * W * Cn, torch.float32, frames.device)
    buf_w, weight = _guarded(N * H * W, torch.float32, frames.device)
    ws = _sums(lib, N, H, W, Cn, frames.device)
    check(fn(_dev.ptr(frames), _dev.ptr(flow), _dev.ptr(mask) if mask is not None else None, t, _dev.ptr(dst),
             _dev.ptr(weight) if want_weight else None, N, H, W, Cn, _dev.ptr(ws), _dev.stream_ptr()), 'splat_frames')
    torch.cuda.synchronize()
    intact = _intact(buf_d, N * H * W * Cn * 4) and _intact(buf_w, N * H * W * 4)
    return (dst.cpu().numpy().view(np.float32).reshape(N, H, W, Cn), weight.cpu().numpy().view(np.float32).reshape(N, H, W)
            if want_weight else weight.cpu().numpy(), intact)


def _interpolate(entry, i1, i2, ff, fb, m1, m2, t, want_holes=True):
    """raft_interpolate_frames_* through the library itself: (dst, holes, guard bytes intact)."""
    from tf_raft_amd import _dev
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    N, H, W, Cn = i1.shape
    out_np = KINDS[entry][1]
    out_t = torch.float32 if out_np == np.float32 else torch.uint8
    size = 4 if out_np == np.float32 else 1
    buf_d, dst = _guarded(N * H * W * Cn, out_t, i1.device)
    buf_h, holes = _guarded(N * H * W, torch.uint8, i1.device)
    ws = _sums(lib, 2 * N, H, W, Cn, i1.device)
    check(getattr(lib, 'raft_interpolate_frames_' + entry)(
        _dev.ptr(i1), _dev.ptr(i2), _dev.ptr(ff), _dev.ptr(fb), _dev.ptr(m1) if m1 is not None else None,
        _dev.ptr(m2) if m2 is not None else None, t, _dev.ptr(dst), _dev.ptr(holes) if want_holes else None, N, H, W, Cn, _dev.ptr(ws),
        _dev.stream_ptr()), 'interpolate_frames')
    torch.cuda.synchronize()
    intact = _intact(buf_d, N * H * W * Cn * size) and _intact(buf_h, N * H * W)
    return dst.cpu().numpy().view(out_np).reshape(N, H, W, Cn), holes.cpu().numpy().reshape(N, H, W), intact


_CASES = {}


def _case(shape, Cn=3):
    """The inputs of one shape and everything the restatement says about them, computed once and left unchanged:
    want['splat', kind, t, masked] = (dst, weight) of frame 1 along the forward flow, want['interpolate', entry, t, masked] =
    (frame, holes); both from the same two sets of sums."""
    key = shape + (Cn,)
    if key not in _CASES:
        N, H, W = shape
        flows, masks = splat_flows(N, H, W), splat_masks(N, H, W)
        frames = {kind: splat_frames(N, H, W, Cn, kind) for kind in ('u8', 'f32')}
        want = {}
        for kind, (i1, i2) in frames.items():
            for t in TIMES:
                for masked in (False, True):
                    m1, m2 = (masks[:N], masks[N:]) if masked else (None, None)
                    acc1 = np_frame_splat_acc(i1, flows[:N], t, m1)
                    acc2 = np_frame_splat_acc(i2, flows[N:], np.float32(1) - np.float32(t), m2)
                    want['splat', kind, t, masked] = np_splat(i1, flows[:N], t, m1, acc=acc1)
                    for entry, (k, out) in KINDS.items():
                        if k == kind:
                            want['interpolate', entry, t, masked] = np_interpolate(i1, i2, flows[:N], flows[N:], t, m1, m2, out, acc1, acc2)
                    if kind == 'u8' and not masked:
                        want['classes', t] = tuple(int(c.sum()) for c in classes(acc1, acc2))
        for v in want.values():
            for a in v:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        for a in (flows, masks, frames['u8'], frames['f32']):
            a.setflags(write=False)
        _CASES[key] = (flows, masks, frames, want)
    return _CASES[key]


def _device_case(shape, Cn=3):
    from tf_raft_amd import _dev
    dev = _dev.require_gpu()
    flows, masks, frames, want = _case(shape, Cn)
    up = lambda a: torch.from_numpy(a.copy()).to(dev)       # noqa: E731
    return up(flows), up(masks), {k: up(v) for k, v in frames.items()}, want


def _check_splats(shape, Cn=3):
    N = shape[0]
    flows, masks, frames, want = _device_case(shape, Cn)
    for kind in ('u8', 'f32'):
        src = frames[kind][0]
        for t in TIMES:
            for masked in (False, True):
                m = masks[:N] if masked else None
                dst, weight, intact = _splat(src, flows[:N], m, t)
                want_dst, want_weight = want['splat', kind, t, masked]
                np.testing.assert_array_equal(_bits(dst), _bits(want_dst), err_msg=f'{kind} t={t} masked={masked}')
                np.testing.assert_array_equal(_bits(weight), _bits(want_weight))
                assert intact
        only, untouched, intact = _splat(src, flows[:N], m, t, want_weight=False)            # weight = NULL
        np.testing.assert_array_equal(_bits(only), _bits(dst))
        assert intact and (untouched == FILL).all()
        for _ in range(5):                                                   # integer sums: any arrival order, the same bits
            again, again_w, _ = _splat(src, flows[:N], masks[:N], 0.3)
            np.testing.assert_array_equal(_bits(again), _bits(want['splat', kind, 0.3, True][0]))
            np.testing.assert_array_equal(_bits(again_w), _bits(want['splat', kind, 0.3, True][1]))
    return want


def _check_interpolations(shape, Cn=3):
    N = shape[0]
    flows, masks, frames, want = _device_case(shape, Cn)
    for entry, (kind, _) in KINDS.items():
        i1, i2 = frames[kind]
        for t in TIMES:
            for masked in (False, True):
                m1, m2 = (masks[:N], masks[N:]) if masked else (None, None)
                dst, holes, intact = _interpolate(entry, i1, i2, flows[:N], flows[N:], m1, m2, t)
                want_dst, want_holes = want['interpolate', entry, t, masked]
                if dst.dtype == np.uint8:
                    np.testing.assert_array_equal(dst, want_dst, err_msg=f'{entry} t={t} masked={masked}')
                else:
                    np.testing.assert_array_equal(_bits(dst), _bits(want_dst), err_msg=f'{entry} t={t} masked={masked}')
                np.testing.assert_array_equal(holes, want_holes)
                assert intact
        only, untouched, intact = _interpolate(entry, i1, i2, flows[:N], flows[N:], m1, m2, t, want_holes=False)      # holes = NULL
        np.testing.assert_array_equal(only, dst)
        assert intact and (untouched == FILL).all()
        only1, holes1, _ = _interpolate(entry, i1, i2, flows[:N], flows[N:], masks[:N], None, 0.25)       # one mask alone
        w1, h1 = np_interpolate(_np(i1), _np(i2), _np(flows[:N]), _np(flows[N:]), 0.25, _np(masks[:N]), None, KINDS[entry][1])
        np.testing.assert_array_equal(only1.view(np.uint8), w1.view(np.uint8))
        np.testing.assert_array_equal(holes1, h1)
        for _ in range(5):
            again, again_h, _ = _interpolate(entry, i1, i2, flows[:N], flows[N:], None, None, 0.3)
            np.testing.assert_array_equal(again.view(np.uint8), want['interpolate', entry, 0.3, False][0].view(np.uint8))
            np.testing.assert_array_equal(again_h, want['interpolate', entry, 0.3, False][1])
    return want


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_the_splat_entries_are_the_restatement_bit_for_bit(shape):
    want = _check_splats(shape)
    report(f'frame splat {shape}', largest_weight=float(want['splat', 'u8', 1.0, False][1].max()))


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_the_interpolate_entries_are_the_restatement_bit_for_bit(shape):
    want = _check_interpolations(shape)
    if shape[1] >= 37:
        for t in (0.25, 0.3):
            assert min(want['classes', t]) > 0                               # both land, only 1, only 2, a hole: every branch ran
    report(f'frame interpolation {shape}', holes_at_quarter=int(want['interpolate', 'u8', 0.25, False][1].sum()))


@pytest.mark.parametrize('Cn', [1, 4])
def test_one_and_four_channels(Cn):
    _check_splats((1, 5, 7), Cn)
    _check_interpolations((1, 5, 7), Cn)


@pytest.mark.parametrize('shape', SHAPES[2:], ids=IDS[2:])
def test_the_public_functions_and_the_weight_at_t_1_is_the_range_map(shape):
    from tf_raft_amd import image_ops
    N, H, W = shape
    flows, masks, frames, want = _device_case(shape)
    for kind in ('u8', 'f32'):
        i1, i2 = frames[kind]
        dst, weight = image_ops.splat(i1, flows[:N], t=1, return_weight=True)
        assert tuple(dst.shape) == (N, H, W, 3) and dst.dtype == torch.float32 and tuple(weight.shape) == (N, H, W)
        np.testing.assert_array_equal(_bits(_np(dst)), _bits(want['splat', kind, 1.0, False][0]))
        np.testing.assert_array_equal(_bits(_np(weight)), _bits(_np(image_ops.range_map(flows[:N]))))      # bit for bit
        got = image_ops.splat(_np(i1)[0], _np(flows)[0], 0.3, mask=_np(masks)[0] != 0)                        # (H, W, C) from the host
        np.testing.assert_array_equal(_bits(_np(got)), _bits(want['splat', kind, 0.3, True][0][0]))
        entry = 'f32' if kind == 'f32' else 'u8_f32'
        many, holes = image_ops.interpolate(i1, i2, flows[:N], flows[N:], t=list(TIMES), return_holes=True)
        assert tuple(many.shape) == (len(TIMES), N, H, W, 3) and tuple(holes.shape) == (len(TIMES), N, H, W)
        for k, t in enumerate(TIMES):
            np.testing.assert_array_equal(_bits(_np(many[k])), _bits(want['interpolate', entry, t, False][0]))
            np.testing.assert_array_equal(_np(holes[k]), want['interpolate', entry, t, False][1])
        one = image_ops.interpolate(_np(i1), _np(i2), _np(flows[:N]), _np(flows[N:]), 0.25, mask1=masks[:N], mask2=_np(masks[N:]) != 0)
        np.testing.assert_array_equal(_bits(_np(one)), _bits(want['interpolate', entry, 0.25, True][0]))
    i1, i2 = frames['u8']
    as_bytes = image_ops.interpolate(i1, i2, flows[:N], flows[N:], dtype=torch.uint8, t=0.3)
    assert as_bytes.dtype == torch.uint8
    np.testing.assert_array_equal(_np(as_bytes), want['interpolate', 'u8', 0.3, False][0])


# ------------------------------------------------------------------ the model
def _plain(t):
    return t.detach().as_subclass(torch.Tensor)


@pytest.mark.parametrize('route', ['plain', 'resize'])
def test_the_model_interpolates_on_the_flows_it_returns(route):
    import tf_raft_amd
    from tf_raft_amd import image_ops
    from tf_raft_amd import weights as wm
    wts = wm.init_weights('small', seed=6, perturb=True)
    if route == 'plain':
        model, (B, H, W) = tf_raft_amd.SmallRAFT(weights=wts, iters_pred=3), (2, 64, 96)
    else:
        model, (B, H, W) = tf_raft_amd.SmallRAFT(weights=wts, iters_pred=3, target_size=(64, 96), fit='resize'), (2, 100, 150)
    rng = np.random.default_rng(60)
    i1, i2 = (rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32) for _ in range(2))
    res = model.predict_step_bidirectional((i1, i2))
    # a scalar t and a sequence, on the returned flows and the caller's frames at their own size
    got = model.interpolate_step((i1, i2), t=0.3)
    assert tuple(got.shape) == (B, H, W, 3) and got.dtype == torch.float32
    want = image_ops.interpolate(i1, i2, res.forward, res.backward, 0.3)
    assert torch.equal(_plain(got).view(torch.int32), _plain(want).view(torch.int32))
    times = [0.25, 0.5, 0.75]
    many = model.interpolate_step((i1, i2), t=times)
    assert tuple(many.shape) == (3, B, H, W, 3)
    want_many = image_ops.interpolate(i1, i2, res.forward, res.backward, times)
    assert torch.equal(_plain(many).view(torch.int32), _plain(want_many).view(torch.int32))
    assert not torch.equal(_plain(many[0]), _plain(many[2]))
    # skip_occluded = the spelled-out masks, with the occlusion keywords passed through
    for kw in ({}, {'occlusion_test': 'range', 'range_threshold': 0.9}):
        occ = model.predict_step_bidirectional((i1, i2), **kw)
        skipped = model.interpolate_step((i1, i2), 0.5, skip_occluded=True, **kw)
        spelled = image_ops.interpolate(i1, i2, occ.forward, occ.backward, 0.5, mask1=_plain(occ.occluded_forward) == 0,
                                        mask2=_plain(occ.occluded_backward) == 0)
        assert torch.equal(_plain(skipped).view(torch.int32), _plain(spelled).view(torch.int32))
        assert _np(occ.occluded_forward).any() and not torch.equal(_plain(skipped), _plain(many[1]))
    # over a data set, as host arrays
    host = model.predict_interpolated([i1, i2], t=0.3, batch_size=1)
    assert isinstance(host, np.ndarray) and host.dtype == np.float32
    np.testing.assert_array_equal(_bits(host), _bits(_np(got)))
    host_many = model.predict_interpolated([i1, i2], t=times, batch_size=1)
    np.testing.assert_array_equal(_bits(host_many), _bits(_np(many)))
    # a video of 3 uint8 frames at twice its rate: 5 frames, the originals verbatim at the even indices
    video = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    out = model.interpolate_video(video, factor=2)
    assert out.shape == (5, H, W, 3) and out.dtype == np.uint8
    np.testing.assert_array_equal(out[::2], video)
    mid = model.interpolate_step((video[:-1], video[1:]), 0.5)
    assert mid.dtype == torch.uint8
    np.testing.assert_array_equal(out[1::2], _np(mid))
    np.testing.assert_array_equal(model.interpolate_video(video.astype(np.float32), factor=1), video.astype(np.float32))
    report(f'model interpolation ({route})', mean_abs_mid_minus_fade=float(np.abs(_np(many[1]) - 0.5 * (i1 + i2)).mean()))

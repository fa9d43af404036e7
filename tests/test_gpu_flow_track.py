"""Points followed through a video on the GPU: ``raft_track_points_f32`` against the float32 NumPy
restatement of tests/test_flow_track.py BIT FOR BIT (positions compared as uint32, codes as bytes: a pure gather with contraction
off has no tolerance), with and without the backward flow, ``start`` and ``lost_in``, guard bands around both outputs, repeats
and the in-place streaming form; the public functions; and the model's ``track_video`` / ``tracker`` against ``image_ops.track``
on the flows the predictor returns.
"""
import numpy as np
import pytest
import torch

from conftest import report
from test_flow_track import IDS, SHAPES, T0, assert_same, bits, np_track, track_case

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xAB
# Random weights predict much the same flow whichever way round the frames come, so forward and backward flow point the same way
# and under UnFlow's alpha every point fails its first step.  |f + b|^2 <= 2 (|f|^2 + |b|^2) always holds, so with alpha = 2 no
# finite pair of vectors fails (the backward flow is still sampled and compared) and points are followed over several steps;
# 1.9 sits in between.  The model tests run all three: equality with image_ops.track is asked for each.
LOOSE_ALPHA = 2.0
ALPHAS = (0.01, 1.9, LOOSE_ALPHA)


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


def _entry(pos, lost, start, t0, fwd, bwd, pos_out, lost_out, alpha=0.01, beta=0.5):
    """raft_track_points_f32 through the library itself, on device tensors (None: a NULL pointer)."""
    from tf_raft_amd import _dev
    from tf_raft_amd._ffi import check
    ptr = lambda t: None if t is None else _dev.ptr(t)       # noqa: E731
    S, N, H, W, _ = fwd.shape
    P = pos.shape[1]
    check(_dev.lib().raft_track_points_f32(ptr(pos), ptr(lost), ptr(start), t0, ptr(fwd), ptr(bwd), ptr(pos_out), ptr(lost_out), S, N, P,
                                           H, W, alpha, beta, _dev.stream_ptr()), 'track_points')
    torch.cuda.synchronize()


def _track(pos, lost, start, t0, fwd, bwd):
    """One call into guarded outputs: (positions (S, N, P, 2), lost (S, N, P), guard bytes intact)."""
    S, N = fwd.shape[:2]
    P = pos.shape[1]
    buf_p, pos_out = _guarded(S * N * P * 2, torch.float32, pos.device)
    buf_l, lost_out = _guarded(S * N * P, torch.uint8, pos.device)
    _entry(pos, lost, start, t0, fwd, bwd, pos_out, lost_out)
    intact = _intact(buf_p, S * N * P * 8) and _intact(buf_l, S * N * P)
    return pos_out.cpu().numpy().view(np.float32).reshape(S, N, P, 2), lost_out.cpu().numpy().reshape(S, N, P), intact


_CASES = {}
VARIANTS = [(b, s) for b in (True, False) for s in (False, True)]       # (with the backward flow, with start and lost_in)


def _case(shape):
    """The inputs of one shape and what the restatement says about them under every variant, computed once and left unchanged."""
    if shape not in _CASES:
        case = track_case(shape)
        want = {}
        for with_bwd, with_state in VARIANTS:
            want[with_bwd, with_state] = np_track(case['points'], case['lost'] if with_state else None, case['forward'],
                                                  case['backward'] if with_bwd else None,
                                                  start=case['start'] if with_state else None, t0=T0 if with_state else 0)
            for a in want[with_bwd, with_state]:
                a.setflags(write=False)
        _CASES[shape] = (case, want)
    return _CASES[shape]


def _device_case(shape):
    from tf_raft_amd import _dev
    dev = _dev.require_gpu()
    case, want = _case(shape)
    return {k: torch.from_numpy(v.copy()).to(dev) for k, v in case.items()}, want


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_the_entry_is_the_restatement_bit_for_bit(shape):
    d, want = _device_case(shape)
    for with_bwd, with_state in VARIANTS:
        args = (d['points'], d['lost'] if with_state else None, d['start'] if with_state else None, T0 if with_state else 0,
                d['forward'], d['backward'] if with_bwd else None)
        pos, lost, intact = _track(*args)
        assert_same((pos, lost), want[with_bwd, with_state])
        assert intact
        again = _track(*args)                                                # a gather: twice the same
        assert_same(again[:2], (pos, lost))
        assert again[2]
    pos, lost = want[True, False]
    report(f'track {shape}', tracked=int((lost[-1] == 0).sum()), left=int((lost[-1] == 1).sum()), failed=int((lost[-1] == 2).sum()))


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_the_in_place_streaming_step(shape):
    """S = 1 with the outputs ON the inputs, step after step: a thread reads its own point first and touches no other."""
    S, N, H, W, P = shape
    d, want = _device_case(shape)
    for with_bwd in (True, False):
        buf_p, pos = _guarded(N * P * 2, torch.float32, d['points'].device)
        buf_l, lost = _guarded(N * P, torch.uint8, d['points'].device)
        pos.view(torch.float32).copy_(d['points'].reshape(-1))
        lost.copy_(d['lost'].reshape(-1))
        state_p, state_l = pos.view(torch.float32).view(N, P, 2), lost.view(N, P)
        for s in range(S):
            _entry(state_p, state_l, d['start'], T0 + s, d['forward'][s:s + 1], d['backward'][s:s + 1] if with_bwd else None, state_p,
                   state_l)
            got = (state_p.cpu().numpy(), state_l.cpu().numpy())
            assert_same(got, (want[with_bwd, True][0][s], want[with_bwd, True][1][s]))
        assert _intact(buf_p, N * P * 8) and _intact(buf_l, N * P)
    # S > 1 with the LAST row on the inputs
    if S > 1:
        pos_all = torch.empty((S, N, P, 2), device=d['points'].device)
        lost_all = torch.empty((S, N, P), device=d['points'].device, dtype=torch.uint8)
        pos_all[-1], lost_all[-1] = d['points'], d['lost']
        _entry(pos_all[-1], lost_all[-1], d['start'], T0, d['forward'], d['backward'], pos_all, lost_all)
        assert_same((pos_all.cpu().numpy(), lost_all.cpu().numpy()), want[True, True])


@pytest.mark.parametrize('shape', SHAPES[3:], ids=IDS[3:])
def test_the_public_functions(shape):
    from tf_raft_amd import image_ops
    S, N, H, W, P = shape
    d, want = _device_case(shape)
    case = {k: v.copy() for k, v in _case(shape)[0].items()}                 # (writable: torch.from_numpy asks for it)
    # host arrays in, device tensors out; bool codes; float64 points narrow
    pos, lost = image_ops.track(case['points'].astype(np.float64), case['forward'], case['backward'], lost=case['lost'] != 0,
                                start=case['start'].astype(np.int64), t0=T0)
    assert tuple(pos.shape) == (S, N, P, 2) and pos.dtype == torch.float32 and tuple(lost.shape) == (S, N, P) and lost.dtype == torch.uint8
    w = np_track(case['points'], (case['lost'] != 0).astype(np.uint8), case['forward'], case['backward'], start=case['start'], t0=T0)
    assert_same((_np(pos), _np(lost)), w)
    # device tensors, no backward flow; one step from a 4-D flow comes without the step axis
    pos, lost = image_ops.track(d['points'], d['forward'])
    assert_same((_np(pos), _np(lost)), want[False, False])
    one_p, one_l = image_ops.track(d['points'], d['forward'][0], d['backward'][0])
    assert tuple(one_p.shape) == (N, P, 2) and tuple(one_l.shape) == (N, P)
    assert_same((_np(one_p), _np(one_l)), (want[True, False][0][0], want[True, False][1][0]))
    # alpha and beta reach the kernel
    loose = image_ops.track(d['points'], d['forward'], d['backward'], alpha=0.5, beta=3.0)
    assert_same((_np(loose[0]), _np(loose[1])), np_track(case['points'], None, case['forward'], case['backward'], alpha=0.5, beta=3.0))
    assert not np.array_equal(_np(loose[1]), want[True, False][1])
    # the launch form: into the caller's tensors, and in place
    out = (torch.empty((S, N, P, 2), device=d['points'].device), torch.empty((S, N, P), device=d['points'].device, dtype=torch.uint8))
    got = image_ops.track_launch(d['points'], d['forward'], d['backward'], d['lost'], d['start'], T0, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    assert_same((_np(out[0]), _np(out[1])), want[True, True])
    state_p, state_l = d['points'].clone(), d['lost'].clone()
    for s in range(S):
        image_ops.track_launch(state_p, d['forward'][s:s + 1], d['backward'][s:s + 1], state_l, d['start'], T0 + s,
                               out=(state_p.view(1, N, P, 2), state_l.view(1, N, P)))
    assert_same((_np(state_p), _np(state_l)), (want[True, True][0][-1], want[True, True][1][-1]))
    # the dense grid is point_grid's, and positions - grid is a long-range flow
    if P == H * W:
        grid = image_ops.point_grid(H, W, N=N)
        np.testing.assert_array_equal(grid, case['points'])
        pos, lost = image_ops.track(grid, d['forward'], d['backward'])
        assert_same((_np(pos), _np(lost)), want[True, False])
        sub = image_ops.point_grid(H, W, stride=4, N=N)
        pos, lost = image_ops.track(sub, d['forward'], d['backward'])
        full = want[True, False][0].reshape(S, N, H, W, 2)[:, :, ::4, ::4].reshape(S, N, -1, 2)
        np.testing.assert_array_equal(bits(_np(pos)), bits(full))


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


def _footage(H, W, T=4, N=2, P=200, seed=70):
    """N videos of T frames (a texture that shifts by a pixel or two per frame, plus noise) and P sub-pixel points in each."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0, 255, (N, H + 16, W + 16, 3))
    videos = np.stack([np.stack([base[n, 8 + t:8 + t + H, 8 - t:8 - t + W] for t in range(T)]) for n in range(N)])
    videos = (videos + rng.normal(0, 4, videos.shape)).clip(0, 255).astype(np.float32)
    points = np.stack([rng.uniform(0, W - 1, (N, P)), rng.uniform(0, H - 1, (N, P))], axis=-1).astype(np.float32)
    start = rng.integers(0, T, (N, P)).astype(np.int32)
    return videos, points, start


@pytest.mark.parametrize('route', ['plain', 'resize'])
def test_track_video_chains_the_flows_the_predictor_returns(route):
    from tf_raft_amd import image_ops
    model, (H, W) = _model(route)
    videos, points, start = _footage(H, W)
    N, T = videos.shape[:2]
    P = points.shape[1]
    for n in range(N):
        for bs in (2, 1):
            res = model.predict_bidirectional([videos[n, :-1], videos[n, 1:]], batch_size=bs)
            for alpha, begin in [(a, b) for a in ALPHAS for b in (None, start[n])]:
                pos, lost = model.track_video(videos[n], points[n], start=begin, batch_size=bs, alpha=alpha)
                assert isinstance(pos, np.ndarray) and pos.shape == (T, P, 2) and pos.dtype == np.float32
                assert isinstance(lost, np.ndarray) and lost.shape == (T, P) and lost.dtype == np.uint8
                np.testing.assert_array_equal(bits(pos[0]), bits(points[n]))
                assert not lost[0].any()
                want = image_ops.track(points[n][None], res.forward[:, None], res.backward[:, None],
                                       start=None if begin is None else begin[None], alpha=alpha)
                assert_same((pos[1:], lost[1:]), (_np(want[0])[:, 0], _np(want[1])[:, 0]))
                if begin is not None:
                    for k in range(T):                                       # given at frame k: rows 0 .. k hold the point
                        for row in range(k + 1):
                            np.testing.assert_array_equal(bits(pos[row][begin == k]), bits(points[n][begin == k]))
                            assert not lost[row][begin == k].any()
        # a stream of one video, frame by frame, is track_video at one pair per call
        by_video = model.track_video(videos[n], points[n], start=start[n], batch_size=1, alpha=LOOSE_ALPHA)
        tracker = model.tracker(points[n][None], start=start[n][None], alpha=LOOSE_ALPHA)
        assert tracker.push(videos[n, 0][None]) is None
        for t in range(1, T):
            p, l = tracker.push(videos[n, t][None])
            assert tuple(p.shape) == (1, P, 2) and tuple(l.shape) == (1, P) and p.is_cuda
            assert_same((_np(p)[0], _np(l)[0]), (by_video[0][t], by_video[1][t]))
    moved = int((bits(by_video[0][-1]) != bits(points[-1])).any(axis=-1).sum())
    report(f'track_video ({route})', tracked=int((by_video[1][-1] == 0).sum()), left=int((by_video[1][-1] == 1).sum()),
           failed=int((by_video[1][-1] == 2).sum()), moved=moved)


@pytest.mark.parametrize('route', ['plain', 'resize'])
def test_the_tracker_over_several_videos_without_the_test_and_after_a_reset(route):
    from tf_raft_amd import image_ops
    model, (H, W) = _model(route)
    videos, points, start = _footage(H, W)
    N, T = videos.shape[:2]
    frames = np.ascontiguousarray(videos.transpose(1, 0, 2, 3, 4))             # (T, N, H, W, 3): one push each
    other = np.ascontiguousarray(_footage(H, W, seed=71)[0].transpose(1, 0, 2, 3, 4))
    # N videos at once, with the test: every push is a track on the flows of that push's bidirectional pass
    tracker = model.tracker(points, start=start, alpha=LOOSE_ALPHA, beta=1.0)
    assert tracker.push(frames[0]) is None
    pos, lost = points, None
    for t in range(1, T):
        got = tracker.push(torch.from_numpy(frames[t]))
        res = model.predict_step_bidirectional((frames[t - 1], frames[t]))
        pos, lost = image_ops.track(pos, res.forward, res.backward, lost=lost, start=start, t0=t - 1, alpha=LOOSE_ALPHA, beta=1.0)
        assert_same((_np(got[0]), _np(got[1])), (_np(pos), _np(lost)))
    with pytest.raises(ValueError, match='reset'):
        tracker.push(frames[0][:, :32])
    # without the test: FlowVideo's flows, with and without the warm start, and only the borders cost points
    for warm in (False, True):
        stream = model.video(warm_start=warm)
        flows = [stream.push(frames[t]) for t in range(T)]
        assert flows[0] is None
        want = image_ops.track(points, torch.stack([_plain(f) for f in flows[1:]]))
        tracker = model.tracker(points, consistency=False, warm_start=warm)
        assert tracker.push(frames[0]) is None
        for t in range(1, T):
            got = tracker.push(frames[t])
            assert_same((_np(got[0]), _np(got[1])), (_np(want[0])[t - 1], _np(want[1])[t - 1]))
        assert not (_np(got[1]) == 2).any() and not np.array_equal(_np(got[0]), points)           # (points did move)
        # a second video through the same tracker after reset() is what a fresh tracker gives
        tracker.reset()
        second = [tracker.push(other[t]) for t in range(T)]
        fresh = model.tracker(points, consistency=False, warm_start=warm)
        for t in range(T):
            b = fresh.push(other[t])
            assert (second[t] is None) == (b is None) == (t == 0)
            if t:
                assert_same((_np(second[t][0]), _np(second[t][1])), (_np(b[0]), _np(b[1])))
    again = model.tracker(points, start=start, alpha=LOOSE_ALPHA)
    for t in range(T):
        again.push(frames[t])
    again.reset()
    second = [again.push(other[t]) for t in range(T)]
    assert second[0] is None
    fresh = model.tracker(points, start=start, alpha=LOOSE_ALPHA)
    for t in range(T):
        want2 = fresh.push(other[t])
    assert_same((_np(second[-1][0]), _np(second[-1][1])), (_np(want2[0]), _np(want2[1])))
    # track_video without the test rides on FlowVideo too
    pos, lost = model.track_video(videos[0], points[0], consistency=False, batch_size=2)
    flows = model.predict_video(videos[0], batch_size=2)
    want = image_ops.track(points[0][None], flows[:, None])
    assert_same((pos[1:], lost[1:]), (_np(want[0])[:, 0], _np(want[1])[:, 0]))
    report(f'tracker ({route})', tracked=int((lost[-1] == 0).sum()), left=int((lost[-1] == 1).sum()))

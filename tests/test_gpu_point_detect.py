"""Corner detection and re-seeding on the GPU: ``raft_corner_score_*``, ``raft_detect_points`` and
``raft_refill_points`` against the float32 NumPy restatements of tests/test_point_detect.py BIT FOR BIT (scores and positions
compared as uint32, counts and codes as they are: contraction is off and everything behind the score works on its bits, so there
is no tolerance anywhere), with guard bands around every output and around the workspace, repeats, mask and ``avoid``, special
values in float32 frames, the in-place refill; the public functions; and the model's tracker with ``points=None`` and
``replenish=True`` against ``image_ops.track`` / ``detect_points`` / ``np_refill`` on the flows the predictor returns.
"""
import numpy as np
import pytest
import torch

from conftest import report
from test_gpu_flow_track import LOOSE_ALPHA, _footage
from test_point_detect import (CASES, EMPTY, IDS, REFILL_SHAPES, assert_same_detection, bits, case_args, case_mask_avoid,
                               np_corner_score, np_detect_points, np_refill, refill_case)

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xAB


def _np(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy()


def _dev():
    from tf_raft_amd import _dev as d
    return d.require_gpu()


def _guarded(n, dtype, device):
    """A buffer of ``n`` elements between two guard bands, every byte FILL: (whole buffer, the typed view a launch writes)."""
    size = torch.empty((), dtype=dtype).element_size()
    buf = torch.full(((2 * GUARD + n) * size,), FILL, dtype=torch.uint8, device=device)
    return buf, buf[GUARD * size:(GUARD + n) * size].view(dtype)


def _intact(buf, view):
    b = buf.cpu().numpy()
    band = (len(b) - view.numel() * view.element_size()) // 2
    return bool((b[:band] == FILL).all() and (b[-band:] == FILL).all())


_WANT = {}


def _want(name):
    """What the restatement says about one case, computed once and left unchanged."""
    if name not in _WANT:
        frames, kw = case_args(name)
        score = np_corner_score(frames, kw['block_radius'], kw['method'], 0.04, kw['border'])
        det = np_detect_points(frames, **kw)
        for a in score + det:
            a.setflags(write=False)
        _WANT[name] = (frames, kw, score, det)
    return _WANT[name]


def _to(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


# ------------------------------------------------------------------ the score map
def _score_entry(frames, r, method, border, with_max=True):
    """raft_corner_score_* through the library itself into guarded outputs: (score, smax or None, guards intact)."""
    from tf_raft_amd import _dev as d
    from tf_raft_amd._ffi import check
    N, H, W, Cn = frames.shape
    buf_s, score = _guarded(N * H * W, torch.float32, frames.device)
    buf_m, smax = _guarded(N, torch.float32, frames.device)
    fn = d.lib().raft_corner_score_u8_f32 if frames.dtype == torch.uint8 else d.lib().raft_corner_score_f32
    check(fn(d.ptr(frames), d.ptr(score), d.ptr(smax) if with_max else None, N, H, W, Cn, r, {'min_eig': 0, 'harris': 1}[method], 0.04,
             border, d.stream_ptr()), 'corner_score')
    torch.cuda.synchronize()
    intact = _intact(buf_s, score) and _intact(buf_m, smax) and (with_max or bool((smax.view(torch.uint8) == FILL).all()))
    return score.cpu().numpy().reshape(N, H, W), smax.cpu().numpy() if with_max else None, intact


@pytest.mark.parametrize('name', IDS)
def test_the_score_map_is_the_restatement_bit_for_bit(name):
    frames, kw, (want, want_max), _ = _want(name)
    x = _to(frames, _dev())
    score, smax, intact = _score_entry(x, kw['block_radius'], kw['method'], kw['border'])
    np.testing.assert_array_equal(bits(score), bits(want))
    np.testing.assert_array_equal(bits(smax), bits(want_max))
    assert intact
    again, _, intact = _score_entry(x, kw['block_radius'], kw['method'], kw['border'], with_max=False)
    np.testing.assert_array_equal(bits(again), bits(score))
    assert intact
    # the other method and the other end of the window sizes on the same frames
    other = 'harris' if kw['method'] == 'min_eig' else 'min_eig'
    r2 = 3 if kw['block_radius'] == 1 else 1
    border2 = max(kw['border'], r2 + 1)
    want2, want2_max = np_corner_score(frames, r2, other, 0.04, border2)
    score2, smax2, intact = _score_entry(x, r2, other, border2)
    np.testing.assert_array_equal(bits(score2), bits(want2))
    np.testing.assert_array_equal(bits(smax2), bits(want2_max))
    assert intact
    report(f'corner_score {name}', positive=int((want > 0).sum()), smax=float(want_max.max()))


# ------------------------------------------------------------------ the detection
def _detect_entry(frames, kw, mask=None, avoid=None):
    """raft_detect_points through the library itself, every output and the workspace guarded: ((points, scores, count, lost),
    guards intact)."""
    from tf_raft_amd import _dev as d
    from tf_raft_amd import image_ops
    from tf_raft_amd._ffi import check
    N, H, W, Cn = frames.shape
    K, m = kw['max_points'], kw['min_distance']
    dev = frames.device
    buf_p, points = _guarded(N * K * 2, torch.float32, dev)
    buf_s, scores = _guarded(N * K, torch.float32, dev)
    buf_c, count = _guarded(N, torch.int32, dev)
    buf_l, lost = _guarded(N * K, torch.uint8, dev)
    buf_w, ws = _guarded(image_ops.detect_workspace_bytes(N, H, W, m), torch.uint8, dev)
    ptr = lambda t: None if t is None else d.ptr(t)       # noqa: E731
    check(d.lib().raft_detect_points(d.ptr(frames), int(frames.dtype == torch.uint8), ptr(mask), ptr(avoid[0]) if avoid else None,
                                     ptr(avoid[1]) if avoid else None, avoid[0].shape[1] if avoid else 0, d.ptr(points), d.ptr(scores),
                                     d.ptr(count), d.ptr(lost), N, H, W, Cn, K, m, kw['quality_level'], kw['block_radius'],
                                     {'min_eig': 0, 'harris': 1}[kw['method']], 0.04, kw['border'], d.ptr(ws), d.stream_ptr()),
          'detect_points')
    torch.cuda.synchronize()
    intact = all(_intact(b, v) for b, v in ((buf_p, points), (buf_s, scores), (buf_c, count), (buf_l, lost), (buf_w, ws)))
    return (points.cpu().numpy().reshape(N, K, 2), scores.cpu().numpy().reshape(N, K), count.cpu().numpy(),
            lost.cpu().numpy().reshape(N, K)), intact


@pytest.mark.parametrize('name', IDS)
def test_the_detection_is_the_restatement_bit_for_bit(name):
    frames, kw, _, want = _want(name)
    x = _to(frames, _dev())
    got, intact = _detect_entry(x, kw)
    assert_same_detection(got, want)
    assert intact
    again, intact = _detect_entry(x, kw)                        # the candidates are gathered in another order: the same bytes
    for a, b in zip(again, got):
        assert a.tobytes() == b.tobytes()
    assert intact
    N, K = want[1].shape
    for n in range(N):
        assert (got[3][n, :got[2][n]] == 0).all() and (got[3][n, got[2][n]:] == EMPTY).all()
        assert (got[0][n, got[2][n]:] == -1).all() and not got[1][n, got[2][n]:].any()
    report(f'detect_points {name}', K=K, count=want[2].tolist())


@pytest.mark.parametrize('name', ['batch_f32_c3', 'periodic_u8_c3', 'tile_edge_u8_c1'])
def test_mask_and_avoid(name):
    from tf_raft_amd import image_ops
    frames, kw, mask, avoid, lost = case_mask_avoid(name)
    dev = _dev()
    x, dm, da, dl = _to(frames, dev), _to(mask, dev), _to(avoid, dev), _to(lost, dev)
    base = _want(name)[3]
    for m_, a_ in ((mask, None), (None, (avoid, lost)), (mask, (avoid, lost))):
        want = np_detect_points(frames, mask=m_, avoid=a_, **kw)
        got, intact = _detect_entry(x, kw, dm if m_ is not None else None, (da, dl) if a_ is not None else None)
        assert_same_detection(got, want)
        assert intact
        assert got[0].tobytes() != base[0].tobytes()             # (points did go)
        # the public function, host arrays and a bool mask in
        pub = image_ops.detect_points(frames.copy(), mask=None if m_ is None else m_ != 0, avoid=a_, return_lost=True, **kw)
        assert_same_detection(tuple(_np(t) for t in pub), want)


def test_the_public_functions():
    from tf_raft_amd import image_ops
    frames, kw, (want, want_max), det = _want('batch_f32_c3')
    score, smax = image_ops.corner_score(frames.copy(), kw['block_radius'], kw['method'], border=kw['border'], return_max=True)
    assert tuple(score.shape) == frames.shape[:3] and score.dtype == torch.float32 and tuple(smax.shape) == (3,) and score.is_cuda
    np.testing.assert_array_equal(bits(_np(score)), bits(want))
    np.testing.assert_array_equal(bits(_np(smax)), bits(want_max))
    one = image_ops.corner_score(frames[2].astype(np.float64), kw['block_radius'], kw['method'], border=kw['border'])      # narrows
    assert tuple(one.shape) == frames.shape[1:3]
    np.testing.assert_array_equal(bits(_np(one)), bits(want[2]))
    res = image_ops.detect_points(torch.from_numpy(frames.copy()), **kw)
    assert len(res) == 3 and res[0].is_cuda and res[2].dtype == torch.int32
    assert_same_detection(tuple(_np(t) for t in res), det[:3])
    # the launch form: into the caller's tensors, through the caller's workspace
    x = _to(frames, _dev())
    N, K = det[1].shape
    out = (torch.empty((N, K, 2), device=x.device), torch.empty((N, K), device=x.device), torch.empty((N,), device=x.device, dtype=torch.int32),
           torch.empty((N, K), device=x.device, dtype=torch.uint8))
    ws = torch.empty((image_ops.detect_workspace_bytes(*frames.shape[:3], kw['min_distance']),), device=x.device, dtype=torch.uint8)
    got = image_ops.detect_points_launch(x, out=out, workspace=ws, want_lost=True, **kw)
    assert all(a is b for a, b in zip(got, out))
    assert_same_detection(tuple(_np(t) for t in out), det)
    # defaults: K alone
    frames_u8, _, _, _ = _want('periodic_u8_c3')
    assert_same_detection(tuple(_np(t) for t in image_ops.detect_points(frames_u8.copy(), 9)), np_detect_points(frames_u8, 9)[:3])


# ------------------------------------------------------------------ the refill
def _refill_entry(pos, lost, new_points, new_count, t, born, ids, next_id, pos_out, lost_out):
    from tf_raft_amd import _dev as d
    from tf_raft_amd._ffi import check
    N, P = lost.shape
    check(d.lib().raft_refill_points(d.ptr(pos), d.ptr(lost), d.ptr(new_points), d.ptr(new_count), t, d.ptr(pos_out), d.ptr(lost_out),
                                     d.ptr(born), d.ptr(ids), d.ptr(next_id), N, P, new_points.shape[1], d.stream_ptr()), 'refill_points')
    torch.cuda.synchronize()


@pytest.mark.parametrize('shape', REFILL_SHAPES, ids=['x'.join(map(str, s)) for s in REFILL_SHAPES])
def test_the_refill_is_the_restatement_bit_for_bit(shape):
    from tf_raft_amd import image_ops
    N, P, K = shape
    case = refill_case(*shape)
    pos, lost, new_points, new_count, born, ids, next_id = case
    T = 11
    want = np_refill(pos, lost, new_points, new_count, T, born, ids, next_id)
    dev = _dev()
    for in_place in (False, True):
        d_pos, d_lost, d_new, d_count = _to(pos, dev), _to(lost, dev), _to(new_points, dev), _to(new_count, dev)
        bufs = [_guarded(N * P * 2, torch.float32, dev), _guarded(N * P, torch.uint8, dev), _guarded(N * P, torch.int32, dev),
                _guarded(N * P, torch.int32, dev), _guarded(N, torch.int32, dev)]
        o_pos, o_lost, d_born, d_ids, d_next = (v for _, v in bufs)
        d_born.copy_(_to(born, dev).reshape(-1)), d_ids.copy_(_to(ids, dev).reshape(-1)), d_next.copy_(_to(next_id, dev))
        if in_place:
            o_pos.copy_(d_pos.reshape(-1)), o_lost.copy_(d_lost.reshape(-1))
            d_pos, d_lost = o_pos.view(N, P, 2), o_lost.view(N, P)
        _refill_entry(d_pos, d_lost, d_new, d_count, T, d_born, d_ids, d_next, o_pos, o_lost)
        got = (o_pos.cpu().numpy().reshape(N, P, 2), o_lost.cpu().numpy().reshape(N, P), d_born.cpu().numpy().reshape(N, P),
               d_ids.cpu().numpy().reshape(N, P), d_next.cpu().numpy())
        np.testing.assert_array_equal(bits(got[0]), bits(want[0]))
        for g, w in zip(got[1:], want[1:]):
            assert g.dtype == w.dtype
            np.testing.assert_array_equal(g, w)
        assert all(_intact(b, v) for b, v in bufs)
        if not in_place:                                         # the inputs of the out-of-place form are untouched
            np.testing.assert_array_equal(bits(_np(d_pos)), bits(pos))
            np.testing.assert_array_equal(_np(d_lost), lost)
    # the Python form, in place
    t = [_to(a, dev) for a in case]
    res = image_ops.refill_points_launch(t[0], t[1], t[2], t[3], T, t[4], t[5], t[6], out=(t[0], t[1]))
    assert res[0] is t[0] and res[1] is t[1]
    for g, w in zip((t[0], t[1], t[4], t[5], t[6]), want):
        assert _np(g).tobytes() == w.tobytes()
    fresh = image_ops.refill_points_launch(*[_to(a, dev) for a in case[:4]], T, *[_to(a, dev) for a in case[4:]])
    assert _np(fresh[0]).tobytes() == want[0].tobytes() and _np(fresh[1]).tobytes() == want[1].tobytes()
    report(f'refill {shape}', lost=int((lost != 0).sum()), filled=int((want[4] - next_id).sum()))


# ------------------------------------------------------------------ the model
DETECT = dict(min_distance=5, quality_level=0.02, block_radius=1, method='min_eig', border=6)
K_MODEL = 96            # more than a 64 x 96 frame yields at min_distance = 5 under the quality level: some slots stay empty


def _model(kind):
    import tf_raft_amd
    from tf_raft_amd import weights as wm
    if kind == 'small':
        return tf_raft_amd.SmallRAFT(weights=wm.init_weights('small', seed=6, perturb=True), iters_pred=3)
    return tf_raft_amd.RAFT(weights=wm.init_weights('raft', seed=6, perturb=True), iters_pred=2)


@pytest.mark.parametrize('kind', ['small', 'raft'])
def test_track_video_detects_its_points_in_frame_0(kind):
    from tf_raft_amd import image_ops
    model = _model(kind)
    H, W = 64, 96
    videos, points, start = _footage(H, W, N=1)
    video = videos[0]
    T = video.shape[0]
    for K in (K_MODEL, 7):                                       # above and below what the detector finds
        det = image_ops.detect_points(video[:1], K, return_lost=True, **DETECT)
        d_pts, d_lost, count = _np(det[0])[0], _np(det[3])[0], int(_np(det[2])[0])
        assert_same_detection(tuple(_np(t) for t in det), np_detect_points(video[:1], K, **DETECT))
        assert (0 < count < K) if K == K_MODEL else count == K
        for bs in (2, 1):
            pos, lost = model.track_video(video, None, max_points=K, detect=DETECT, batch_size=bs, alpha=LOOSE_ALPHA)
            assert pos.shape == (T, K, 2) and lost.shape == (T, K) and lost.dtype == np.uint8
            want = model.track_video(video, d_pts[:count], batch_size=bs, alpha=LOOSE_ALPHA)
            np.testing.assert_array_equal(bits(pos[:, :count]), bits(want[0]))
            np.testing.assert_array_equal(lost[:, :count], want[1])
            assert (lost[:, count:] == EMPTY).all() and (pos[:, count:] == -1).all()          # empty in every row
            np.testing.assert_array_equal(lost[0], d_lost)
    # the existing calling forms: the same bytes as image_ops.track on the returned flows
    res = model.predict_bidirectional([video[:-1], video[1:]], batch_size=2)
    pos, lost = model.track_video(video, points[0], start=start[0], batch_size=2, alpha=LOOSE_ALPHA)
    want = image_ops.track(points[0][None], res.forward[:, None], res.backward[:, None], start=start[0][None], alpha=LOOSE_ALPHA)
    np.testing.assert_array_equal(bits(pos[1:]), bits(_np(want[0])[:, 0]))
    np.testing.assert_array_equal(lost[1:], _np(want[1])[:, 0])
    report(f'track_video detect ({kind})', found=count, tracked=int((lost[-1] == 0).sum()))


@pytest.mark.parametrize('kind,alpha', [('small', LOOSE_ALPHA), ('raft', LOOSE_ALPHA), ('small', 0.01)])
def test_the_replenishing_tracker_push_by_push(kind, alpha):
    """After every push the state is np_refill applied to the tracker's own previous state, tracked along the flows of that push,
    and detect_points on the pushed frames.  Under UnFlow's alpha nearly every point fails each push and every slot is refilled."""
    from tf_raft_amd import image_ops
    model = _model(kind)
    H, W = 64, 96
    videos, _, _ = _footage(H, W, N=2)
    N, T = videos.shape[:2]
    frames = np.ascontiguousarray(videos.transpose(1, 0, 2, 3, 4))
    K = K_MODEL
    tracker = model.tracker(None, max_points=K, replenish=True, detect=DETECT, alpha=alpha)
    assert tracker.push(frames[0]) is None
    det = np_detect_points(frames[0], K, **DETECT)
    assert (det[2] > 0).all() and (det[2] < K).all()
    pos, lost = det[0], det[3]
    np.testing.assert_array_equal(bits(_np(tracker._pos)), bits(pos))
    np.testing.assert_array_equal(_np(tracker._lost), lost)
    ids = np.where(lost == EMPTY, -1, np.arange(K, dtype=np.int32)[None]).astype(np.int32)
    born = np.where(lost == EMPTY, -1, 0).astype(np.int32)
    next_id = np.full(N, K, np.int32)
    np.testing.assert_array_equal(_np(tracker.ids), ids)
    np.testing.assert_array_equal(_np(tracker.born), born)
    seen = [set(ids[n][ids[n] >= 0].tolist()) for n in range(N)]
    refilled = 0
    for t in range(1, T):
        got = tracker.push(frames[t])
        res = model.predict_step_bidirectional((frames[t - 1], frames[t]))
        tp, tl = image_ops.track(pos, res.forward, res.backward, lost=lost, alpha=alpha)
        tp, tl = _np(tp), _np(tl)
        new = image_ops.detect_points(frames[t], K, avoid=(tp, tl), **DETECT)
        new_np = np_detect_points(frames[t], K, avoid=(tp, tl), **DETECT)
        assert_same_detection(tuple(_np(a) for a in new), new_np[:3])
        before = ids.copy()
        pos, lost, born, ids, next_id = np_refill(tp, tl, new_np[0], new_np[2], t, born, ids, next_id)
        np.testing.assert_array_equal(bits(_np(got[0])), bits(pos))
        np.testing.assert_array_equal(_np(got[1]), lost)
        np.testing.assert_array_equal(_np(tracker.ids), ids)
        np.testing.assert_array_equal(_np(tracker.born), born)
        assert tuple(got[0].shape) == (N, K, 2) and got[0].is_cuda and tracker.ids.dtype == torch.int32
        for n in range(N):                                       # ids never repeat
            fresh = ids[n][ids[n] != before[n]]
            assert not (set(fresh.tolist()) & seen[n]) and len(set(fresh.tolist())) == len(fresh)
            seen[n] |= set(fresh.tolist())
            refilled += len(fresh)
    assert refilled > 0
    if alpha == 0.01:
        assert (born[lost == 0] == T - 1).mean() > 0.8           # nearly every live point came in at the last push
    report(f'replenish ({kind}, alpha={alpha})', refilled=refilled, live=int((lost == 0).sum()), empty=int((lost == EMPTY).sum()))


def test_replenish_with_given_points_a_start_and_track_video():
    from tf_raft_amd import image_ops
    model = _model('small')
    H, W = 64, 96
    videos, points, start = _footage(H, W, N=1, P=40)
    video = videos[0]
    T = video.shape[0]
    # the tracker with given points: P is theirs, a slot that waits for its start is left alone
    tracker = model.tracker(points, start=start, replenish=True, detect=DETECT, alpha=0.01)
    assert tracker.push(video[:1]) is None
    pos, lost = points, np.zeros((1, 40), np.uint8)
    born, ids, next_id = start.astype(np.int32), np.arange(40, dtype=np.int32)[None].copy(), np.array([40], np.int32)
    for t in range(1, T):
        got = tracker.push(video[t:t + 1])
        res = model.predict_step_bidirectional((video[t - 1:t], video[t:t + 1]))
        tp, tl = image_ops.track(pos, res.forward, res.backward, lost=lost, start=born, t0=t - 1, alpha=0.01)
        tp, tl = _np(tp), _np(tl)
        new = np_detect_points(video[t:t + 1], 40, avoid=(tp, tl), **DETECT)
        pos, lost, born, ids, next_id = np_refill(tp, tl, new[0], new[2], t, born, ids, next_id)
        np.testing.assert_array_equal(bits(_np(got[0])), bits(pos))
        np.testing.assert_array_equal(_np(got[1]), lost)
        np.testing.assert_array_equal(_np(tracker.ids), ids)
        np.testing.assert_array_equal(_np(tracker.born), born)
    assert next_id[0] > 40
    # track_video refills at the chunk boundaries only, and one push per frame is batch_size = 1
    by_push = model.tracker(None, max_points=K_MODEL, replenish=True, detect=DETECT, alpha=0.01)
    by_push.push(video[:1])
    first_ids = _np(by_push.ids)[0].copy()
    rows = [by_push.push(video[t:t + 1]) + (by_push.ids.clone(),) for t in range(1, T)]
    pos, lost, all_ids = model.track_video(video, None, max_points=K_MODEL, replenish=True, detect=DETECT, batch_size=1, alpha=0.01)
    assert pos.shape == (T, K_MODEL, 2) and lost.shape == (T, K_MODEL) and all_ids.shape == (T, K_MODEL) and all_ids.dtype == np.int32
    np.testing.assert_array_equal(all_ids[0], first_ids)
    for t in range(1, T):
        np.testing.assert_array_equal(bits(pos[t]), bits(_np(rows[t - 1][0])[0]))
        np.testing.assert_array_equal(lost[t], _np(rows[t - 1][1])[0])
        np.testing.assert_array_equal(all_ids[t], _np(rows[t - 1][2])[0])
    pos2, lost2, ids2 = model.track_video(video, None, max_points=K_MODEL, replenish=True, detect=DETECT, batch_size=2, alpha=0.01)
    plain = model.track_video(video, None, max_points=K_MODEL, detect=DETECT, batch_size=2, alpha=0.01)
    np.testing.assert_array_equal(bits(pos2[:2]), bits(plain[0][:2]))         # nothing comes in before the first boundary (frame 2)
    np.testing.assert_array_equal(lost2[:2], plain[1][:2])
    np.testing.assert_array_equal(ids2[1], ids2[0])
    came_in = ids2[2] != ids2[1]
    assert came_in.any() and (lost2[2] == 0).sum() > (plain[1][2] == 0).sum()
    np.testing.assert_array_equal(bits(pos2[2][~came_in]), bits(plain[0][2][~came_in]))     # the other slots are the plain track's
    assert (plain[1][2][came_in] != 0).all()                                                # only lost slots were refilled

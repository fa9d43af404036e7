"""Object identity through a video on the GPU: ``raft_object_overlap``, ``raft_match_objects`` and
``raft_chain_object_ids`` against the NumPy restatements of tests/test_object_track.py on the cases built there.  Every comparison
is equality of integers: there is NO tolerance anywhere.  Outputs arrive filled with 0xAB between guard bands (the entries zero what
they count into), every entry runs twice on the same buffers, a slice is run alone and inside a batch; then the public functions,
a scripted clip with the model taken out, and ``ObjectTracker`` / ``track_objects_video`` on both models against
``moving_objects_step`` per pair plus the restatement chained on the host.
"""
import numpy as np
import pytest
import torch

from conftest import report
from test_object_track import (CASES, SLOTS, case_args, np_chain_ids, np_match_objects, np_object_overlap, random_chain, slot_areas,
                               want_overlap)

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xAB


def _np(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy()


def _dev():
    from tf_raft_amd import _dev as d
    return d.require_gpu()


def _to(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _guarded(shape, dev):
    """An int32 array between two guard bands, every byte FILL: (whole buffer, the view a launch writes)."""
    n = int(np.prod(shape))
    buf = torch.full(((2 * GUARD + n) * 4,), FILL, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD * 4:(GUARD + n) * 4].view(torch.int32).view(shape)


def _intact(buf):
    b = buf.cpu().numpy()
    return bool((b[:GUARD * 4] == FILL).all() and (b[-GUARD * 4:] == FILL).all())


def _untouched(view):
    return bool((view.contiguous().view(torch.uint8) == FILL).all())


def _ptr(t):
    from tf_raft_amd import _dev as d
    return None if t is None else d.ptr(t)


def _overlap_entry(prev, flow, nxt, K, out):
    from tf_raft_amd import _dev as d
    from tf_raft_amd._ffi import check
    M, H, W = prev.shape
    check(d.lib().raft_object_overlap(d.ptr(prev), d.ptr(flow), d.ptr(nxt), d.ptr(out[0]), d.ptr(out[1]), M, H, W, K, d.stream_ptr()),
          'object_overlap')
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def _match_entry(overlap, landed, area, share, match, count, origin):
    from tf_raft_amd import _dev as d
    from tf_raft_amd._ffi import check
    M, K, _ = overlap.shape
    check(d.lib().raft_match_objects(d.ptr(overlap), d.ptr(landed), d.ptr(area), share, d.ptr(match), _ptr(count), _ptr(origin), M, K,
                                     d.stream_ptr()), 'match_objects')
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (match, count, origin))


def _chain_entry(match, count, t0, ids_in, born_in, next_id, ids, born):
    from tf_raft_amd import _dev as d
    from tf_raft_amd._ffi import check
    S, N, K = match.shape
    check(d.lib().raft_chain_object_ids(d.ptr(match), d.ptr(count), t0, d.ptr(ids_in), d.ptr(born_in), d.ptr(next_id), d.ptr(ids),
                                        d.ptr(born), S, N, K, d.stream_ptr()), 'chain_object_ids')
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the overlap counts
@pytest.mark.parametrize('K', SLOTS)
@pytest.mark.parametrize('name', list(CASES))
def test_the_overlap_entry_is_the_restatement_integer_for_integer(name, K):
    c = case_args(name)
    want, want_landed, _ = want_overlap(name, K)
    dev = _dev()
    prev, flow, nxt = _to(c['prev'], dev), _to(c['flow'], dev), _to(c['next'], dev)
    M = prev.shape[0]
    (b0, overlap), (b1, landed) = _guarded((M, K, K), dev), _guarded((M, K), dev)
    got = _overlap_entry(prev, flow, nxt, K, (overlap, landed))               # 0xAB everywhere: the entry zeroes what it counts into
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], want_landed)
    again = _overlap_entry(prev, flow, nxt, K, (overlap, landed))             # on its own results: zeroed again, not added to
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    assert _intact(b0) and _intact(b1)
    with torch.cuda.stream(torch.cuda.Stream()):
        other = _overlap_entry(prev, flow, nxt, K, (torch.empty_like(overlap), torch.empty_like(landed)))
    assert other[0].tobytes() == got[0].tobytes() and other[1].tobytes() == got[1].tobytes()
    for m in range(M):                                                        # a slice does not depend on its neighbours
        alone = _overlap_entry(prev[m:m + 1].contiguous(), flow[m:m + 1].contiguous(), nxt[m:m + 1].contiguous(), K,
                               (torch.empty((1, K, K), dtype=torch.int32, device=dev), torch.empty((1, K), dtype=torch.int32, device=dev)))
        assert alone[0][0].tobytes() == got[0][m].tobytes() and alone[1][0].tobytes() == got[1][m].tobytes()


# ------------------------------------------------------------------ the matching
QUARTER_UP = float(np.nextafter(np.float32(0.25), np.float32(1)))


def _check_match(overlap, landed, area, share, dev):
    M, K, _ = overlap.shape
    want = np_match_objects(overlap, landed, area, share)
    o, l, a = _to(overlap, dev), _to(landed, dev), _to(area, dev)
    bufs = [_guarded((M, K), dev) for _ in range(3)]
    got = _match_entry(o, l, a, share, *(v for _, v in bufs))
    for g, w, what in zip(got, want, ('match', 'match_overlap', 'origin')):
        np.testing.assert_array_equal(g, w, what)
    again = _match_entry(o, l, a, share, *(v for _, v in bufs))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, got))
    assert all(_intact(b) for b, _ in bufs)
    # the optional outputs: NULL leaves them alone and changes nothing else
    fresh = [_guarded((M, K), dev) for _ in range(3)]
    only = _match_entry(o, l, a, share, fresh[0][1], None, None)
    assert only[0].tobytes() == got[0].tobytes() and _untouched(fresh[1][1]) and _untouched(fresh[2][1])
    _match_entry(o, l, a, share, fresh[0][1], None, fresh[2][1])
    assert _untouched(fresh[1][1]) and fresh[2][1].cpu().numpy().tobytes() == got[2].tobytes()
    for m in range(M):                                                        # a slice does not depend on its neighbours
        alone = _match_entry(o[m:m + 1].contiguous(), l[m:m + 1].contiguous(), a[m:m + 1].contiguous(), share,
                             *(torch.empty((1, K), dtype=torch.int32, device=dev) for _ in range(3)))
        assert all(x[0].tobytes() == y[m].tobytes() for x, y in zip(alone, got))
    return got


@pytest.mark.parametrize('share', (0.25, 0.5, 1.0, QUARTER_UP))
@pytest.mark.parametrize('K', SLOTS)
@pytest.mark.parametrize('name', list(CASES))
def test_the_match_entry_is_the_walk(name, K, share):
    overlap, landed, area = want_overlap(name, K)
    match, count, origin = _check_match(overlap, landed, area, share, _dev())
    if name == 'objects' and K >= 64:                                         # (the answers known by hand, once more, from the device)
        assert match[0, :4].tolist() == [2, 0, -1, 3] and origin[0, :4].tolist() == [2, 0, 0, 3]
        assert match[1, :5].tolist() == {0.25: [1, 0, 2, 3, 4], 0.5: [1, 0, -1, 3, 4], 1.0: [1, 0, -1, -1, 4], QUARTER_UP: [1, 0, -1, 3, 4]}[share]
    if name == 'empty':
        assert (match[:2] == -1).all() and (origin[:2] == -1).all() and (count[:2] == 0).all() and match[2, 0] == 1


@pytest.mark.parametrize('K', (1, 7, 64, 128))
def test_the_match_entry_on_random_tables_and_on_a_chain_of_k_rounds(K):
    rng = np.random.default_rng(320 + K)
    M = 4
    table = (rng.integers(0, 5, (M, K, K)) * (rng.random((M, K, K)) < 0.3)).astype(np.int32)      # small counts: ties everywhere
    table[1] = rng.integers(0, 1000, (K, K)).astype(np.int32) * (rng.random((K, K)) < 0.05)
    table[2] = 0
    for i in range(K):                                # every pair but the largest waits for the one above it: K rounds
        table[2, i, i] = 2 * (K - i)
        if i + 1 < K:
            table[2, i + 1, i] = 2 * (K - i) - 1
    table[3] = rng.integers(-5, 3, (K, K)).astype(np.int32)                   # negative counts are no counts
    landed = (np.maximum(table, 0).sum(2) + rng.integers(0, 3, (M, K))).astype(np.int32)
    area = (np.maximum(table, 0).sum(1) + rng.integers(0, 3, (M, K))).astype(np.int32)
    landed[2], area[2] = 1, 1
    for share in (0.05, 0.5, 1.0):
        match = _check_match(table, landed, area, share, _dev())[0]
    assert match[2].tolist() == list(range(K))


# ------------------------------------------------------------------ the identities
@pytest.mark.parametrize('K', SLOTS)
def test_the_chain_entry_is_the_loops(K):
    dev = _dev()
    S, N, t0 = 5, 3, 4
    match, count, ids_in, born_in, next_id = random_chain(330 + K, S, N, K)
    want_ids, want_born, want_next = np_chain_ids(match, count, t0, ids_in, born_in, next_id)
    m, c = _to(match, dev), _to(count, dev)
    (b0, ids), (b1, born) = _guarded((S, N, K), dev), _guarded((S, N, K), dev)
    nxt = _to(next_id, dev)
    _chain_entry(m, c, t0, _to(ids_in, dev), _to(born_in, dev), nxt, ids, born)
    np.testing.assert_array_equal(_np(ids), want_ids)
    np.testing.assert_array_equal(_np(born), want_born)
    np.testing.assert_array_equal(_np(nxt), want_next)
    assert _intact(b0) and _intact(b1)
    # S = 5 is five times S = 1, in place
    state = (_to(ids_in, dev), _to(born_in, dev), _to(next_id, dev))
    for s in range(S):
        _chain_entry(m[s:s + 1], c[s:s + 1], t0 + s, state[0], state[1], state[2], state[0], state[1])       # ids == ids_in
        np.testing.assert_array_equal(_np(state[0]), want_ids[s])
        np.testing.assert_array_equal(_np(state[1]), want_born[s])
    np.testing.assert_array_equal(_np(state[2]), want_next)
    # a video from its start: ids never repeat and next_id adds up
    start = torch.full((N, K), -1, dtype=torch.int32, device=dev)
    zero = torch.zeros((N,), dtype=torch.int32, device=dev)
    m0 = m.clone()
    m0[0] = -1
    _chain_entry(m0, c, 0, start, start.clone(), zero, ids, born)
    got_ids, got_born = _np(ids), _np(born)
    w_ids, w_born, w_next = np_chain_ids(_np(m0), count, 0, _np(start), _np(start), np.zeros((N,), np.int32))
    np.testing.assert_array_equal(got_ids, w_ids), np.testing.assert_array_equal(got_born, w_born)
    np.testing.assert_array_equal(_np(zero), w_next)
    filled = np.clip(count, 0, K)
    for n in range(N):
        new = [got_ids[s, n, b] for s in range(S) for b in range(filled[s, n]) if got_born[s, n, b] == s]
        assert sorted(new) == list(range(len(new))) == list(range(int(_np(zero)[n])))
        assert (got_ids[0, n, :filled[0, n]] == np.arange(filled[0, n])).all()       # the first objects: 0 .. count - 1
        for s in range(S):
            assert (got_ids[s, n, filled[s, n]:] == -1).all() and (got_born[s, n, filled[s, n]:] == -1).all()


# ------------------------------------------------------------------ the public functions
def test_match_objects_takes_host_arrays_and_leading_axes():
    from tf_raft_amd import image_ops
    from tf_raft_amd.image_ops import Objects
    c = {k: v.copy() for k, v in case_args('objects').items()}               # (the cases are read-only; torch wants writable arrays)
    K = 64
    overlap, landed, area = (a.copy() for a in want_overlap('objects', K))
    want = np_match_objects(overlap, landed, area, 0.25)

    def side(labels, areas, lead):
        return Objects(labels.reshape(lead + labels.shape[1:]), None, areas.reshape(lead + (K,)), None, None, None)

    for lead in ((2,), (1, 2), (2, 1)):
        got = image_ops.match_objects(side(c['prev'], area, lead), c['flow'].reshape(lead + c['flow'].shape[1:]), side(c['next'], area, lead))
        assert isinstance(got, image_ops.ObjectMatch) and all(t.is_cuda and tuple(t.shape) == lead + (K,) for t in got)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(_np(g).reshape(2, K), w)
    dev = _dev()
    got = image_ops.match_objects(side(_to(c['prev'], dev), _to(area, dev), (2,)), _to(c['flow'], dev), side(_to(c['next'], dev), _to(area, dev), (2,)),
                                  min_overlap=0.5)
    np.testing.assert_array_equal(_np(got.match), np_match_objects(overlap, landed, area, 0.5)[0])
    o, l = image_ops.object_overlap_launch(_to(c['prev'], dev), _to(c['flow'], dev), _to(c['next'], dev), 3)
    w = want_overlap('objects', 3)
    np.testing.assert_array_equal(_np(o), w[0]), np.testing.assert_array_equal(_np(l), w[1])
    only = image_ops.match_objects_launch(o, l, _to(w[2], dev), 0.25, want_overlap=False, want_origin=False)
    assert only.overlap is None and only.origin is None
    np.testing.assert_array_equal(_np(only.match), np_match_objects(*w, 0.25)[0])


# ------------------------------------------------------------------ a scripted clip, the model taken out
def _slots_by_area(canvas, K):
    """A map of object names (1, 2, ...; 0 = background) as ``raft_find_objects`` would number it: slots by area, largest first,
    of equal areas the one that starts earlier in raster order.  Returns (labels, {name: slot})."""
    names = [v for v in np.unique(canvas) if v > 0]
    order = sorted(names, key=lambda v: (-int((canvas == v).sum()), int(np.flatnonzero(canvas == v)[0])))[:K]
    labels = np.zeros(canvas.shape, np.int32)
    for slot, v in enumerate(order):
        labels[canvas == v] = slot + 1
    return labels, {int(v): slot for slot, v in enumerate(order)}


def _scripted_clip(T=6, H=32, W=64):
    """Rectangles 1 and 2 cross (1 passes in front, 2 stays half visible), 3 leaves on the right while 4 enters on the left; every
    pixel carries the exact vector of the rectangle it shows."""
    speed = {1: 6, 2: -6, 3: 6, 4: 6}
    rows = {1: (4, 12), 2: (8, 16), 3: (20, 28), 4: (22, 30)}
    x0 = {1: 4, 2: 44, 3: 50, 4: -18}
    canvases, flows = [], []
    for t in range(T):
        canvas, flow = np.zeros((H, W), np.int32), np.zeros((H, W, 2), np.float32)
        for name in (2, 1, 4, 3):                                            # (1 is drawn over 2)
            a, b = x0[name] + speed[name] * t, x0[name] + speed[name] * t + 10
            a, b = max(a, 0), min(b, W)
            if a < b:
                canvas[rows[name][0]:rows[name][1], a:b] = name
                flow[rows[name][0]:rows[name][1], a:b, 0] = speed[name]
        canvases.append(canvas), flows.append(flow)
    return canvases, flows


def test_rectangles_keep_their_ids_through_a_crossing_and_a_newcomer_gets_a_new_one():
    from tf_raft_amd import image_ops
    from tf_raft_amd.image_ops import Objects
    dev = _dev()
    K, T = 8, 6
    canvases, flows = _scripted_clip(T)
    sides, slots = zip(*(_slots_by_area(c, K) for c in canvases))
    areas = [slot_areas(l[None], K) for l in sides]
    ids = torch.full((1, K), -1, dtype=torch.int32, device=dev)
    born = ids.clone()
    next_id = torch.zeros((1,), dtype=torch.int32, device=dev)
    host = (np.full((1, K), -1, np.int32), np.full((1, K), -1, np.int32), np.zeros((1,), np.int32))
    seen = {}
    for t in range(T):
        count = torch.tensor([[len(slots[t])]], dtype=torch.int32, device=dev)
        if t == 0:
            match = torch.full((1, 1, K), -1, dtype=torch.int32, device=dev)
        else:
            prev = Objects(sides[t - 1][None], None, areas[t - 1], None, None, None)
            nxt = Objects(sides[t][None], None, areas[t], None, None, None)
            res = image_ops.match_objects(prev, flows[t - 1][None], nxt)
            o, l = np_object_overlap(sides[t - 1][None], flows[t - 1][None], sides[t][None], K)
            for g, w in zip(res, np_match_objects(o, l, areas[t], 0.25)):
                np.testing.assert_array_equal(_np(g), w)
            match = res.match[None]
        image_ops.chain_object_ids_launch(match, count, t, ids, born, next_id, out=(ids[None], born[None]))       # in place
        host = tuple(x[0] if x.ndim == 3 else x for x in np_chain_ids(_np(match), _np(count), t, *host))
        np.testing.assert_array_equal(_np(ids), host[0]), np.testing.assert_array_equal(_np(born), host[1])
        now = _np(ids)[0]
        for name, slot in slots[t].items():
            seen.setdefault(name, []).append(int(now[slot]))
    assert seen[1] == [0] * T and seen[2] == [1] * T                          # both keep their ids through the crossing
    assert seen[3] == [2, 2, 2]                                               # leaves after frame 2
    assert seen[4] == [3, 3, 3, 3]                                            # enters at frame 2 under a new id
    assert _np(next_id).tolist() == [4] and _np(born)[0, slots[T - 1][4]] == 2
    assert any(slots[t][1] != slots[0][1] or slots[t][2] != slots[0][2] for t in range(T))       # the slots did change hands


# ------------------------------------------------------------------ the model
# Random weights predict much the same flow whichever way round the frames come, so under UnFlow's alpha nearly every pixel fails the
# forward-backward test (tests/test_gpu_components.py says the same of its model test).  alpha = 1.9 is an input of the test, not a
# tuned value of the project.
ALPHA = 1.9
STEP = dict(alpha=ALPHA, min_area=12, connectivity=8)
_MODELS = {}


def _model(kind):
    if kind not in _MODELS:
        import tf_raft_amd
        from tf_raft_amd import weights as wm
        _MODELS[kind] = (tf_raft_amd.SmallRAFT(weights=wm.init_weights('small', seed=6, perturb=True), iters_pred=3) if kind == 'small' else
                         tf_raft_amd.RAFT(weights=wm.init_weights('raft', seed=6, perturb=True), iters_pred=2))
    return _MODELS[kind]


def _clip(T, H=64, W=96, seed=91):
    """A texture that drifts by a pixel per frame with two patches that move against it, plus noise."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0, 255, (H + 16, W + 16, 3))
    video = np.stack([base[8:8 + H, 8 - t:8 - t + W] for t in range(T)])
    one, two = rng.uniform(0, 255, (20, 20, 3)), rng.uniform(0, 255, (14, 24, 3))
    for t in range(T):
        video[t, 8 + 2 * t:28 + 2 * t, 10 + 3 * t:30 + 3 * t] = one
        video[t, 44 - t:58 - t, 60 - 3 * t:84 - 3 * t] = two
    return (video + rng.normal(0, 4, video.shape)).clip(0, 255).astype(np.float32)


def _host_chain(pairs, K, share):
    """ids, born, match, origin per pair from the label maps, flows, areas and counts of consecutive ``moving_objects_step``
    results, by the restatement: lists over the pairs of (N, K) arrays."""
    out = []
    N = pairs[0]['labels'].shape[0]
    state = (np.full((N, K), -1, np.int32), np.full((N, K), -1, np.int32), np.zeros((N,), np.int32))
    for t, p in enumerate(pairs):
        if t == 0:
            match = origin = np.full((N, K), -1, np.int32)
        else:
            q = pairs[t - 1]
            o, l = np_object_overlap(q['labels'], q['forward'], p['labels'], K)
            match, _, origin = np_match_objects(o, l, p['area'], share)
        ids, born, nxt = np_chain_ids(match[None], p['count'][None], t, *state)
        state = (ids[0], born[0], nxt)
        out.append(dict(ids=ids[0], born=born[0], match=match, origin=origin))
    return out


@pytest.mark.parametrize('kind', ('small', 'raft'))
def test_the_tracker_is_moving_objects_step_plus_the_restatement_chained_on_the_host(kind):
    from tf_raft_amd.video import ObjectTracker, TrackedObjects
    model = _model(kind)
    K, T = 16, 4
    clips = np.stack([_clip(T, seed=91), _clip(T, seed=92)], axis=1)          # (T, N = 2, H, W, 3)
    tracker = model.object_tracker(max_objects=K, **STEP)
    assert isinstance(tracker, ObjectTracker)
    assert tracker.push(clips[0]) is None
    got = [tracker.push(clips[t]) for t in range(1, T)]
    pairs = []
    for t, res in enumerate(got):
        assert isinstance(res, TrackedObjects) and all(x.is_cuda for x in res)
        step = model.moving_objects_step((clips[t], clips[t + 1]), max_objects=K, **STEP)
        for a, b, name in zip(res[:12], step, step._fields):
            assert _np(a).tobytes() == _np(b).tobytes(), name
        pairs.append({k: _np(getattr(res, k)) for k in ('labels', 'forward', 'area', 'count')})
    want = _host_chain(pairs, K, 0.25)
    matched = fresh = 0
    for t, (res, w) in enumerate(zip(got, want)):
        for name in ('ids', 'born', 'match', 'origin'):
            np.testing.assert_array_equal(_np(getattr(res, name)), w[name], f'{name} of pair {t}')
        matched += int((w['match'] >= 0).sum())
        fresh += int((w['born'] == t).sum())
    report(f'object tracker {kind}', count=[p['count'].tolist() for p in pairs], matched=matched, new=fresh,
           next_id=_np(tracker._next_id).tolist())
    assert all(p['count'].min() >= 1 for p in pairs)                          # not vacuous: every pair of every video holds an object
    np.testing.assert_array_equal(_np(got[0].ids)[0, :pairs[0]['count'][0]], np.arange(pairs[0]['count'][0]))
    with pytest.raises(ValueError, match='reset'):
        tracker.push(clips[0][:, :32])
    with pytest.raises(ValueError, match='reset'):
        tracker.push(clips[0].astype(np.uint8))
    tracker.reset()
    assert tracker.ids is None and tracker.push(clips[1]) is None             # the stream starts again, from another frame
    again = tracker.push(clips[2])
    assert _np(again.labels).tobytes() == _np(got[1].labels).tobytes()
    assert (_np(again.match) == -1).all() and (_np(again.born).max(axis=1) == 0).all()
    np.testing.assert_array_equal(_np(again.ids)[1, :pairs[1]['count'][1]], np.arange(pairs[1]['count'][1]))


def test_track_objects_video_does_not_depend_on_the_batch_size():
    """``track_objects_video`` with ``batch_size`` 1, 2 and 4: identical arrays, every field.  The predictor's flow for a pair differs
    in its last bits with the batch it runs in (measured at 64 x 96: one pair alone against the same pair among four, up to 7.6e-6 px
    with SmallRAFT and 4.8e-6 px with RAFT, and ``mean_flow`` with it by up to 6.6e-5 px), which is why every pair is predicted in a
    call of its own and ``batch_size`` only cuts the uploads and the identity launches."""
    model = _model('small')
    K, T = 16, 6
    clip = _clip(T, seed=93)
    runs = [model.track_objects_video(clip, batch_size=bs, max_objects=K, return_labels=True, **STEP) for bs in (1, 2, 4)]
    for bs, other in zip((2, 4), runs[1:]):
        report(f'track_objects_video batch_size 1 against {bs}',
               **{name: float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) for a, b, name in zip(runs[0], other, runs[0]._fields)})
    for other in runs[1:]:
        for a, b, name in zip(runs[0], other, runs[0]._fields):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name


def test_track_objects_video_at_one_pair_per_call_is_the_tracker():
    model = _model('small')
    K, T = 16, 6
    clip = _clip(T, seed=93)
    first = model.track_objects_video(clip, batch_size=1, max_objects=K, return_labels=True, **STEP)
    assert first.count.shape == (T - 1,) and first.ids.shape == (T - 1, K) and first.boxes.shape == (T - 1, K, 4)
    assert first.labels.shape == (T - 1, 64, 96) and first.labels.dtype == np.int32 and first.centroid.dtype == np.float32
    assert model.track_objects_video(clip[:3], batch_size=4, max_objects=K, **STEP).labels is None
    tracker = model.object_tracker(max_objects=K, **STEP)
    tracker.push(clip[0][None])
    for t in range(1, T):
        res = tracker.push(clip[t][None])
        for name in ('count', 'ids', 'born', 'area', 'boxes', 'centroid', 'mean_flow', 'labels'):
            assert _np(getattr(res, name))[0].tobytes() == getattr(first, name)[t - 1].tobytes(), (name, t)
    report('track_objects_video', count=first.count.tolist(), ids=[r[:c].tolist() for r, c in zip(first.ids, first.count)])
    assert first.count.min() >= 1


class _ScriptedPredictor:
    """Stands in for the model under ``track_objects_video``: frame t of the video holds the value t, and the "step" of the pairs
    (t, t + 1) returns the scripted label maps and exact flows of ``_scripted_clip``."""

    def __init__(self, K, T, dev):
        canvases, flows = _scripted_clip(T)
        sides, self.slots = zip(*(_slots_by_area(c, K) for c in canvases))
        self.labels, self.flows = _to(np.stack(sides), dev), _to(np.stack(flows), dev)
        self.area = _to(np.concatenate([slot_areas(l[None], K) for l in sides]), dev)
        self.count = _to(np.array([len(s) for s in self.slots], np.int32), dev)
        rng = np.random.default_rng(340)                                      # (carried through untouched: any values will do)
        self.boxes = _to(rng.integers(0, 64, (T, K, 4)).astype(np.int32), dev)
        self.centroid, self.mean_flow = (_to(rng.uniform(-9, 9, (T, K, 2)).astype(np.float32), dev) for _ in range(2))
        self.calls = []

    def moving_objects_step(self, data, max_objects, **options):
        from tf_raft_amd.model import MovingObjects
        t = data[0][:, 0, 0, 0].to(torch.int64)
        assert (data[1][:, 0, 0, 0].to(torch.int64) == t + 1).all()
        self.calls.append(len(t))
        pick = lambda x: x[t].contiguous()       # noqa: E731
        return MovingObjects(None, None, None, None, pick(self.flows), None, pick(self.labels), pick(self.count), pick(self.area),
                             pick(self.boxes), pick(self.centroid), pick(self.mean_flow))


def test_the_chunks_of_track_objects_video_with_the_model_taken_out():
    from tf_raft_amd.video import track_objects_video
    dev = _dev()
    K, P = 8, 6                                                               # 6 pairs: chunks of 1+1+1+1+1+1, 2+2+2, 4+2 and 6
    video = np.broadcast_to(np.arange(P + 1, dtype=np.uint8)[:, None, None, None], (P + 1, 32, 64, 3)).copy()
    runs = {}
    for bs in (1, 2, 4, 8):
        stub = _ScriptedPredictor(K, P, dev)
        runs[bs] = track_objects_video(stub, video, batch_size=bs, max_objects=K, return_labels=True)
        assert stub.calls == [1] * P                                          # every pair in a call of its own, whatever the chunks
    first = runs[1]
    for bs in (2, 4, 8):
        for a, b, name in zip(first, runs[bs], first._fields):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (bs, name)
    stub = _ScriptedPredictor(K, P, dev)
    np.testing.assert_array_equal(first.labels, _np(stub.labels))
    np.testing.assert_array_equal(first.count, _np(stub.count))
    seen = {}
    for t in range(P):
        for name, slot in stub.slots[t].items():
            seen.setdefault(name, []).append((int(first.ids[t, slot]), int(first.born[t, slot])))
        assert (first.ids[t, first.count[t]:] == -1).all()
    assert seen[1] == [(0, 0)] * P and seen[2] == [(1, 0)] * P                # through the crossing
    assert seen[3] == [(2, 0)] * 3 and seen[4] == [(3, 2)] * 4                # one leaves, one enters under a new id
    # the restatement chained on the host says the same
    pairs = [dict(labels=_np(stub.labels)[t:t + 1], forward=_np(stub.flows)[t:t + 1], area=_np(stub.area)[t:t + 1],
                  count=_np(stub.count)[t:t + 1]) for t in range(P)]
    for t, w in enumerate(_host_chain(pairs, K, 0.25)):
        np.testing.assert_array_equal(first.ids[t], w['ids'][0]), np.testing.assert_array_equal(first.born[t], w['born'][0])



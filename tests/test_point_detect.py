"""Corner detection and re-seeding, host side (no GPU): the float32 NumPy restatements ``np_corner_score``, ``np_detect_points``
and ``np_refill`` of DESIGN.md section 29 in the operation order of include/raft_hip.h, their known answers, the fixed cases
tests/test_gpu_point_detect.py runs and the conditions those cases must meet (so that no GPU test is vacuous), the C entries'
declarations and argument checks, and the errors of the Python layer.  The GPU file compares the kernels with the restatements
BIT FOR BIT: contraction is off in csrc/point_detect.hip, every product and sum here is one float32 operation in the kernel's
order, the square root is correctly rounded on both sides, and everything behind the score works on its bits.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tf_raft_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F2, F4 = np.float32(2), np.float32(4)
EMPTY = 3                                # the code of a slot that never held a point


# ------------------------------------------------------------------ the restatements
def np_gray(frames):
    f = np.asarray(frames)
    assert f.dtype in (np.uint8, np.float32) and f.ndim == 4 and f.shape[-1] in (1, 3)
    f = f.astype(np.float32)
    if f.shape[-1] == 1:
        return f[..., 0]
    with np.errstate(invalid='ignore', over='ignore'):
        g = (np.float32(0.299) * f[..., 0] + np.float32(0.587) * f[..., 1]) + np.float32(0.114) * f[..., 2]
    assert g.dtype == np.float32
    return g


def _window_sum(p, r):
    """Sums over the (2r + 1)^2 window of (N, H, W): each window row left to right, then the rows' sums top to bottom.  Zeros
    stand outside the frame (they reach only pixels that the border zeroes)."""
    N, H, W = p.shape
    q = np.pad(p, ((0, 0), (r, r), (r, r)))
    with np.errstate(invalid='ignore', over='ignore'):
        h = q[:, :, 0:W]
        for j in range(1, 2 * r + 1):
            h = h + q[:, :, j:j + W]
        s = h[:, 0:H]
        for j in range(1, 2 * r + 1):
            s = s + h[:, j:j + H]
    assert s.dtype == np.float32 and s.shape == (N, H, W)
    return s


def np_corner_score(frames, block_radius=1, method='min_eig', harris_k=0.04, border=8):
    """frames (N, H, W, C) uint8 / float32 -> (score (N, H, W) float32, smax (N,) float32)."""
    g = np_gray(frames)
    N, H, W = g.shape
    assert border >= block_radius + 1 and H > 2 * border and W > 2 * border
    p = np.pad(g, ((0, 0), (1, 1), (1, 1)))
    tl, tm, tr = p[:, :-2, :-2], p[:, :-2, 1:-1], p[:, :-2, 2:]
    ml, mr = p[:, 1:-1, :-2], p[:, 1:-1, 2:]
    bl, bm, br = p[:, 2:, :-2], p[:, 2:, 1:-1], p[:, 2:, 2:]
    with np.errstate(invalid='ignore', over='ignore'):
        gx = ((tr - tl) + F2 * (mr - ml)) + (br - bl)
        gy = ((bl - tl) + F2 * (bm - tm)) + (br - tr)
        a, b, c = _window_sum(gx * gx, block_radius), _window_sum(gx * gy, block_radius), _window_sum(gy * gy, block_radius)
        if method == 'min_eig':
            d = a - c
            s = ((a + c) - np.sqrt(d * d + F4 * (b * b))) / F2
        else:
            assert method == 'harris'
            t = a + c
            s = (a * c - b * b) - np.float32(harris_k) * (t * t)
        score = np.where(s > 0, s, np.float32(0)).astype(np.float32)
    assert s.dtype == np.float32
    inner = np.zeros((H, W), bool)
    inner[border:H - border, border:W - border] = True
    score = np.where(inner[None], score, np.float32(0))
    smax = score.reshape(N, -1).view(np.uint32).max(axis=1).view(np.float32)
    return np.ascontiguousarray(score), smax


def np_keys(score):
    """(N, H, W) float32 scores -> uint64 keys: score bits << 32 | 0xFFFFFFFF - raster index."""
    N, H, W = score.shape
    idx = np.arange(H * W, dtype=np.uint64).reshape(1, H, W)
    return (np.ascontiguousarray(score).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx)


def np_local_maxima(key, m):
    """A pixel is a local maximum iff its key is the largest of its (2m + 1)^2 window clipped to the frame."""
    N, H, W = key.shape
    q = np.pad(key, ((0, 0), (m, m), (m, m)))
    h = q[:, :, 0:W]
    for j in range(1, 2 * m + 1):
        h = np.maximum(h, q[:, :, j:j + W])
    v = h[:, 0:H]
    for j in range(1, 2 * m + 1):
        v = np.maximum(v, h[:, j:j + H])
    return v == key


def np_occupancy(avoid, N, H, W, m):
    occ = np.zeros((N, H, W), bool)
    if avoid is None:
        return occ
    pts, lost = np.asarray(avoid[0]), np.asarray(avoid[1])
    assert pts.dtype == np.float32 and pts.shape[0] == N and pts.shape[2] == 2 and lost.shape == pts.shape[:2]
    fm = np.float32(m)
    for n in range(N):
        for (px, py), code in zip(pts[n], lost[n]):
            if code != 0 or not (px >= 0 and px <= np.float32(W - 1) and py >= 0 and py <= np.float32(H - 1)):
                continue
            xa, xb = int(np.ceil(px - fm)), int(np.floor(px + fm))
            ya, yb = int(np.ceil(py - fm)), int(np.floor(py + fm))
            occ[n, max(ya, 0):min(yb, H - 1) + 1, max(xa, 0):min(xb, W - 1) + 1] = True
    return occ


def np_detect_points(frames, max_points, min_distance=7, quality_level=0.01, block_radius=1, method='min_eig', harris_k=0.04, border=8,
                     mask=None, avoid=None, want_candidates=False):
    """-> (points (N, K, 2) float32, scores (N, K) float32, count (N,) int32, lost (N, K) uint8); ``want_candidates``: also the
    number of candidates per image, before the cut at K."""
    score, smax = np_corner_score(frames, block_radius, method, harris_k, border)
    N, H, W = score.shape
    K, m = int(max_points), int(min_distance)
    key = np_keys(score)
    thr = np.float32(quality_level) * smax
    assert thr.dtype == np.float32
    cand = np_local_maxima(key, m) & (score > 0) & (score >= thr[:, None, None])
    if mask is not None:
        cand &= np.asarray(mask).reshape(N, H, W) != 0
    cand &= ~np_occupancy(avoid, N, H, W, m)
    points = np.full((N, K, 2), -1, np.float32)
    scores = np.zeros((N, K), np.float32)
    count = np.zeros(N, np.int32)
    lost = np.full((N, K), EMPTY, np.uint8)
    for n in range(N):
        best = np.sort(key[n][cand[n]])[::-1][:K]
        k = len(best)
        idx = (np.uint64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF))).astype(np.int64)
        points[n, :k, 0], points[n, :k, 1] = idx % W, idx // W
        scores[n, :k] = (best >> np.uint64(32)).astype(np.uint32).view(np.float32)
        count[n], lost[n, :k] = k, 0
    out = (points, scores, count, lost)
    return out + (cand.reshape(N, -1).sum(axis=1),) if want_candidates else out


def np_refill(pos, lost, new_points, new_count, t, born, ids, next_id):
    """A tracker's state and a detection -> (pos, lost, born, ids, next_id) after the refill; nothing is changed in place."""
    pos, lost, born, ids, next_id = (np.array(a) for a in (pos, lost, born, ids, next_id))
    N, P = lost.shape
    K = new_points.shape[1]
    for n in range(N):
        slots = np.nonzero(lost[n] != 0)[0]
        k = min(len(slots), int(np.clip(new_count[n], 0, K)))
        slots = slots[:k]
        pos[n, slots], lost[n, slots], born[n, slots] = new_points[n, :k], 0, t
        ids[n, slots] = next_id[n] + np.arange(k, dtype=np.int32)
        next_id[n] += k
    return pos, lost, born, ids, next_id


def bits(x):
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32
    return x.view(np.uint32)


def assert_same_detection(got, want):
    """points and scores as uint32, count and codes as they are: no tolerance and nothing left out."""
    np.testing.assert_array_equal(bits(got[0]), bits(want[0]))
    np.testing.assert_array_equal(bits(got[1]), bits(want[1]))
    assert np.asarray(got[2]).dtype == np.int32
    np.testing.assert_array_equal(got[2], want[2])
    if len(want) > 3 and len(got) > 3:
        assert np.asarray(got[3]).dtype == np.uint8
        np.testing.assert_array_equal(got[3], want[3])


# ------------------------------------------------------------------ the inputs both test files use
def _box(a, k):
    for axis in (1, 2):
        pad = [(0, 0)] * a.ndim
        pad[axis] = (k // 2, k - 1 - k // 2)
        p = np.pad(a, pad, mode='edge')
        a = sum(np.take(p, range(j, j + a.shape[axis]), axis=axis) for j in range(k)) / k
    return a


def make_frames(shape, channels, dtype, pattern, seed=1):
    """(N, H, W, C) test frames.  'noise': white noise filtered over 3 taps, full contrast; image 1 of a batch of three is
    CONSTANT and image 2 has a tenth of the contrast.  'periodic': a tile of 32 x 32 pixels repeated exactly, so that the same
    corner appears several times with the same bits.  'special': noise with a NaN, an Inf and a -Inf inside (float32 only)."""
    N, H, W = shape
    rng = np.random.default_rng([seed, N, H, W, channels])
    if pattern == 'periodic':
        tile = np.zeros((32, 32, channels))
        tile[6:17, 5:19] = rng.uniform(120, 255, channels)
        tile[20:29, 22:30] = rng.uniform(60, 200, channels)
        f = np.tile(tile, (N, (H + 31) // 32, (W + 31) // 32, 1))[:, :H, :W]
    else:
        f = _box(rng.uniform(0, 1, (N, H, W, channels)), 3)
        f = (f - f.min()) / (f.max() - f.min()) * 255
        if N == 3:
            f[1] = 93
            f[2] = 100 + (f[2] - 100) * 0.1
    if dtype == np.uint8:
        return np.ascontiguousarray(np.rint(f).clip(0, 255).astype(np.uint8))
    f = np.ascontiguousarray(f.astype(np.float32))
    if pattern == 'special':
        f[0, H // 2, W // 2, 0] = np.nan
        f[0, H // 3, W // 3, -1] = np.inf
        f[0, 2 * H // 3, W // 4, 0] = -np.inf
        f[0, 1, 1, 0] = np.nan                   # in the border: its window never counts
    return f


# id: (shape, C, dtype, pattern, K, min_distance, quality_level, block_radius, method, border)
CASES = {
    'narrow_u8_c1':     ((1, 20, 23), 1, np.uint8, 'noise', 3, 1, 0.01, 1, 'min_eig', 8),
    'batch_f32_c3':     ((3, 37, 70), 3, np.float32, 'noise', 64, 7, 0.01, 1, 'harris', 8),
    'batch_u8_c3_r3':   ((3, 37, 70), 3, np.uint8, 'noise', 5, 7, 0.05, 3, 'min_eig', 8),
    'periodic_u8_c3':   ((2, 64, 129), 3, np.uint8, 'periodic', 16, 15, 0.01, 3, 'min_eig', 8),
    'periodic_f32_c1':  ((2, 64, 129), 1, np.float32, 'periodic', 40, 7, 0.0, 1, 'harris', 4),
    'tile_edge_u8_c1':  ((2, 64, 129), 1, np.uint8, 'noise', 100, 1, 0.01, 1, 'min_eig', 2),
    'tall_f32_c1':      ((1, 130, 67), 1, np.float32, 'noise', 4096, 1, 0.0, 1, 'min_eig', 8),
    'tall_u8_c3':       ((1, 130, 67), 3, np.uint8, 'noise', 50, 1, 0.3, 1, 'harris', 8),
    'many_u8_c1':       ((1, 200, 150), 1, np.uint8, 'noise', 1500, 1, 0.0, 1, 'min_eig', 2),
    'special_f32_c1':   ((1, 37, 70), 1, np.float32, 'special', 32, 2, 0.001, 1, 'min_eig', 8),
    'special_f32_c3':   ((1, 37, 70), 3, np.float32, 'special', 32, 7, 0.001, 3, 'harris', 8),
}
IDS = list(CASES)


def case_args(name):
    shape, channels, dtype, pattern, K, m, q, r, method, border = CASES[name]
    frames = make_frames(shape, channels, dtype, pattern)
    frames.setflags(write=False)
    return frames, dict(max_points=K, min_distance=m, quality_level=q, block_radius=r, method=method, border=border)


def case_mask_avoid(name):
    """A mask that forbids a band of the frame and an ``avoid`` built around the case's own detection: the strongest point of every
    image as a live point, the second as a LOST one (it bars nothing), and a NaN and an out-of-frame live point."""
    frames, kw = case_args(name)
    N, H, W = frames.shape[:3]
    pts, _, count, _ = np_detect_points(frames, **kw)
    mask = np.ones((N, H, W), np.uint8)
    mask[:, :, W // 2:W // 2 + 9] = 0
    avoid = np.zeros((N, 5, 2), np.float32)
    lost = np.zeros((N, 5), np.uint8)
    for n in range(N):
        avoid[n, 0] = pts[n, 0] + np.float32(0.4) if count[n] > 0 else (3, 3)
        avoid[n, 1] = pts[n, 1] if count[n] > 1 else (5, 5)
        lost[n, 1] = 2
        avoid[n, 2] = (np.nan, 4)
        avoid[n, 3] = (W + 3, H // 2)
        avoid[n, 4] = (-0.5, H // 2)
    return frames, kw, mask, avoid, lost


def refill_case(N, P, K, seed=3):
    """A tracker's state with every code in it, a detection with a different count per video (0, more than the lost slots, fewer
    than them), and the ids so far."""
    rng = np.random.default_rng([seed, N, P, K])
    pos = rng.uniform(0, 100, (N, P, 2)).astype(np.float32)
    lost = rng.choice(np.array([0, 0, 1, 2, 3, 7], np.uint8), size=(N, P))
    lost[-1] = rng.choice(np.array([0, 0, 0, 0, 0, 0, 0, 1], np.uint8), size=P)          # few lost slots: more new points than them
    new_points = rng.integers(0, 100, (N, K, 2)).astype(np.float32)
    new_count = rng.integers(0, K + 1, N).astype(np.int32)
    new_count[0], new_count[-1] = 0 if N > 1 else K // 2, K
    if N > 2:
        new_count[1] = min(K, max(1, int((lost[1] != 0).sum()) // 2))                           # fewer new points than lost slots
    born = rng.integers(0, 5, (N, P)).astype(np.int32)
    ids = np.broadcast_to(np.arange(P, dtype=np.int32), (N, P)).copy()
    ids[lost == 3], born[lost == 3] = -1, -1
    next_id = np.full(N, P, np.int32) + rng.integers(0, 50, N).astype(np.int32)
    return pos, lost, new_points, new_count, born, ids, next_id


REFILL_SHAPES = [(1, 1, 1), (3, 7, 4), (3, 300, 64), (2, 1000, 4096), (4, 257, 256)]


# ------------------------------------------------------------------ known answers
def test_a_bright_rectangle_gives_its_four_corners():
    img = np.full((1, 60, 80, 1), 10, np.uint8)
    img[0, 20:41, 25:61] = 200
    corners = {(25, 20), (60, 20), (25, 40), (60, 40)}
    for r in (1, 2, 3):
        for method in ('min_eig', 'harris'):
            pts, scores, count, lost = np_detect_points(img, 8, block_radius=r, method=method)
            assert count[0] >= 4 and (lost[0, :count[0]] == 0).all() and (lost[0, count[0]:] == EMPTY).all()
            found = set()
            for x, y in pts[0, :4]:
                near = [c for c in corners if max(abs(c[0] - x), abs(c[1] - y)) <= r]
                assert len(near) == 1, (r, method, x, y)
                found.add(near[0])
            assert found == corners
            assert (np.diff(scores[0, :count[0]]) <= 0).all()                           # strongest first
            assert (pts[0, count[0]:] == -1).all() and (scores[0, count[0]:] == 0).all()


def test_a_constant_image_and_a_straight_edge_have_no_corner():
    const = np.full((1, 40, 50, 3), 77, np.uint8)
    for method in ('min_eig', 'harris'):
        pts, scores, count, lost = np_detect_points(const, 16, method=method)
        assert count[0] == 0 and (pts == -1).all() and (scores == 0).all() and (lost == EMPTY).all()
    edge = np.zeros((1, 40, 50, 1), np.float32)
    edge[0, :, 25:] = 180
    score, smax = np_corner_score(edge, method='min_eig')
    assert not score.any() and smax[0] == 0
    assert np_detect_points(edge, 16)[2][0] == 0
    edge_h = np.ascontiguousarray(edge.transpose(0, 2, 1, 3))
    assert np_detect_points(edge_h, 16, block_radius=3)[2][0] == 0


def test_the_score_follows_the_written_order():
    """One pixel computed by hand, scalar by scalar, in the header's order."""
    rng = np.random.default_rng(5)
    img = rng.uniform(0, 255, (1, 12, 13, 3)).astype(np.float32)
    g = np_gray(img)[0]
    assert g[3, 4] == (np.float32(0.299) * img[0, 3, 4, 0] + np.float32(0.587) * img[0, 3, 4, 1]) + np.float32(0.114) * img[0, 3, 4, 2]
    r, y, x = 2, 6, 5

    def grad(v, u):
        gx = ((g[v - 1, u + 1] - g[v - 1, u - 1]) + F2 * (g[v, u + 1] - g[v, u - 1])) + (g[v + 1, u + 1] - g[v + 1, u - 1])
        gy = ((g[v + 1, u - 1] - g[v - 1, u - 1]) + F2 * (g[v + 1, u] - g[v - 1, u])) + (g[v + 1, u + 1] - g[v - 1, u + 1])
        return gx, gy

    sums = []
    for pick in (lambda gx, gy: gx * gx, lambda gx, gy: gx * gy, lambda gx, gy: gy * gy):
        rows = []
        for v in range(y - r, y + r + 1):
            s = pick(*grad(v, x - r))
            for u in range(x - r + 1, x + r + 1):
                s = s + pick(*grad(v, u))
            rows.append(s)
        tot = rows[0]
        for s in rows[1:]:
            tot = tot + s
        assert tot.dtype == np.float32
        sums.append(tot)
    a, b, c = sums
    d = a - c
    want = ((a + c) - np.sqrt(d * d + F4 * (b * b))) / F2
    score, _ = np_corner_score(img, block_radius=r, border=3)
    assert bits(score[0, y, x]) == bits(np.float32(max(want, 0)))
    t = a + c
    want = (a * c - b * b) - np.float32(0.04) * (t * t)
    score, _ = np_corner_score(img, block_radius=r, method='harris', border=3)
    assert bits(score[0, y, x]) == bits(np.float32(max(want, 0)))
    assert not score[0, :3].any() and not score[0, :, -3:].any() and score[0, 3:-3, 3:-3].any()


def test_suppression_ties_and_what_applies_after_it():
    frames, kw = case_args('periodic_u8_c3')
    score, _ = np_corner_score(frames, kw['block_radius'], kw['method'], 0.04, kw['border'])
    m = kw['min_distance']
    peaks = np_local_maxima(np_keys(score), m) & (score > 0)
    ys, xs = np.nonzero(peaks[0])
    for i in range(len(ys)):                                                 # any two local maxima are more than m apart
        d = np.maximum(abs(ys - ys[i]), abs(xs - xs[i]))
        assert (d[np.arange(len(ys)) != i] > m).all()
    H, W = score.shape[1:]
    assert peaks.reshape(2, -1).sum(axis=1).max() <= -(-H // (m + 1)) * -(-W // (m + 1))
    # of two equal scores in one window the earlier pixel wins; its later twin is suppressed and nothing moves up
    flat = np.zeros((1, 30, 30), np.float32)
    flat[0, 10, 10] = flat[0, 10, 13] = flat[0, 12, 9] = 5
    flat[0, 20, 20] = 4
    got = np_local_maxima(np_keys(flat), 3) & (flat > 0)
    assert sorted(zip(*np.nonzero(got[0]))) == [(10, 10), (20, 20)]
    # a mask or a live point of avoid that bars a maximum does not promote its neighbours
    frames, kw, mask, avoid, lost = case_mask_avoid('batch_f32_c3')
    base = np_detect_points(frames, **kw)
    barred = np_detect_points(frames, mask=mask, avoid=(avoid, lost), **kw)
    for n in range(frames.shape[0]):
        before = {tuple(p) for p in base[0][n, :base[2][n]]}
        after = {tuple(p) for p in barred[0][n, :barred[2][n]]}
        assert after <= before


def test_np_refill_fills_lost_slots_in_order():
    pos = np.arange(12, dtype=np.float32).reshape(1, 6, 2)
    lost = np.array([[0, 2, 0, 3, 1, 0]], np.uint8)
    new = np.array([[(50, 51), (60, 61), (70, 71), (80, 81)]], np.float32)
    born, ids = np.array([[0, 0, 0, -1, 0, 0]], np.int32), np.array([[0, 1, 2, -1, 4, 5]], np.int32)
    p, l, b, i, nxt = np_refill(pos, lost, new, np.array([2], np.int32), 9, born, ids, np.array([6], np.int32))
    np.testing.assert_array_equal(l, [[0, 0, 0, 0, 1, 0]])
    np.testing.assert_array_equal(p[0, [1, 3]], new[0, :2])
    np.testing.assert_array_equal(p[0, [0, 2, 4, 5]], pos[0, [0, 2, 4, 5]])
    np.testing.assert_array_equal(b, [[0, 9, 0, 9, 0, 0]])
    np.testing.assert_array_equal(i, [[0, 6, 2, 7, 4, 5]])
    assert nxt[0] == 8
    p, l, b, i, nxt = np_refill(pos, lost, new, np.array([4], np.int32), 9, born, ids, np.array([6], np.int32))
    np.testing.assert_array_equal(l, [[0, 0, 0, 0, 0, 0]])
    np.testing.assert_array_equal(i, [[0, 6, 2, 7, 8, 5]])
    assert nxt[0] == 9                                                       # the fourth new point found no slot
    assert lost[0, 1] == 2 and ids[0, 1] == 1                                # (the inputs are untouched)


# ------------------------------------------------------------------ what the GPU cases rely on
def test_the_fixed_cases_meet_the_conditions_the_gpu_tests_rely_on():
    more, partial, empty_in_batch, ties, first_and_last_tile = [], [], [], [], []
    for name in IDS:
        frames, kw = case_args(name)
        pts, scores, count, lost, cands = np_detect_points(frames, want_candidates=True, **kw)
        K = kw['max_points']
        N, H, W = frames.shape[:3]
        for n in range(N):
            if cands[n] > K:
                more.append(name)
            if 0 < count[n] < K:
                partial.append(name)
            sel = bits(scores[n, :count[n]])
            if len(sel) - len(np.unique(sel)) >= 1:
                ties.append(name)
            if count[n] and pts[n, :count[n], 0].max() >= 64 and pts[n, :count[n], 0].min() < 32:
                first_and_last_tile.append(name)
        if (count == 0).any() and (count > 0).any():
            empty_in_batch.append(name)
    assert len(set(more)) >= 3 and 'tile_edge_u8_c1' in more and 'tall_u8_c3' in more, more
    assert len(set(partial)) >= 3 and 'tall_f32_c1' in partial, partial
    assert {'batch_f32_c3', 'batch_u8_c3_r3'} <= set(empty_in_batch), empty_in_batch
    assert {'periodic_u8_c3', 'periodic_f32_c1'} <= set(ties), ties
    assert first_and_last_tile
    # more candidates than one pass of the selecting workgroup reads, and more than K: the radix select runs and strides
    frames, kw = case_args('many_u8_c1')
    assert np_detect_points(frames, want_candidates=True, **kw)[4].max() > kw['max_points'] > 1024
    # the special values reach scored windows and leave finite scores around them
    for name in ('special_f32_c1', 'special_f32_c3'):
        frames, kw = case_args(name)
        assert np.isnan(frames).sum() >= 2 and np.isinf(frames).sum() == 2
        score, smax = np_corner_score(frames, kw['block_radius'], kw['method'], 0.04, kw['border'])
        assert np.isfinite(score).all() and smax[0] > 0
        H, W = score.shape[1:]
        assert score[0, H // 2, W // 2] == 0 and np_detect_points(frames, **kw)[2][0] > 0


@pytest.mark.parametrize('name', ['batch_f32_c3', 'periodic_u8_c3', 'tile_edge_u8_c1'])
def test_mask_and_avoid_remove_selected_points(name):
    frames, kw, mask, avoid, lost = case_mask_avoid(name)
    base = np_detect_points(frames, **kw)
    for m_, a_ in ((mask, None), (None, (avoid, lost)), (mask, (avoid, lost))):
        got = np_detect_points(frames, mask=m_, avoid=a_, **kw)
        removed = 0
        for n in range(frames.shape[0]):
            before = {tuple(p) for p in base[0][n, :base[2][n]]}
            after = {tuple(p) for p in got[0][n, :got[2][n]]}
            removed += len(before - after)
            if a_ is not None and base[2][n] > 1:
                assert tuple(base[0][n, 0]) not in after                     # the live point bars the strongest corner
                if m_ is None:
                    assert tuple(base[0][n, 1]) in after                     # the lost one bars nothing
        assert removed >= 1


@pytest.mark.parametrize('shape', REFILL_SHAPES, ids=['x'.join(map(str, s)) for s in REFILL_SHAPES])
def test_the_refill_cases_cover_both_shortages(shape):
    pos, lost, new_points, new_count, born, ids, next_id = refill_case(*shape)
    p, l, b, i, nxt = np_refill(pos, lost, new_points, new_count, 4, born, ids, next_id)
    n_lost = (lost != 0).sum(axis=1)
    filled = nxt - next_id
    np.testing.assert_array_equal(filled, np.minimum(n_lost, new_count))
    if shape[0] >= 3:
        assert (n_lost > new_count).any() and (n_lost < new_count).any()
    for n in range(shape[0]):
        fresh = i[n][(l[n] == 0) & (lost[n] != 0)]
        np.testing.assert_array_equal(fresh, next_id[n] + np.arange(filled[n]))           # ascending slot order, no id twice
        assert len(set(i[n][i[n] >= 0])) == (i[n] >= 0).sum()


# ------------------------------------------------------------------ the C entries
ENTRIES = ('raft_corner_score_f32', 'raft_corner_score_u8_f32', 'raft_detect_points_workspace_bytes', 'raft_detect_points',
           'raft_refill_points')


def test_the_header_declares_and_the_library_exports_the_entries():
    from tf_raft_amd import build, image_ops
    assert 'point_detect.hip' in build.SOURCES
    with open(os.path.join(ROOT, 'include', 'raft_hip.h')) as f:
        text = f.read()
    header = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    sigs = _ffi.header_signatures(text)
    P, I, F, L = C.c_void_p, C.c_int, C.c_float, C.c_int64
    score = (I, [P, P, P, I, I, I, I, I, I, F, I, P])
    assert sigs['raft_corner_score_f32'] == score and sigs['raft_corner_score_u8_f32'] == score
    assert sigs['raft_detect_points_workspace_bytes'] == (L, [I, I, I, I])
    assert sigs['raft_detect_points'] == (I, [P, I, P, P, P, L, P, P, P, P, I, I, I, I, I, I, F, I, I, F, I, P, P])
    assert sigs['raft_refill_points'] == (I, [P, P, P, P, I, P, P, P, P, P, I, L, I, P])
    assert set(ENTRIES) <= set(_ffi.EXPORTED_SYMBOLS)
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, header)
    assert not re.search(r'raft_(detect|refill|corner)\w*\s*\([^)]*\bstruct\b', header)          # no struct crosses by value
    assert _ffi.ABI_VERSION == 222                                   # entries were added, no signature changed
    lib = _ffi.load_library()
    assert lib.raft_version() == 222
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == sigs[name][1] and getattr(lib, name).restype is sigs[name][0]
    consts = _ffi.header_constants(text)
    assert consts['RAFT_DETECT_MAX_POINTS'] == image_ops.DETECT_MAX_POINTS == 4096
    assert consts['RAFT_DETECT_MAX_MIN_DISTANCE'] == image_ops.DETECT_MAX_MIN_DISTANCE >= 15
    src = open(os.path.join(ROOT, 'tf_raft_amd', 'csrc', 'point_detect.hip')).read()
    assert '#pragma clang fp contract(off)' in src
    assert 'the sorted top-K of a set is the same bits' in src           # why the unordered gather is allowed, said at the top


def test_the_workspace_size():
    fn = _ffi.load_library().raft_detect_points_workspace_bytes
    for (N, H, W, m) in [(1, 20, 23, 1), (3, 37, 70, 7), (2, 64, 129, 15), (4, 1080, 1920, 7)]:
        bound = -(-H // (m + 1)) * -(-W // (m + 1))
        up8 = lambda v: (v + 7) // 8 * 8                                       # noqa: E731
        assert fn(N, H, W, m) == N * bound * 8 + up8(N * H * W * 4) + up8(N * 8) + up8(N * H * W)
    for bad in [(0, 20, 23, 1), (1, 0, 23, 1), (1, 20, -1, 1), (1, 20, 23, 0), (1, 20, 23, 16), (1, 1 << 16, 1 << 16, 1),
                (2, 1 << 15, 1 << 15, 7), (1 << 20, 1 << 6, 1 << 6, 7)]:
        assert fn(*bad) == 0, bad


def test_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off4, off1 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 1)
    nan, inf = float('nan'), float('inf')
    # ---- the score entries
    #       frames score smax N  H   W   C  r  method k     border stream
    good = [p, p, p, 2, 20, 23, 3, 1, 0, 0.04, 8, None]
    for fn in (lib.raft_corner_score_f32, lib.raft_corner_score_u8_f32):
        for k in (0, 1):
            args = list(good)
            args[k] = None
            assert fn(*args) == -1, k
        for k, values in {3: (0, -1), 4: (0, 16, -5), 5: (0, 16), 6: (0, 2, 4), 7: (0, 4, -1), 8: (-1, 2), 9: (nan, inf, -0.5),
                          10: (1, 0, -3, 10, 1 << 30)}.items():
            for v in values:
                args = list(good)
                args[k] = v
                assert fn(*args) == -2, (k, v)
        args = list(good)
        args[7], args[10] = 3, 3                                           # border < block_radius + 1
        assert fn(*args) == -2
        for bad in ((1, 1 << 16, 1 << 16), (2, 1 << 15, 1 << 15), (1 << 20, 1 << 6, 1 << 6)):
            args = list(good)
            args[3:6] = bad
            assert fn(*args) == -2, bad
        for k in (1, 2):
            args = list(good)
            args[k] = off1
            assert fn(*args) == -4, k
        args = list(good)
        args[1], args[6], args[2] = None, 2, off1                           # precedence: NULL before shape before alignment
        assert fn(*args) == -1
        args[1] = p
        assert fn(*args) == -2
    args = list(good)
    args[0] = off1
    assert lib.raft_corner_score_f32(*args) == -4                         # (bytes may lie at any address)
    # ---- the detection
    #       frames u8 mask avoid_p avoid_l P  points scores count lost N  H   W   C  K   m  q     r  method k     border ws stream
    good = [p, 1, p, p, p, 5, p, p, p, p, 2, 20, 23, 3, 16, 1, 0.01, 1, 0, 0.04, 8, p, None]
    fn = lib.raft_detect_points
    for k in (0, 6, 7, 8, 21):
        for opt in (p, None):                                                # (mask, avoid and lost may be NULL)
            args = list(good)
            args[k], args[2], args[3], args[4], args[9] = None, opt, opt, opt, opt
            assert fn(*args) == -1, k
    for k in (3, 4):                                                         # only one of the avoid pair
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    bad_values = {1: (2, -1), 5: (0, -1, 1 << 30), 10: (0, -1), 11: (0, 16), 12: (0, 16), 13: (0, 2, 4), 14: (0, -1, 4097),
                  15: (0, -1, 16), 16: (nan, -0.01, 1.0, inf), 17: (0, 4), 18: (2, -1), 19: (nan, inf, -1.0), 20: (1, 0, 10)}
    for k, values in bad_values.items():
        for v in values:
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    args = list(good)
    args[3], args[4], args[5] = None, None, 0                                # (avoid_P is not looked at without avoid)
    args[21] = off4
    assert fn(*args) == -4
    for k in (6, 7, 8, 3):
        args = list(good)
        args[k] = off1
        assert fn(*args) == -4, k
    args = list(good)
    args[0], args[1] = off1, 0                                               # float32 frames are read as floats
    assert fn(*args) == -4
    args = list(good)
    args[8], args[14], args[21] = None, 0, off4
    assert fn(*args) == -1
    args[8] = p
    assert fn(*args) == -2
    args[14], args[16] = 16, nan
    assert fn(*args) == -2
    # ---- the refill
    #       pos lost new count t  pos_out lost_out born ids next N  P  K  stream
    good = [p, p, p, p, 3, p, p, p, p, p, 2, 7, 4, None]
    fn = lib.raft_refill_points
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 9):
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    for k, values in {4: (-1,), 10: (0, -2), 11: (0, -1, 1 << 30, 1 << 40), 12: (0, 4097)}.items():
        for v in values:
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for k in (0, 2, 3, 5, 7, 8, 9):
        args = list(good)
        args[k] = off1
        assert fn(*args) == -4, k
    args = list(good)
    args[9], args[12], args[0] = None, 0, off1
    assert fn(*args) == -1
    args[9] = p
    assert fn(*args) == -2


# ------------------------------------------------------------------ the Python layer, nothing reaches the device
def test_detect_points_checks_its_arguments_without_a_gpu():
    import torch
    from tf_raft_amd import image_ops
    frames = np.zeros((2, 40, 50, 3), np.uint8)
    for fn in (lambda **kw: image_ops.detect_points(frames, 16, **kw), lambda **kw: image_ops.corner_score(frames, **kw)):
        for bad in (0, 4, -1, 1.0, True, None):
            with pytest.raises(ValueError, match='block_radius must'):
                fn(block_radius=bad)
        for bad in ('shi', None, 0):
            with pytest.raises(ValueError, match='method must'):
                fn(method=bad)
        for bad in (-0.1, float('nan'), float('inf'), True, None, 'x'):
            with pytest.raises(ValueError, match='harris_k must'):
                fn(harris_k=bad)
        for bad in (1, 0, -1, 2.0, True, None):
            with pytest.raises(ValueError, match='border must'):
                fn(border=bad)
        with pytest.raises(ValueError, match=r'border must be an integer >= block_radius \+ 1 = 4'):
            fn(block_radius=3, border=3)
        with pytest.raises(ValueError, match=r'greater than 2 \* border'):
            fn(border=20)
    for bad in (0, -1, 4097, 2.0, True, None):
        with pytest.raises(ValueError, match='max_points must'):
            image_ops.detect_points(frames, bad)
    for bad in (0, 16, -1, 1.5, True, None):
        with pytest.raises(ValueError, match='min_distance must'):
            image_ops.detect_points(frames, 16, min_distance=bad)
    for bad in (-0.01, 1.0, 2, float('nan'), True, None, 'x'):
        with pytest.raises(ValueError, match='quality_level must'):
            image_ops.detect_points(frames, 16, quality_level=bad)
    with pytest.raises(ValueError, match=r'\(N, H, W, C\)'):
        image_ops.detect_points(frames[0], 16)
    with pytest.raises(ValueError, match='1 or 3 channels'):
        image_ops.detect_points(np.zeros((2, 40, 50, 2), np.uint8), 16)
    with pytest.raises(ValueError, match='1 or 3 channels'):
        image_ops.corner_score(np.zeros((40, 50, 4), np.float32))
    with pytest.raises(TypeError):
        image_ops.detect_points(frames.astype(np.int32), 16)
    with pytest.raises(ValueError, match='empty'):
        image_ops.detect_points(frames[:0], 16)
    with pytest.raises(ValueError, match='expects a mask'):
        image_ops.detect_points(frames, 16, mask=np.ones((2, 40, 49), np.uint8))
    with pytest.raises(ValueError, match='expects a mask'):
        image_ops.detect_points(frames, 16, mask=np.ones((40, 50), np.uint8))
    with pytest.raises(TypeError, match='a mask is uint8 or bool'):
        image_ops.detect_points(frames, 16, mask=np.ones((2, 40, 50), np.float32))
    pts, lost = np.zeros((2, 5, 2), np.float32), np.zeros((2, 5), np.uint8)
    for bad in (pts, (pts,), (pts, None), 'x'):
        with pytest.raises(ValueError, match='avoid must be a pair'):
            image_ops.detect_points(frames, 16, avoid=bad)
    with pytest.raises(ValueError, match=r'points \(N, P, 2\)'):
        image_ops.detect_points(frames, 16, avoid=(pts[0], lost[0]))
    with pytest.raises(ValueError, match='expects lost'):
        image_ops.detect_points(frames, 16, avoid=(pts, lost[:, :4]))
    with pytest.raises(TypeError, match='points are float32'):
        image_ops.detect_points(frames, 16, avoid=(pts.astype(np.uint8), lost))
    with pytest.raises(ValueError, match='of 3 videos'):
        image_ops.detect_points(frames, 16, avoid=(np.zeros((3, 5, 2), np.float32), np.zeros((3, 5), np.uint8)))
    with pytest.raises(ValueError, match='too large'):
        image_ops.detect_points(torch.empty((1, 1 << 16, 1 << 15, 1), dtype=torch.uint8, device='meta'), 16)
    # the launch forms check what they are handed, too
    df = torch.zeros((2, 40, 50, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match='max_points must'):
        image_ops.detect_points_launch(df, 0)
    with pytest.raises(ValueError, match=r'contiguous frames \(N, H, W, C\)'):
        image_ops.detect_points_launch(df[0], 16)
    with pytest.raises(TypeError, match='uint8 or float32'):
        image_ops.detect_points_launch(df.to(torch.int32), 16)
    with pytest.raises(ValueError, match='out must be a contiguous'):
        image_ops.detect_points_launch(df, 16, mask=torch.ones((2, 40, 49), dtype=torch.uint8))
    with pytest.raises(ValueError, match='out must be a tuple'):
        image_ops.detect_points_launch(df, 16, out=(torch.zeros((2, 16, 2)),))
    with pytest.raises(ValueError, match='out must be a contiguous'):
        image_ops.detect_points_launch(df, 16, out=(torch.zeros((2, 15, 2)), None, None, None))
    with pytest.raises(ValueError, match='workspace must be'):
        image_ops.detect_points_launch(df, 16, workspace=torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r'contiguous frames \(N, H, W, C\)'):
        image_ops.corner_score_launch(df[:, :, ::2], 1)
    assert image_ops.detect_workspace_bytes(4, 1080, 1920) == _ffi.load_library().raft_detect_points_workspace_bytes(4, 1080, 1920, 7)
    with pytest.raises(ValueError, match='too large'):
        image_ops.detect_workspace_bytes(1, 1 << 16, 1 << 16)


def test_refill_points_launch_checks_its_arguments_without_a_gpu():
    import torch
    from tf_raft_amd import image_ops
    N, P, K = 2, 7, 4
    pos, lost = torch.zeros((N, P, 2)), torch.zeros((N, P), dtype=torch.uint8)
    new, count = torch.zeros((N, K, 2)), torch.zeros((N,), dtype=torch.int32)
    born, ids, nxt = torch.zeros((N, P), dtype=torch.int32), torch.zeros((N, P), dtype=torch.int32), torch.zeros((N,), dtype=torch.int32)
    good = dict(pos=pos, lost=lost, new_points=new, new_count=count, t=3, born=born, ids=ids, next_id=nxt)
    bad = [(dict(t=-1), 't0 must'), (dict(t=1.5), 't0 must'), (dict(t=True), 't0 must'),
           (dict(pos=pos[0]), r'positions \(N, P, 2\)'), (dict(pos=pos.to(torch.float64)), r'positions \(N, P, 2\)'),
           (dict(pos=np.zeros((N, P, 2), np.float32)), r'positions \(N, P, 2\)'),
           (dict(lost=lost[:, :6]), 'out must be a contiguous'), (dict(lost=lost.to(torch.int32)), 'out must be a contiguous'),
           (dict(new_points=new[:1]), r'new points \(2, K, 2\)'), (dict(new_points=torch.zeros((N, 4097, 2))), r'new points \(2, K, 2\)'),
           (dict(new_points=new.to(torch.float64)), 'out must be a contiguous'),
           (dict(new_count=count.to(torch.int64)), 'out must be a contiguous'), (dict(new_count=torch.zeros((N, 1), dtype=torch.int32)), 'out must'),
           (dict(born=born.to(torch.int64)), 'out must be a contiguous'), (dict(ids=ids[:, :3]), 'out must be a contiguous'),
           (dict(next_id=torch.zeros((3,), dtype=torch.int32)), 'out must be a contiguous'),
           (dict(out=pos), 'out must be a pair'), (dict(out=(pos, lost.to(torch.int32))), 'out must be a contiguous'),
           (dict(out=(pos[:, :3], lost)), 'out must be a contiguous')]
    for change, match in bad:
        with pytest.raises(ValueError, match=match):
            image_ops.refill_points_launch(**{**good, **change})
    with pytest.raises(ValueError, match='too large'):
        image_ops.refill_points_launch(**{**good, 'pos': torch.empty((1, 1 << 30, 2), dtype=torch.float32, device='meta')})


def test_the_tracker_checks_its_new_arguments_before_any_device_work():
    import inspect
    from tf_raft_amd.model import RAFT, SmallRAFT
    from tf_raft_amd.video import FlowTracker
    pts = np.zeros((1, 7, 2), np.float32)
    video = np.zeros((3, 64, 96, 3), np.uint8)
    for cls in (RAFT, SmallRAFT):
        for fn in (cls.tracker, cls.track_video):
            sig = inspect.signature(fn).parameters
            assert sig['max_points'].default is None and sig['replenish'].default is False and sig['detect'].default is None
            assert list(sig)[-3:] == ['max_points', 'replenish', 'detect']              # behind every existing argument
        model = cls.__new__(cls)                                             # (no device: anything enqueued would fail)
        for call in (lambda **kw: model.tracker(None, **kw), lambda **kw: model.track_video(video, None, **kw)):
            with pytest.raises(ValueError, match='pass max_points=K'):
                call()
            for bad in (0, 4097, -1, 2.5, True):
                with pytest.raises(ValueError, match='max_points must'):
                    call(max_points=bad)
            with pytest.raises(ValueError, match='start belongs to given points'):
                call(max_points=8, start=np.zeros((1, 8), np.int32))
            for bad in (1, None, 'yes'):
                with pytest.raises(ValueError, match='replenish must'):
                    call(max_points=8, replenish=bad)
            for bad in ('x', ['min_distance'], {'distance': 3}, {'max_points': 3}):
                with pytest.raises(ValueError, match='detect must be a dict'):
                    call(max_points=8, detect=bad)
            for bad, match in (({'min_distance': 0}, 'min_distance must'), ({'min_distance': 16}, 'min_distance must'),
                               ({'quality_level': 1.0}, 'quality_level must'), ({'quality_level': float('nan')}, 'quality_level must'),
                               ({'block_radius': 4}, 'block_radius must'), ({'method': 'fast'}, 'method must'),
                               ({'harris_k': -1}, 'harris_k must'), ({'border': 1}, 'border must'),
                               ({'block_radius': 3, 'border': 3}, 'border must'),
                               ({'mask': np.ones((64, 96), np.uint8)}, 'mask of detect'),
                               ({'mask': np.ones((1, 64, 96), np.float32)}, 'mask of detect')):
                with pytest.raises(ValueError, match=match):
                    call(max_points=8, detect=bad)
        with pytest.raises(ValueError, match='detect belongs to'):
            model.tracker(pts, detect={'min_distance': 3})
        with pytest.raises(ValueError, match='detect belongs to'):
            model.track_video(video, pts[0], detect={})
        with pytest.raises(ValueError, match='max_points must'):
            model.tracker(pts, replenish=True, max_points=0)
        with pytest.raises(ValueError, match='warm_start'):
            model.tracker(None, max_points=8, warm_start=True)
        # a mask of another shape than the frames fails at the push, before anything reaches a device
        with pytest.raises(ValueError, match=r'mask of detect must be \(1, 64, 96\)'):
            model.track_video(video, None, max_points=8, detect={'mask': np.ones((1, 64, 95), np.uint8)})
        for kw in ({}, {'consistency': False}, {'replenish': True}):
            tracker = model.tracker(None, max_points=8, detect={'mask': np.ones((2, 64, 95), bool)}, **kw)
            assert isinstance(tracker, FlowTracker) and tracker.ids is None and tracker.born is None
            with pytest.raises(ValueError, match=r'mask of detect must be \(2, 64, 96\)'):
                tracker.push(np.zeros((2, 64, 96, 3), np.uint8))
            with pytest.raises(ValueError, match=r'\(N, H, W, 3\)'):
                tracker.push(video[0])
            tracker.reset()
        tracker = model.tracker(pts, replenish=True)
        assert tracker.replenish and tracker._K == 7
        assert model.tracker(np.zeros((1, 5000, 2), np.float32), replenish=True)._K == 4096
        assert model.tracker(pts, replenish=True, max_points=3)._K == 3
        with pytest.raises(ValueError, match=r'\(N, H, W, 3\) with N = 1'):
            tracker.push(video[:2])

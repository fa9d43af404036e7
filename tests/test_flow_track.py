"""Points followed through a video, host side (no GPU): the float32 NumPy restatement ``np_track`` of DESIGN.md section 26 with its
known answers, the inputs tests/test_gpu_flow_track.py runs and what they exercise, the C entry's declaration and argument checks,
and the errors of the Python layer.  The GPU file compares the kernel with ``np_track`` BIT FOR BIT: the kernel is a pure gather
with contraction switched off, so every product and sum here is one float32 operation in the kernel's order and there is no
tolerance anywhere.

The definition, for a point that is tracked (code 0) at ``(x, y)`` and has started (``start <= t0 + s``): the point is in frame
iff ``0 <= x <= W - 1`` and ``0 <= y <= H - 1`` (a NaN is not), else code 1; ``f`` = the forward flow of step ``s`` sampled
bilinearly there (``x0 = floor(x)``, ``x1 = min(x0 + 1, W - 1)``, ``a = x - x0``, the same for y, and ``(1 - b) * ((1 - a) * g00 +
a * g01) + b * ((1 - a) * g10 + a * g11)``); ``q = (x + f.x, y + f.y)``; ``q`` out of frame: code 1; with a backward flow ``b``
sampled at ``q``, ``!(|f + b|^2 <= alpha * (|f|^2 + |b|^2) + beta)``: code 2; otherwise the point moves to ``q``.  A nonzero code
is sticky and freezes the position.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tf_raft_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, BETA = 0.01, 0.5
F1 = np.float32(1)

# (S, N, H, W, P): what tests/test_gpu_flow_track.py runs
SHAPES = [(1, 1, 1, 1, 1), (2, 1, 5, 1, 7), (3, 1, 1, 9, 5), (3, 2, 9, 13, 300), (4, 3, 37, 53, 37 * 53), (6, 1, 64, 96, 1000)]
IDS = ['x'.join(map(str, s)) for s in SHAPES]


# ------------------------------------------------------------------ the restatement
def np_taps(x, y, H, W):
    """``sample_taps`` of csrc/flow_sample.h for float32 arrays: (in, x0, x1, y0, y1, a, b)."""
    assert x.dtype == y.dtype == np.float32
    with np.errstate(invalid='ignore'):
        inside = (x >= 0) & (x <= np.float32(W - 1)) & (y >= 0) & (y <= np.float32(H - 1))
    px, py = np.where(inside, x, np.float32(0)), np.where(inside, y, np.float32(0))
    fx, fy = np.floor(px), np.floor(py)
    x0, y0 = np.clip(fx.astype(np.int64), 0, W - 1), np.clip(fy.astype(np.int64), 0, H - 1)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    a, b = px - fx, py - fy
    assert a.dtype == b.dtype == np.float32
    return inside, x0, x1, y0, y1, a, b


def np_sample_flow(g, n, taps):
    """Both components of the flows ``g`` (N, H, W, 2) of the points' videos ``n`` at ``taps``, every operation in float32."""
    _, x0, x1, y0, y1, a, b = taps
    a, b = a[:, None], b[:, None]
    g00, g01, g10, g11 = g[n, y0, x0], g[n, y0, x1], g[n, y1, x0], g[n, y1, x1]
    with np.errstate(invalid='ignore', over='ignore'):
        na, nb = F1 - a, F1 - b
        v = nb * (na * g00 + a * g01) + b * (na * g10 + a * g11)
    assert v.dtype == np.float32
    return v


def np_disagree(f, b, alpha, beta):
    """``flows_disagree`` of csrc/flow_sample.h: the comparison of ``occluded_at`` in its operation order."""
    alpha, beta = np.float32(alpha), np.float32(beta)
    with np.errstate(invalid='ignore', over='ignore'):
        dx, dy = f[:, 0] + b[:, 0], f[:, 1] + b[:, 1]
        lhs = dx * dx + dy * dy
        rhs = alpha * ((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1])) + beta
        assert lhs.dtype == rhs.dtype == np.float32
        return ~(lhs <= rhs)


def np_track(pos, lost, fwd, bwd, alpha=ALPHA, beta=BETA, start=None, t0=0, outcomes=None):
    """pos (N, P, 2) float32, lost (N, P) uint8 or None, fwd / bwd (S, N, H, W, 2) float32 (bwd may be None), start (N, P) integers
    or None -> (positions (S, N, P, 2) float32, lost (S, N, P) uint8).  ``outcomes``: a list that receives, per step, the numbers
    of active points that stayed tracked, left the frame and failed the test."""
    pos, fwd = np.asarray(pos), np.asarray(fwd)
    assert pos.dtype == np.float32 and fwd.dtype == np.float32 and pos.ndim == 3 and fwd.ndim == 5
    S, N, H, W, _ = fwd.shape
    P = pos.shape[1]
    assert pos.shape == (N, P, 2) and (bwd is None or (bwd.shape == fwd.shape and bwd.dtype == np.float32))
    cur = pos.reshape(N * P, 2).copy()
    code = np.zeros(N * P, np.uint8) if lost is None else np.asarray(lost).astype(np.uint8).reshape(N * P).copy()
    first = np.zeros(N * P, np.int64) if start is None else np.asarray(start).astype(np.int64).reshape(N * P)
    video = np.repeat(np.arange(N), P)
    pos_out, lost_out = np.empty((S, N * P, 2), np.float32), np.empty((S, N * P), np.uint8)
    for s in range(S):
        idx = np.nonzero((code == 0) & (first <= t0 + s))[0]
        x, y, n = cur[idx, 0], cur[idx, 1], video[idx]
        t1 = np_taps(x, y, H, W)
        f = np_sample_flow(fwd[s], n, t1)
        with np.errstate(invalid='ignore', over='ignore'):
            qx, qy = x + f[:, 0], y + f[:, 1]
        t2 = np_taps(qx, qy, H, W)
        left = ~t1[0] | ~t2[0]
        failed = np.zeros(len(idx), bool)
        if bwd is not None:
            failed = ~left & np_disagree(f, np_sample_flow(bwd[s], n, t2), alpha, beta)
        moved = ~left & ~failed
        code[idx[left]], code[idx[failed]] = 1, 2
        cur[idx[moved], 0], cur[idx[moved], 1] = qx[moved], qy[moved]
        if outcomes is not None:
            outcomes.append((int(moved.sum()), int(left.sum()), int(failed.sum())))
        pos_out[s], lost_out[s] = cur, code
    return pos_out.reshape(S, N, P, 2), lost_out.reshape(S, N, P)


def bits(x):
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32
    return x.view(np.uint32)


def assert_same(got, want):
    """Positions as uint32, codes as bytes: no tolerance and nothing left out."""
    np.testing.assert_array_equal(bits(got[0]), bits(want[0]))
    assert np.asarray(got[1]).dtype == np.uint8
    np.testing.assert_array_equal(got[1], want[1])


# ------------------------------------------------------------------ the inputs both test files use
def _box7(a):
    """The mean over 7 taps along H and along W of (..., H, W, 2), the borders repeated."""
    for axis in (-3, -2):
        pad = [(0, 0)] * a.ndim
        pad[axis] = (3, 3)
        p = np.pad(a, pad, mode='edge')
        n = a.shape[axis]
        a = sum(np.take(p, range(k, k + n), axis=axis) for k in range(7)) / 7.0
    return a


def track_flows(S, N, H, W, seed=1):
    """Smooth flows: white normal noise box-filtered over 7 taps along both axes, times 2, on top of a drift of about 0.08 of the
    frame's shorter side per step in one direction per video, so that points keep arriving at a border at EVERY step (under a
    flow without a drift the points near the borders are used up after a step or two); the backward flow is the forward flow's
    negative plus 2.6 times another filtered field, so that the test fails for a share of the points at every step."""
    rng = np.random.default_rng([seed, S, N, H, W])
    theta = rng.uniform(0, 2 * np.pi, (1, N, 1, 1))
    length = 0.08 * min(H, W) * rng.uniform(0.8, 1.2, (S, N, 1, 1))
    drift = length[..., None] * np.stack([np.cos(theta), np.sin(theta)], axis=-1)
    fwd = drift + _box7(rng.standard_normal((S, N, H, W, 2))) * 2
    bwd = -fwd + _box7(rng.standard_normal((S, N, H, W, 2))) * 2.6
    return np.ascontiguousarray(fwd, np.float32), np.ascontiguousarray(bwd, np.float32)


def dense_grid(H, W, N=1):
    """Every pixel as a point (x, y), rows first: what image_ops.point_grid(H, W, 1, N) has to return."""
    ys, xs = np.mgrid[0:H, 0:W]
    grid = np.stack([xs, ys], axis=-1).reshape(1, H * W, 2).astype(np.float32)
    return np.ascontiguousarray(np.repeat(grid, N, axis=0))


def track_points(N, H, W, P, seed=1):
    """The dense grid where P = H * W; else sub-pixel random points, some outside the frame and (from 20 points on) some NaN."""
    if P == H * W:
        return dense_grid(H, W, N)
    rng = np.random.default_rng([seed, N, H, W, P])
    pts = np.stack([rng.uniform(-1.5, W + 0.5, (N, P)), rng.uniform(-1.5, H + 0.5, (N, P))], axis=-1).astype(np.float32)
    inside = rng.random((N, P)) < 0.8                           # most of them well inside, so that they live for some steps
    pts[inside] = np.stack([rng.uniform(0, W - 1, inside.sum()), rng.uniform(0, H - 1, inside.sum())], axis=-1).astype(np.float32)
    if P >= 20:
        pts[:, 3::25, 0] = np.nan
        pts[:, 11::50, 1] = np.array([0x7FC01234], np.uint32).view(np.float32)[0]      # a NaN with a payload
    return np.ascontiguousarray(pts)


T0 = 3                                  # the frame index the cases with a `start` begin at


def track_case(shape, seed=1):
    """Everything one shape runs with: points, flows, the codes to begin with (0, 1, 2 and 7) and the start frames."""
    S, N, H, W, P = shape
    rng = np.random.default_rng([seed, 99] + list(shape))
    fwd, bwd = track_flows(S, N, H, W, seed)
    pts = track_points(N, H, W, P, seed)
    lost = rng.choice(np.array([0, 0, 0, 0, 0, 1, 2, 7], np.uint8), size=(N, P))
    start = rng.integers(T0 - 1, T0 + S + 1, size=(N, P)).astype(np.int32)       # before the first step ... after the last
    for a in (fwd, bwd, pts, lost, start):
        a.setflags(write=False)
    return {'points': pts, 'forward': fwd, 'backward': bwd, 'lost': lost, 'start': start}


# ------------------------------------------------------------------ known answers
def moving_square(T=7, H=40, W=56, side=12, top=16, left=10, d=(3, -2)):
    """A square that moves by ``d`` per frame over a static background: the flows of the T - 1 pairs and the square's maps."""
    S = T - 1
    fwd, bwd = np.zeros((S, 1, H, W, 2), np.float32), np.zeros((S, 1, H, W, 2), np.float32)
    sq = np.zeros((T, H, W), bool)
    for t in range(T):
        y, x = top + t * d[1], left + t * d[0]
        assert 0 <= y and y + side <= H and 0 <= x and x + side <= W
        sq[t, y:y + side, x:x + side] = True
    for s in range(S):
        fwd[s, 0, sq[s]] = d
        bwd[s, 0, sq[s + 1]] = (-d[0], -d[1])
    return fwd, bwd, sq


def test_the_moving_square_is_followed_and_what_it_covers_is_lost():
    fwd, bwd, sq = moving_square()
    T, H, W = sq.shape
    d = np.array((3, -2), np.float32)
    grid = dense_grid(H, W)
    pos, lost = np_track(grid, None, fwd, bwd)
    on = sq[0].reshape(-1)
    covered_at = np.full(H * W, T, np.int64)                    # the first frame >= 1 in which the square covers a pixel
    for t in range(T - 1, 0, -1):
        covered_at[sq[t].reshape(-1)] = t
    for s in range(T - 1):
        np.testing.assert_array_equal(pos[s, 0, on], grid[0, on] + np.float32(s + 1) * d)
        assert not lost[s, 0, on].any()
        hit = ~on & (covered_at <= s + 1)                       # covered in the frame this step ends in, or earlier
        assert (lost[s, 0, hit] == 2).all() and not lost[s, 0, ~on & ~hit].any()
        np.testing.assert_array_equal(bits(pos[s, 0, ~on]), bits(grid[0, ~on]))      # lost or not, the background never moves
    assert int((lost[-1] == 2).sum()) == 324 and round(100 * 324 / (H * W), 2) == 14.46
    # without the backward flow nothing is ever lost here, and the square's points arrive all the same
    pos1, lost1 = np_track(grid, None, fwd, None)
    assert not lost1.any()
    np.testing.assert_array_equal(pos1[:, 0, on], pos[:, 0, on])


def test_a_point_that_drifts_off_the_frame_keeps_its_last_position():
    fwd = np.zeros((4, 1, 8, 8, 2), np.float32)
    fwd[..., 0] = 2.5
    nan = np.float32(np.nan)
    pts = np.array([[(1, 3), (7, 7), (nan, 2), (2, nan), (-0.25, 3)]], np.float32)
    for bwd in (None, -fwd):
        pos, lost = np_track(pts, None, fwd, bwd)
        np.testing.assert_array_equal(pos[:, 0, 0, 0], np.array([3.5, 6, 6, 6], np.float32))
        np.testing.assert_array_equal(pos[:, 0, 0, 1], np.float32(3))
        np.testing.assert_array_equal(lost[:, 0, 0], [0, 0, 1, 1])
        assert (lost[:, 0, 1:] == 1).all()                      # (7, 7) steps out at once; a NaN or a point outside is not in frame
        for s in range(4):
            np.testing.assert_array_equal(bits(pos[s, 0, 1:]), bits(pts[0, 1:]))     # bit for bit, the NaNs too


def test_the_flow_conventions():
    pts = np.array([[(2, 2), (5, 5)]], np.float32)
    fwd = np.zeros((1, 1, 8, 8, 2), np.float32)
    fwd[..., 0] = 1
    bwd = np.full((1, 1, 8, 8, 2), 40, np.float32)                   # wildly inconsistent
    assert (np_track(pts, None, fwd, bwd)[1] == 2).all()
    assert not np_track(pts, None, fwd, None)[1].any()               # no backward flow: never code 2
    ok = -fwd
    assert not np_track(pts, None, fwd, ok)[1].any()
    bad = ok.copy()
    bad[0, 0, 2, 3, 1] = np.nan                                       # where (2, 2) arrives
    np.testing.assert_array_equal(np_track(pts, None, fwd, bad)[1][0, 0], [2, 0])
    nanf = fwd.copy()
    nanf[0, 0, 5, 5, 0] = np.nan                                      # where (5, 5) is
    pos, lost = np_track(pts, None, nanf, ok)
    np.testing.assert_array_equal(lost[0, 0], [0, 1])                 # a NaN in the forward flow: the new position is not in frame
    np.testing.assert_array_equal(pos[0, 0], np.array([(3, 2), (5, 5)], np.float32))
    # alpha and beta are the test's: a large beta forgives everything finite
    assert not np_track(pts, None, fwd, bwd, alpha=0.0, beta=1e6)[1].any()
    # codes that come in are sticky, whatever their value
    pos, lost = np_track(pts, np.array([[7, 0]], np.uint8), fwd, ok)
    np.testing.assert_array_equal(lost[0, 0], [7, 0])
    np.testing.assert_array_equal(pos[0, 0], np.array([(2, 2), (6, 5)], np.float32))


@pytest.mark.parametrize('shape', SHAPES[3:], ids=IDS[3:])
def test_s_steps_in_one_call_equal_s_calls_of_one_step(shape):
    case = track_case(shape)
    S = shape[0]
    for bwd in (case['backward'], None):
        want = np_track(case['points'], case['lost'], case['forward'], bwd)
        pos, lost = case['points'], case['lost']
        for s in range(S):
            p1, l1 = np_track(pos, lost, case['forward'][s:s + 1], None if bwd is None else bwd[s:s + 1])
            assert_same((p1[0], l1[0]), (want[0][s], want[1][s]))
            pos, lost = p1[0], l1[0]


@pytest.mark.parametrize('shape', SHAPES[3:], ids=IDS[3:])
def test_a_point_waits_for_its_start_and_then_runs_as_if_the_call_began_there(shape):
    case = track_case(shape)
    S, N, _, _, P = shape
    pos, lost = np_track(case['points'], case['lost'], case['forward'], case['backward'], start=case['start'], t0=T0)
    assert len(np.unique(case['start'])) >= min(S + 2, 3)
    for k in np.unique(case['start']):
        sel = case['start'] == k
        first = max(int(k) - T0, 0)                                   # the first step these points take part in
        for s in range(min(first, S)):                                # untouched before it, the codes that came in too
            np.testing.assert_array_equal(bits(pos[s][sel]), bits(case['points'][sel]))
            np.testing.assert_array_equal(lost[s][sel], case['lost'][sel])
        if first < S:                                                 # from there on: a call that begins at frame k
            want = np_track(case['points'], case['lost'], case['forward'][first:], case['backward'][first:], t0=T0 + first)
            np.testing.assert_array_equal(bits(pos[first:][:, sel]), bits(want[0][:, sel]))
            np.testing.assert_array_equal(lost[first:][:, sel], want[1][:, sel])
    # a start in the past is no start at all
    assert_same(np_track(case['points'], None, case['forward'], None, start=np.zeros((N, P), np.int32), t0=T0),
                np_track(case['points'], None, case['forward'], None))


@pytest.mark.parametrize('shape', [s for s in SHAPES if s[2] * s[3] >= 35], ids=[i for s, i in zip(SHAPES, IDS) if s[2] * s[3] >= 35])
def test_the_test_flows_leave_every_outcome_its_share_at_every_step(shape):
    """A condition on the INPUTS: at every step at least 2 % of the points that are still active stay tracked, 2 % leave the
    frame and 2 % fail the consistency test, so every branch of the kernel decides a visible share of every row."""
    case = track_case(shape)
    outcomes = []
    np_track(case['points'], None, case['forward'], case['backward'], outcomes=outcomes)
    assert len(outcomes) == shape[0]
    for s, counts in enumerate(outcomes):
        active = sum(counts)
        assert active > 0 and min(counts) >= 0.02 * active, (s, counts)


# ------------------------------------------------------------------ the C entry
def test_the_header_declares_and_the_library_exports_the_entry():
    from tf_raft_amd import build
    assert 'flow_track.hip' in build.SOURCES and 'flow_check.hip' in build.SOURCES and 'flow_sample.h' in build.HEADERS
    with open(os.path.join(ROOT, 'include', 'raft_hip.h')) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    assert re.search(r'int\s+raft_track_points_f32\s*\(\s*const float \*pos_in,\s*const uint8_t \*lost_in,\s*const int32_t \*start,\s*int t0,'
                     r'\s*const float \*flow_forward,\s*const float \*flow_backward,\s*float \*pos_out,\s*uint8_t \*lost_out,\s*int S,'
                     r'\s*int N,\s*int64_t P,\s*int H,\s*int W,\s*float alpha,\s*float beta,\s*void \*stream\s*\)', header)
    sigs = _ffi.header_signatures(header)
    P, I, F = C.c_void_p, C.c_int, C.c_float
    assert sigs['raft_track_points_f32'] == (I, [P, P, P, I, P, P, P, P, I, I, C.c_int64, I, I, F, F, P])
    assert len(sigs['raft_track_points_f32'][1]) == 16
    assert _ffi.ABI_VERSION == 222                                   # an entry was added, no signature changed
    lib = _ffi.load_library()
    assert lib.raft_version() == 222
    assert lib.raft_track_points_f32.argtypes == sigs['raft_track_points_f32'][1]
    # the comparison and the pair load have ONE definition, in the header both kernels include
    src = {n: open(os.path.join(ROOT, 'tf_raft_amd', 'csrc', n)).read() for n in ('flow_sample.h', 'flow_check.hip', 'flow_track.hip')}
    assert 'struct alignas(8) FlowPair' in src['flow_sample.h'] and 'flows_disagree(float2' in src['flow_sample.h']
    for name in ('flow_check.hip', 'flow_track.hip'):
        assert 'FlowPair {' not in src[name] and 'flows_disagree(' in src[name] and 'sample_flow<PAIR>' in src[name], name
        assert '#pragma clang fp contract(off)' in src[name], name


def test_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    fn = _ffi.load_library().raft_track_points_f32
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off = C.c_void_p(p.value + 4)
    #       pos_in lost_in start t0 fwd bwd pos_out lost_out S  N  P  H  W  alpha beta stream
    good = [p, p, p, 0, p, p, p, p, 2, 1, 7, 4, 5, 0.01, 0.5, None]
    for k in (0, 4, 6, 7):                                          # (lost_in, start and flow_backward may be NULL)
        for opt in (p, None):
            args = list(good)
            args[k], args[1], args[2], args[5] = None, opt, opt, opt
            assert fn(*args) == -1, k
    for k in (8, 9, 10, 11, 12):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    args = list(good)
    args[3] = -1                                                    # t0
    assert fn(*args) == -2
    too_large = ((1 << 10, 1 << 10, 7, 1 << 5, 1 << 5), (1, 1, 7, 1 << 15, 1 << 15), (1 << 16, 1 << 16, 1, 1, 1),       # S * N * H * W * 2
                 (1, 1 << 30, 1, 1, 1), (1 << 15, 1 << 15, 1, 1, 1),                                                    #   >= 2^31
                 (1, 1, 1 << 30, 4, 5), (2, 1, 1 << 29, 4, 5), (1, 1, 1 << 40, 4, 5), (3, 5, 1 << 27, 4, 5))            # S * N * P * 2 >= 2^31
    for bad in too_large:
        args = list(good)
        args[8:13] = bad
        assert fn(*args) == -2, bad
    for k in (13, 14):
        for v in (-1.0, float('nan'), float('inf'), -float('inf'), -2.0 ** -100):
            for bwd in (p, None):                                   # (checked with and without a backward flow)
                args = list(good)
                args[k], args[5] = v, bwd
                assert fn(*args) == -2, (k, v)
    for k in (0, 4, 5, 6):
        args = list(good)
        args[k] = off
        assert fn(*args) == -4, k
    args = list(good)                                               # precedence: NULL before shape before alignment
    args[7], args[11], args[4] = None, 0, off
    assert fn(*args) == -1
    args[7] = p
    assert fn(*args) == -2
    args[11], args[14] = 4, float('nan')
    assert fn(*args) == -2
    args[14], args[3] = 0.0, 1 << 30                                # (beta = 0 and a late t0 are allowed)
    assert fn(*args) == -4


# ------------------------------------------------------------------ the Python layer, nothing reaches the device
BAD_AB = (-1, float('nan'), float('inf'), 1e39, True, None, 'x')


def test_point_grid():
    from tf_raft_amd import image_ops
    g = image_ops.point_grid(3, 4)
    assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == (1, 12, 2) and g.flags.c_contiguous
    np.testing.assert_array_equal(g, dense_grid(3, 4))
    np.testing.assert_array_equal(image_ops.point_grid(37, 53, N=3), dense_grid(37, 53, 3))
    g = image_ops.point_grid(5, 7, stride=3, N=2)
    assert g.shape == (2, 2 * 3, 2)
    np.testing.assert_array_equal(g[1], np.array([(0, 0), (3, 0), (6, 0), (0, 3), (3, 3), (6, 3)], np.float32))
    for bad in ({'H': 0}, {'W': -1}, {'stride': 0}, {'N': 0}, {'H': 2.5}, {'stride': True}, {'N': None}):
        with pytest.raises(ValueError, match='integer >= 1'):
            image_ops.point_grid(**{'H': 4, 'W': 5, **bad})


def test_shapes_types_and_the_test_s_arguments_are_checked_without_a_gpu():
    import torch
    from tf_raft_amd import image_ops
    pts = np.zeros((2, 7, 2), np.float32)
    fwd = np.zeros((3, 2, 4, 5, 2), np.float32)
    for bad in BAD_AB:
        with pytest.raises(ValueError, match='alpha must'):
            image_ops.track(pts, fwd, alpha=bad)
        with pytest.raises(ValueError, match='beta must'):
            image_ops.track(pts, fwd, fwd, beta=bad)
    with pytest.raises(ValueError, match=r'points \(N, P, 2\)'):
        image_ops.track(pts[0], fwd)
    with pytest.raises(ValueError, match=r'points \(N, P, 2\)'):
        image_ops.track(np.zeros((2, 7, 3), np.float32), fwd)
    with pytest.raises(ValueError, match='empty'):
        image_ops.track(pts[:, :0], fwd)
    with pytest.raises(TypeError, match='points are float32'):
        image_ops.track(pts.astype(np.uint8), fwd)
    with pytest.raises(TypeError):
        image_ops.track(pts.astype(np.int32), fwd)
    with pytest.raises(ValueError, match=r'flows \(S, N, H, W, 2\) or \(N, H, W, 2\)'):
        image_ops.track(pts, fwd[0, 0])
    with pytest.raises(ValueError, match='with N = 2'):
        image_ops.track(pts, fwd[:, :1])
    with pytest.raises(ValueError, match='with N = 2'):
        image_ops.track(pts, fwd[..., :1])
    with pytest.raises(TypeError, match='a flow is float32'):
        image_ops.track(pts, fwd.astype(np.uint8))
    with pytest.raises(ValueError, match='expects a flow'):
        image_ops.track(pts, fwd, fwd[0])
    with pytest.raises(ValueError, match='expects a flow'):
        image_ops.track(pts, fwd[0], fwd)
    with pytest.raises(TypeError, match='a flow is float32'):
        image_ops.track(pts, fwd, fwd.astype(np.uint8))
    with pytest.raises(ValueError, match='expects lost'):
        image_ops.track(pts, fwd, lost=np.zeros((2, 6), np.uint8))
    with pytest.raises(TypeError, match='lost is uint8 or bool'):
        image_ops.track(pts, fwd, lost=np.zeros((2, 7), np.float32))
    with pytest.raises(ValueError, match='expects start'):
        image_ops.track(pts, fwd, start=np.zeros((7,), np.int32))
    with pytest.raises(TypeError, match='start holds integers'):
        image_ops.track(pts, fwd, start=np.zeros((2, 7), np.float32))
    with pytest.raises(ValueError, match='frame indices >= 0'):
        image_ops.track(pts, fwd, start=np.full((2, 7), -1))
    with pytest.raises(ValueError, match='frame indices >= 0'):
        image_ops.track(pts, fwd, start=torch.full((2, 7), 1 << 31, dtype=torch.int64))
    for bad in (-1, 1.0, True, None, (1 << 31) - 3):
        with pytest.raises(ValueError, match='t0 must'):
            image_ops.track(pts, fwd, t0=bad)
    with pytest.raises(ValueError, match='too large'):
        image_ops.track(torch.empty((1, 1 << 30, 2), dtype=torch.float32, device='meta'),
                        torch.empty((1, 4, 5, 2), dtype=torch.float32, device='meta'))
    with pytest.raises(ValueError, match='too large'):
        image_ops.track(torch.empty((1, 7, 2), dtype=torch.float32, device='meta'),
                        torch.empty((1 << 10, 1, 1 << 10, 1 << 10, 2), dtype=torch.float32, device='meta'))
    # the launch form checks what it is handed, too
    dp, df = torch.zeros((2, 7, 2)), torch.zeros((3, 2, 4, 5, 2))
    with pytest.raises(ValueError, match='alpha must'):
        image_ops.track_launch(dp, df, alpha=-1)
    with pytest.raises(ValueError, match=r'points \(N, P, 2\)'):
        image_ops.track_launch(dp[0], df)
    with pytest.raises(ValueError, match='need flows'):
        image_ops.track_launch(dp, df[0])
    with pytest.raises(ValueError, match='expected a backward flow'):
        image_ops.track_launch(dp, df, df[:2])
    with pytest.raises(ValueError, match='out must be a contiguous'):
        image_ops.track_launch(dp, df, lost=torch.zeros((2, 7)))
    with pytest.raises(ValueError, match='out must be a pair'):
        image_ops.track_launch(dp, df, out=torch.zeros((3, 2, 7, 2)))
    with pytest.raises(ValueError, match='out must be a contiguous'):
        image_ops.track_launch(dp, df, out=(torch.zeros((3, 2, 7, 2)), torch.zeros((3, 2, 7))))


def test_the_model_checks_its_arguments_before_any_device_work():
    import inspect
    from tf_raft_amd import image_ops
    from tf_raft_amd.model import RAFT, SmallRAFT
    from tf_raft_amd.video import FlowTracker
    pts = np.zeros((1, 7, 2), np.float32)
    video = np.zeros((3, 64, 96, 3), np.uint8)
    for cls in (RAFT, SmallRAFT):
        for fn in (cls.tracker, cls.track_video):
            sig = inspect.signature(fn).parameters
            assert sig['consistency'].default is True and sig['start'].default is None
            assert (sig['alpha'].default, sig['beta'].default) == (image_ops.CONSISTENCY_ALPHA, image_ops.CONSISTENCY_BETA) == (0.01, 0.5)
        assert inspect.signature(cls.tracker).parameters['warm_start'].default is False
        assert inspect.signature(cls.track_video).parameters['batch_size'].default == 4
        model = cls.__new__(cls)                                             # (no device: anything enqueued would fail)
        for bad in BAD_AB:
            with pytest.raises(ValueError, match='alpha must'):
                model.tracker(pts, alpha=bad)
            with pytest.raises(ValueError, match='beta must'):
                model.track_video(video, pts[0], beta=bad)
        with pytest.raises(ValueError, match='warm_start'):
            model.tracker(pts, warm_start=True)
        with pytest.raises(ValueError, match=r'points \(N, P, 2\)'):
            model.tracker(pts[0])
        with pytest.raises(TypeError, match='points are float32'):
            model.tracker(pts.astype(np.uint8))
        with pytest.raises(ValueError, match='expects start'):
            model.tracker(pts, start=np.zeros((7,), np.int32))
        with pytest.raises(ValueError, match='frame indices >= 0'):
            model.tracker(pts, start=np.full((1, 7), -2))
        for kw in ({}, {'consistency': False}, {'consistency': False, 'warm_start': True}):
            tracker = model.tracker(pts, **kw)
            assert isinstance(tracker, FlowTracker) and tracker.consistency is kw.get('consistency', True)
            with pytest.raises(ValueError, match=r'\(N, H, W, 3\) with N = 1'):
                tracker.push(video[0])
            with pytest.raises(ValueError, match=r'\(N, H, W, 3\) with N = 1'):
                tracker.push(video[:2])
            tracker.reset()
        with pytest.raises(ValueError, match=r'\(T, H, W, 3\)'):
            model.track_video(video[0], pts[0])
        with pytest.raises(ValueError, match='at least two frames'):
            model.track_video(video[:1], pts[0])
        with pytest.raises(ValueError, match=r'points \(P, 2\)'):
            model.track_video(video, pts)
        with pytest.raises(ValueError, match='expects start'):
            model.track_video(video, pts[0], start=np.zeros((1, 7), np.int32))
        for bad in (0, -1, 1.5, True, None):
            with pytest.raises(ValueError, match='batch_size'):
                model.track_video(video, pts[0], batch_size=bad)

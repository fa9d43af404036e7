"""The student's view, host side (no GPU): the float64 yardstick of ``raft_view_frames_f32`` and
``raft_view_flow_f32``, the float32 NumPy restatement in the kernels' operation order and its distance to the yardstick per case
(the tolerances of tests/test_gpu_student_view.py), known answers, one equivariance check, ``StudentTransform``'s draws, the C
entries' declarations and argument checks, and ``compile``'s validation.

The asserted bound on the restatement's distance is derived, not picked (``derived_bound``): the float32 coordinate
``(m0 * x + m1 * y) + o`` carries seven roundings (the three numbers of the record, two products, two sums), each at most 2^-24 of
``C = |m0| (W - 1) + |m1| (H - 1) + |o|``, the sample moves by at most that distance times the largest difference D between
neighbouring taps per axis (bilinear interpolation is continuous, with slope at most D per pixel), and its own eleven operations
add 2^-24 of the largest value each; the colour map scales that by |gain| and adds four roundings of its own, the flow's
``Minv f`` scales it by the largest absolute row sum of ``Minv`` and adds five.

Masks and in-frame decisions against float64 are compared outside a band: pixels whose float64 coordinate lies within 1e-3 of an
integer or of the frame's border are left out wherever the float32 coordinates differ from the float64 ones at all (the generic
view; the other views' coordinates are dyadic and exact, nothing is left out).  The float32 coordinates are asserted to lie
within 1e-4 of the float64 ones, so outside the band both floors agree.  At most 1 % of a case's pixels may be left out.

Measured distances of the restatement to the yardstick (absolute; noise frames of 0..255, noise flows of a few pixels; `pytest -s`
prints them for every case).  The identity view: exactly 0.  The mirrors, the quarter turn and the scaled views have exact
coordinates, but their weights (halves, quarters) make the products round: at most 2.8e-5 (frames) and 1.3e-6 (target), exactly 0
where the taps fall on pixels.  The generic view, whose float32 coordinates differ from the float64 ones by up to 1e-5 on noise
whose neighbouring taps differ by up to 250:

    teacher -> student, generic view         frames     bound      target     bound      left out
    (1,3,3) -> (1,1,1)                       2.1e-05    3.7e-04    9.7e-08    1.9e-05    0 %
    (1,5,7) -> (1,5,7)                       8.0e-05    2.5e-03    3.3e-06    1.9e-04    0 %
    (2,45,69) -> (2,40,56)                   1.4e-03    2.4e-02    5.4e-05    2.1e-03    0.47 %
    (1,16,24) -> (1,24,40)                   4.2e-04    1.4e-02    2.0e-05    1.1e-03    0.63 %
    (2,45,69) -> (2,40,56), gain/bias/clamp  1.4e-03    4.1e-02
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import report
from tf_raft_amd import _ffi
from tf_raft_amd.augment import StudentTransform, StudentView

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
BAND = 1e-3

# (teacher (B, Ht, Wt), student (B, H, W))
GEOMS = [((1, 3, 3), (1, 1, 1)),
         ((1, 5, 7), (1, 5, 7)),
         ((2, 45, 69), (2, 40, 56)),           # odd sizes, no multiple of the 32 x 8 tile, several workgroups, two records
         ((1, 16, 24), (1, 24, 40))]           # the student is larger: part of it is out of frame
VIEWS = ['identity', 'flip_x', 'flip_y', 'flip_xy', 'quarter', 'scale0.75', 'scale1.25', 'scale2', 'generic']
GENERIC = dict(rotate=7.0, zoom=1.13, shift=(0.37, -0.21))
CASES = [(g, v) for g in GEOMS for v in VIEWS] + [(g, 'colour') for g in GEOMS]
COLOUR_GAIN, COLOUR_BIAS = (1.7, 0.6, 1.0), (40.0, -30.0, 5.0)          # 0..255 frames: both ends of the clamp are reached


def case_id(case):
    (t, s), v = case
    return f"{'x'.join(map(str, t))}to{'x'.join(map(str, s[1:]))}-{v}"


CASE_IDS = [case_id(c) for c in CASES]
FLOW_CASES = [c for c in CASES if c[1] != 'colour']
FLOW_IDS = [case_id(c) for c in FLOW_CASES]


def linear_part(kind):
    if kind in ('generic', 'colour'):
        t = np.deg2rad(GENERIC['rotate'])
        return np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]) / GENERIC['zoom'] @ np.diag([-1.0, 1.0])
    if kind.startswith('scale'):
        return float(kind[5:]) * np.eye(2)
    return {'identity': np.eye(2), 'flip_x': np.diag([-1.0, 1.0]), 'flip_y': np.diag([1.0, -1.0]), 'flip_xy': -np.eye(2),
            'quarter': np.array([[0.0, -1.0], [1.0, 0.0]])}[kind]


def make_view(case):
    """The ``StudentView`` of a case, one view per slice.  The identity sits at the integer offset of the crop-or-pad window;
    every other view maps centre to centre, ``p - c_t - shift = M (q - c_s)``, slice b shifted by another (b / 2, -b / 4) -- all
    dyadic, so that only the generic view has coordinates that float32 cannot hold."""
    ((B, Ht, Wt), (_, H, W)), kind = case
    theta = np.zeros((B, 2, 3))
    M = linear_part(kind)
    for b in range(B):
        theta[b, :, :2] = M
        if kind == 'identity':
            theta[b, :, 2] = (-((W - Wt) // 2) if W > Wt else (Wt - W) // 2, -((H - Ht) // 2) if H > Ht else (Ht - H) // 2)
        else:
            shift = np.array(GENERIC['shift'] if kind in ('generic', 'colour') else (0.0, 0.0)) + (0.5 * b, -0.25 * b)
            theta[b, :, 2] = np.array([(Wt - 1) / 2.0, (Ht - 1) / 2.0]) + shift - M @ np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    if kind == 'colour':
        gain = np.tile(np.array(COLOUR_GAIN), (B, 2, 1))
        bias = np.tile(np.array(COLOUR_BIAS), (B, 2, 1))
        return StudentView(theta, gain, bias)
    return StudentView(theta)


@functools.lru_cache(maxsize=None)
def view_case(case):
    """``(frames (B, Ht, Wt, 3), flow (B, Ht, Wt, 2), teacher_visible (B, Ht, Wt) uint8, view)``; read-only, the tests share it."""
    ((B, Ht, Wt), _), kind = case
    rng = np.random.default_rng(100 * Ht + Wt)
    frames = rng.uniform(0, 255, (B, Ht, Wt, 3)).astype(np.float32)
    flow = rng.normal(0.0, 3.0, (B, Ht, Wt, 2)).astype(np.float32)
    tv = ((rng.uniform(size=(B, Ht, Wt)) < 0.9) * rng.integers(1, 256, (B, Ht, Wt))).astype(np.uint8)
    for a in (frames, flow, tv):
        a.setflags(write=False)
    return frames, flow, tv, make_view(case)


# ------------------------------------------------------------------ the restatement (float32, the kernels' operation order)
def records_of(view, slices=None):
    """The float32 numbers the device receives: a list of ``_ffi.ViewParams``."""
    return list(view.records(doubled=slices is not None and slices == 2 * len(view)))


def _coords32(r, H, W):
    x, y = np.arange(W, dtype=np.float32)[None, :], np.arange(H, dtype=np.float32)[:, None]
    m, o = [np.float32(v) for v in r.m], [np.float32(v) for v in r.o]
    with np.errstate(all='ignore'):
        return (m[0] * x + m[1] * y) + o[0], (m[2] * x + m[3] * y) + o[1]


def _taps(px, py, Ht, Wt):
    """flow_sample.h ``sample_taps`` for coordinate arrays of one float type: ``(in, y0, y1, x0, x1, a, b)``."""
    ft = px.dtype.type
    with np.errstate(invalid='ignore'):
        inn = (px >= 0) & (px <= ft(Wt - 1)) & (py >= 0) & (py <= ft(Ht - 1))
    qx, qy = np.where(inn, px, ft(0)), np.where(inn, py, ft(0))
    fx, fy = np.floor(qx), np.floor(qy)
    x0, y0 = np.clip(fx.astype(np.int64), 0, Wt - 1), np.clip(fy.astype(np.int64), 0, Ht - 1)
    return inn, y0, np.minimum(y0 + 1, Ht - 1), x0, np.minimum(x0 + 1, Wt - 1), qx - fx, qy - fy


def _bilinear(a, b, g00, g01, g10, g11):
    one = a.dtype.type(1)
    na, nb = one - a, one - b
    with np.errstate(all='ignore'):
        return nb * (na * g00 + a * g01) + b * (na * g10 + a * g11)


def np_view_frames(src, records, size):
    """csrc/student_view.hip ``view_frames_kernel`` operation for operation in float32."""
    H, W = size
    B, Ht, Wt, Cn = src.shape
    out = np.zeros((B, H, W, Cn), np.float32)
    for b, r in enumerate(records):
        inn, y0, y1, x0, x1, a, bb = _taps(*_coords32(r, H, W), Ht, Wt)
        g = src[b]
        v = _bilinear(a[..., None], bb[..., None], g[y0, x0], g[y0, x1], g[y1, x0], g[y1, x1])
        v = np.where(inn[..., None], v, np.float32(0))
        if r.colour:
            idx = [min(c, 2) for c in range(Cn)]
            gain, bias = np.array([r.gain[i] for i in idx], np.float32), np.array([r.bias[i] for i in idx], np.float32)
            v = np.minimum(np.maximum(v * gain + bias, np.float32(0)), np.float32(255))
        out[b] = v
    return out


def np_view_flow(flow, teacher_visible, records, size):
    """csrc/student_view.hip ``view_flow_kernel`` in float32: ``(target, target_visible)``."""
    H, W = size
    B, Ht, Wt, _ = flow.shape
    target, visible = np.zeros((B, H, W, 2), np.float32), np.zeros((B, H, W), np.uint8)
    zero = np.float32(0)
    for b, r in enumerate(records):
        inn, y0, y1, x0, x1, a, bb = _taps(*_coords32(r, H, W), Ht, Wt)
        wx, wy = a != 0, bb != 0
        g = flow[b]
        g00, g01, g10, g11 = g[y0, x0], np.where(wx[..., None], g[y0, x1], zero), np.where(wy[..., None], g[y1, x0], zero), \
            np.where((wx & wy)[..., None], g[y1, x1], zero)
        f = _bilinear(a[..., None], bb[..., None], g00, g01, g10, g11)
        i = [np.float32(v) for v in r.inv]
        with np.errstate(all='ignore'):
            t = np.stack([i[0] * f[..., 0] + i[1] * f[..., 1], i[2] * f[..., 0] + i[3] * f[..., 1]], -1)
        ok = inn & np.isfinite(t).all(-1)
        if teacher_visible is not None:
            m = teacher_visible[b] != 0
            ok &= m[y0, x0] & (~wx | m[y0, x1]) & (~wy | m[y1, x0]) & (~(wx & wy) | m[y1, x1])
        target[b] = np.where(ok[..., None], t, zero)
        visible[b] = ok
    return target, visible


# ------------------------------------------------------------------ the yardstick (float64, the definition)
def coords64(theta_b, H, W):
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    return theta_b[0, 0] * x + theta_b[0, 1] * y + theta_b[0, 2], theta_b[1, 0] * x + theta_b[1, 1] * y + theta_b[1, 2]


def sample64(g, px, py):
    """A float64 map ``(Ht, Wt, C)`` sampled at float64 positions by the bilinear rule: ``(values, in frame)``."""
    Ht, Wt = g.shape[:2]
    inn, y0, y1, x0, x1, a, b = _taps(px, py, Ht, Wt)
    return _bilinear(a[..., None], b[..., None], g[y0, x0], g[y0, x1], g[y1, x0], g[y1, x1]), inn


def band_of(theta_b, H, W, Ht, Wt):
    """Pixels whose float64 coordinate lies within ``BAND`` of an integer or of the frame's border."""
    px, py = coords64(theta_b, H, W)
    near = np.zeros((H, W), bool)
    for p in (px, py):
        near |= np.abs(p - np.rint(p)) <= BAND              # (the borders 0 and size - 1 are integers)
    return near


def frames_f64(src, view, size, frame=0):
    """``raft_view_frames_f32`` by its definition in float64, from the float64 view: ``(frames, in frame)``."""
    H, W = size
    B, Ht, Wt, Cn = src.shape
    out, inside = np.zeros((B, H, W, Cn)), np.zeros((B, H, W), bool)
    for b in range(B):
        n, fr = b % len(view), (b // len(view) if B == 2 * len(view) else frame)
        v, inn = sample64(src[b].astype(np.float64), *coords64(view.theta[n], H, W))
        v = np.where(inn[..., None], v, 0.0)
        if view.gain is not None:
            idx = [min(c, 2) for c in range(Cn)]
            v = np.clip(v * view.gain[n, fr][idx] + view.bias[n, fr][idx], 0.0, 255.0)
        out[b], inside[b] = v, inn
    return out, inside


def flow_f64(flow, teacher_visible, view, size):
    """``raft_view_flow_f32`` by its definition in float64: ``(target, target_visible)``.  ``flow`` may be float64."""
    H, W = size
    B, Ht, Wt, _ = flow.shape
    target, visible = np.zeros((B, H, W, 2)), np.zeros((B, H, W), bool)
    inv = view.inverse()
    for b in range(B):
        n = b % len(view)
        inn, y0, y1, x0, x1, a, bb = _taps(*coords64(view.theta[n], H, W), Ht, Wt)
        wx, wy = a != 0, bb != 0
        g = flow[b].astype(np.float64)
        f = _bilinear(a[..., None], bb[..., None], g[y0, x0], np.where(wx[..., None], g[y0, x1], 0.0),
                      np.where(wy[..., None], g[y1, x0], 0.0), np.where((wx & wy)[..., None], g[y1, x1], 0.0))
        with np.errstate(all='ignore'):
            t = f @ inv[n].T
        ok = inn & np.isfinite(t).all(-1)
        if teacher_visible is not None:
            m = teacher_visible[b] != 0
            ok &= m[y0, x0] & (~wx | m[y0, x1]) & (~wy | m[y1, x0]) & (~(wx & wy) | m[y1, x1])
        target[b], visible[b] = np.where(ok[..., None], t, 0.0), ok
    return target, visible


def compare_outside_band(case):
    """Per slice, the pixels the comparisons with float64 leave out (empty where the float32 coordinates are the float64 ones),
    with the checks that make the band valid: coordinates within 1e-4, at most 1 % left out."""
    ((B, Ht, Wt), (_, H, W)), _ = case
    view = view_case(case)[3]
    out = np.zeros((B, H, W), bool)
    worst = 0.0
    for b, r in enumerate(records_of(view)):
        px32, py32 = _coords32(r, H, W)
        px64, py64 = coords64(view.theta[b], H, W)
        px32, py32 = np.broadcast_to(px32, (H, W)).astype(np.float64), np.broadcast_to(py32, (H, W)).astype(np.float64)
        if not (np.array_equal(px32, px64) and np.array_equal(py32, py64)):
            worst = max(worst, float(np.abs(px32 - px64).max()), float(np.abs(py32 - py64).max()))
            out[b] = band_of(view.theta[b], H, W, Ht, Wt)
    assert worst <= 1e-4
    assert out.mean() <= 0.01, f'{out.mean():.4f} of the pixels lie in the band'
    return out, worst


def derived_bound(case):
    """``(frames bound, target bound)``: see the module's docstring."""
    ((B, Ht, Wt), (_, H, W)), kind = case
    frames, flow, _, view = view_case(case)

    def per_map(g, b, scale, extra_ops, offset):
        th = view.theta[b]
        cmax = max(abs(th[k, 0]) * (W - 1) + abs(th[k, 1]) * (H - 1) + abs(th[k, 2]) for k in (0, 1))
        g = g[b].astype(np.float64)
        d = max(float(np.abs(np.diff(g, axis=0)).max()) if Ht > 1 else 0.0, float(np.abs(np.diff(g, axis=1)).max()) if Wt > 1 else 0.0)
        vmax = float(np.abs(g).max())
        sample = 2 * (7 * EPS32 * cmax) * d + 11 * EPS32 * vmax
        return scale * sample + extra_ops * EPS32 * (scale * vmax + offset)

    fb = tb = 0.0
    for b in range(B):
        gain = float(np.abs(view.gain[b]).max()) if view.gain is not None else 1.0
        bias = float(np.abs(view.bias[b]).max()) if view.gain is not None else 0.0
        fb = max(fb, per_map(frames, b, gain, 4 if view.gain is not None else 0, bias))
        tb = max(tb, per_map(flow, b, float(np.abs(view.inverse()[b]).sum(1).max()), 5, 0.0))
    return fb, tb


@functools.lru_cache(maxsize=None)
def restatement_distance(case):
    """``(frames distance, target distance, share left out)`` of the float32 restatement to the float64 yardstick, with the masks
    compared exactly outside the band on the way.  The GPU test allows the kernels four times these."""
    (_, (_, H, W)), kind = case
    frames, flow, tv, view = view_case(case)
    recs = records_of(view)
    out, _ = compare_outside_band(case)
    got, (want, inside) = np_view_frames(frames, recs, (H, W)), frames_f64(frames, view, (H, W))
    dist_f = float(np.abs(got - want)[~out].max()) if (~out).any() else 0.0
    dist_t = 0.0
    for mask in (None, tv):
        tg, vis = np_view_flow(flow, mask, recs, (H, W))
        wt, wvis = flow_f64(flow, mask, view, (H, W))
        assert np.array_equal(vis[~out] != 0, wvis[~out])
        if (~out).any():
            dist_t = max(dist_t, float(np.abs(tg - wt)[~out].max()))
    return dist_f, dist_t, float(out.mean())


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_the_restatement_and_its_distance_to_the_yardstick(case):
    dist_f, dist_t, left_out = restatement_distance(case)
    bound_f, bound_t = derived_bound(case)
    report(f'student view {case_id(case)}', frames=dist_f, frames_bound=bound_f, target=dist_t, target_bound=bound_t, left_out=left_out)
    assert dist_f <= bound_f
    assert dist_t <= bound_t
    if case[1] != 'generic' and case[1] != 'colour':       # dyadic coordinates: exact in float32, nothing is left out
        assert left_out == 0.0
    if case[1] == 'identity':                              # weights 1, 0, 0, 0: nothing rounds
        assert dist_f == 0.0 and dist_t == 0.0


# ------------------------------------------------------------------ known answers, each exact (shared with the GPU tests)
class Restatement:
    """The two gathers as the tests of the known answers call them; tests/test_gpu_student_view.py has the device's."""

    @staticmethod
    def frames(src, view, size):
        return np_view_frames(np.asarray(src, np.float32), records_of(view), size)

    @staticmethod
    def flow(flow, view, size, visible=None):
        return np_view_flow(np.asarray(flow, np.float32), visible, records_of(view), size)


def window_of(a, size):
    """``resize_with_crop_or_pad`` of a NumPy ``(B, Ht, Wt, ...)`` array: the known answer of the identity view."""
    H, W = size
    _, Ht, Wt = a.shape[:3]
    out = np.zeros((a.shape[0], H, W) + a.shape[3:], a.dtype)
    cy, py, ey = max(-(H - Ht) // 2, 0), max((H - Ht) // 2, 0), min(H, Ht)
    cx, px, ex = max(-(W - Wt) // 2, 0), max((W - Wt) // 2, 0), min(W, Wt)
    out[:, py:py + ey, px:px + ex] = a[:, cy:cy + ey, cx:cx + ex]
    return out


def check_identity_is_the_window(impl, geom):
    case = (geom, 'identity')
    frames, flow, tv, view = view_case(case)
    size = geom[1][1:]
    np.testing.assert_array_equal(impl.frames(frames, view, size), window_of(frames, size))
    for mask in (None, tv):
        target, vis = impl.flow(flow, view, size, mask)
        want_vis = window_of(np.ones(flow.shape[:3], np.uint8) if mask is None else (mask != 0).astype(np.uint8), size)
        np.testing.assert_array_equal(vis, want_vis)
        np.testing.assert_array_equal(target, window_of(flow, size) * want_vis[..., None])


def _single(M, Ht, Wt, H, W, shift=(0.0, 0.0)):
    M = np.asarray(M, np.float64)
    o = np.array([(Wt - 1) / 2.0, (Ht - 1) / 2.0]) + shift - M @ np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    return StudentView(np.concatenate([M, o[:, None]], 1)[None])


def check_constant_teacher(impl):
    a, b = np.float32(1.75), np.float32(-0.625)
    flow = np.empty((1, 12, 20, 2), np.float32)
    flow[...] = (a, b)
    for M, want in ((np.diag([-1.0, 1.0]), (-a, b)), (2.0 * np.eye(2), (a / 2, b / 2)), ([[0.0, -1.0], [1.0, 0.0]], (b, -a))):
        # (the quarter turn M = [[0, -1], [1, 0]] has Minv = [[0, 1], [-1, 0]]: (a, b) -> (b, -a))
        target, vis = impl.flow(flow, _single(M, 12, 20, 6, 6), (6, 6))
        assert vis.all()
        assert (target[..., 0] == np.float32(want[0])).all() and (target[..., 1] == np.float32(want[1])).all(), (M, want)


def check_affine_teacher(impl):
    """f(p) = G p + g on a dyadic view: the closed form ``Minv (G (M q + o) + g)``, exact in float32 (every number a small dyadic)."""
    Ht, Wt, H, W = 16, 24, 8, 10
    G, g = np.array([[0.25, -0.5], [0.125, 0.75]]), np.array([1.5, -2.25])
    ys, xs = np.mgrid[0:Ht, 0:Wt].astype(np.float64)
    flow = np.stack([G[0, 0] * xs + G[0, 1] * ys + g[0], G[1, 0] * xs + G[1, 1] * ys + g[1]], -1)[None].astype(np.float32)
    M = np.array([[0.0, -0.5], [1.0, 0.5]])                                    # Minv = [[1, 1], [-2, 0]]: a transpose would show
    view = _single(M, Ht, Wt, H, W, shift=(0.5, -0.25))
    o, Minv = view.theta[0, :, 2], np.linalg.inv(M)
    target, vis = impl.flow(flow, view, (H, W))
    qy, qx = np.mgrid[0:H, 0:W].astype(np.float64)
    p = np.stack([M[0, 0] * qx + M[0, 1] * qy + o[0], M[1, 0] * qx + M[1, 1] * qy + o[1]], -1)
    assert (p[..., 0] >= 0).all() and (p[..., 0] <= Wt - 1).all() and (p[..., 1] >= 0).all() and (p[..., 1] <= Ht - 1).all()
    want = (p @ G.T + g) @ Minv.T
    assert vis.all()
    np.testing.assert_array_equal(target[0].astype(np.float64), want)
    for wrong in ((p @ G.T + g) @ Minv, (p @ G.T + g) @ M.T, (p[..., ::-1] @ G.T + g) @ Minv.T):
        assert np.abs(wrong - want).max() > 0.1                                # a transposed matrix, M for Minv, a swapped offset


def dependants(view, Ht, Wt, size, ty, tx):
    """The student pixels with a tap of nonzero weight on teacher pixel (ty, tx), from the float32 records."""
    H, W = size
    inn, y0, y1, x0, x1, a, b = _taps(*_coords32(records_of(view)[0], H, W), Ht, Wt)
    inn, y0, y1, x0, x1, a, b = (np.broadcast_to(v, (H, W)) for v in (inn, y0, y1, x0, x1, a, b))
    hit = ((y0 == ty) & (x0 == tx)) | ((y0 == ty) & (x1 == tx) & (a != 0)) | ((y1 == ty) & (x0 == tx) & (b != 0)) \
        | ((y1 == ty) & (x1 == tx) & (a != 0) & (b != 0))
    return hit & inn


def check_one_zero_and_one_nan(impl):
    Ht, Wt, size = 16, 24, (12, 14)
    rng = np.random.default_rng(5)
    flow = rng.normal(0, 2, (1, Ht, Wt, 2)).astype(np.float32)
    for M, shift in ((np.eye(2), (0.0, 0.0)), (np.eye(2), (0.5, 0.0)), (0.75 * np.eye(2), (0.25, -0.5)), ([[0.0, -1.0], [1.0, 0.0]], (0.0, 0.0))):
        view = _single(M, Ht, Wt, *size, shift=shift)
        hit = dependants(view, Ht, Wt, size, 8, 11)
        assert 1 <= hit.sum() <= 9
        base_t, base_v = impl.flow(flow, view, size)
        assert base_v.all()
        tv = np.ones((1, Ht, Wt), np.uint8)
        tv[0, 8, 11] = 0
        target, vis = impl.flow(flow, view, size, tv)
        np.testing.assert_array_equal(vis[0] == 0, hit)
        np.testing.assert_array_equal(target[0][~hit], base_t[0][~hit])
        assert not target[0][hit].any()
        for bad in ((np.nan, 1.0), (1.0, np.inf), (-np.inf, np.nan)):
            poisoned = flow.copy()
            poisoned[0, 8, 11] = bad
            target, vis = impl.flow(poisoned, view, size)
            np.testing.assert_array_equal(vis[0] == 0, hit)
            np.testing.assert_array_equal(target[0][~hit], base_t[0][~hit])
            assert not target[0][hit].any() and np.isfinite(target).all()


def check_out_of_frame_is_zero(impl):
    geom = GEOMS[3]
    for kind in ('identity', 'scale2', 'generic'):
        frames, flow, tv, view = view_case((geom, kind))
        size = geom[1][1:]
        inside = frames_f64(frames, view, size)[1]
        near = band_of(view.theta[0], *size, *geom[0][1:])[None] if kind == 'generic' else np.zeros_like(inside)
        outside = ~inside & ~near
        assert 0.1 < outside.mean() < 0.95
        assert not impl.frames(frames, view, size)[outside].any()
        target, vis = impl.flow(flow, view, size)
        assert not vis[outside].any() and not target[outside].any()
        assert vis[inside & ~near].all()


@pytest.mark.parametrize('geom', GEOMS, ids=[case_id((g, ''))[:-1] for g in GEOMS])
def test_the_identity_view_is_the_window(geom):
    check_identity_is_the_window(Restatement, geom)


def test_a_constant_teacher_is_mapped_as_a_vector():
    check_constant_teacher(Restatement)


def test_an_affine_teacher_gives_the_closed_form():
    check_affine_teacher(Restatement)


def test_one_untrusted_or_non_finite_teacher_pixel_clears_exactly_its_dependants():
    check_one_zero_and_one_nan(Restatement)


def test_out_of_frame_student_pixels_are_zero_and_not_visible():
    check_out_of_frame_is_zero(Restatement)


def test_the_colour_map_reaches_both_ends_of_the_clamp():
    case = (GEOMS[2], 'colour')
    frames, _, _, view = view_case(case)
    out = np_view_frames(frames, records_of(view), GEOMS[2][1][1:])
    assert (out == 0).mean() > 0.01 and (out == 255).mean() > 0.01 and ((out > 0) & (out < 255)).mean() > 0.5
    assert out.min() == 0.0 and out.max() == 255.0


# ------------------------------------------------------------------ equivariance (float64)
EQUIVARIANCE_BOUND = 0.02


def test_view_of_the_warp_is_the_warp_of_the_views():
    """``warp(view(frame2), view_flow(f))`` against ``view(warp(frame2, f))`` in float64 on smooth analytic frames (periods of 40
    pixels and more, amplitude 1) under the generic view, on the pixels that are in frame for both.  The two differ by bilinear
    interpolation error only (the frame is interpolated twice on one side, the flow once on the other).  Measured here: 4.1e-3;
    the bound is five times that, 0.02.  M used for Minv gives 0.096, no mapping of the vector or a wrong sign far more.  (The
    generic M is a rotation times a mirror, a symmetric matrix: its transpose cannot show here, the affine teacher's does.)"""
    Ht, Wt, H, W = 64, 96, 48, 64
    ys, xs = np.mgrid[0:Ht, 0:Wt].astype(np.float64)
    frame2 = (np.sin(xs / 7.0 + 0.3) * np.cos(ys / 9.0) + 0.5 * np.sin((xs + ys) / 11.0))[None, ..., None]
    flow = np.stack([2.0 + 1.5 * np.sin(ys / 13.0), -1.0 + 1.2 * np.cos(xs / 15.0)], -1)[None]
    view = make_view((((1, Ht, Wt), (1, H, W)), 'generic'))

    def warp(frame, f):
        h, w = frame.shape[1:3]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        v, inn = sample64(frame[0], xx + f[0, ..., 0], yy + f[0, ..., 1])
        return v[None], inn[None]

    def run(view_flow):
        student2, in2 = frames_f64(frame2, view, (H, W))
        target, vis = view_flow(flow, None, view, (H, W))
        left, in_l = warp(student2, target)
        warped, in_w = warp(frame2, flow)
        right, in_r = frames_f64(warped, view, (H, W))
        # in frame for both: the student pixel, its end point in the student, and (right side) the teacher pixel's end point
        px, py = coords64(view.theta[0], H, W)
        ok = vis & in_l & in_r & in2
        ok[0] &= sample64(in_w[0][..., None].astype(np.float64), px, py)[0][..., 0] == 1.0
        return float(np.abs(left - right)[ok].max()), float(ok.mean())

    diff, share = run(flow_f64)
    inv = view.inverse()[0]

    def wrong(matrix):
        def view_flow(f, tv, v, size):
            t, vis = flow_f64(f, tv, v, size)
            return (t @ np.linalg.inv(inv.T)) @ matrix.T, vis          # undo Minv, apply another matrix
        return run(view_flow)[0]
    bad = [wrong(np.eye(2)), wrong(view.matrix()[0]), wrong(-inv)]
    report('student view equivariance', difference=diff, share_compared=share, unmapped=bad[0], m_for_minv=bad[1], sign=bad[2])
    assert share > 0.5
    assert diff <= EQUIVARIANCE_BOUND
    assert min(bad) > 4 * EQUIVARIANCE_BOUND


# ------------------------------------------------------------------ the host side: views and draws
def test_student_view_holds_float64_and_rounds_once():
    view = StudentView.identity(3, (8, 16))
    assert len(view) == 3 and view.theta.dtype == np.float64 and view.gain is None
    np.testing.assert_array_equal(view.theta[1], [[1, 0, 16], [0, 1, 8]])
    recs = view.records()
    assert len(recs) == 3 and len(view.records(doubled=True)) == 6
    r = recs[2]
    assert (list(r.m), list(r.o), list(r.inv), r.colour) == ([1, 0, 0, 1], [16, 8], [1, 0, 0, 1], 0)
    th = np.array([[[0.8, -0.1, 3.3], [0.1, 0.8, -1.7]]])
    gain, bias = np.array([[[1.1, 1.2, 1.3], [0.7, 0.8, 0.9]]]), np.array([[[1.0, 2.0, 3.0], [-1.0, -2.0, -3.0]]])
    view = StudentView(th, gain, bias)
    np.testing.assert_allclose(view.inverse()[0] @ view.matrix()[0], np.eye(2), atol=1e-15)
    r0, r1 = view.records(doubled=True)
    assert list(r0.m) == [float(np.float32(v)) for v in (0.8, -0.1, 0.1, 0.8)] == list(r1.m)
    assert list(r0.inv) == [float(np.float32(v)) for v in np.linalg.inv(th[0, :, :2]).reshape(-1)]
    assert list(r0.gain) == [float(np.float32(v)) for v in gain[0, 0]] and list(r1.gain) == [float(np.float32(v)) for v in gain[0, 1]]
    assert list(r0.bias) == [1.0, 2.0, 3.0] and list(r1.bias) == [-1.0, -2.0, -3.0] and r0.colour == r1.colour == 1
    for bad in (dict(theta=np.zeros((2, 3))), dict(theta=np.zeros((1, 2, 3))), dict(theta=np.full((1, 2, 3), np.nan)),
                dict(theta=th, gain=gain), dict(theta=th, gain=gain[:, :1], bias=bias[:, :1]), dict(theta=th, gain=gain * np.inf, bias=bias)):
        with pytest.raises(ValueError):
            StudentView(**bad)


def test_the_default_transform_draws_the_identity():
    before = np.random.get_state()[1].copy()
    view = StudentTransform().draw(3, (80, 112), (64, 96))
    ident = StudentView.identity(3, (8, 8))
    assert view.theta.tobytes() == ident.theta.tobytes() and view.gain is None and view.bias is None      # (no negative zeros either)
    assert not np.array_equal(np.random.get_state()[1], before)               # it draws from np.random, as FlowAugmentor does
    assert bytes(view.records(doubled=True)) == bytes(ident.records(doubled=True))


GENERIC_DRAW = dict(flip_x=0.5, flip_y=0.5, zoom=(0.9, 1.3), rotate=10.0, gain=(0.8, 1.2), bias=(-10.0, 10.0), asymmetric=0.5)


def test_the_draw_order_is_the_documented_one_and_reproducible():
    a = StudentTransform(rng=np.random.RandomState(7), **GENERIC_DRAW).draw(8, (80, 112), (64, 96))
    b = StudentTransform(rng=np.random.RandomState(7), **GENERIC_DRAW).draw(8, (80, 112), (64, 96))
    assert a.theta.tobytes() == b.theta.tobytes() and a.gain.tobytes() == b.gain.tobytes() and a.bias.tobytes() == b.bias.tobytes()
    rng = np.random.RandomState(7)                                           # the documented order, replayed by hand
    ct, cs = np.array([55.5, 39.5]), np.array([47.5, 31.5])
    some_asymmetric = some_shared = False
    for n in range(8):
        fx = -1.0 if rng.rand() < 0.5 else 1.0
        fy = -1.0 if rng.rand() < 0.5 else 1.0
        s = rng.uniform(0.9, 1.3)
        t = np.deg2rad(rng.uniform(-10.0, 10.0))
        M = np.array([[np.cos(t) * fx, -np.sin(t) * fy], [np.sin(t) * fx, np.cos(t) * fy]]) / s
        slack = np.maximum(ct - np.abs(M) @ cs, 0.0)
        shift = (2.0 * np.array([rng.rand(), rng.rand()]) - 1.0) * slack
        np.testing.assert_allclose(a.theta[n, :, :2], M, atol=1e-15)
        np.testing.assert_allclose(a.theta[n, :, 2], ct + shift - M @ cs, atol=1e-12)
        g1, b1 = rng.uniform(0.8, 1.2), rng.uniform(-10.0, 10.0)
        g2, b2 = (rng.uniform(0.8, 1.2), rng.uniform(-10.0, 10.0)) if rng.rand() < 0.5 else (g1, b1)
        some_asymmetric |= g2 != g1
        some_shared |= g2 == g1
        assert (a.gain[n] == [[g1] * 3, [g2] * 3]).all() and (a.bias[n] == [[b1] * 3, [b2] * 3]).all()
        assert abs(np.linalg.det(M)) == pytest.approx(1 / s ** 2)
    assert some_asymmetric and some_shared
    np.testing.assert_allclose(a.inverse() @ a.matrix(), np.tile(np.eye(2), (8, 1, 1)), atol=4e-16)
    # the global generator when rng is None
    np.random.seed(11)
    c = StudentTransform(**GENERIC_DRAW).draw(2, (80, 112), (64, 96))
    d = StudentTransform(rng=np.random.RandomState(11), **GENERIC_DRAW).draw(2, (80, 112), (64, 96))
    assert c.theta.tobytes() == d.theta.tobytes()


def test_translate_keeps_the_corners_inside_whenever_there_is_slack():
    H, W, Hs, Ws = 80, 112, 48, 64
    tr = StudentTransform(flip_x=0.5, zoom=(1.0, 1.4), rotate=12.0, rng=np.random.RandomState(3))
    views = tr.draw(200, (H, W), (Hs, Ws))
    corners = np.array([[0, 0], [Ws - 1, 0], [0, Hs - 1], [Ws - 1, Hs - 1]], np.float64)
    moved = 0
    for th in views.theta:
        p = corners @ th[:, :2].T + th[:, 2]
        assert (p[:, 0] >= -1e-9).all() and (p[:, 0] <= W - 1 + 1e-9).all() and (p[:, 1] >= -1e-9).all() and (p[:, 1] <= H - 1 + 1e-9).all()
        centre = th[:, :2] @ np.array([(Ws - 1) / 2, (Hs - 1) / 2]) + th[:, 2]
        moved += bool(np.abs(centre - [(W - 1) / 2, (H - 1) / 2]).max() > 0.5)
    assert moved > 100
    # no slack: the view is centred, whatever the draws
    tight = StudentTransform(zoom=(0.5, 0.6), rng=np.random.RandomState(3)).draw(5, (H, W), (72, 104))
    for th in tight.theta:
        np.testing.assert_allclose(th[:, :2] @ np.array([51.5, 35.5]) + th[:, 2], [55.5, 39.5], atol=1e-12)
    still = StudentTransform(zoom=(1.0, 1.4), rotate=12.0, translate=False, rng=np.random.RandomState(3)).draw(5, (H, W), (Hs, Ws))
    for th in still.theta:
        np.testing.assert_allclose(th[:, :2] @ np.array([(Ws - 1) / 2, (Hs - 1) / 2]) + th[:, 2], [55.5, 39.5], atol=1e-12)
    for kw in (dict(flip_x=1.5), dict(flip_y=-0.1), dict(zoom=(0.0, 1.0)), dict(zoom=(1.2, 1.0)), dict(zoom=1.0), dict(rotate=-1.0),
               dict(rotate=float('nan')), dict(translate=1), dict(gain=(1.0,)), dict(bias=(0.0, float('inf'))), dict(asymmetric=2)):
        with pytest.raises(ValueError):
            StudentTransform(**kw)


# ------------------------------------------------------------------ the C entries
def test_the_header_declares_and_the_library_exports_the_entries():
    with open(os.path.join(ROOT, 'include', 'raft_hip.h')) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    assert re.search(r'int\s+raft_view_params_bytes\s*\(\s*void\s*\)', header)
    body = re.search(r'typedef struct \{([^{}]*)\} RaftViewParams;', header).group(1)
    fields = [re.sub(r'\[.*?\]|\s', '', n) for decl in body.split(';') if decl.strip() for n in decl.split(None, 1)[1].split(',')]
    assert fields == [f[0] for f in _ffi.ViewParams._fields_] == ['m', 'o', 'inv', 'gain', 'bias', 'colour']
    sigs = _ffi.header_signatures(header)
    P, I = C.c_void_p, C.c_int
    assert sigs['raft_view_params_bytes'] == (I, [])
    assert sigs['raft_view_frames_f32'] == (I, [P, P, P, I, I, I, I, I, I, P])
    assert sigs['raft_view_flow_f32'] == (I, [P, P, P, P, P, I, I, I, I, I, P])
    assert _ffi.ABI_VERSION == 222                                   # entries and one record type were added, no signature changed
    lib = _ffi.load_library()                                        # (runs the record's size check)
    assert lib.raft_view_params_bytes() == C.sizeof(_ffi.ViewParams) == 68
    assert len(lib.raft_view_frames_f32.argtypes) == 10 and len(lib.raft_view_flow_f32.argtypes) == 11
    with open(os.path.join(ROOT, 'tf_raft_amd', 'build.py')) as f:
        assert "'student_view.hip'" in f.read()


def test_argument_errors_are_returned_in_the_stated_order_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off = C.c_void_p(p.value + 4)

    def caller(fn, good):
        def call(**changes):
            args = list(good)
            for k, v in changes.items():
                args[int(k[1:])] = v
            return fn(*args)
        return call
    # 0 src 1 params 2 dst 3 B 4 Ht 5 Wt 6 H 7 W 8 C 9 stream
    frames = caller(lib.raft_view_frames_f32, [p, p, p, 1, 6, 8, 4, 5, 3, None])
    for k in (0, 1, 2):
        assert frames(**{f'a{k}': None}) == -1, k
    assert frames() > 0                                                       # past the checks: the launch fails without a device
    for k in (3, 4, 5, 6, 7, 8):
        for v in (0, -3):
            assert frames(**{f'a{k}': v}) == -2, (k, v)
    assert frames(a4=1 << 15, a5=1 << 15) == -2                               # B*Ht*Wt*C reaches 2^31
    assert frames(a6=1 << 15, a7=1 << 15) == -2                               # B*H*W*C reaches 2^31
    assert frames(a6=8 * 65535 + 1, a7=1, a8=1) == -2                         # more rows of tiles than a grid axis holds
    assert frames(a0=off, a2=off) > 0                                         # floats need no 8-byte alignment
    assert frames(a6=40, a7=50) > 0                                           # the student may be larger than the teacher
    assert frames(a0=None, a3=0) == -1                                        # precedence: NULL before shape
    # 0 flow 1 teacher_visible 2 params 3 target 4 target_visible 5 B 6 Ht 7 Wt 8 H 9 W 10 stream
    flow = caller(lib.raft_view_flow_f32, [p, p, p, p, p, 1, 6, 8, 4, 5, None])
    for k in (0, 2, 3, 4):
        assert flow(**{f'a{k}': None}) == -1, k
    assert flow(a1=None) > 0                                                  # (the mask may be NULL)
    for k in (5, 6, 7, 8, 9):
        for v in (0, -3):
            assert flow(**{f'a{k}': v}) == -2, (k, v)
    assert flow(a6=1 << 15, a7=1 << 15) == -2 and flow(a8=1 << 15, a9=1 << 15) == -2
    for k in (0, 3):
        assert flow(**{f'a{k}': off}) == -4, k
    assert flow(a1=off, a2=off, a4=off) > 0                                   # bytes and records need no 8-byte alignment
    assert flow(a8=40, a9=50) > 0
    # precedence: NULL, then shape, then alignment
    assert flow(a0=None, a5=0, a3=off) == -1
    assert flow(a5=0, a3=off) == -2
    assert flow(a3=off) == -4


# ------------------------------------------------------------------ the Python layers, nothing reaches the device
def test_the_python_ops_check_shapes_and_records_before_anything_moves():
    from tf_raft_amd import image_ops
    frames, flow = np.zeros((2, 9, 11, 3), np.float32), np.zeros((2, 9, 11, 2), np.float32)
    view = StudentView.identity(2, (1, 1))
    assert len(image_ops.view_host_records(view, 2)) == 2 * 68 and len(image_ops.view_host_records(view, 4)) == 4 * 68
    huge = StudentView(np.array([[[1e39, 0.0, 0.0], [0.0, 1.0, 0.0]]] * 2))      # finite in float64, infinite in the float32 record
    for kw in (dict(images=frames[0]), dict(views=StudentView.identity(3, (1, 1))), dict(views=[1, 2]), dict(views=None),
               dict(views=huge), dict(size=(7,)), dict(size=(7, 0)), dict(size=(7.0, 9)), dict(size=(True, 9)), dict(size=7)):
        with pytest.raises(ValueError):
            image_ops.view_frames(**dict(dict(images=frames, views=view, size=(7, 9)), **kw))
    with pytest.raises(TypeError):
        image_ops.view_frames(frames.astype(np.uint8), view, (7, 9))
    for kw in (dict(flow=frames), dict(flow=flow[0]), dict(views=StudentView.identity(3, (1, 1))), dict(size=(0, 9)),
               dict(visible=np.zeros((2, 7, 9), np.uint8)), dict(views=huge)):
        with pytest.raises(ValueError):
            image_ops.view_flow(**dict(dict(flow=flow, views=view, size=(7, 9)), **kw))
    with pytest.raises(TypeError):
        image_ops.view_flow(flow.astype(np.float16), view, (7, 9))


def test_compile_validates_the_transform():
    import inspect
    from tf_raft_amd import losses
    from tf_raft_amd.model import RAFT, SmallRAFT
    assert inspect.signature(RAFT.compile).parameters['selfsup_transform'].default is None
    ph = losses.PhotometricSequenceLoss
    for cls in (RAFT, SmallRAFT):
        model = cls.__new__(cls)
        with pytest.raises(ValueError, match='selfsup_crop'):
            model.compile(optimizer=None, loss=ph(), bidirectional=True, selfsup_transform=StudentTransform())
        for bad in (object(), 3, 'flip'):
            with pytest.raises(ValueError, match='selfsup_transform'):
                model.compile(optimizer=None, loss=ph(), bidirectional=True, selfsup_crop=(8, 8), selfsup_transform=bad)
        tr = StudentTransform(flip_x=0.5)
        model.compile(optimizer=None, loss=ph(), bidirectional=True, selfsup_crop=(8, 8), selfsup_transform=tr)
        assert model.selfsup_transform is tr and model.last_student_view is None
        assert model._unlabelled_keys() == ('loss', 'photometric', 'smoothness', 'occluded', 'selfsup', 'selfsup_used')
        fixed = lambda N, frame, student: StudentView.identity(N, (8, 8))      # noqa: E731  (a callable with draw's signature)
        model.compile(optimizer=None, loss=ph(), bidirectional=True, selfsup_crop=(8, 8), selfsup_transform=fixed)
        assert model.selfsup_transform is fixed
        model.compile(optimizer=None, loss=ph(), bidirectional=True, selfsup_crop=(8, 8))
        assert model.selfsup_transform is None and model.last_student_view is None

"""The camera's motion from a flow, host side (no GPU): the float64 NumPy restatements ``np_fit_motion`` and
``np_residual`` of csrc/flow_motion.hip with their known answers, the inputs tests/test_gpu_flow_motion.py runs and what they
exercise, the condition that lets the GPU comparison be stated in float32 units, ``video.smooth_trajectory``, the C entries'
declarations and argument checks, and the errors of the Python layer.

The fit, per slice of a flow (N, H, W, 2): a pixel is USED iff both components of its vector are finite and its mask byte admits it
(no mask; ``mask_invert == 0`` and the byte nonzero; ``mask_invert == 1`` and the byte zero).  With ``X = x - (W - 1) / 2``, ``Y = y -
(H - 1) / 2`` the displacement field ``d(X, Y) = L (X, Y) + t`` is fitted by iteratively reweighted least squares, all in float64
with every operation rounded on its own: solve 1 weights every used pixel 1, solve k > 1 weights it ``1 / (1 + r2 / scale^2)``,
evaluated with one division as ``s2 / (s2 + r2)``, with ``r2`` its squared residual under solve k - 1.  The kernel and the
restatement differ in ONE thing, the order in which the twelve sums of a solve are added up; ``np_fit_motion`` has a switch for that order, and the condition test below shows that on these
inputs the order moves no result by more than 2^-30 of its size, a million times less than a float32 ulp.

On the statuses: 0 = the model asked for was fitted, 1 = its normal equations had no rank and the translation took its place, 2 =
nothing to fit.  A translation has no rank to lose, so status 1 cannot occur for model 0 under the rule as DESIGN.md states it; the
coverage test asks for 0 and 2 there and for all three of the other two models.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tf_raft_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ('translation', 'similarity', 'affine')
RECORD_CAP, THREADS = 256, 256             # csrc/flow_motion.hip kMotionRecords, kMotionThreads
ORDERS = ('pairwise', 'fsum', 'reversed')

# (N, H, W): what tests/test_gpu_flow_motion.py runs.  The last two have more pixels per slice than a slice's records have threads:
# 300 x 450 is even, so a thread takes two pixels per trip and needs more than 2 * 256 * RECORD_CAP of them; 257 x 263 is odd (one
# pixel per trip, odd slice offsets).
SHAPES = [(1, 1, 1), (1, 1, 9), (1, 5, 1), (2, 2, 13), (3, 37, 53), (1, 64, 96), (1, 300, 450), (2, 257, 263)]
IDS = ['x'.join(map(str, s)) for s in SHAPES]
MASKS = ('none', 'random', 'slice_unused', 'one_pixel')
ZOOM, ANGLE, SHIFT, NOISE, BLOCK_MOVE = 1.02, math.radians(1.0), (3.0, -2.0), 0.05, (8.0, 5.0)


# ------------------------------------------------------------------ the restatements
def _total(values, order):
    """One sum of float64 ``values`` in row-major pixel order, added up in the given order."""
    if order == 'pairwise':
        return float(np.sum(values))
    if order == 'fsum':
        return math.fsum(values.tolist())
    assert order == 'reversed'
    return float(np.cumsum(values[::-1])[-1]) if len(values) else 0.0     # (cumsum adds one after the other)


def np_solve(S, model, stuck):
    """The solve kernel on the twelve sums, Python floats (IEEE float64, nothing fused): (l00, l01, l10, l11, tx, ty, status)."""
    Sw, SwX, SwY, SwXX, SwXY, SwYY, Swu, SwXu, SwYu, Swv, SwXv, SwYv = S
    if stuck or not Sw > 0.0:
        return (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2)
    mX, mY, mu, mv = SwX / Sw, SwY / Sw, Swu / Sw, Swv / Sw
    pX, pY = Sw * mX, Sw * mY
    cxx, cxy, cyy = SwXX - pX * mX, SwXY - pX * mY, SwYY - pY * mY
    bxu, byu, bxv, byv = SwXu - pX * mu, SwYu - pY * mu, SwXv - pX * mv, SwYv - pY * mv
    l00 = l01 = l10 = l11 = 0.0
    full = model == 0
    if model == 2:
        D, m = cxx * cyy - cxy * cxy, max(cxx, cyy)
        if D > 1e-12 * (m * m):
            full = True
            l00, l01 = (bxu * cyy - byu * cxy) / D, (byu * cxx - bxu * cxy) / D
            l10, l11 = (bxv * cyy - byv * cxy) / D, (byv * cxx - bxv * cxy) / D
    elif model == 1:
        q = cxx + cyy
        if q > 0.0:
            full = True
            a, b = (bxu + byv) / q, (bxv - byu) / q
            l00, l01, l10, l11 = a, -b, b, a
    if full:
        return (l00, l01, l10, l11, mu - (l00 * mX + l01 * mY), mv - (l10 * mX + l11 * mY), 0)
    return (0.0, 0.0, 0.0, 0.0, mu, mv, 1)


def _residual2(e, X, Y, u, v):
    ru = u - ((e[0] * X + e[1] * Y) + e[4])
    rv = v - ((e[2] * X + e[3] * Y) + e[5])
    return ru * ru + rv * rv


def np_fit_motion(flow, mask=None, mask_invert=0, model=2, iterations=5, scale=1.0, order='pairwise'):
    """csrc/flow_motion.hip's fit restated: flow (N, H, W, 2) float32, mask uint8 (N, H, W) or None -> a dict with ``motion``
    (N, 2, 3) and ``stats`` (N, 4) as float32, the same before their one rounding (``motion64``, ``stats64``), the float64 estimates
    ``est`` (N, 6) in centred coordinates and ``first`` (N, 6), the estimate of solve 1."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 4 and flow.shape[-1] == 2 and model in (0, 1, 2) and 1 <= iterations <= 32
    N, H, W, _ = flow.shape
    s2 = float(np.float32(scale)) * float(np.float32(scale))
    cx, cy = (W - 1) * 0.5, (H - 1) * 0.5
    ys, xs = np.mgrid[0:H, 0:W]
    out = {k: np.zeros((N,) + s, np.float64) for k, s in (('motion64', (2, 3)), ('stats64', (4,)), ('est', (6,)), ('first', (6,)))}
    for n in range(N):
        u, v = flow[n, ..., 0], flow[n, ..., 1]
        used = np.isfinite(u) & np.isfinite(v)
        if mask is not None:
            used &= (mask[n] == 0) if mask_invert else (mask[n] != 0)
        X, Y = (xs[used] - cx).astype(np.float64), (ys[used] - cy).astype(np.float64)
        u, v = u[used].astype(np.float64), v[used].astype(np.float64)
        e = None
        for k in range(iterations):
            w = np.ones_like(X) if k == 0 else s2 / (s2 + _residual2(e, X, Y, u, v))
            wX, wY = w * X, w * Y
            S = [_total(t, order) for t in (w, wX, wY, wX * X, wX * Y, wY * Y, w * u, wX * u, wY * u, w * v, wX * v, wY * v)]
            e = np_solve(S, model, e is not None and e[6] == 2)
            if k == 0:
                out['first'][n] = e[:6]
        r2 = _residual2(e, X, Y, u, v)
        w = s2 / (s2 + r2)
        count, Sw, Swr2 = _total(np.ones_like(X), order), _total(w, order), _total(w * r2, order)
        if count > 0.0:
            with np.errstate(invalid='ignore', divide='ignore'):
                out['stats64'][n, :3] = count / (float(H) * float(W)), Sw / count, np.sqrt(np.float64(Swr2) / np.float64(Sw))
        out['stats64'][n, 3] = e[6]
        out['est'][n] = e[:6]
        out['motion64'][n] = [[1.0 + e[0], e[1], e[4] - (e[0] * cx + e[1] * cy)], [e[2], 1.0 + e[3], e[5] - (e[2] * cx + e[3] * cy)]]
    out['motion'], out['stats'] = out['motion64'].astype(np.float32), out['stats64'].astype(np.float32)
    return out


def np_motion_flow(motion, H, W):
    """The dense flow of motions (N, 2, 3) float32 as float64 (N, H, W, 2): ((m0 * x + m1 * y) + m2) - x, likewise for y."""
    m = np.asarray(motion)
    assert m.dtype == np.float32 and m.shape[1:] == (2, 3)
    m = m.astype(np.float64)[:, None, None]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        gu = ((m[..., 0, 0] * xs + m[..., 0, 1] * ys) + m[..., 0, 2]) - xs
        gv = ((m[..., 1, 0] * xs + m[..., 1, 1] * ys) + m[..., 1, 2]) - ys
    return np.stack([gu, gv], axis=-1)


def np_residual(flow, motion, threshold=None):
    """raft_flow_residual_f32 restated: (residual (N, H, W, 2) float32, moving (N, H, W) uint8 or None)."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32
    with np.errstate(invalid='ignore', over='ignore'):
        r = flow.astype(np.float64) - np_motion_flow(motion, flow.shape[1], flow.shape[2])
        residual = r.astype(np.float32)
        if threshold is None:
            return residual, None
        t = float(np.float32(threshold))
        return residual, (~(r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1] <= t * t)).astype(np.uint8)


def bits(x):
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32
    return x.view(np.uint32)


# ------------------------------------------------------------------ the inputs both test files use
def true_estimate():
    """(L, t) of the test flows in centred coordinates: zoom 1.02, 1 degree, shift (3, -2)."""
    c, s = ZOOM * math.cos(ANGLE), ZOOM * math.sin(ANGLE)
    return np.array([[c - 1.0, -s], [s, c - 1.0]]), np.array(SHIFT)


def motion_flow_field(N, H, W, seed=1, noise=NOISE, block=True, bad=True):
    """(N, H, W, 2) float32: the affine field of ``true_estimate`` plus Gaussian noise; on frames taller than 20 rows a block of about
    a ninth of the frame moves by (8, 5) instead; with at least 26 pixels per slice a few vectors are NaN or infinite."""
    rng = np.random.default_rng(1000 * seed + 31 * H + W)
    L, t = true_estimate()
    ys, xs = np.mgrid[0:H, 0:W]
    X, Y = xs - (W - 1) * 0.5, ys - (H - 1) * 0.5
    flow = np.stack([L[0, 0] * X + L[0, 1] * Y + t[0], L[1, 0] * X + L[1, 1] * Y + t[1]], axis=-1)[None].repeat(N, axis=0)
    flow = flow + rng.normal(0.0, noise, flow.shape) if noise else flow
    if block and H > 20:
        for n in range(N):
            y0, x0 = H // 5 + n, W // 2 - n
            flow[n, y0:y0 + H // 3, x0:x0 + W // 3] = np.array(BLOCK_MOVE) + rng.normal(0.0, noise, (H // 3, W // 3, 2))
    flow = flow.astype(np.float32)
    if bad and H * W >= 26:
        for n in range(N):
            for k, value in enumerate((np.nan, np.inf, -np.inf, np.nan)):
                i = int(rng.integers(0, H * W))
                flow[n].reshape(-1, 2)[i, k % 2] = value
    return flow


def motion_mask(kind, N, H, W, seed=1):
    """uint8 (N, H, W) with nonzero = used (any nonzero byte), or None: 'random' keeps 70 %, 'slice_unused' empties slice 0,
    'one_pixel' keeps exactly one pixel per slice."""
    if kind == 'none':
        return None
    rng = np.random.default_rng(2000 * seed + 17 * H + W)
    keep = rng.random((N, H, W)) < 0.7
    if kind == 'slice_unused':
        keep[0] = False
    elif kind == 'one_pixel':
        keep[:] = False
        for n in range(N):
            keep[n].reshape(-1)[(n * 7 + (H * W) // 2) % (H * W)] = True
    else:
        assert kind == 'random'
    return np.where(keep, rng.integers(1, 256, (N, H, W)), 0).astype(np.uint8)


def inverted(mask):
    """The mask that says the same with mask_invert = 1: zero where ``mask`` is nonzero, some nonzero byte elsewhere."""
    rng = np.random.default_rng(5)
    return np.where(mask != 0, 0, rng.integers(1, 256, mask.shape)).astype(np.uint8)


_CASES, _FITS = {}, {}


def motion_case(shape, kind):
    """The shared input ``(flow, mask)`` of one shape and mask kind, made once and left unchanged."""
    if (shape, kind) not in _CASES:
        flow, mask = motion_flow_field(*shape), motion_mask(kind, *shape)
        for a in (flow, mask):
            if a is not None:
                a.setflags(write=False)
        _CASES[shape, kind] = (flow, mask)
    return _CASES[shape, kind]


def expected_fit(shape, kind, model, iterations, order='pairwise'):
    """``np_fit_motion`` of a shared input at the default scale, computed once and shared between the tests."""
    key = (shape, kind, model, iterations, order)
    if key not in _FITS:
        flow, mask = motion_case(shape, kind)
        _FITS[key] = np_fit_motion(flow, mask, 0, model, iterations, 1.0, order)
        for a in _FITS[key].values():
            a.setflags(write=False)
    return _FITS[key]


# ------------------------------------------------------------------ what the inputs exercise
def test_the_inputs_hit_every_status_of_every_model_and_the_multi_record_case():
    with open(os.path.join(ROOT, 'tf_raft_amd', 'csrc', 'flow_motion.hip')) as f:
        src = f.read()
    assert f'kMotionRecords = {RECORD_CAP};' in src and f'kMotionThreads = {THREADS};' in src
    # a thread takes more than one trip: two pixels per trip on an even slice, one on an odd one
    assert any(h * w % 2 == 0 and h * w > 2 * THREADS * RECORD_CAP for _, h, w in SHAPES)
    assert any(h * w % 2 == 1 and h * w > THREADS * RECORD_CAP for _, h, w in SHAPES)
    assert any(h * w <= THREADS for _, h, w in SHAPES) and any(n > 1 for n, _, _ in SHAPES)
    seen = {m: set() for m in range(3)}
    for shape in SHAPES[:6]:
        for kind in MASKS:
            for model in range(3):
                for iterations in (1, 5):
                    seen[model] |= set(expected_fit(shape, kind, model, iterations)['stats'][:, 3].astype(int).tolist())
    # (a translation has no rank to lose: see the module's docstring)
    assert seen == {0: {0, 2}, 1: {0, 1, 2}, 2: {0, 1, 2}}
    # the unused vectors: NaN and infinities are in the inputs and are left out
    flow, _ = motion_case((3, 37, 53), 'none')
    assert np.isnan(flow).any() and np.isinf(flow).any()
    fit = expected_fit((3, 37, 53), 'none', 2, 5)
    assert (fit['stats'][:, 0] < 1).all() and (fit['stats'][:, 0] > 0.99).all() and np.isfinite(fit['motion']).all()


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_the_order_of_summation_moves_no_result_by_more_than_2_to_the_minus_30(shape):
    """The condition on the inputs: under pairwise, exactly rounded and reversed sequential sums every number the fit returns agrees
    within 2^-30 * max(1, |value|).  (A prototype showed 1e-14.)  It is what lets tests/test_gpu_flow_motion.py state its bounds in
    float32 units: the kernel's order of summation is a fourth one."""
    worst = 0.0
    for kind in MASKS:
        for model in range(3):
            for iterations in (1, 5):
                fits = [expected_fit(shape, kind, model, iterations, order) for order in ORDERS]
                for key in ('motion64', 'stats64', 'est'):
                    ref = fits[0][key]
                    for other in fits[1:]:
                        with np.errstate(invalid='ignore'):
                            err = np.abs(other[key] - ref) / np.maximum(1.0, np.abs(ref))
                        assert np.array_equal(np.isnan(other[key]), np.isnan(ref))
                        worst = max(worst, float(np.nanmax(err)))
                        assert not (err > 2.0 ** -30).any(), (kind, model, iterations, key, float(np.nanmax(err)))
    print(f'summation order {shape}: worst relative difference {worst:.3g}')


# ------------------------------------------------------------------ known answers on the restatement
def test_an_exact_affine_field_is_recovered_by_the_first_solve():
    L, t = true_estimate()
    for H, W in ((37, 53), (64, 96)):
        flow = motion_flow_field(2, H, W, noise=0.0, block=False, bad=False)
        fit = np_fit_motion(flow, None, 0, 2, 1)
        assert (fit['stats'][:, 3] == 0).all()
        # (the flow is float32: about 1e-7 of rounding per vector, averaged over the frame)
        np.testing.assert_allclose(fit['est'][:, :4], np.broadcast_to(L.reshape(4), (2, 4)), atol=1e-8)
        np.testing.assert_allclose(fit['est'][:, 4:], np.broadcast_to(t, (2, 2)), atol=1e-7)
        cx, cy = (W - 1) * 0.5, (H - 1) * 0.5
        want = np.array([[1 + L[0, 0], L[0, 1], t[0] - (L[0, 0] * cx + L[0, 1] * cy)], [L[1, 0], 1 + L[1, 1], t[1] - (L[1, 0] * cx + L[1, 1] * cy)]])
        np.testing.assert_allclose(fit['motion64'][0], want, atol=1e-6)
        sim = np_fit_motion(flow, None, 0, 1, 1)
        np.testing.assert_allclose(sim['est'][:, :4], np.broadcast_to(L.reshape(4), (2, 4)), atol=1e-8)
        # a translation fits the mean vector: the centred coordinates average to zero over a whole frame
        tr = np_fit_motion(flow, None, 0, 0, 1)
        np.testing.assert_allclose(tr['est'][:, 4:], np.broadcast_to(t, (2, 2)), atol=1e-6)
        assert (tr['est'][:, :4] == 0).all()
    zero = np_fit_motion(np.zeros((1, 5, 7, 2), np.float32), None, 0, 2, 5)
    np.testing.assert_array_equal(zero['motion'], np.array([[[1, 0, 0], [0, 1, 0]]], np.float32))
    np.testing.assert_array_equal(zero['stats'], np.array([[1, 1, 0, 0]], np.float32))


# Measured on the restatement at (3, 37, 53), affine, scale 1: the error of the translation in centred coordinates, in pixels, after
# 1 solve (0.875, 0.875, 0.880 for the three slices) and after 5 (0.0153, 0.0125, 0.0126); the noise is 0.05 px per component.
LEAST_SQUARES_ERROR, IRLS_ERROR = 0.875, 0.0153


def test_five_iterations_bring_the_translation_from_the_least_squares_level_to_the_noise_level():
    _, t = true_estimate()
    first = expected_fit((3, 37, 53), 'none', 2, 1)['est'][:, 4:]
    last = expected_fit((3, 37, 53), 'none', 2, 5)['est'][:, 4:]
    e1, e5 = np.linalg.norm(first - t, axis=1), np.linalg.norm(last - t, axis=1)
    print(f'translation error at (37, 53): least squares {e1}, 5 iterations {e5}')
    assert (e1 >=LEAST_SQUARES_ERROR / 2).all() and (e5 <= IRLS_ERROR * 2).all()
    # solve 1 of a longer fit is the one-solve fit, and the block loses its say: the inlier share is about eight ninths
    np.testing.assert_array_equal(expected_fit((3, 37, 53), 'none', 2, 5)['first'], expected_fit((3, 37, 53), 'none', 2, 1)['est'])
    share = expected_fit((3, 37, 53), 'none', 2, 5)['stats'][:, 1]
    assert ((share > 0.8) & (share < 0.95)).all()


def test_the_residual_of_a_fitted_field_marks_the_block():
    flow, _ = motion_case((3, 37, 53), 'none')
    fit = expected_fit((3, 37, 53), 'none', 2, 5)
    residual, moving = np_residual(flow, fit['motion'], 1.0)
    assert residual.dtype == np.float32 and moving.dtype == np.uint8
    H, W = 37, 53
    for n in range(3):
        y0, x0 = H // 5 + n, W // 2 - n
        block = np.zeros((H, W), bool)
        block[y0:y0 + H // 3, x0:x0 + W // 3] = True
        finite = np.isfinite(flow[n]).all(axis=-1)
        assert moving[n][block].all() and not moving[n][~block & finite].any() and moving[n][~finite].all()
    # the motion's own flow has no residual, and np_motion_flow is what the zero flow leaves with the sign turned
    own = np_motion_flow(fit['motion'], H, W).astype(np.float32)
    assert np.abs(np_residual(own, fit['motion'])[0]).max() < 1e-6
    np.testing.assert_array_equal(np_residual(np.zeros_like(own), fit['motion'])[0], -own)


# ------------------------------------------------------------------ the trajectory smoother
def _shift(dx, dy=0.0):
    return np.array([[1.0, 0.0, dx], [0.0, 1.0, dy]])


def test_smooth_trajectory():
    from tf_raft_amd.video import smooth_trajectory
    eye = np.broadcast_to(np.eye(3)[:2], (12, 2, 3))
    # identity motions, and any motions with a window of one frame: identity corrections, exactly
    np.testing.assert_array_equal(smooth_trajectory(eye[:-1], radius=4), eye)
    rng = np.random.default_rng(3)
    wild = eye[:-1] + rng.normal(0, 0.05, (11, 2, 3))
    np.testing.assert_array_equal(smooth_trajectory(wild, radius=0), eye)
    np.testing.assert_array_equal(smooth_trajectory(np.zeros((0, 2, 3))), eye[:1])
    # a constant pan: the mean of a straight line under symmetric weights is the line itself, away from the ends
    pan = np.broadcast_to(_shift(1.5, -0.5), (29, 2, 3))
    got = smooth_trajectory(pan, radius=5)
    assert got.shape == (30, 2, 3) and got.dtype == np.float64
    np.testing.assert_allclose(got[5:-5], np.broadcast_to(np.eye(3)[:2], (20, 2, 3)), atol=1e-12)
    assert abs(got[0, 0, 2]) > 0.5                                             # (at the ends the window is one-sided)
    # alternating jitter of +-2 px: the path is 0, 2, 0, 2, ... = 1 - (-1)^t, and a symmetric window leaves 1 - A (-1)^t with
    # A = sum_k w_k (-1)^k / sum_k w_k, the response of the Gaussian at the highest frequency
    T, radius = 41, 6
    jitter = np.stack([_shift(2.0 if t % 2 == 0 else -2.0) for t in range(T - 1)])
    for sigma in (None, 1.5):
        s = radius / 2 if sigma is None else sigma
        k = np.arange(-radius, radius + 1)
        w = np.exp(-k * k / (2 * s * s))
        A = float((w * (-1.0) ** k).sum() / w.sum())
        assert abs(A) < 0.05
        got = smooth_trajectory(jitter, radius=radius, sigma=sigma)
        t = np.arange(T)
        path = 1.0 - (-1.0) ** t
        steady = path - got[:, 0, 2]                                           # correction = G S^-1: for shifts, G - S
        inner = slice(radius, T - radius)
        np.testing.assert_allclose(steady[inner], (1.0 - A * (-1.0) ** t)[inner], atol=1e-12)
        np.testing.assert_allclose(got[:, :, :2], np.broadcast_to(np.eye(2), (T, 2, 2)), atol=1e-12)
        np.testing.assert_allclose(got[:, 1, 2], 0.0, atol=1e-12)
    # a correction maps the steadied frame to the frame: G_t S_t^-1 with 3 x 3 products, for maps that do not commute
    turn = np.stack([np.array([[math.cos(a), -math.sin(a), 1.0], [math.sin(a), math.cos(a), 0.5 * a]]) for a in rng.normal(0, 0.02, 9)])
    got = smooth_trajectory(turn, radius=2, sigma=1.0)
    G = [np.eye(3)]
    for m in turn:
        G.append(np.vstack([m, [0, 0, 1]]) @ G[-1])
    w = np.exp(-np.arange(-2, 3) ** 2 / 2.0)
    S4 = sum(wk * g for wk, g in zip(w, G[2:7])) / w.sum()
    np.testing.assert_allclose(got[4], (G[4] @ np.linalg.inv(S4))[:2], atol=1e-12)
    for bad in (-1, 1.5, True, None, 'x'):
        with pytest.raises(ValueError, match='radius must'):
            smooth_trajectory(eye, radius=bad)
    for bad in (0, -1.0, float('nan'), float('inf'), True, 'x'):
        with pytest.raises(ValueError, match='sigma must'):
            smooth_trajectory(eye, radius=2, sigma=bad)
    for bad in (np.zeros((2, 3)), np.zeros((4, 3, 3)), np.zeros((4, 2, 2))):
        with pytest.raises(ValueError, match=r'\(T - 1, 2, 3\)'):
            smooth_trajectory(bad)
    with pytest.raises(ValueError, match='finite'):
        smooth_trajectory(np.full((3, 2, 3), np.nan))


# ------------------------------------------------------------------ the C entries
def test_the_header_declares_and_the_library_exports_the_entries():
    from tf_raft_amd import build
    assert 'flow_motion.hip' in build.SOURCES and 'loss_common.h' in build.HEADERS
    with open(os.path.join(ROOT, 'include', 'raft_hip.h')) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    assert re.search(r'int64_t\s+raft_flow_motion_workspace_doubles\s*\(\s*int N,\s*int H,\s*int W\s*\)', header)
    assert re.search(r'int\s+raft_flow_fit_motion_f32\s*\(\s*const float \*flow,\s*const uint8_t \*mask,\s*int mask_invert,\s*float \*motion,'
                     r'\s*float \*stats,\s*int N,\s*int H,\s*int W,\s*int model,\s*int iterations,\s*float scale,\s*double \*workspace,'
                     r'\s*void \*stream\s*\)', header)
    assert re.search(r'int\s+raft_flow_residual_f32\s*\(\s*const float \*flow,\s*const float \*motion,\s*float \*residual,\s*uint8_t \*moving,'
                     r'\s*int N,\s*int H,\s*int W,\s*float threshold,\s*void \*stream\s*\)', header)
    assert re.search(r'int\s+raft_motion_flow_f32\s*\(\s*const float \*motion,\s*float \*flow,\s*int N,\s*int H,\s*int W,\s*void \*stream\s*\)', header)
    sigs = _ffi.header_signatures(header)
    P, I, F = C.c_void_p, C.c_int, C.c_float
    assert sigs['raft_flow_motion_workspace_doubles'] == (C.c_int64, [I, I, I])
    assert sigs['raft_flow_fit_motion_f32'] == (I, [P, P, I, P, P, I, I, I, I, I, F, P, P]) and len(sigs['raft_flow_fit_motion_f32'][1]) == 13
    assert sigs['raft_flow_residual_f32'] == (I, [P, P, P, P, I, I, I, F, P]) and len(sigs['raft_flow_residual_f32'][1]) == 9
    assert sigs['raft_motion_flow_f32'] == (I, [P, P, I, I, I, P]) and len(sigs['raft_motion_flow_f32'][1]) == 6
    assert _ffi.ABI_VERSION == 222                                   # entries were added, no signature changed
    lib = _ffi.load_library()
    assert lib.raft_version() == 222
    for name in ('raft_flow_motion_workspace_doubles', 'raft_flow_fit_motion_f32', 'raft_flow_residual_f32', 'raft_motion_flow_f32'):
        assert getattr(lib, name).argtypes == sigs[name][1], name
    with open(os.path.join(ROOT, 'tf_raft_amd', 'csrc', 'flow_motion.hip')) as f:
        src = f.read()
    assert '#pragma clang fp contract(off)' in src and 'raft_block_sum_store(' in src and 'raft_sum_records(' in src
    code = re.sub(r'//[^\n]*', '', src)
    assert not re.search(r'atomic|hipMemset|Synchronize|cooperative', code)
    # the workspace: the estimates and RECORD_CAP records of twelve doubles per slice; 0 where the sizes are refused
    ws = lib.raft_flow_motion_workspace_doubles
    assert ws(1, 1, 1) == 8 + RECORD_CAP * 12 and ws(4, 1080, 1920) == 4 * (8 + RECORD_CAP * 12)
    for bad in ((0, 4, 5), (1, -1, 5), (1, 4, 0), (1, 1 << 15, 1 << 15), (1 << 16, 1, 1), (65536, 1, 1), (1 << 10, 1 << 10, 1 << 10)):
        assert ws(*bad) == 0, bad
    assert ws(65535, 1, 1) > 0


def test_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off4 = C.c_void_p(p.value + 4)
    nan, inf = float('nan'), float('inf')
    # ---- the fit:  flow mask invert motion stats N H W model iterations scale workspace stream
    fit = lib.raft_flow_fit_motion_f32
    good = [p, p, 0, p, p, 2, 4, 5, 2, 5, 1.0, p, None]
    for k in (0, 3, 4, 11):
        for mask in (p, None):                                      # (the mask may be NULL)
            args = list(good)
            args[k], args[1] = None, mask
            assert fit(*args) == -1, k
    for k, values in ((5, (0, -3, 65536, 1 << 30)), (6, (0, -3)), (7, (0, -3)), (8, (-1, 3)), (9, (0, -1, 33)), (2, (-1, 2)),
                      (10, (0.0, -1.0, nan, inf, -inf, -0.0))):
        for v in values:
            args = list(good)
            args[k] = v
            assert fit(*args) == -2, (k, v)
    for bad in ((1, 1 << 15, 1 << 15), (1 << 10, 1 << 10, 1 << 10), (2, 1 << 29, 1), (1, 1, 1 << 30), (3, 1 << 14, 1 << 15)):
        args = list(good)
        args[5:8] = bad
        assert fit(*args) == -2, bad
    for k in (0, 11):
        args = list(good)
        args[k] = off4
        assert fit(*args) == -4, k
    args = list(good)                                              # precedence: NULL before shape before alignment
    args[4], args[9], args[0] = None, 0, off4
    assert fit(*args) == -1
    args[4] = p
    assert fit(*args) == -2
    args[9], args[10] = 32, nan
    assert fit(*args) == -2
    args[10] = 1e-30
    assert fit(*args) == -4
    # ---- the residual:  flow motion residual moving N H W threshold stream
    res = lib.raft_flow_residual_f32
    good = [p, p, p, p, 2, 4, 5, 1.0, None]
    for k in (0, 1):
        args = list(good)
        args[k] = None
        assert res(*args) == -1, k
    args = list(good)
    args[2] = args[3] = None
    assert res(*args) == -1
    for k in (4, 5, 6):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert res(*args) == -2, (k, v)
    for bad in ((1, 1 << 15, 1 << 15), (1 << 30, 1, 1), (1 << 10, 1 << 10, 1 << 10)):
        args = list(good)
        args[4:7] = bad
        assert res(*args) == -2, bad
    for v in (-1.0, nan, inf, -inf, -2.0 ** -100):
        for moving in (p, None):                                    # (checked with and without the mask)
            args = list(good)
            args[7], args[3] = v, moving
            assert res(*args) == -2, v
    for k in (0, 2):
        args = list(good)
        args[k] = off4
        assert res(*args) == -4, k
    args = list(good)
    args[1], args[5], args[0] = None, 0, off4
    assert res(*args) == -1
    args[1] = p
    assert res(*args) == -2
    args[5], args[7] = 4, nan
    assert res(*args) == -2
    args[7] = 0.0                                                   # (a threshold of 0 is allowed)
    assert res(*args) == -4
    # ---- the dense flow:  motion flow N H W stream
    dense = lib.raft_motion_flow_f32
    good = [p, p, 2, 4, 5, None]
    for k in (0, 1):
        args = list(good)
        args[k] = None
        assert dense(*args) == -1, k
    for k in (2, 3, 4):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert dense(*args) == -2, (k, v)
    args = list(good)
    args[2:5] = (1, 1 << 15, 1 << 15)
    assert dense(*args) == -2
    args = list(good)
    args[1] = off4
    assert dense(*args) == -4
    args[3] = 0
    assert dense(*args) == -2


# ------------------------------------------------------------------ the Python layer, nothing reaches the device
BAD_MODEL = ('homography', 2, None, True, b'affine')
BAD_ITERATIONS = (0, -1, 33, 2.0, True, None, '5')
BAD_SCALE = (0, -1.0, float('nan'), float('inf'), 1e39, 1e-50, True, None, 'x')
BAD_THRESHOLD = (-1.0, float('nan'), float('inf'), 1e39, True, 'x')


def test_shapes_types_and_the_fit_s_arguments_are_checked_without_a_gpu():
    import inspect
    import torch
    from tf_raft_amd import image_ops
    sig = inspect.signature(image_ops.fit_motion).parameters
    assert (sig['model'].default, sig['iterations'].default, sig['scale'].default) == ('affine', 5, 1.0)
    assert sig['mask'].default is None and sig['occluded'].default is None and sig['return_stats'].default is False
    assert image_ops.MOTION_MODELS == MODELS
    flow = np.zeros((2, 4, 5, 2), np.float32)
    mask = np.ones((2, 4, 5), np.uint8)
    motion = np.zeros((2, 2, 3), np.float32)
    for bad in BAD_MODEL:
        with pytest.raises(ValueError, match='model must'):
            image_ops.fit_motion(flow, model=bad)
    for bad in BAD_ITERATIONS:
        with pytest.raises(ValueError, match='iterations must'):
            image_ops.fit_motion(flow, iterations=bad)
    for bad in BAD_SCALE:
        with pytest.raises(ValueError, match='scale must'):
            image_ops.fit_motion(flow, scale=bad)
    with pytest.raises(ValueError, match=r'flow \(\.\.\., H, W, 2\)'):
        image_ops.fit_motion(flow[0, 0])
    with pytest.raises(ValueError, match=r'flow \(\.\.\., H, W, 2\)'):
        image_ops.fit_motion(flow[..., :1])
    with pytest.raises(ValueError, match='empty'):
        image_ops.fit_motion(flow[:, :0])
    with pytest.raises(TypeError, match='a flow is float32'):
        image_ops.fit_motion(flow.astype(np.uint8))
    with pytest.raises(TypeError):
        image_ops.fit_motion(flow.astype(np.int32))
    with pytest.raises(ValueError, match='not both'):
        image_ops.fit_motion(flow, mask=mask, occluded=mask)
    for kw in ('mask', 'occluded'):
        with pytest.raises(ValueError, match='expects a mask'):
            image_ops.fit_motion(flow, **{kw: mask[0]})
        with pytest.raises(TypeError, match='a mask is uint8 or bool'):
            image_ops.fit_motion(flow, **{kw: mask.astype(np.float32)})
    with pytest.raises(ValueError, match='too large'):
        image_ops.fit_motion(torch.empty((1, 1 << 15, 1 << 15, 2), dtype=torch.float32, device='meta'))
    with pytest.raises(ValueError, match='too large'):
        image_ops.fit_motion(torch.empty((65536, 1, 1, 2), dtype=torch.float32, device='meta'))
    # the residual and the dense flow
    for bad in BAD_THRESHOLD:
        with pytest.raises(ValueError, match='threshold must'):
            image_ops.residual_flow(flow, motion, threshold=bad)
    with pytest.raises(ValueError, match=r'flow \(\.\.\., H, W, 2\)'):
        image_ops.residual_flow(flow[0, 0], motion)
    with pytest.raises(TypeError, match='a flow is float32'):
        image_ops.residual_flow(flow.astype(np.uint8), motion)
    with pytest.raises(ValueError, match='expects motions'):
        image_ops.residual_flow(flow, motion[0])
    with pytest.raises(ValueError, match='expects motions'):
        image_ops.residual_flow(flow[0], motion)
    with pytest.raises(ValueError, match='expects motions'):
        image_ops.residual_flow(flow, np.zeros((2, 3, 3), np.float32))
    with pytest.raises(TypeError, match='a motion is float32'):
        image_ops.residual_flow(flow, motion.astype(np.uint8))
    with pytest.raises(ValueError, match='too large'):
        image_ops.residual_flow(torch.empty((1, 1 << 15, 1 << 15, 2), dtype=torch.float32, device='meta'),
                                torch.empty((1, 2, 3), dtype=torch.float32, device='meta'))
    with pytest.raises(ValueError, match=r'motions \(\.\.\., 2, 3\)'):
        image_ops.motion_flow(np.zeros((2, 3, 2), np.float32), 4, 5)
    with pytest.raises(ValueError, match=r'motions \(\.\.\., 2, 3\)'):
        image_ops.motion_flow(np.zeros((3,), np.float32), 4, 5)
    with pytest.raises(TypeError, match='a motion is float32'):
        image_ops.motion_flow(motion.astype(np.uint8), 4, 5)
    for bad in ((0, 5), (4, -1), (4.0, 5), (True, 5)):
        with pytest.raises(ValueError, match='size must'):
            image_ops.motion_flow(motion, *bad)
    with pytest.raises(ValueError, match='too large'):
        image_ops.motion_flow(motion, 1 << 15, 1 << 15)
    # the launch forms check what they are handed, too
    df, dm, dk = torch.zeros((2, 4, 5, 2)), torch.zeros((2, 2, 3)), torch.ones((2, 4, 5), dtype=torch.uint8)
    with pytest.raises(ValueError, match='model must'):
        image_ops.fit_motion_launch(df, model='rigid')
    with pytest.raises(ValueError, match='iterations must'):
        image_ops.fit_motion_launch(df, iterations=0)
    with pytest.raises(ValueError, match='scale must'):
        image_ops.fit_motion_launch(df, scale=0.0)
    with pytest.raises(ValueError, match=r'flow \(N, H, W, 2\)'):
        image_ops.fit_motion_launch(df[0])
    with pytest.raises(TypeError, match='a flow is float32'):
        image_ops.fit_motion_launch(df.to(torch.float64))
    with pytest.raises(ValueError, match='contiguous'):
        image_ops.fit_motion_launch(df.transpose(1, 2))
    with pytest.raises(ValueError, match='out must be a contiguous'):
        image_ops.fit_motion_launch(df, dk[0])
    with pytest.raises(ValueError, match='out must be a contiguous'):
        image_ops.fit_motion_launch(df, dk.to(torch.float32))
    with pytest.raises(ValueError, match='threshold must'):
        image_ops.residual_flow_launch(df, dm, threshold=-1)
    with pytest.raises(ValueError, match=r'flow \(N, H, W, 2\)'):
        image_ops.residual_flow_launch(df[0], dm)
    with pytest.raises(ValueError, match='motion must be a contiguous float32'):
        image_ops.residual_flow_launch(df, dm[0])
    with pytest.raises(ValueError, match='motion must be a contiguous float32'):
        image_ops.residual_flow_launch(df, dm.to(torch.float64))
    with pytest.raises(ValueError, match='nothing to compute'):
        image_ops.residual_flow_launch(df, dm, want_residual=False)
    with pytest.raises(ValueError, match=r'motions \(N, 2, 3\)'):
        image_ops.motion_flow_launch(dm[0], 4, 5)
    with pytest.raises(ValueError, match='motion must be a contiguous float32'):
        image_ops.motion_flow_launch(torch.zeros((2, 3, 2)), 4, 5)
    # the records of a correction: M and o of the map, each number rounded once, no colour change
    views = image_ops.MotionViews(np.array([[[1.0, 0.1, 3.0], [-0.1, 1.0 + 2.0 ** -30, -2.5]]]))
    assert len(views) == 1
    rec = views.records()[0]
    assert list(rec.m) == [1.0, float(np.float32(0.1)), float(np.float32(-0.1)), 1.0] and list(rec.o) == [3.0, -2.5] and rec.colour == 0
    np.testing.assert_allclose(np.array(list(rec.inv)).reshape(2, 2) @ np.array(list(rec.m)).reshape(2, 2), np.eye(2), atol=1e-6)
    assert len(image_ops.view_host_records(views, 1)) == C.sizeof(_ffi.ViewParams)
    with pytest.raises(ValueError, match='not finite'):
        image_ops.view_host_records(image_ops.MotionViews(np.zeros((1, 2, 3))), 1)         # (a map without an inverse)
    with pytest.raises(ValueError, match=r'motions \(N, 2, 3\)'):
        image_ops.MotionViews(np.zeros((2, 3)))


def test_the_model_checks_its_arguments_before_any_device_work():
    import inspect
    from tf_raft_amd.model import RAFT, CameraMotion, SmallRAFT
    assert CameraMotion._fields == ('motion', 'stats', 'residual', 'moving', 'forward', 'occluded_forward')
    pair = (np.zeros((1, 64, 96, 3), np.uint8), np.zeros((1, 64, 96, 3), np.uint8))
    video = np.zeros((3, 64, 96, 3), np.uint8)
    for cls in (RAFT, SmallRAFT):
        sig = inspect.signature(cls.camera_motion_step).parameters
        assert (sig['model'].default, sig['occlusion_test'].default, sig['iterations'].default, sig['scale'].default) == (
            'affine', 'consistency', 5, 1.0)
        sig = inspect.signature(cls.stabilize_video).parameters
        assert [sig[k].default for k in ('model', 'radius', 'iterations', 'scale', 'batch_size', 'occlusion_test', 'return_motion')] == [
            'similarity', 15, 5, 1.0, 4, 'consistency', False]
        assert not hasattr(cls, 'stabilizer')                                  # (the smoother needs the future: no streaming form)
        model = cls.__new__(cls)                                                # (no device: anything enqueued would fail)
        for bad in BAD_MODEL:
            with pytest.raises(ValueError, match='model must'):
                model.camera_motion_step(pair, model=bad)
            with pytest.raises(ValueError, match='model must'):
                model.stabilize_video(video, model=bad)
        for bad in BAD_ITERATIONS:
            with pytest.raises(ValueError, match='iterations must'):
                model.camera_motion_step(pair, iterations=bad)
            with pytest.raises(ValueError, match='iterations must'):
                model.stabilize_video(video, iterations=bad)
        for bad in BAD_SCALE:
            with pytest.raises(ValueError, match='scale must'):
                model.camera_motion_step(pair, scale=bad)
            with pytest.raises(ValueError, match='scale must'):
                model.stabilize_video(video, scale=bad)
        for bad in BAD_THRESHOLD + (None,):
            with pytest.raises(ValueError, match='threshold must'):
                model.camera_motion_step(pair, threshold=bad)
        with pytest.raises(TypeError, match='unexpected keyword'):
            model.camera_motion_step(pair, gamma=1.0)
        with pytest.raises(ValueError, match='occlusion_test must'):
            model.stabilize_video(video, occlusion_test='both')
        with pytest.raises(ValueError, match=r'\(T, H, W, 3\)'):
            model.stabilize_video(video[0])
        with pytest.raises(ValueError, match=r'\(T, H, W, 3\)'):
            model.stabilize_video(video[..., :2])
        with pytest.raises(ValueError, match='at least two frames'):
            model.stabilize_video(video[:1])
        with pytest.raises(TypeError, match='uint8 or float32 frames'):
            model.stabilize_video(video.astype(bool))
        for bad in (-1, 1.5, True, None):
            with pytest.raises(ValueError, match='radius must'):
                model.stabilize_video(video, radius=bad)
        for bad in (0, -1, 1.5, True, None):
            with pytest.raises(ValueError, match='batch_size must'):
                model.stabilize_video(video, batch_size=bad)

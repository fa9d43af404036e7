"""Soft census term of the self-supervised sequence loss, host side (no GPU).  This file holds

* the YARDSTICK ``torch_census_terms``: the definition in float64 torch, differentiated by autograd, checked here against
  central differences of its own value (``torch_total_loss`` adds it to tests/test_photometric_loss.py's yardstick);
* the float32 NumPy RESTATEMENT ``np_census_loss`` with the analytic gather gradient, in the kernel's operation order, and its
  measured distance to the yardstick per case (``census_restatement_distance`` for the loss an unlabelled training step sees,
  photometric + smoothness + census; ``census_only_distance`` for the term alone): tests/test_gpu_census_loss.py takes four
  times those distances as the kernel's tolerances;
* the cases with a known answer (``equal_frames_case``, ``brighter_case``; ``out_of_frame_case`` is the photometric file's);
* the C entries' declarations and argument checks, and the Python-side validation.

The definition.  gray(c) = (0.299f*R + 0.587f*G) + 0.114f*B on 0..255, g1 = gray(image1), g2 = gray(image2); under prediction i
the sample of pixel (x, y) is the one of the photometric term (position, ``inside``, taps, a, b) and w(x) = inside ? the
bilinear sample of g2 : 0.  f(d) = d / sqrt(0.81f + d*d), h(e) = e*e / (0.1f + e*e); interior(x, y) = 3 <= x <= W-4 and
3 <= y <= H-4; M = mask & inside & interior;
    D(x)  = (1/48) * sum over the 48 neighbours k != 0 of the 7x7 patch of h(f(w(x+k) - w(x)) - f(g1(x+k) - g1(x)))
    cen_i = sum_x M(x) * D(x) / (B*H*W)
    loss  = sum_i w_i * (ph_i + census_weight * cen_i + smooth_weight * sm_i),   w_i = float32(gamma**(n-i-1))
The five constants are the float32 values the kernel uses, in the yardstick too (as the photometric yardstick rounds its
parameters).  ``inside`` and ``mask`` are constants of the gradient.  Inputs: ``make_case`` of tests/test_photometric_loss.py (flows
1/16 or more away from cell borders).

Measured here (restatement against yardstick, with mask; loss relative, gradient over max|g|):

    case (B,H,W,n)   all terms, census_weight = 1        the census term alone
    1x6x20x1         8.2e-08, 1.3e-06                    exactly 0, exactly 0  (no interior pixel)
    1x8x9x2          4.8e-08, 8.8e-06                    5.4e-08, 8.9e-06
    2x37x53x3        3.6e-08, 1.8e-04                    7.2e-09, 1.9e-04
    1x9x2051x2       3.8e-07, 4.8e-03                    4.5e-07, 4.9e-03   (7.7e-03 without a mask)
    2x64x96x12       1.2e-08, 7.5e-04                    4.7e-09, 7.7e-04
    1x100x150x2      4.0e-08, 1.1e-03                    8.7e-09, 1.1e-03
The gradient distance is large where e = f(.) - f(.) cancels: the rounding of the two f values (6e-8 each) is a relative error of
6e-8 / |e| in e, h' and f' carry it on, and a pixel with a small gradient inherits the absolute error of its large neighbours.
The bounds asserted here are 1e-5 for the loss (float32 terms of relative error <= 6e-8 / |e| each, averaged) and 2e-2 of max|g|
for the gradient; the GPU file does not use them, it uses the measured distances.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tf_raft_amd import _ffi
from test_photometric_loss import (DEFAULTS, make_case, np_photometric_loss, out_of_frame_case, pred_weights, torch_photometric_loss)
from windowed_loss import check_argument_errors

# (B, H, W, n)        what it exercises on the GPU
CASES = [(1, 6, 20, 1),           # no interior pixel: the value and every gradient element are exactly 0
         (1, 8, 9, 2),            # smaller than a wave
         (2, 37, 53, 3),          # nothing a multiple of 64 or 256
         (1, 9, 2051, 2),         # a row longer than a workgroup, crossing the grid-stride loop
         (2, 64, 96, 12),         # the model's smallest frame, the training n
         (1, 100, 150, 2)]        # several workgroups per image
CASE_IDS = ['x'.join(map(str, c)) for c in CASES]
NO_INTERIOR = CASES[0]
RADIUS = 3
OFFSETS = [(dy, dx) for dy in range(-RADIUS, RADIUS + 1) for dx in range(-RADIUS, RADIUS + 1) if (dy, dx) != (0, 0)]   # rows first
C_R, C_G, C_B, C_F, C_H = (float(np.float32(v)) for v in (0.299, 0.587, 0.114, 0.81, 0.1))


def interior_mask(H, W, radius=RADIUS):
    ys, xs = np.mgrid[0:H, 0:W]
    return (xs >= radius) & (xs <= W - 1 - radius) & (ys >= radius) & (ys <= H - 1 - radius)


# ------------------------------------------------------------------ the yardstick: float64 torch, autograd
def _t64(a):
    return a.double() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=torch.float64)


def torch_census_terms(image1, image2, mask, preds, gamma=0.8):
    """``(sum_i w_i * cen_i, cen_last)`` as 0-d float64 tensors; ``preds`` float64 tensors (B, H, W, 2) that may require grad."""
    i1, i2 = _t64(image1), _t64(image2)
    B, H, W, _ = i1.shape
    m = torch.ones((B, H, W), dtype=torch.bool) if mask is None else torch.as_tensor(np.asarray(mask)) != 0
    gray = lambda c: (C_R * c[..., 0] + C_G * c[..., 1]) + C_B * c[..., 2]
    g1, g2 = gray(i1), gray(i2)
    f = lambda d: d / torch.sqrt(C_F + d * d)
    h = lambda e: e * e / (C_H + e * e)
    pad = lambda t: torch.nn.functional.pad(t, (RADIUS, RADIUS, RADIUS, RADIUS))
    shift = lambda tp, dy, dx: tp[:, RADIUS + dy:RADIUS + dy + H, RADIUS + dx:RADIUS + dx + W]
    g1p = pad(g1)
    fg = [f(shift(g1p, dy, dx) - g1) for dy, dx in OFFSETS]
    interior = torch.as_tensor(interior_mask(H, W))[None]
    xs = torch.arange(W, dtype=torch.float64)[None, None, :]
    ys = torch.arange(H, dtype=torch.float64)[None, :, None]
    nb = torch.arange(B)[:, None, None]
    total, cen = 0.0, None
    for w_i, p in zip(pred_weights(gamma, len(preds)), preds):
        sx, sy = xs + p[..., 0], ys + p[..., 1]
        inside = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
        px, py = torch.where(inside, sx, torch.zeros_like(sx)), torch.where(inside, sy, torch.zeros_like(sy))
        x0, y0 = torch.floor(px).detach().long(), torch.floor(py).detach().long()
        x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
        a, b = px - x0, py - y0
        w2 = (1 - b) * ((1 - a) * g2[nb, y0, x0] + a * g2[nb, y0, x1]) + b * ((1 - a) * g2[nb, y1, x0] + a * g2[nb, y1, x1])
        w = torch.where(inside, w2, torch.zeros_like(w2))
        wp = pad(w)
        D = sum(h(f(shift(wp, dy, dx) - w) - fg_k) for (dy, dx), fg_k in zip(OFFSETS, fg)) / 48.0
        M = (m & inside & interior).double()
        cen = (M * D).sum() / (B * H * W)
        total = total + w_i * cen
    return total, cen


def torch_total_loss(image1, image2, mask, preds, census_weight, **params):
    """``(loss, ph_last, cen_last, sm_last)``: the photometric yardstick plus ``float32(census_weight)`` times the census one."""
    loss, ph, sm = torch_photometric_loss(image1, image2, mask, preds, **params)
    total, cen = torch_census_terms(image1, image2, mask, preds, params.get('gamma', 0.8))
    return loss + float(np.float32(census_weight)) * total, ph, cen, sm


def _autograd(fn, preds):
    ps = [torch.tensor(np.asarray(p), dtype=torch.float64, requires_grad=True) for p in preds]
    vals = fn(ps)
    grads = torch.autograd.grad(vals[0], ps, allow_unused=True) if vals[0].requires_grad else [None] * len(ps)
    grads = [np.zeros(tuple(p.shape)) if g is None else g.numpy() for g, p in zip(grads, ps)]
    return [float(v.detach()) for v in vals], grads


def census_yardstick(case, gamma=0.8):
    """The census term alone on ``case`` = (image1, image2, mask, preds): ``(sum_i w_i cen_i, cen_last, [gradients])``."""
    image1, image2, mask, preds = case
    (total, cen), grads = _autograd(lambda ps: torch_census_terms(image1, image2, mask, ps, gamma), preds)
    return total, cen, grads


def total_yardstick(case, census_weight, **params):
    """``(loss, ph_last, cen_last, sm_last, [gradients])`` of ``torch_total_loss``."""
    image1, image2, mask, preds = case
    vals, grads = _autograd(lambda ps: torch_total_loss(image1, image2, mask, ps, census_weight, **params), preds)
    return (*vals, grads)


# ------------------------------------------------------------------ the restatement: float32 NumPy, analytic gather gradient
def np_census_loss(image1, image2, mask, preds, gamma=0.8, census_weight=1.0, upstream=1.0, add_to=None, prefill=None):
    """raft_census_loss_f32's arithmetic: every per-pixel operation in float32 in the kernel's order (the 48 pairs rows first),
    the sums over pixels in float64.  ``(out2[0], out2[1], [d_preds])``: two float32 scalars and float32 arrays; ``add_to`` is the
    float32 the entry adds its term to, ``prefill`` the arrays it accumulates the gradient into (None: stores)."""
    f = np.float32
    i1, i2 = np.asarray(image1, f), np.asarray(image2, f)
    B, H, W, _ = i1.shape
    use = np.ones((B, H, W), bool) if mask is None else np.asarray(mask) != 0
    gray = lambda c: (f(0.299) * c[..., 0] + f(0.587) * c[..., 1]) + f(0.114) * c[..., 2]
    g1, g2 = gray(i1), gray(i2)
    npix = B * H * W
    inv48n, scale = f(1.0 / (48.0 * npix)), f(upstream) * f(census_weight)
    interior = interior_mask(H, W)[None]
    ys, xs = np.mgrid[0:H, 0:W]
    pad = lambda t: np.pad(t, ((0, 0), (RADIUS, RADIUS), (RADIUS, RADIUS)))
    shift = lambda tp, dy, dx: tp[:, RADIUS + dy:RADIUS + dy + H, RADIUS + dx:RADIUS + dx + W]
    in_frame = {(dy, dx): ((ys + dy >= 0) & (ys + dy < H) & (xs + dx >= 0) & (xs + dx < W))[None] for dy, dx in OFFSETS}
    g1p = pad(g1)
    soft_sign = lambda d: d / np.sqrt(f(0.81) + d * d)
    fg = [soft_sign(shift(g1p, dy, dx) - g1) for dy, dx in OFFSETS]
    nb = np.arange(B)[:, None, None]
    weights = pred_weights(gamma, len(preds))
    tot, last, grads = 0.0, 0.0, []
    for i, (w_i, p) in enumerate(zip(weights, preds)):
        p = np.asarray(p, f)
        sx = np.arange(W, dtype=f)[None, None, :] + p[..., 0]
        sy = np.arange(H, dtype=f)[None, :, None] + p[..., 1]
        inside = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
        px, py = np.where(inside, sx, f(0)), np.where(inside, sy, f(0))
        fx, fy = np.floor(px), np.floor(py)
        x0, y0 = np.clip(fx.astype(np.int64), 0, W - 1), np.clip(fy.astype(np.int64), 0, H - 1)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        a, b = px - fx, py - fy
        na, nbb = f(1) - a, f(1) - b
        q00, q01, q10, q11 = g2[nb, y0, x0], g2[nb, y0, x1], g2[nb, y1, x0], g2[nb, y1, x1]
        w = np.where(inside, nbb * (na * q00 + a * q01) + b * (na * q10 + a * q11), f(0))
        du = np.where(inside, nbb * (q01 - q00) + b * (q11 - q10), f(0))
        dv = np.where(inside, na * (q10 - q00) + a * (q11 - q01), f(0))
        M = use & inside & interior
        Mf = M.astype(f)
        wp, Mp = pad(w), pad(Mf)
        hs, S = np.zeros((B, H, W), f), np.zeros((B, H, W), f)
        for (dy, dx), fg_k in zip(OFFSETS, fg):
            d = shift(wp, dy, dx) - w
            r = f(0.81) + d * d
            sr = np.sqrt(r)
            e = d / sr - fg_k
            q = f(0.1) + e * e
            hs = hs + (e * e) / q
            term = ((Mf + shift(Mp, dy, dx)) * (((f(2) * e) * f(0.1)) / (q * q))) * (f(0.81) / (r * sr))
            S = S + np.where(in_frame[(dy, dx)], term, f(0))
        D = np.where(M, hs / f(48), f(0))
        gw = f(0) - (scale * f(w_i)) * (S * inv48n)
        g = np.stack([gw * du, gw * dv], -1)
        assert g.dtype == f and D.dtype == f
        grads.append(g if prefill is None else np.asarray(prefill[i], f) + g)
        last = float(D.astype(np.float64).sum())
        tot += w_i * last
    inv = 1.0 / npix
    before = 0.0 if add_to is None else float(f(add_to))
    return f(before + float(f(census_weight)) * (tot * inv)), f(last * inv), grads


def np_total_loss(image1, image2, mask, preds, census_weight, upstream=1.0, **params):
    """What the Python entries compute with ``census_weight > 0``: the photometric restatement, then the census one on top of its
    loss and its gradient.  ``(loss, ph_last, cen_last, sm_last, [gradients])``."""
    loss, ph, sm, grads = np_photometric_loss(image1, image2, mask, preds, upstream=upstream, **params)
    total, cen, grads = np_census_loss(image1, image2, mask, preds, params.get('gamma', 0.8), census_weight, upstream, add_to=loss,
                                       prefill=grads)
    return total, ph, cen, sm, grads


def _distance(got_loss, got_g, want_loss, want_g):
    diff = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(got_g, want_g))
    rel = abs(float(got_loss) - want_loss) / abs(want_loss) if want_loss != 0 else abs(float(got_loss))
    return rel, diff, max(float(np.abs(b).max()) for b in want_g)


@functools.lru_cache(maxsize=None)
def census_restatement_distance(B, H, W, n, with_mask, census_weight=1.0):
    """The restatement of the whole loss (``np_total_loss``) against ``total_yardstick`` on ``make_case(B, H, W, n)``:
    ``(relative distance of the loss, max |difference| of the gradient, max |gradient|)``.  The GPU test's tolerances are four
    times the first two."""
    case = make_case(B, H, W, n, with_mask=with_mask)
    want = total_yardstick(case, census_weight, **DEFAULTS)
    got = np_total_loss(*case, census_weight, **DEFAULTS)
    return _distance(got[0], got[4], want[0], want[4])


@functools.lru_cache(maxsize=None)
def census_only_distance(B, H, W, n, with_mask):
    """The same for the census term alone (``np_census_loss`` with census_weight = 1 against ``census_yardstick``)."""
    case = make_case(B, H, W, n, with_mask=with_mask)
    want_total, _, want_g = census_yardstick(case, DEFAULTS['gamma'])
    total, _, g = np_census_loss(*case, gamma=DEFAULTS['gamma'])
    return _distance(total, g, want_total, want_g)


def valid_counts(case):
    """Number of pixels with M = 1 per prediction (float64 positions: the flows of ``make_case`` sit away from every border)."""
    image1, _, mask, preds = case
    B, H, W, _ = image1.shape
    use = np.ones((B, H, W), bool) if mask is None else np.asarray(mask) != 0
    ys, xs = np.mgrid[0:H, 0:W]
    out = []
    for p in preds:
        sx, sy = xs[None] + p[..., 0].astype(np.float64), ys[None] + p[..., 1].astype(np.float64)
        inside = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
        out.append(int((use & inside & interior_mask(H, W)[None]).sum()))
    return out


# ------------------------------------------------------------------ cases with a known answer
def equal_frames_case(B, H, W, n, seed=3):
    """image2 == image1 and zero flow: every e is exactly 0 (w = g1 bit for bit), so the term and its gradient are exactly 0."""
    image1, _, mask, preds = make_case(B, H, W, n, seed=seed)
    return image1, image1.copy(), mask, [np.zeros_like(p) for p in preds]


def brighter_case(B, H, W, n, seed=4):
    """image2 = image1 + 20 (values kept <= 235) and zero flow: the census term is below 1e-6 (|e| <= ~1e-4 from the float32
    rounding of the gray values, h <= e*e / 0.1), while the Charbonnier term of the pair is about 20/255."""
    rng = np.random.default_rng(seed)
    image1 = rng.integers(0, 216, size=(B, H, W, 3)).astype(np.float32)
    mask = (rng.uniform(size=(B, H, W)) < 0.8).astype(np.uint8)
    return image1, image1 + np.float32(20), mask, [np.zeros((B, H, W, 2), np.float32) for _ in range(n)]


BRIGHTER_BOUND = 1e-6


# ------------------------------------------------------------------ yardstick and restatement
def test_the_census_yardstick_gradient_matches_central_differences():
    rng = np.random.default_rng(11)
    case = make_case(2, 11, 13, 2)
    image1, image2, mask, preds = case
    _, _, grads = census_yardstick(case)
    value = lambda ps: float(torch_census_terms(image1, image2, mask, [torch.tensor(p, dtype=torch.float64) for p in ps])[0])
    base = [np.asarray(p, np.float64) for p in preds]
    nonzero = [(i,) + tuple(int(v) for v in idx) for i, g in enumerate(grads) for idx in np.argwhere(g != 0)]
    assert len(nonzero) >= 20
    picks = [nonzero[int(k)] for k in rng.choice(len(nonzero), 16, replace=False)]
    picks += [(int(rng.integers(len(preds))),) + tuple(int(rng.integers(d)) for d in base[0].shape) for _ in range(8)]
    h, worst = 1e-6, 0.0
    for i, *idx in picks:
        idx = tuple(idx)
        hi, lo = [b.copy() for b in base], [b.copy() for b in base]
        hi[i][idx] += h
        lo[i][idx] -= h
        fd = (value(hi) - value(lo)) / (2 * h)
        want = grads[i][idx]
        worst = max(worst, abs(fd - want) / (1e-5 * abs(want) + 1e-10))
        assert abs(fd - want) <= 1e-5 * abs(want) + 1e-10, (i, idx, fd, want)       # (1e-10: rounding of the value over 2h)
    print(f'[census] yardstick against central differences: worst |difference| / bound = {worst:.2e}')


@pytest.mark.parametrize('with_mask', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('shape', CASES, ids=CASE_IDS)
def test_the_census_restatement_is_close_to_the_yardstick(shape, with_mask):
    case = make_case(*shape, with_mask=with_mask)
    rel_loss, diff_g, max_g = census_restatement_distance(*shape, with_mask)
    only_loss, only_g, only_max = census_only_distance(*shape, with_mask)
    print(f'[census] restatement {shape} mask={with_mask}: all terms loss rel {rel_loss:.2e}, gradient {diff_g / max_g:.2e} of max|g| = '
          f'{max_g:.3e}; census alone loss rel {only_loss:.2e}, gradient {only_g / max(only_max, 1e-300):.2e} of max|g| = {only_max:.3e}')
    total, cen, grads = np_census_loss(*case, gamma=DEFAULTS['gamma'])
    if shape == NO_INTERIOR:
        assert valid_counts(case) == [0] * shape[3]
        assert float(total) == 0.0 and float(cen) == 0.0 and all(not g.any() for g in grads)
        assert census_yardstick(case)[0] == 0.0 and only_max == 0.0
    else:
        assert min(valid_counts(case)) >= 1, 'a prediction of the case has no pixel with M = 1'
        assert only_max > 0 and float(cen) > 0
        assert only_loss <= 1e-5
        assert only_g / only_max <= 2e-2
        want_cen = census_yardstick(case)[1]
        assert abs(float(cen) - want_cen) <= 1e-5 * want_cen
    assert rel_loss <= 1e-5
    assert diff_g / max_g <= 2e-2


def test_the_census_restatement_on_the_cases_with_a_known_answer():
    B, H, W, n = 2, 37, 53, 2
    total, cen, grads = np_census_loss(*equal_frames_case(B, H, W, n))
    assert float(total) == 0.0 and float(cen) == 0.0 and all(not g.any() for g in grads)
    case = brighter_case(B, H, W, n)
    total, cen, grads = np_census_loss(*case)
    ph = float(np_photometric_loss(*case, **DEFAULTS)[1])
    print(f'[census] image2 = image1 + 20: census {float(cen):.3e}, photometric {ph:.4f}')
    assert 0.0 <= float(cen) < BRIGHTER_BOUND and 0.0 <= float(total) < 2 * BRIGHTER_BOUND
    assert abs(ph - 0.8 * 20 / 255) < 0.01                              # (mask density 0.8)
    assert census_yardstick(case)[1] < BRIGHTER_BOUND
    random_cen = float(np_census_loss(*make_case(B, H, W, n))[1])
    assert random_cen > 0.05                                            # random frames are far from each other in this distance
    case = out_of_frame_case(B, H, W, n)
    total, cen, grads = np_census_loss(*case)
    assert float(total) == 0.0 and float(cen) == 0.0 and all(not g.any() for g in grads)
    assert census_yardstick(case)[0] == 0.0
    # a pixel that is not interior has M = 0 and still receives gradient from interior neighbours; upstream = 2 doubles bit for bit;
    # accumulate adds in float32; add_to is added in double
    case = make_case(B, H, W, n, with_mask=False)
    total, cen, grads = np_census_loss(*case)
    ring = ~interior_mask(H, W)
    assert any(g[:, ring].any() for g in grads)
    _, _, doubled = np_census_loss(*case, upstream=2.0)
    for a, b in zip(grads, doubled):
        np.testing.assert_array_equal(2 * a, b)
    fill = [np.full_like(g, 0.25) for g in grads]
    total2, _, acc = np_census_loss(*case, add_to=np.float32(1.5), prefill=fill)
    for a, b in zip(grads, acc):
        np.testing.assert_array_equal(np.float32(0.25) + a, b)
    assert abs(float(total2) - (1.5 + float(total))) <= 2.0 ** -23


# ------------------------------------------------------------------ the C entries
def test_census_entries_are_declared_exported_and_typed():
    from tf_raft_amd import build
    assert 'census_loss.hip' in build.SOURCES and 'warped_gray.h' in build.HEADERS       # (a header outside the digest goes stale)
    _P, _I, _F = C.c_void_p, C.c_int, C.c_float
    assert _ffi._SIGNATURES['raft_census_loss_workspace_bytes'] == (C.c_int64, [_I, _I, _I, _I])
    assert _ffi._SIGNATURES['raft_census_loss_f32'] == (_I, [_P, _P, _P, _P, C.c_int64, _I, _I, _I, _I, C.c_double, _F, _F, _P, _P, _P,
                                                             _I, _P, _P])
    lib = _ffi.load_library()
    npix = 4 * 368 * 496
    need = lib.raft_census_loss_workspace_bytes(12, 4, 368, 496)
    assert need >= 4 * npix + 12 * npix * 8 and need % 8 == 0 and need < 80 << 20      # g1, and per prediction two float planes
    assert lib.raft_census_loss_workspace_bytes(1, 1, 1, 1) > 0
    for bad in ((0, 1, 8, 8), (65, 1, 8, 8), (1, 0, 8, 8), (1, 1, -1, 8), (1, 1, 1 << 15, 1 << 15)):
        assert lib.raft_census_loss_workspace_bytes(*bad) == 0, bad


def test_census_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    check_argument_errors(_ffi.load_library().raft_census_loss_f32)


# ------------------------------------------------------------------ Python-side validation (nothing here reaches the device)
def test_census_weight_is_validated_and_sits_last():
    import inspect
    from tf_raft_amd import grad, losses
    loss = losses.PhotometricSequenceLoss()
    assert loss.census_weight == 0.0 and loss._params()['census_weight'] == 0.0
    assert losses.PhotometricSequenceLoss(0.8, 0.1, 10.0, 0.01, 2).census_weight == 2.0
    assert losses.PhotometricSequenceLoss(census_weight=np.float32(0.5))._params()['census_weight'] == 0.5
    for bad in (-0.1, float('nan'), float('inf'), 1e39, 'x', None, True, 1j, (1.0,)):
        with pytest.raises(ValueError, match='census_weight'):
            losses.PhotometricSequenceLoss(census_weight=bad)
    for fn in (losses.PhotometricSequenceLoss.__init__, losses.photometric_sequence_loss, grad.photometric_sequence_loss_value_and_grad,
               grad.photometric_sequence_loss_grad):
        names = list(inspect.signature(fn).parameters)
        assert names[-1] == 'census_weight', (fn, names)
        assert inspect.signature(fn).parameters['census_weight'].default == 0.0
    i1 = np.zeros((2, 8, 9, 3), np.float32)
    p = np.zeros((2, 8, 9, 2), np.float32)
    for fn in (losses.photometric_sequence_loss, grad.photometric_sequence_loss_grad, grad.photometric_sequence_loss_value_and_grad):
        with pytest.raises(ValueError, match='census_weight'):
            fn((i1, i1), [p], census_weight=-1.0)
        with pytest.raises(ValueError, match='prediction'):                  # the shape checks still come before the device
            fn((i1, i1), [p[:, :4]], census_weight=1.0)


def test_compile_adds_the_census_mean_only_for_a_positive_weight():
    from tf_raft_amd import losses
    from tf_raft_amd.model import RAFT, SmallRAFT
    for cls in (RAFT, SmallRAFT):
        model = cls.__new__(cls)
        model.compile(optimizer=None, loss=losses.PhotometricSequenceLoss(census_weight=0.5))
        assert list(model.flow_metrics) == ['loss', 'epe', 'u1', 'u3', 'u5', 'photometric', 'census', 'smoothness']
        with pytest.raises(ValueError, match=r'\(image1, image2\) or \(image1, image2, mask\)'):
            model.train_step((np.zeros((1, 64, 96, 3), np.float32),))
        for loss in (losses.PhotometricSequenceLoss(), losses.PhotometricSequenceLoss(census_weight=0.0)):
            model.compile(optimizer=None, loss=loss)
            assert list(model.flow_metrics) == ['loss', 'epe', 'u1', 'u3', 'u5', 'photometric', 'smoothness']
        model.compile(optimizer=None)
        assert list(model.flow_metrics) == ['loss', 'epe', 'u1', 'u3', 'u5']

"""SSIM term of the self-supervised sequence loss, host side (no GPU).  This file holds

* the YARDSTICK ``torch_ssim_terms``: the definition in float64 torch, differentiated by autograd, checked here against central
  differences of its own value (``torch_ssim_total_loss`` adds it to the photometric and census yardsticks);
* the float32 NumPy RESTATEMENT ``np_ssim_loss`` with the analytic gather gradient, in the kernel's operation order, and its
  measured distance to the yardstick per case (``ssim_restatement_distance`` for the loss an unlabelled training step sees,
  ``ssim_only_distance`` for the term alone): tests/test_gpu_ssim_loss.py takes four times those distances as the kernel's
  tolerances;
* the cases with a known answer (equal frames, every vector out of frame, two constant frames);
* the C entries' declarations and argument checks, and the Python-side validation.

The definition.  Gray values g1, g2, the sample of a pixel under prediction i (position, ``inside``, taps, a, b) and the warped
plane w (0 out of frame) are tests/test_census_loss.py's.  Over the 3x3 window of z, rows first, x = g1:
    mx = (sum x) / 9, mw = (sum w) / 9, sxx = (sum (x-mx)^2) / 9, sww = (sum (w-mw)^2) / 9, sxw = (sum (x-mx)*(w-mw)) / 9
    n1 = 2*mx*mw + C1, d1 = mx*mx + mw*mw + C1, n2 = 2*sxw + C2, d2 = sxx + sww + C2,  C1 = (0.01f*255.f)^2, C2 = (0.03f*255.f)^2
    S(z) = (n1*n2) / (d1*d2),  D(z) = (1 - S(z)) / 2,  interior(z) = 1 <= zx <= W-2 and 1 <= zy <= H-2,  M = mask & inside & interior
    ssim_i = sum_z M(z) * D(z) / (B*H*W)
    loss   = sum_i w_i * (ph_i + census_weight * cen_i + ssim_weight * ssim_i + smooth_weight * sm_i),   w_i = float32(gamma**(n-i-1))
The constants are the float32 values the kernel uses, in the yardstick too.  ``inside`` and ``mask`` are constants of the gradient.
The restatement's gradient is the gather of csrc/ssim_loss.hip: with r1 = n1/d1, r2 = n2/d2, A = ((2*mx - (2*mw)*r1) * r2) / d1,
R = (2*r1) / d2, Q2 = 0 - R*r2 per window, G(y) = sum over the (up to) nine windows z around y with M(z) = 1, rows first, of
(A + Q2*(w(y) - mw)) + R*(x(y) - mx), and d ssim_i / d w(y) = -G(y) / (18*B*H*W).

Inputs: ``make_case`` of tests/test_photometric_loss.py (flows 1/16 or more away from cell borders), through ``ssim_case``: the
one-window shape 1x3x3x1 takes ``amp=0`` (vectors of less than a pixel), since with vectors of up to three pixels its only window
would be out of frame.

Measured here (restatement against yardstick, with mask; loss relative, gradient over max|g|):

    case (B,H,W,n)   ssim_weight = 1, census off      census 0.7 / ssim 0.5        the SSIM term alone
    1x2x20x1         2.1e-08, 2.3e-07                 2.1e-08, 2.3e-07             exactly 0, exactly 0  (no interior pixel)
    1x3x3x1          1.2e-08, 6.8e-08                 6.3e-08, 8.5e-08             1.9e-08, 2.0e-07
    1x8x9x2          2.9e-08, 4.9e-07                 4.3e-08, 7.4e-06             3.8e-10, 2.8e-07
    2x37x53x3        6.6e-08, 6.4e-06                 2.8e-08, 1.5e-04             1.3e-08, 2.5e-06
    1x9x2051x2       1.1e-07, 3.0e-04                 2.3e-07, 4.1e-03             7.0e-08, 9.6e-05
    2x64x96x12       1.3e-08, 9.7e-06                 1.7e-08, 6.6e-04             3.5e-09, 3.5e-06
    (without a mask the largest are 1.7e-07, 2.8e-04; 2.7e-07, 6.2e-03; 9.6e-08, 9.1e-05, all at 1x9x2051x2)
The SSIM term's own gradient distance grows with W: the sample position x + u is ONE float32 addition (flow_sample.h), so at
x ~ 2000 the fraction a carries an absolute error of up to 2^-13 = 1.2e-4 of a pixel, which float64 does not have, and w and
dwdu inherit it times the gray slope.  That is the mechanism behind the photometric file's distances too, so the bounds asserted
here are that file's: 1e-5 for the loss and 2e-3 of max|g| for the gradient (2e-2 with the census term on, the census file's
bound); the GPU file does not use them, it uses the measured distances.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tf_raft_amd import _ffi
from test_census_loss import _autograd, _distance, _t64, np_census_loss, torch_census_terms
from test_census_loss import interior_mask as census_interior_mask
from test_photometric_loss import DEFAULTS, make_case, np_photometric_loss, out_of_frame_case, pred_weights, torch_photometric_loss
from windowed_loss import check_argument_errors

# (B, H, W, n)        what it exercises on the GPU
CASES = [(1, 2, 20, 1),           # no interior pixel: the value and every gradient element are exactly 0
         (1, 3, 3, 1),            # one window
         (1, 8, 9, 2),            # smaller than a wave; every pixel within two of a border
         (2, 37, 53, 3),          # nothing a multiple of 64 or 256
         (1, 9, 2051, 2),         # a row longer than a workgroup's stride
         (2, 64, 96, 12)]         # the model's smallest frame, the training n
CASE_IDS = ['x'.join(map(str, c)) for c in CASES]
NO_INTERIOR, ONE_WINDOW = CASES[0], CASES[1]
OFFSETS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]              # rows first
_K1, _K2 = np.float32(0.01) * np.float32(255), np.float32(0.03) * np.float32(255)
C1, C2 = _K1 * _K1, _K2 * _K2                                              # float32, each product rounded once
assert C1.dtype == np.float32 and C2.dtype == np.float32
C_R, C_G, C_B = (float(np.float32(v)) for v in (0.299, 0.587, 0.114))


def ssim_case(shape, with_mask=True):
    """``make_case`` for a shape of ``CASES``; the one-window shape with vectors of less than a pixel (its window is in frame)."""
    return make_case(*shape, amp=0, with_mask=with_mask) if tuple(shape) == ONE_WINDOW else make_case(*shape, with_mask=with_mask)


interior_mask = functools.partial(census_interior_mask, radius=1)              # 1 <= x <= W-2 and 1 <= y <= H-2


# ------------------------------------------------------------------ the yardstick: float64 torch, autograd
def torch_ssim_terms(image1, image2, mask, preds, gamma=0.8):
    """``(sum_i w_i * ssim_i, ssim_last)`` as 0-d float64 tensors; ``preds`` float64 tensors (B, H, W, 2) that may require grad."""
    i1, i2 = _t64(image1), _t64(image2)
    B, H, W, _ = i1.shape
    m = torch.ones((B, H, W), dtype=torch.bool) if mask is None else torch.as_tensor(np.asarray(mask)) != 0
    gray = lambda c: (C_R * c[..., 0] + C_G * c[..., 1]) + C_B * c[..., 2]
    g1, g2 = gray(i1), gray(i2)
    c1, c2 = float(C1), float(C2)
    pad = lambda t: torch.nn.functional.pad(t, (1, 1, 1, 1))
    window = lambda t: [pad(t)[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in OFFSETS]
    xs9 = window(g1)
    mx = sum(xs9) / 9.0
    sxx = sum((x - mx) ** 2 for x in xs9) / 9.0
    interior = torch.as_tensor(interior_mask(H, W))[None]
    xs = torch.arange(W, dtype=torch.float64)[None, None, :]
    ys = torch.arange(H, dtype=torch.float64)[None, :, None]
    nb = torch.arange(B)[:, None, None]
    total, last = 0.0, None
    for w_i, p in zip(pred_weights(gamma, len(preds)), preds):
        sx, sy = xs + p[..., 0], ys + p[..., 1]
        inside = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
        px, py = torch.where(inside, sx, torch.zeros_like(sx)), torch.where(inside, sy, torch.zeros_like(sy))
        x0, y0 = torch.floor(px).detach().long(), torch.floor(py).detach().long()
        x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
        a, b = px - x0, py - y0
        w2 = (1 - b) * ((1 - a) * g2[nb, y0, x0] + a * g2[nb, y0, x1]) + b * ((1 - a) * g2[nb, y1, x0] + a * g2[nb, y1, x1])
        w = torch.where(inside, w2, torch.zeros_like(w2))
        ws9 = window(w)
        mw = sum(ws9) / 9.0
        sww = sum((v - mw) ** 2 for v in ws9) / 9.0
        sxw = sum((x - mx) * (v - mw) for x, v in zip(xs9, ws9)) / 9.0
        S = ((2 * mx * mw + c1) * (2 * sxw + c2)) / ((mx * mx + mw * mw + c1) * (sxx + sww + c2))
        M = (m & inside & interior).double()
        last = (M * ((1 - S) / 2)).sum() / (B * H * W)
        total = total + w_i * last
    return total, last


def torch_ssim_total_loss(image1, image2, mask, preds, census_weight, ssim_weight, **params):
    """``(loss, ph_last, cen_last, ssim_last, sm_last)``: the photometric yardstick plus ``float32(census_weight)`` times the census
    one plus ``float32(ssim_weight)`` times the SSIM one."""
    loss, ph, sm = torch_photometric_loss(image1, image2, mask, preds, **params)
    gamma = params.get('gamma', 0.8)
    cen_total, cen = torch_census_terms(image1, image2, mask, preds, gamma)
    ssim_total, ssim = torch_ssim_terms(image1, image2, mask, preds, gamma)
    return loss + float(np.float32(census_weight)) * cen_total + float(np.float32(ssim_weight)) * ssim_total, ph, cen, ssim, sm


def ssim_yardstick(case, gamma=0.8):
    """The SSIM term alone on ``case`` = (image1, image2, mask, preds): ``(sum_i w_i ssim_i, ssim_last, [gradients])``."""
    image1, image2, mask, preds = case
    (total, last), grads = _autograd(lambda ps: torch_ssim_terms(image1, image2, mask, ps, gamma), preds)
    return total, last, grads


def ssim_total_yardstick(case, census_weight, ssim_weight, **params):
    """``(loss, ph_last, cen_last, ssim_last, sm_last, [gradients])`` of ``torch_ssim_total_loss``."""
    image1, image2, mask, preds = case
    vals, grads = _autograd(lambda ps: torch_ssim_total_loss(image1, image2, mask, ps, census_weight, ssim_weight, **params), preds)
    return (*vals, grads)


# ------------------------------------------------------------------ the restatement: float32 NumPy, analytic gather gradient
def _mean9(v):
    s = v[0]
    for k in range(1, 9):
        s = s + v[k]
    return s / np.float32(9)


def _cov9(a, ma, b, mb):
    s = (a[0] - ma) * (b[0] - mb)
    for k in range(1, 9):
        s = s + (a[k] - ma) * (b[k] - mb)
    return s / np.float32(9)


def np_ssim_loss(image1, image2, mask, preds, gamma=0.8, ssim_weight=1.0, upstream=1.0, add_to=None, prefill=None):
    """raft_ssim_loss_f32's arithmetic: every per-pixel operation in float32 in the kernel's order (windows rows first), the sums
    over pixels in float64.  ``(out2[0], out2[1], [d_preds])``: two float32 scalars and float32 arrays; ``add_to`` is the float32
    the entry adds its term to, ``prefill`` the arrays it accumulates the gradient into (None: stores)."""
    f = np.float32
    i1, i2 = np.asarray(image1, f), np.asarray(image2, f)
    B, H, W, _ = i1.shape
    use = np.ones((B, H, W), bool) if mask is None else np.asarray(mask) != 0
    gray = lambda c: (f(0.299) * c[..., 0] + f(0.587) * c[..., 1]) + f(0.114) * c[..., 2]
    g1, g2 = gray(i1), gray(i2)
    npix = B * H * W
    inv18n, scale = f(1.0 / (18.0 * npix)), f(upstream) * f(ssim_weight)
    interior = interior_mask(H, W)[None]
    pad = lambda t: np.pad(t, ((0, 0), (1, 1), (1, 1)))
    shift = lambda tp, dy, dx: tp[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    window = lambda t: [shift(pad(t), dy, dx) for dy, dx in OFFSETS]
    xs9 = window(g1)
    mx = _mean9(xs9)
    sxx = _cov9(xs9, mx, xs9, mx)
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
        ws9 = window(w)
        mw = _mean9(ws9)
        sww, sxw = _cov9(ws9, mw, ws9, mw), _cov9(xs9, mx, ws9, mw)
        n1 = (f(2) * mx) * mw + C1
        d1 = (mx * mx + mw * mw) + C1
        n2 = f(2) * sxw + C2
        d2 = (sxx + sww) + C2
        S = (n1 * n2) / (d1 * d2)
        r1, r2 = n1 / d1, n2 / d2
        R = (f(2) * r1) / d2
        Q2 = f(0) - R * r2
        A = ((f(2) * mx - (f(2) * mw) * r1) * r2) / d1
        # the gather: the windows z = y + (dy, dx) around every pixel y, rows first (M is 0 beyond the frame)
        Mp, Ap, Qp, Rp, mxp, mwp = (pad(t) for t in (M.astype(f), A, Q2, R, mx, mw))
        G = np.zeros((B, H, W), f)
        for dy, dx in OFFSETS:
            share = (shift(Ap, dy, dx) + shift(Qp, dy, dx) * (w - shift(mwp, dy, dx))) + shift(Rp, dy, dx) * (g1 - shift(mxp, dy, dx))
            G = G + np.where(shift(Mp, dy, dx) != 0, share, f(0))
        D = np.where(M, (f(1) - S) / f(2), f(0))
        gw = f(0) - (scale * f(w_i)) * (G * inv18n)
        g = np.stack([gw * du, gw * dv], -1)
        assert g.dtype == f and D.dtype == f
        grads.append(g if prefill is None else np.asarray(prefill[i], f) + g)
        last = float(D.astype(np.float64).sum())
        tot += w_i * last
    inv = 1.0 / npix
    before = 0.0 if add_to is None else float(f(add_to))
    return f(before + float(f(ssim_weight)) * (tot * inv)), f(last * inv), grads


def np_ssim_total_loss(image1, image2, mask, preds, census_weight, ssim_weight, upstream=1.0, **params):
    """What the Python entries compute: the photometric restatement, then (for a positive weight each) the census one and the
    SSIM one on top of the loss and the gradient so far.  ``(loss, ph_last, cen_last or None, ssim_last or None, sm_last,
    [gradients])``."""
    loss, ph, sm, grads = np_photometric_loss(image1, image2, mask, preds, upstream=upstream, **params)
    gamma, cen, ssim = params.get('gamma', 0.8), None, None
    if census_weight > 0:
        loss, cen, grads = np_census_loss(image1, image2, mask, preds, gamma, census_weight, upstream, add_to=loss, prefill=grads)
    if ssim_weight > 0:
        loss, ssim, grads = np_ssim_loss(image1, image2, mask, preds, gamma, ssim_weight, upstream, add_to=loss, prefill=grads)
    return loss, ph, cen, ssim, sm, grads


@functools.lru_cache(maxsize=None)
def ssim_restatement_distance(B, H, W, n, with_mask, census_weight=0.0, ssim_weight=1.0):
    """The restatement of the whole loss (``np_ssim_total_loss``) against ``ssim_total_yardstick`` on ``ssim_case``:
    ``(relative distance of the loss, max |difference| of the gradient, max |gradient|)``.  The GPU test's tolerances are four
    times the first two."""
    case = ssim_case((B, H, W, n), with_mask)
    want = ssim_total_yardstick(case, census_weight, ssim_weight, **DEFAULTS)
    got = np_ssim_total_loss(*case, census_weight, ssim_weight, **DEFAULTS)
    return _distance(got[0], got[5], want[0], want[5])


@functools.lru_cache(maxsize=None)
def ssim_only_distance(B, H, W, n, with_mask):
    """The same for the SSIM term alone (``np_ssim_loss`` with ssim_weight = 1 against ``ssim_yardstick``)."""
    case = ssim_case((B, H, W, n), with_mask)
    want_total, _, want_g = ssim_yardstick(case, DEFAULTS['gamma'])
    total, _, g = np_ssim_loss(*case, gamma=DEFAULTS['gamma'])
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
    """image2 == image1 and zero flow: w = g1 bit for bit, so every window has n1 == d1 and n2 == d2, S == 1 and the term exactly
    0; in the gather r1 = r2 = 1, A = 0 and Q2 = -R, so the restatement's (and the kernel's) gradient is exactly 0 too."""
    image1, _, mask, preds = make_case(B, H, W, n, seed=seed)
    return image1, image1.copy(), mask, [np.zeros_like(p) for p in preds]


def constant_frames_case(B, H, W, n, level1=90.0, level2=140.0):
    """Two frames of one colour each at zero flow, no mask: ``(case, closed form of ssim_i)`` with a, b the float32 gray levels:
    (1 - (2ab + C1) / (a*a + b*b + C1)) / 2 on the (H-2)*(W-2) interior pixels of the H*W."""
    image1 = np.full((B, H, W, 3), level1, np.float32)
    image2 = np.full((B, H, W, 3), level2, np.float32)
    f = np.float32
    a, b = (float((f(0.299) * f(v) + f(0.587) * f(v)) + f(0.114) * f(v)) for v in (level1, level2))
    c1 = float(C1)
    closed = (1 - (2 * a * b + c1) / (a * a + b * b + c1)) / 2 * ((H - 2) * (W - 2) / (H * W))
    return (image1, image2, None, [np.zeros((B, H, W, 2), np.float32) for _ in range(n)]), closed


# ------------------------------------------------------------------ yardstick and restatement
def test_the_ssim_yardstick_gradient_matches_central_differences():
    rng = np.random.default_rng(11)
    case = make_case(2, 11, 13, 2)
    image1, image2, mask, preds = case
    _, _, grads = ssim_yardstick(case)
    value = lambda ps: float(torch_ssim_terms(image1, image2, mask, [torch.tensor(p, dtype=torch.float64) for p in ps])[0])
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
    print(f'[ssim] yardstick against central differences: worst |difference| / bound = {worst:.2e}')


@pytest.mark.parametrize('with_mask', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('shape', CASES, ids=CASE_IDS)
def test_the_ssim_restatement_is_close_to_the_yardstick(shape, with_mask):
    case = ssim_case(shape, with_mask)
    rel_loss, diff_g, max_g = ssim_restatement_distance(*shape, with_mask)
    both_loss, both_g, both_max = ssim_restatement_distance(*shape, with_mask, 0.7, 0.5)
    only_loss, only_g, only_max = ssim_only_distance(*shape, with_mask)
    print(f'[ssim] restatement {shape} mask={with_mask}: ssim_weight 1 loss rel {rel_loss:.2e}, gradient {diff_g / max_g:.2e} of max|g| = '
          f'{max_g:.3e}; census 0.7 / ssim 0.5 loss rel {both_loss:.2e}, gradient {both_g / both_max:.2e} of max|g|; SSIM alone loss rel '
          f'{only_loss:.2e}, gradient {only_g / max(only_max, 1e-300):.2e} of max|g| = {only_max:.3e}')
    total, last, grads = np_ssim_loss(*case, gamma=DEFAULTS['gamma'])
    if shape == NO_INTERIOR:
        assert valid_counts(case) == [0] * shape[3]
        assert float(total) == 0.0 and float(last) == 0.0 and all(not g.any() for g in grads)
        assert ssim_yardstick(case)[0] == 0.0 and only_max == 0.0
    else:
        assert min(valid_counts(case)) >= 1, 'a prediction of the case has no pixel with M = 1'
        assert only_max > 0 and float(last) > 0
        assert only_loss <= 1e-5
        assert only_g / only_max <= 2e-3
        want_last = ssim_yardstick(case)[1]
        assert abs(float(last) - want_last) <= 1e-5 * want_last
    assert rel_loss <= 1e-5 and both_loss <= 1e-5
    assert diff_g / max_g <= 2e-3                   # (tests/test_photometric_loss.py's bound: its terms are in this loss)
    assert both_g / both_max <= 2e-2                # (tests/test_census_loss.py's)


def test_the_ssim_restatement_on_the_cases_with_a_known_answer():
    B, H, W, n = 2, 37, 53, 2
    total, last, grads = np_ssim_loss(*equal_frames_case(B, H, W, n))
    assert float(total) == 0.0 and float(last) == 0.0 and all(not g.any() for g in grads)
    case = out_of_frame_case(B, H, W, n)
    total, last, grads = np_ssim_loss(*case)
    assert float(total) == 0.0 and float(last) == 0.0 and all(not g.any() for g in grads)
    assert ssim_yardstick(case)[0] == 0.0
    # (levels well apart: S near 1 is rounded to 2^-24 absolute, so a relative 1e-4 of D = (1 - S) / 2 needs D of 1e-3 or more)
    for levels in ((90.0, 140.0), (10.0, 250.0), (200.0, 60.0)):
        case, closed = constant_frames_case(B, H, W, n, *levels)
        total, last, grads = np_ssim_loss(*case)
        print(f'[ssim] constant frames {levels}: ssim {float(last):.6e}, closed form {closed:.6e}')
        assert abs(float(last) - closed) <= 1e-4 * closed
        assert abs(float(total) - (1 + DEFAULTS['gamma']) * closed) <= 1e-4 * (1 + DEFAULTS['gamma']) * closed
        assert abs(ssim_yardstick(case)[1] - closed) <= 1e-4 * closed
    # a pixel outside the interior has M = 0 and still receives gradient from the interior windows that contain it; upstream = 2
    # doubles bit for bit; accumulate adds in float32; add_to is added in double
    case = make_case(B, H, W, n, with_mask=False)
    total, last, grads = np_ssim_loss(*case)
    ring = ~interior_mask(H, W)
    assert any(g[:, ring].any() for g in grads)
    _, _, doubled = np_ssim_loss(*case, upstream=2.0)
    for a, b in zip(grads, doubled):
        np.testing.assert_array_equal(2 * a, b)
    fill = [np.full_like(g, 0.25) for g in grads]
    total2, _, acc = np_ssim_loss(*case, add_to=np.float32(1.5), prefill=fill)
    for a, b in zip(grads, acc):
        np.testing.assert_array_equal(np.float32(0.25) + a, b)
    assert abs(float(total2) - (1.5 + float(total))) <= 2.0 ** -23
    assert 0.0 < float(last) < 1.0                                       # |S| <= 1


# ------------------------------------------------------------------ the C entries
def test_ssim_entries_are_declared_exported_and_typed():
    from tf_raft_amd import build
    assert 'ssim_loss.hip' in build.SOURCES
    for name in ('raft_ssim_loss_workspace_bytes', 'raft_ssim_loss_f32'):
        assert _ffi._SIGNATURES[name] == _ffi._SIGNATURES[name.replace('ssim', 'census')], name
    _P, _I, _F = C.c_void_p, C.c_int, C.c_float
    assert _ffi._SIGNATURES['raft_ssim_loss_workspace_bytes'] == (C.c_int64, [_I, _I, _I, _I])
    assert _ffi._SIGNATURES['raft_ssim_loss_f32'] == (_I, [_P, _P, _P, _P, C.c_int64, _I, _I, _I, _I, C.c_double, _F, _F, _P, _P, _P,
                                                           _I, _P, _P])
    lib = _ffi.load_library()
    npix = 4 * 368 * 496
    need = lib.raft_ssim_loss_workspace_bytes(12, 4, 368, 496)
    assert need >= 4 * npix + 12 * npix * 8 and need % 8 == 0 and need < 80 << 20      # g1, and per prediction two float planes
    assert need <= lib.raft_census_loss_workspace_bytes(12, 4, 368, 496)
    assert lib.raft_ssim_loss_workspace_bytes(1, 1, 1, 1) > 0
    for bad in ((0, 1, 8, 8), (65, 1, 8, 8), (1, 0, 8, 8), (1, 1, -1, 8), (1, 1, 1 << 15, 1 << 15)):
        assert lib.raft_ssim_loss_workspace_bytes(*bad) == 0, bad


def test_ssim_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash.  The body of
    tests/test_census_loss.py::test_census_argument_errors_are_returned_before_any_device_work."""
    check_argument_errors(_ffi.load_library().raft_ssim_loss_f32)


# ------------------------------------------------------------------ Python-side validation (nothing here reaches the device)
def test_ssim_weight_is_validated_and_the_parent_signatures_stay():
    import inspect
    from tf_raft_amd import grad, losses
    loss = losses.SSIMSequenceLoss()
    assert isinstance(loss, losses.PhotometricSequenceLoss)
    assert loss.ssim_weight == 0.0 and loss.census_weight == 0.0
    assert loss._params() == dict(losses.PhotometricSequenceLoss()._params(), ssim_weight=0.0)
    assert losses.SSIMSequenceLoss(0.8, 0.1, 10.0, 0.01, 2, 3).ssim_weight == 3.0
    assert losses.SSIMSequenceLoss(0.8, 0.1, 10.0, 0.01, 2, 3).census_weight == 2.0
    assert losses.SSIMSequenceLoss(ssim_weight=np.float32(0.5))._params()['ssim_weight'] == 0.5
    for bad in (-0.1, float('nan'), float('inf'), 1e39, 'x', None, True, 1j, (1.0,)):
        with pytest.raises(ValueError, match='ssim_weight'):
            losses.SSIMSequenceLoss(ssim_weight=bad)
    with pytest.raises(ValueError, match='census_weight'):
        losses.SSIMSequenceLoss(census_weight=-1.0, ssim_weight=1.0)
    want = ['gamma', 'smooth_weight', 'edge_weight', 'eps', 'census_weight', 'ssim_weight']
    assert list(inspect.signature(losses.SSIMSequenceLoss.__init__).parameters) == ['self'] + want
    want = ['y_true', 'y_pred', 'gamma', 'smooth_weight', 'edge_weight', 'eps', 'upstream', 'census_weight', 'ssim_weight']
    for fn in (grad.ssim_sequence_loss_value_and_grad, grad.ssim_sequence_loss_grad):
        sig = inspect.signature(fn).parameters
        assert list(sig) == want, fn
        assert [sig[k].default for k in want[2:]] == [0.8, 0.1, 10.0, 0.01, 1.0, 0.0, 0.0]
    assert 'ssim_weight' not in inspect.signature(losses.PhotometricSequenceLoss.__init__).parameters
    assert inspect.signature(losses._photometric_launch).parameters['ssim_weight'].default == 0.0
    i1 = np.zeros((2, 8, 9, 3), np.float32)
    p = np.zeros((2, 8, 9, 2), np.float32)
    for fn in (grad.ssim_sequence_loss_grad, grad.ssim_sequence_loss_value_and_grad):
        with pytest.raises(ValueError, match='ssim_weight'):
            fn((i1, i1), [p], ssim_weight=-1.0)
        with pytest.raises(ValueError, match='upstream'):
            fn((i1, i1), [p], upstream=float('inf'), ssim_weight=1.0)
        with pytest.raises(ValueError, match='prediction'):                  # the shape checks still come before the device
            fn((i1, i1), [p[:, :4]], ssim_weight=1.0)
    with pytest.raises(ValueError, match='prediction'):
        losses.SSIMSequenceLoss(ssim_weight=1.0)((i1, i1), [p[:, :4]])


def test_compile_adds_the_ssim_mean_only_for_a_positive_weight():
    from tf_raft_amd import losses
    from tf_raft_amd.model import RAFT, SmallRAFT
    for cls in (RAFT, SmallRAFT):
        model = cls.__new__(cls)
        model.compile(optimizer=None, loss=losses.SSIMSequenceLoss(ssim_weight=0.5))
        assert list(model.flow_metrics) == ['loss', 'epe', 'u1', 'u3', 'u5', 'photometric', 'ssim', 'smoothness']
        with pytest.raises(ValueError, match=r'\(image1, image2\) or \(image1, image2, mask\)'):
            model.train_step((np.zeros((1, 64, 96, 3), np.float32),))
        model.compile(optimizer=None, loss=losses.SSIMSequenceLoss(census_weight=0.5, ssim_weight=0.5))
        assert list(model.flow_metrics) == ['loss', 'epe', 'u1', 'u3', 'u5', 'photometric', 'census', 'ssim', 'smoothness']
        model.compile(optimizer=None, loss=losses.SSIMSequenceLoss(census_weight=0.5))
        assert list(model.flow_metrics) == ['loss', 'epe', 'u1', 'u3', 'u5', 'photometric', 'census', 'smoothness']
        for loss in (losses.SSIMSequenceLoss(), losses.SSIMSequenceLoss(ssim_weight=0.0), losses.PhotometricSequenceLoss()):
            model.compile(optimizer=None, loss=loss)
            assert list(model.flow_metrics) == ['loss', 'epe', 'u1', 'u3', 'u5', 'photometric', 'smoothness']
        model.compile(optimizer=None)
        assert list(model.flow_metrics) == ['loss', 'epe', 'u1', 'u3', 'u5']

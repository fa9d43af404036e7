"""Self-supervised sequence loss, host side (no GPU).  This file holds

* the YARDSTICK ``torch_photometric_loss``: the definition in float64 torch, differentiated by autograd, checked here against
  central differences of its own value;
* the float32 NumPy RESTATEMENT ``np_photometric_loss`` with the analytic gradient, in the kernel's operation order, and its
  measured distance to the yardstick per case (``restatement_distance``): tests/test_gpu_photometric_loss.py takes four times
  that distance as the kernel's tolerance;
* the inputs both files use (``make_case``) and the cases with a known answer (``zero_flow_case``, ``shift_case``,
  ``out_of_frame_case``);
* the C entries' declarations and argument checks, the Python-side validation, and ``train_step``'s tuple-arity errors.

The definition, with s = 1/255, rho(d) = sqrt(d*d + eps*eps) (eps*eps rounded once to float32), w_i = float32(gamma**(n-i-1)):
the sample position of pixel (x, y) under (u, v) is sx = x + u, sy = y + v, in frame iff 0 <= sx <= W-1 and 0 <= sy <= H-1,
x0 = floor(sx), x1 = min(x0+1, W-1), a = sx - x0 (same along y), W2 the bilinear sample of image2 there;
    ph_i = sum mask * inside * rho(s * (W2_c - image1_c)) / (B*H*W*3)
    wx(x,y) = exp(-edge_weight * mean_c |s * (image1(x+1,y)_c - image1(x,y)_c)|), wy along y
    sm_i = [sum wx * rho(p(x+1,y)_k - p(x,y)_k) + sum wy * rho(p(x,y+1)_k - p(x,y)_k)] / (B*H*W*2)
    loss = sum_i w_i * (ph_i + smooth_weight * sm_i)
``smooth_weight``, ``edge_weight`` and ``eps`` cross the C ABI as float32, so both functions round them to float32 first.

Inputs (``make_case``): uint8-valued random images; flow components equal to an integer in [-amp, amp] plus a fraction drawn
from [1/16, 15/16], so that no sample position lies within 1/16 of a cell border or of the frame edge (the gradient is
discontinuous there and float32 and float64 may pick different cells); a mask at density 0.8.  ONE exception, so that the cases
with an axis of one pixel still have pixels in frame: along an axis of size 1 the component is exactly 0 (the sample sits on
the only row / column, x1 == x0, and the derivative along that axis is 0 in every precision).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tf_raft_amd import _ffi

DEFAULTS = dict(gamma=0.8, smooth_weight=0.1, edge_weight=10.0, eps=0.01)
# (B, H, W, n)        what it exercises on the GPU
CASES = [(1, 3, 5, 1),            # smaller than a wave
         (1, 1, 7, 2),            # no smoothness term along y
         (1, 6, 1, 2),            # no smoothness term along x
         (2, 37, 53, 3),          # nothing a multiple of 64 or 256
         (1, 3, 2051, 2),         # a row longer than a workgroup
         (2, 64, 96, 12),         # the model's smallest frame, the training n
         (1, 100, 150, 2)]        # several workgroups per image
CASE_IDS = ['x'.join(map(str, c)) for c in CASES]


def _f32(v):
    return float(np.float32(v))


def pred_weights(gamma, n):
    """gamma ** (n - i - 1) in double, rounded to float32 once (as raft_sequence_loss_f32 builds them)."""
    out = []
    for i in range(n):
        w = 1.0
        for _ in range(n - i - 1):
            w *= gamma
        out.append(_f32(w))
    return out


# ------------------------------------------------------------------ the yardstick: float64 torch, autograd
def torch_photometric_loss(image1, image2, mask, preds, gamma=0.8, smooth_weight=0.1, edge_weight=10.0, eps=0.01):
    """``(loss, ph_last, sm_last)`` as 0-d float64 tensors; ``preds`` float64 tensors (B, H, W, 2) that may require grad."""
    i1 = torch.as_tensor(np.asarray(image1), dtype=torch.float64) if not isinstance(image1, torch.Tensor) else image1.double()
    i2 = torch.as_tensor(np.asarray(image2), dtype=torch.float64) if not isinstance(image2, torch.Tensor) else image2.double()
    B, H, W, _ = i1.shape
    m = torch.ones((B, H, W), dtype=torch.float64) if mask is None else (torch.as_tensor(np.asarray(mask)) != 0).double()
    s = 1.0 / 255.0
    sw, ew = _f32(smooth_weight), _f32(edge_weight)
    eps2 = float(np.float32(eps) * np.float32(eps))
    wx = torch.exp(-ew * (s * (i1[:, :, 1:] - i1[:, :, :-1])).abs().mean(-1))          # (B, H, W-1)
    wy = torch.exp(-ew * (s * (i1[:, 1:] - i1[:, :-1])).abs().mean(-1))                # (B, H-1, W)
    rho = lambda d: torch.sqrt(d * d + eps2)
    xs = torch.arange(W, dtype=torch.float64)[None, None, :]
    ys = torch.arange(H, dtype=torch.float64)[None, :, None]
    nb = torch.arange(B)[:, None, None]
    total, ph, sm = 0.0, None, None
    for w_i, p in zip(pred_weights(gamma, len(preds)), preds):
        sx, sy = xs + p[..., 0], ys + p[..., 1]
        inside = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
        px, py = torch.where(inside, sx, torch.zeros_like(sx)), torch.where(inside, sy, torch.zeros_like(sy))
        x0, y0 = torch.floor(px).detach().long(), torch.floor(py).detach().long()
        x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
        a, b = (px - x0)[..., None], (py - y0)[..., None]
        w2 = (1 - b) * ((1 - a) * i2[nb, y0, x0] + a * i2[nb, y0, x1]) + b * ((1 - a) * i2[nb, y1, x0] + a * i2[nb, y1, x1])
        ph = ((m * inside.double())[..., None] * rho(s * (w2 - i1))).sum() / (B * H * W * 3)
        sm = ((wx[..., None] * rho(p[:, :, 1:] - p[:, :, :-1])).sum() + (wy[..., None] * rho(p[:, 1:] - p[:, :-1])).sum()) / (B * H * W * 2)
        total = total + w_i * (ph + sw * sm)
    return total, ph, sm


def yardstick(case, **params):
    """Value and autograd gradient of the yardstick on ``case`` = (image1, image2, mask, preds as float32 arrays):
    ``(loss, ph_last, sm_last, [gradients])`` as float64 NumPy."""
    image1, image2, mask, preds = case
    ps = [torch.tensor(np.asarray(p), dtype=torch.float64, requires_grad=True) for p in preds]
    loss, ph, sm = torch_photometric_loss(image1, image2, mask, ps, **params)
    grads = torch.autograd.grad(loss, ps, allow_unused=True)
    grads = [np.zeros(tuple(p.shape)) if g is None else g.numpy() for g, p in zip(grads, ps)]
    return float(loss.detach()), float(ph.detach()), float(sm.detach()), grads


# ------------------------------------------------------------------ the restatement: float32 NumPy, analytic gradient
def np_photometric_loss(image1, image2, mask, preds, gamma=0.8, smooth_weight=0.1, edge_weight=10.0, eps=0.01, upstream=1.0):
    """The kernel's arithmetic: every per-pixel operation in float32 in the kernel's order, the sums over pixels in float64.
    ``(loss, ph_last, sm_last, [gradients])``: three float32 scalars and float32 arrays."""
    f = np.float32
    i1, i2 = np.asarray(image1, f), np.asarray(image2, f)
    B, H, W, _ = i1.shape
    use = np.ones((B, H, W), bool) if mask is None else np.asarray(mask) != 0
    s, eps2, sw, ew, up = f(1) / f(255), f(eps) * f(eps), f(smooth_weight), f(edge_weight), f(upstream)
    npix = B * H * W
    inv3d, inv2d = 1.0 / (npix * 3.0), 1.0 / (npix * 2.0)
    inv3, inv2 = f(inv3d), f(inv2d)

    def edge(d):
        m = ((np.abs(s * d[..., 0]) + np.abs(s * d[..., 1])) + np.abs(s * d[..., 2])) / f(3)
        return np.exp(-ew * m)

    rho = lambda d: np.sqrt(d * d + eps2)
    wx, wy = np.zeros((B, H, W), f), np.zeros((B, H, W), f)
    wx[:, :, :-1] = edge(i1[:, :, 1:] - i1[:, :, :-1])
    wy[:, :-1] = edge(i1[:, 1:] - i1[:, :-1])
    nb = np.arange(B)[:, None, None]
    weights = pred_weights(gamma, len(preds))
    tot_ph = tot_sm = 0.0
    last = (0.0, 0.0)
    grads = []
    for w_i, p in zip(weights, preds):
        p = np.asarray(p, f)
        sx = np.arange(W, dtype=f)[None, None, :] + p[..., 0]
        sy = np.arange(H, dtype=f)[None, :, None] + p[..., 1]
        inside = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
        px, py = np.where(inside, sx, f(0)), np.where(inside, sy, f(0))
        fx, fy = np.floor(px), np.floor(py)
        x0, y0 = np.clip(fx.astype(np.int64), 0, W - 1), np.clip(fy.astype(np.int64), 0, H - 1)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        a, b = (px - fx)[..., None], (py - fy)[..., None]
        na, nbb = f(1) - a, f(1) - b
        g00, g01, g10, g11 = i2[nb, y0, x0], i2[nb, y0, x1], i2[nb, y1, x0], i2[nb, y1, x1]
        w2 = nbb * (na * g00 + a * g01) + b * (na * g10 + a * g11)
        d = s * (w2 - i1)
        r = rho(d)
        on = inside & use
        ph_pix = np.where(on, (r[..., 0] + r[..., 1]) + r[..., 2], f(0))
        q = (d / r) * s
        du = nbb * (g01 - g00) + b * (g11 - g10)
        dv = na * (g10 - g00) + a * (g11 - g01)
        gu = (q[..., 0] * du[..., 0] + q[..., 1] * du[..., 1]) + q[..., 2] * du[..., 2]
        gv = (q[..., 0] * dv[..., 0] + q[..., 1] * dv[..., 1]) + q[..., 2] * dv[..., 2]
        gph = np.where(on[..., None], np.stack([gu, gv], -1), f(0))
        # smoothness: value of the differences each pixel owns, gradient as a gather of the four t's
        dx, dy = p[:, :, 1:] - p[:, :, :-1], p[:, 1:] - p[:, :-1]
        rx, ry = rho(dx), rho(dy)
        sm_pix = np.zeros((B, H, W), f)
        sm_pix[:, :, :-1] = wx[:, :, :-1] * (rx[..., 0] + rx[..., 1])
        sm_pix[:, :-1] = sm_pix[:, :-1] + wy[:, :-1] * (ry[..., 0] + ry[..., 1])
        tx, ty = np.zeros((B, H, W, 2), f), np.zeros((B, H, W, 2), f)
        tx[:, :, :-1] = wx[:, :, :-1, None] * (dx / rx)
        ty[:, :-1] = wy[:, :-1, :, None] * (dy / ry)
        gsm = -tx - ty
        gsm[:, :, 1:] = gsm[:, :, 1:] + tx[:, :, :-1]
        gsm[:, 1:] = gsm[:, 1:] + ty[:, :-1]
        g = (up * f(w_i)) * (gph * inv3 + sw * (gsm * inv2))
        assert g.dtype == f and ph_pix.dtype == f and sm_pix.dtype == f
        grads.append(g)
        last = (float(ph_pix.astype(np.float64).sum()), float(sm_pix.astype(np.float64).sum()))
        tot_ph += w_i * last[0]
        tot_sm += w_i * last[1]
    loss = f(tot_ph * inv3d + float(sw) * (tot_sm * inv2d))
    return loss, f(last[0] * inv3d), f(last[1] * inv2d), grads


# ------------------------------------------------------------------ the inputs both test files use
def make_case(B, H, W, n, seed=0, amp=3, with_mask=True):
    """``(image1, image2, mask or None, [n flows])`` as described in the module docstring (float32 / uint8 NumPy)."""
    rng = np.random.default_rng(1000 * seed + 7 * H + W + n)
    image1 = rng.integers(0, 256, size=(B, H, W, 3)).astype(np.float32)
    image2 = rng.integers(0, 256, size=(B, H, W, 3)).astype(np.float32)
    mask = (rng.uniform(size=(B, H, W)) < 0.8).astype(np.uint8)
    preds = []
    for _ in range(n):
        whole = rng.integers(-amp, amp + 1, size=(B, H, W, 2)).astype(np.float64)
        p = (whole + rng.uniform(1 / 16, 15 / 16, size=(B, H, W, 2))).astype(np.float32)
        if W == 1:
            p[..., 0] = 0
        if H == 1:
            p[..., 1] = 0
        preds.append(p)
    return image1, image2, (mask if with_mask else None), preds


@functools.lru_cache(maxsize=None)
def restatement_distance(B, H, W, n, with_mask):
    """The restatement against the yardstick on ``make_case(B, H, W, n)``: ``(relative distance of the loss, max |difference| of
    the gradient, max |gradient|)``.  The GPU test's tolerances are four times the first two."""
    case = make_case(B, H, W, n, with_mask=with_mask)
    want_loss, _, _, want_g = yardstick(case, **DEFAULTS)
    loss, _, _, g = np_photometric_loss(*case, **DEFAULTS)
    diff = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(g, want_g))
    return abs(float(loss) - want_loss) / abs(want_loss), diff, max(float(np.abs(b).max()) for b in want_g)


# ------------------------------------------------------------------ cases with a known answer
def edge_weight_sums(image1, edge_weight=10.0):
    """sum wx + sum wy in float64."""
    i1 = np.asarray(image1, np.float64) / 255.0
    ew = _f32(edge_weight)
    return float(np.exp(-ew * np.abs(i1[:, :, 1:] - i1[:, :, :-1]).mean(-1)).sum() + np.exp(-ew * np.abs(i1[:, 1:] - i1[:, :-1]).mean(-1)).sum())


def rho0(eps=0.01):
    """rho(0) = sqrt(float32(eps)^2 rounded to float32), in float64."""
    return float(np.sqrt(np.float64(np.float32(eps) * np.float32(eps))))


def zero_flow_case(B, H, W, n, seed=3):
    """image2 == image1 and zero flow: ``(case, closed)`` with ``closed`` = {'photometric', 'smoothness'} (gradient 0 everywhere)."""
    image1, _, mask, preds = make_case(B, H, W, n, seed=seed)
    preds = [np.zeros_like(p) for p in preds]
    closed = {'photometric': rho0() * float(mask.mean()),
              'smoothness': rho0() * edge_weight_sums(image1) * 2 / (B * H * W * 2)}
    return (image1, image1.copy(), mask, preds), closed


def shift_case(B, H, W, n, d, seed=4):
    """A constant integer flow ``d`` = (dx, dy) with image2 the matching shift of image1 (image2(x + dx, y + dy) = image1(x, y)
    wherever that is in frame, noise elsewhere): gradient 0, photometric = rho(0) * |inside & mask| / (B*H*W), smoothness =
    rho(0) * (sum wx + sum wy) * 2 / (B*H*W*2)."""
    image1, image2, mask, preds = make_case(B, H, W, n, seed=seed)
    dx, dy = d
    ys, xs = np.mgrid[0:H, 0:W]
    inside = (xs + dx >= 0) & (xs + dx <= W - 1) & (ys + dy >= 0) & (ys + dy <= H - 1)
    image2 = image2.copy()
    image2[:, (ys + dy)[inside], (xs + dx)[inside]] = image1[:, ys[inside], xs[inside]]
    preds = [np.broadcast_to(np.array(d, np.float32), p.shape).copy() for p in preds]
    closed = {'photometric': rho0() * float((inside[None] & (mask != 0)).sum()) / (B * H * W),
              'smoothness': rho0() * edge_weight_sums(image1) * 2 / (B * H * W * 2)}
    return (image1, image2, mask, preds), closed


def out_of_frame_case(B, H, W, n, seed=5):
    """Every vector points out of frame (alternately past each border, by non-integer amounts): with smooth_weight = 0 the loss and
    the gradient are exactly 0."""
    image1, image2, mask, preds = make_case(B, H, W, n, seed=seed)
    ys, xs = np.mgrid[0:H, 0:W]
    out = []
    for i, p in enumerate(preds):
        q = p.copy()
        way = (ys + xs + i) % 4
        q[:, way == 0, 0] = (-xs - 0.5)[way == 0]              # half a pixel past the left border
        q[:, way == 1, 0] = (W - xs - 0.75)[way == 1]          # a quarter past the right border
        q[:, way == 2, 1] = (-ys - 1.5)[way == 2]
        q[:, way == 3, 1] = (H - ys + 0.25)[way == 3]
        out.append(q)
    return image1, image2, mask, out


def ulps(got, want):
    """|got - want| in units of the float32 spacing at ``want``."""
    return abs(float(got) - float(want)) / float(np.spacing(np.float32(abs(want))))


# ------------------------------------------------------------------ yardstick and restatement
def test_the_yardstick_gradient_matches_central_differences():
    rng = np.random.default_rng(11)
    case = make_case(2, 9, 13, 2)
    image1, image2, mask, preds = case
    _, _, _, grads = yardstick(case, **DEFAULTS)
    value = lambda ps: float(torch_photometric_loss(image1, image2, mask, [torch.tensor(p, dtype=torch.float64) for p in ps], **DEFAULTS)[0])
    base = [np.asarray(p, np.float64) for p in preds]
    h, worst = 1e-6, 0.0
    for _ in range(20):
        i = int(rng.integers(len(preds)))
        idx = tuple(int(rng.integers(d)) for d in base[i].shape)
        hi, lo = [b.copy() for b in base], [b.copy() for b in base]
        hi[i][idx] += h
        lo[i][idx] -= h
        fd = (value(hi) - value(lo)) / (2 * h)
        want = grads[i][idx]
        worst = max(worst, abs(fd - want) / (1e-5 * abs(want) + 1e-10))
        assert abs(fd - want) <= 1e-5 * abs(want) + 1e-10, (i, idx, fd, want)       # (1e-10: rounding of the value over 2h)
    assert any(np.abs(g).max() > 0 for g in grads)
    print(f'[photometric] yardstick against central differences: worst |difference| / bound = {worst:.2e}')


@pytest.mark.parametrize('with_mask', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('shape', CASES, ids=CASE_IDS)
def test_the_restatement_is_close_to_the_yardstick(shape, with_mask):
    rel_loss, diff_g, max_g = restatement_distance(*shape, with_mask)
    print(f'[photometric] restatement {shape} mask={with_mask}: loss rel {rel_loss:.2e}, gradient {diff_g / max_g:.2e} of max|g| = {max_g:.3e}')
    assert max_g > 0
    assert rel_loss <= 2e-3
    assert diff_g / max_g <= 2e-3
    case = make_case(*shape, with_mask=with_mask)
    _, want_ph, want_sm, _ = yardstick(case, **DEFAULTS)
    _, ph, sm, _ = np_photometric_loss(*case, **DEFAULTS)
    assert abs(float(ph) - want_ph) <= 2e-3 * abs(want_ph) and abs(float(sm) - want_sm) <= 2e-3 * max(abs(want_sm), 1e-30)
    inside_any = float(ph) > 0
    assert inside_any, 'no pixel of the case is in frame'


def test_the_restatement_on_the_cases_with_a_known_answer():
    B, H, W, n = 2, 37, 53, 2
    case, closed = zero_flow_case(B, H, W, n)
    loss, ph, sm, grads = np_photometric_loss(*case, **DEFAULTS)
    assert all(not g.any() for g in grads)
    assert ulps(ph, closed['photometric']) <= 4 and ulps(sm, closed['smoothness']) <= 4
    for d in ((3, -2), (-5, 1)):
        case, closed = shift_case(B, H, W, n, d)
        loss, ph, sm, grads = np_photometric_loss(*case, **DEFAULTS)
        assert all(not g.any() for g in grads), d
        assert ulps(ph, closed['photometric']) <= 4 and ulps(sm, closed['smoothness']) <= 4, d
        want = yardstick(case, **DEFAULTS)
        assert abs(want[1] - closed['photometric']) <= 1e-12 and abs(want[2] - closed['smoothness']) <= 1e-12
        assert all(np.abs(g).max() <= 1e-15 for g in want[3])
    case = out_of_frame_case(B, H, W, n)
    params = dict(DEFAULTS, smooth_weight=0.0)
    loss, ph, sm, grads = np_photometric_loss(*case, **params)
    assert float(loss) == 0.0 and float(ph) == 0.0 and all(not g.any() for g in grads)
    assert yardstick(case, **params)[0] == 0.0
    # masked pixels receive exactly the smoothness-only gradient: image2 does not reach them
    image1, image2, mask, preds = make_case(B, H, W, n)
    noise = np.random.default_rng(9).integers(0, 256, size=image2.shape).astype(np.float32)
    g_a = np_photometric_loss(image1, image2, mask, preds, **DEFAULTS)[3]
    g_b = np_photometric_loss(image1, noise, mask, preds, **DEFAULTS)[3]
    for a, b in zip(g_a, g_b):
        np.testing.assert_array_equal(a[mask == 0], b[mask == 0])
        assert (a[mask != 0] != b[mask != 0]).any()
    # gamma = 1: the sum of the single-prediction losses; upstream = 2 doubles the gradient bit for bit
    one = dict(DEFAULTS, gamma=1.0)
    total = float(np_photometric_loss(image1, image2, mask, preds, **one)[0])
    parts = sum(float(np_photometric_loss(image1, image2, mask, [p], **one)[0]) for p in preds)
    assert abs(total - parts) <= 1e-6 * abs(parts)
    g_2 = np_photometric_loss(image1, image2, mask, preds, upstream=2.0, **DEFAULTS)[3]
    for a, b in zip(g_a, g_2):
        np.testing.assert_array_equal(2 * a, b)


# ------------------------------------------------------------------ the C entries
def test_photometric_entries_are_declared_exported_and_mirrored():
    """The unit is built and sizes its workspace (the prototypes: tests/test_host_logic.py test_the_binding_is_the_header)."""
    from tf_raft_amd import build
    assert 'photometric_loss.hip' in build.SOURCES and 'flow_sample.h' in build.HEADERS
    assert _ffi.load_library().raft_photometric_loss_workspace_doubles() >= 4


def test_photometric_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    fn = lib.raft_photometric_loss_f32
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off = C.c_void_p(p.value + 4)
    #       image1 image2 mask preds stride n  B  H  W  gamma sw   ew    eps  upstream out3 d_preds ws stream
    good = [p, p, p, p, 2 * 20, 3, 1, 4, 5, 0.8, 0.1, 10.0, 0.01, 1.0, p, p, p, None]
    for k in (0, 1, 3, 14, 16):                                             # (mask and d_preds may be NULL)
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    for k in (5, 6, 7, 8):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for bad in ((1, 1 << 15, 1 << 15), (1 << 10, 1 << 10, 1 << 10), (1, 1, 1 << 30), (1, 26755, 26755)):   # B*H*W*3 reaches 2^31
        args = list(good)
        args[6:9] = bad
        args[4] = 1 << 40
        assert fn(*args) == -2, bad
    args = list(good)
    args[4] = 2 * 20 - 2                                                    # predictions would overlap
    assert fn(*args) == -2
    args[4] = 2 * 20 + 1                                                    # read as float2
    assert fn(*args) == -3
    args = list(good)
    args[5] = 65
    assert fn(*args) == -3
    for v in (0.0, -0.01, 1e-30, 1e30, float('nan'), float('inf')):         # (1e-30, 1e30: eps * eps is 0 / infinite in float32)
        args = list(good)
        args[12] = v
        assert fn(*args) == -2, v
    for k in (9, 10, 11):
        for v in (-1e-3, float('nan'), float('inf'), -float('inf')):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for v in (float('nan'), float('inf')):
        args = list(good)
        args[13] = v
        assert fn(*args) == -2, v
    for k in (3, 15, 16):
        args = list(good)
        args[k] = off
        assert fn(*args) == -4, k
    for m, d in ((None, None), (p, None), (None, p)):                       # a NULL mask or d_preds is not an error of its own
        args = list(good)
        args[2], args[15], args[5] = m, d, 65
        assert fn(*args) == -3, (m, d)


# ------------------------------------------------------------------ Python-side validation (nothing here reaches the device)
def test_parameters_and_shapes_are_checked_without_a_gpu():
    from tf_raft_amd import grad, losses
    loss = losses.PhotometricSequenceLoss()
    assert (loss.gamma, loss.smooth_weight, loss.edge_weight, loss.eps) == (0.8, 0.1, 10.0, 0.01)
    assert losses.PhotometricSequenceLoss(1, 0, np.float32(2), 1e-3).gamma == 1.0
    for name in ('gamma', 'smooth_weight', 'edge_weight'):
        for bad in (-0.1, float('nan'), float('inf'), 1e39, 'x', None, True, 1j, (1.0,)):
            with pytest.raises(ValueError, match=name):
                losses.PhotometricSequenceLoss(**{name: bad})
    for bad in (0, -1e-3, 1e-50, 1e-30, 1e30, float('nan'), float('inf'), 'x', None):
        with pytest.raises(ValueError, match='eps'):
            losses.PhotometricSequenceLoss(eps=bad)
    i1, i2 = np.zeros((2, 4, 5, 3), np.float32), np.zeros((2, 4, 5, 3), np.float32)
    p = np.zeros((2, 4, 5, 2), np.float32)
    m = np.ones((2, 4, 5), np.uint8)
    calls = (loss, loss.terms, losses.photometric_sequence_loss, grad.photometric_sequence_loss_grad,
             grad.photometric_sequence_loss_value_and_grad)
    for fn in calls:
        for y_true, preds, what in (((i1,), [p], 'y_true'), ((i1, i2, m, m), [p], 'y_true'), (None, [p], 'y_true'),
                                    ((i1[..., :2], i2), [p], 'image1'), ((i1[0], i2[0]), [p], 'image1'),
                                    ((i1, i2[:, :3]), [p], 'image2'), ((i1, torch.zeros((2, 4, 5, 1))), [p], 'image2'),
                                    ((i1, i2, m[:1]), [p], 'mask'), ((i1, i2, np.ones((2, 4, 5, 1))), [p], 'mask'),
                                    ((i1, i2), [p, p[:, :, :4]], 'prediction'), ((i1, i2, m), [i1], 'prediction'),
                                    ((i1, i2), [p] * 65, '64')):
            with pytest.raises(ValueError, match=what):
                fn(y_true, preds)
    for fn in calls[2:]:
        with pytest.raises(ValueError, match='eps'):
            fn((i1, i2), [p], eps=0.0)
        with pytest.raises(ValueError, match='smooth_weight'):
            fn((i1, i2), [p], smooth_weight=-1.0)
    for fn in calls[3:]:
        with pytest.raises(ValueError, match='upstream'):
            fn((i1, i2), [p], upstream=float('nan'))


def test_compile_and_train_step_check_the_loss_and_the_tuple_arity():
    from tf_raft_amd import losses
    from tf_raft_amd.model import RAFT, SmallRAFT
    x = np.zeros((1, 64, 96, 3), np.float32)
    flow, valid, mask = np.zeros((1, 64, 96, 2), np.float32), np.ones((1, 64, 96), bool), np.ones((1, 64, 96), np.uint8)
    for cls in (RAFT, SmallRAFT):
        model = cls.__new__(cls)
        model.compile(optimizer=None, loss=losses.PhotometricSequenceLoss(smooth_weight=0.2))
        assert isinstance(model.loss, losses.PhotometricSequenceLoss) and model.loss.smooth_weight == 0.2
        assert {'loss', 'photometric', 'smoothness'} <= set(model.flow_metrics)
        for data in ((x, x, flow, valid), (x,), ()):
            with pytest.raises(ValueError, match=r'\(image1, image2\) or \(image1, image2, mask\)'):
                model.train_step(data)
        model.compile(optimizer=None)
        assert model.loss is losses.sequence_loss and list(model.flow_metrics) == ['loss', 'epe', 'u1', 'u3', 'u5']
        for data in ((x, x), (x, x, mask)):
            with pytest.raises(ValueError, match=r'\(image1, image2, flow, valid\)'):
                model.train_step(data)
        model.compile(optimizer=None, loss=lambda y_true, y_pred: 0.0)
        with pytest.raises(NotImplementedError):
            model.train_step((x, x, flow, valid))

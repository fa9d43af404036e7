"""Second-order, edge-aware smoothness of the self-supervised loss, host side (no GPU).  This file holds

* the YARDSTICK ``torch_smooth2_loss``: the definition in float64 torch, differentiated by autograd, checked here against
  central differences of its own value;
* the float32 NumPy RESTATEMENT ``np_smooth2_loss`` with the analytic gradient, in the kernel's operation order, and its measured
  distance to the yardstick per shape (``smooth2_restatement_distance``): tests/test_gpu_smooth2_loss.py takes four times that
  distance as the kernel's tolerance, the rule of sections 17 to 19;
* the cases with a known answer (``affine_case``, ``quadratic_case``, a constant ``image1``);
* the C entries' declarations and argument checks, the Python-side validation, and the keys ``train_step`` reports.

The definition, with s = 1/255, eps2 = float32(eps)^2 rounded once to float32, rho(d) = sqrt(d*d + eps2),
w_i = float32(gamma**(n-i-1)), for prediction p = p_i and component k:
    cx(x,y) = exp(-edge_weight * mean_c |s * (image1(x+1,y)_c - image1(x-1,y)_c)|)   1 <= x <= W-2 (no term otherwise)
    cy(x,y) = the same along y                                                        1 <= y <= H-2
    Dx_k(x,y) = (p(x+1,y)_k - 2*p(x,y)_k) + p(x-1,y)_k,    Dy_k likewise
    sm2_i = [sum cx * rho(Dx_k) + sum cy * rho(Dy_k)] / (B*H*W*2)
    value = add_to + smooth2_weight * sum_i w_i * sm2_i
``smooth2_weight``, ``edge_weight`` and ``eps`` cross the C ABI as float32, so both functions round them to float32 first.
The inputs are ``test_photometric_loss.make_case``'s (``image2`` and the mask play no part).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tf_raft_amd import _ffi
from test_photometric_loss import DEFAULTS, make_case, pred_weights, rho0, ulps

PARAMS = dict(gamma=DEFAULTS['gamma'], edge_weight=DEFAULTS['edge_weight'], eps=DEFAULTS['eps'])
TILE = (32, 8)                    # csrc/smooth2_loss.hip: kTW x kTH
# (B, H, W, n)        what it exercises on the GPU
CASES = [(1, 3, 3, 1),            # one stencil per axis
         (1, 2, 7, 2),            # no stencil along y
         (1, 1, 9, 2),            # no stencil along y, one row
         (1, 6, 2, 2),            # no stencil along x
         (1, 2, 2, 1),            # no stencil at all: value 0, gradient 0
         (2, 37, 53, 3),          # no multiple of anything
         (1, 5, 2051, 2),         # a row across many tiles
         (2, 64, 96, 12),         # the model's smallest frame, the training n
         (1, 33, 65, 2)]          # both sides one more than a multiple of the tile's
CASE_IDS = ['x'.join(map(str, c)) for c in CASES]
NO_STENCIL = (1, 2, 2, 1)


def _f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------ the yardstick: float64 torch, autograd
def torch_smooth2_loss(image1, preds, gamma=0.8, smooth2_weight=1.0, edge_weight=10.0, eps=0.01, add_to=0.0):
    """``(value, sm2_last)`` as 0-d float64 tensors; ``preds`` float64 tensors (B, H, W, 2) that may require grad."""
    i1 = torch.as_tensor(np.asarray(image1), dtype=torch.float64) if not isinstance(image1, torch.Tensor) else image1.double()
    B, H, W, _ = i1.shape
    s = 1.0 / 255.0
    w2, ew = _f32(smooth2_weight), _f32(edge_weight)
    eps2 = float(np.float32(eps) * np.float32(eps))
    cx = torch.exp(-ew * (s * (i1[:, :, 2:] - i1[:, :, :-2])).abs().mean(-1))          # (B, H, W-2): centres 1 .. W-2
    cy = torch.exp(-ew * (s * (i1[:, 2:] - i1[:, :-2])).abs().mean(-1))                # (B, H-2, W)
    rho = lambda d: torch.sqrt(d * d + eps2)
    total, sm2 = torch.zeros((), dtype=torch.float64) + add_to, torch.zeros((), dtype=torch.float64)
    for w_i, p in zip(pred_weights(gamma, len(preds)), preds):
        dx = (p[:, :, 2:] - 2 * p[:, :, 1:-1]) + p[:, :, :-2]
        dy = (p[:, 2:] - 2 * p[:, 1:-1]) + p[:, :-2]
        sm2 = ((cx[..., None] * rho(dx)).sum() + (cy[..., None] * rho(dy)).sum()) / (B * H * W * 2)
        total = total + w2 * w_i * sm2
    return total, sm2


def smooth2_yardstick(image1, preds, **params):
    """Value and autograd gradient of the yardstick: ``(value, sm2_last, [gradients])`` as float64 NumPy."""
    ps = [torch.tensor(np.asarray(p), dtype=torch.float64, requires_grad=True) for p in preds]
    value, last = torch_smooth2_loss(image1, ps, **params)
    if value.requires_grad:
        grads = torch.autograd.grad(value, ps, allow_unused=True)
    else:                                                    # (no stencil anywhere: the value does not depend on the predictions)
        grads = [None] * len(ps)
    grads = [np.zeros(tuple(p.shape)) if g is None else g.numpy() for g, p in zip(grads, ps)]
    return float(value.detach()), float(last.detach()), grads


# ------------------------------------------------------------------ the restatement: float32 NumPy, analytic gradient
def np_smooth2_loss(image1, preds, gamma=0.8, smooth2_weight=1.0, edge_weight=10.0, eps=0.01, upstream=1.0, add_to=None):
    """The kernel's arithmetic: every per-pixel operation in float32 in the kernel's order, the sums over pixels in float64.
    ``(out2 as two float32, [gradients as float32 arrays])``."""
    f = np.float32
    i1 = np.asarray(image1, f)
    B, H, W, _ = i1.shape
    s, eps2, w2, ew, up = f(1) / f(255), f(eps) * f(eps), f(smooth2_weight), f(edge_weight), f(upstream)
    inv2d = 1.0 / (B * H * W * 2.0)
    inv2 = f(inv2d)

    def edge(d):
        m = ((np.abs(s * d[..., 0]) + np.abs(s * d[..., 1])) + np.abs(s * d[..., 2])) / f(3)
        return np.exp(-ew * m)

    rho = lambda d: np.sqrt(d * d + eps2)
    cx, cy = np.zeros((B, H, W), f), np.zeros((B, H, W), f)                # 0 where no stencil is centred
    cx[:, :, 1:-1] = edge(i1[:, :, 2:] - i1[:, :, :-2])
    cy[:, 1:-1] = edge(i1[:, 2:] - i1[:, :-2])
    hasx, hasy = np.zeros((B, H, W), bool), np.zeros((B, H, W), bool)
    hasx[:, :, 1:-1] = True
    hasy[:, 1:-1] = True
    weights = pred_weights(gamma, len(preds))
    total, last, grads = 0.0, 0.0, []
    for w_i, p in zip(weights, preds):
        p = np.asarray(p, f)
        dx, dy = np.zeros_like(p), np.zeros_like(p)                        # (a centre without a stencil: D = 0, weight 0)
        dx[:, :, 1:-1] = (p[:, :, 2:] - f(2) * p[:, :, 1:-1]) + p[:, :, :-2]
        dy[:, 1:-1] = (p[:, 2:] - f(2) * p[:, 1:-1]) + p[:, :-2]
        rx, ry = rho(dx), rho(dy)
        sm = cx * (rx[..., 0] + rx[..., 1]) + cy * (ry[..., 0] + ry[..., 1])          # (an edge weight that does not exist is 0)
        qx = np.where(hasx[..., None], cx[..., None] * (dx / rx), f(0))
        qy = np.where(hasy[..., None], cy[..., None] * (dy / ry), f(0))
        qxp = np.pad(qx, ((0, 0), (0, 0), (1, 1), (0, 0)))
        qyp = np.pad(qy, ((0, 0), (1, 1), (0, 0), (0, 0)))
        g = ((qxp[:, :, :-2] - f(2) * qx) + qxp[:, :, 2:]) + ((qyp[:, :-2] - f(2) * qy) + qyp[:, 2:])
        d = ((up * w2) * f(w_i)) * (g * inv2)
        assert d.dtype == f and sm.dtype == f
        grads.append(d)
        last = float(sm.astype(np.float64).sum())
        total += w_i * last
    before = 0.0 if add_to is None else float(f(add_to))
    return np.array([f(before + float(w2) * (total * inv2d)), f(last * inv2d)], f), grads


@functools.lru_cache(maxsize=None)
def smooth2_restatement_distance(B, H, W, n):
    """The restatement against the yardstick on ``make_case(B, H, W, n)``: ``(relative distance of the loss, max |difference| of
    the gradient, max |gradient|)``.  The GPU test's tolerances are four times the first two.  (Without a stencil all are 0.)"""
    image1, _, _, preds = make_case(B, H, W, n)
    want, _, want_g = smooth2_yardstick(image1, preds, **PARAMS)
    out2, g = np_smooth2_loss(image1, preds, **PARAMS)
    diff = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(g, want_g))
    rel = abs(float(out2[0]) - want) / abs(want) if want != 0.0 else abs(float(out2[0]))
    return rel, diff, max(float(np.abs(b).max()) for b in want_g)


# ------------------------------------------------------------------ cases with a known answer
def central_edge_weight_sums(image1, edge_weight=10.0):
    """sum cx + sum cy in float64."""
    i1 = np.asarray(image1, np.float64) / 255.0
    ew = _f32(edge_weight)
    return float(np.exp(-ew * np.abs(i1[:, :, 2:] - i1[:, :, :-2]).mean(-1)).sum() + np.exp(-ew * np.abs(i1[:, 2:] - i1[:, :-2]).mean(-1)).sum())


def affine_case(B, H, W, n, seed=6):
    """Flows ``u = a + b*x + c*y``, ``v`` likewise, slopes multiples of 1/16 that differ per prediction: every second difference is
    exactly 0 in float32, the gradient exactly 0 and the value ``sqrt(eps2) * (2*sum cx + 2*sum cy) / (B*H*W*2)``.
    ``(image1, preds, closed sm2)``."""
    image1 = make_case(B, H, W, n, seed=seed)[0]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    preds = []
    for i in range(n):
        u = np.float32(0.5 + i) + np.float32((3 + i) / 16) * xs - np.float32(5 / 16) * ys
        v = np.float32(-1.25) - np.float32(7 / 16) * xs + np.float32((1 + 2 * i) / 16) * ys
        preds.append(np.broadcast_to(np.stack([u, v], -1)[None], (B, H, W, 2)).astype(np.float32).copy())
    return image1, preds, rho0(PARAMS['eps']) * 2 * central_edge_weight_sums(image1, PARAMS['edge_weight']) / (B * H * W * 2)


def quadratic_case(B, H, W, n, seed=7, constant_image=False):
    """``u = x^2/8``, ``v = y^2/16``: ``Dx_u = 1/4`` and ``Dy_v = 1/8`` exactly, ``Dx_v = Dy_u = 0``, so
    ``sm2 = [sum cx * (rho(1/4) + rho(0)) + sum cy * (rho(0) + rho(1/8))] / (B*H*W*2)``.  ``(image1, preds, closed sm2)``."""
    image1 = make_case(B, H, W, n, seed=seed)[0]
    if constant_image:
        image1 = np.full_like(image1, 77.0)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    flow = np.stack([xs * xs / np.float32(8), ys * ys / np.float32(16)], -1)
    assert (flow == np.stack([xs.astype(np.float64) ** 2 / 8, ys.astype(np.float64) ** 2 / 16], -1)).all()        # exact in float32
    preds = [np.broadcast_to(flow[None], (B, H, W, 2)).astype(np.float32).copy() for _ in range(n)]
    i1 = np.asarray(image1, np.float64) / 255.0
    ew = _f32(PARAMS['edge_weight'])
    sum_cx = float(np.exp(-ew * np.abs(i1[:, :, 2:] - i1[:, :, :-2]).mean(-1)).sum())
    sum_cy = float(np.exp(-ew * np.abs(i1[:, 2:] - i1[:, :-2]).mean(-1)).sum())
    eps2 = float(np.float32(PARAMS['eps']) * np.float32(PARAMS['eps']))
    r = lambda d: float(np.sqrt(d * d + eps2))
    return image1, preds, (sum_cx * (r(0.25) + r(0.0)) + sum_cy * (r(0.0) + r(0.125))) / (B * H * W * 2)


# ------------------------------------------------------------------ yardstick and restatement
def test_the_yardstick_gradient_matches_central_differences():
    rng = np.random.default_rng(12)
    image1, _, _, preds = make_case(1, 5, 7, 2)
    _, _, grads = smooth2_yardstick(image1, preds, **PARAMS)
    value = lambda ps: float(torch_smooth2_loss(image1, [torch.tensor(p, dtype=torch.float64) for p in ps], **PARAMS)[0])
    base = [np.asarray(p, np.float64) for p in preds]
    h, worst = 1e-6, 0.0
    for _ in range(30):
        i = int(rng.integers(len(preds)))
        idx = tuple(int(rng.integers(d)) for d in base[i].shape)
        hi, lo = [b.copy() for b in base], [b.copy() for b in base]
        hi[i][idx] += h
        lo[i][idx] -= h
        fd = (value(hi) - value(lo)) / (2 * h)
        want = grads[i][idx]
        worst = max(worst, abs(fd - want) / (1e-5 * abs(want) + 1e-10))
        assert abs(fd - want) <= 1e-5 * abs(want) + 1e-10, (i, idx, fd, want)       # (1e-10: rounding of the value over 2h)
    assert all(np.abs(g).max() > 0 for g in grads)
    print(f'[smooth2] yardstick against central differences: worst |difference| / bound = {worst:.2e}')


@pytest.mark.parametrize('shape', CASES, ids=CASE_IDS)
def test_the_restatement_is_close_to_the_yardstick(shape):
    rel_loss, diff_g, max_g = smooth2_restatement_distance(*shape)
    image1, _, _, preds = make_case(*shape)
    out2, grads = np_smooth2_loss(image1, preds, **PARAMS)
    if shape == NO_STENCIL:
        assert (rel_loss, diff_g, max_g) == (0.0, 0.0, 0.0)
        assert out2.tolist() == [0.0, 0.0] and all(not g.any() and not np.signbit(g).any() for g in grads)
        return
    print(f'[smooth2] restatement {shape}: loss rel {rel_loss:.2e}, gradient {diff_g / max_g:.2e} of max|g| = {max_g:.3e}')
    assert max_g > 0
    # float32 arithmetic per pixel, float64 sums, one float32 rounding of the result: a few 2^-24 = 6e-8 for the loss; the gradient
    # carries the rounding of D (2^-24 of |p|, a few pixels) through 1 / rho <= 1 / eps = 100.  Measured: <= 1.3e-7 and <= 2.2e-6.
    # The GPU file's tolerance is four times the measured distance, so these caps keep the restatement from drifting under it.
    assert rel_loss <= 1e-6
    assert diff_g / max_g <= 1e-5
    _, want_last, _ = smooth2_yardstick(image1, preds, **PARAMS)
    assert abs(float(out2[1]) - want_last) <= 1e-6 * want_last


def test_the_restatement_on_the_cases_with_a_known_answer():
    B, H, W, n = 2, 37, 53, 2
    image1, preds, closed = affine_case(B, H, W, n)
    out2, grads = np_smooth2_loss(image1, preds, **PARAMS)
    assert all(not g.any() for g in grads)                                  # exactly 0.0 everywhere
    assert ulps(out2[1], closed) <= 4
    want = smooth2_yardstick(image1, preds, **PARAMS)
    assert abs(want[1] - closed) <= 1e-12 * closed and all(np.abs(g).max() <= 1e-15 for g in want[2])
    assert ulps(out2[0], (0.8 + 1.0) * closed) <= 4
    # the first-order term does pull on it: that is the difference between the two
    from test_photometric_loss import np_photometric_loss
    case = make_case(B, H, W, n, seed=6)
    first = np_photometric_loss(case[0], case[1], None, preds, **DEFAULTS)[3]
    assert any(np.abs(g).max() > 0 for g in first)
    for constant_image in (False, True):
        image1, preds, closed = quadratic_case(B, H, W, n, constant_image=constant_image)
        out2, grads = np_smooth2_loss(image1, preds, **PARAMS)
        assert ulps(out2[1], closed) <= 4, constant_image
        assert abs(smooth2_yardstick(image1, preds, **PARAMS)[1] - closed) <= 1e-12 * closed
        # D is constant along its axis, so q is too wherever the edge weights are: with a constant image the gradient is
        # nonzero only within two pixels of a border, where stencils are missing
        if constant_image:
            eps2 = float(np.float32(PARAMS['eps']) * np.float32(PARAMS['eps']))
            r = lambda d: float(np.sqrt(d * d + eps2))
            count = B * H * (W - 2) * (r(0.25) + r(0.0)) + B * (H - 2) * W * (r(0.0) + r(0.125))        # all edge weights exactly 1
            assert ulps(out2[1], count / (B * H * W * 2)) <= 4
            assert all(not g[:, 2:-2, 2:-2].any() for g in grads) and all(g[:, :, :2].any() for g in grads)
    # add_to is added in double; upstream = 2 doubles the gradient bit for bit; gamma = 1 sums the single-prediction values
    image1, _, _, preds = make_case(B, H, W, n)
    out2, g_a = np_smooth2_loss(image1, preds, smooth2_weight=0.5, **PARAMS)
    plus, _ = np_smooth2_loss(image1, preds, smooth2_weight=0.5, add_to=0.375, **PARAMS)
    assert abs(float(plus[0]) - (0.375 + float(out2[0]))) <= 2 * 2.0 ** -24 and plus[1] == out2[1]
    g_2 = np_smooth2_loss(image1, preds, smooth2_weight=0.5, upstream=2.0, **PARAMS)[1]
    for a, b in zip(g_a, g_2):
        np.testing.assert_array_equal(2 * a, b)
    one = dict(PARAMS, gamma=1.0)
    total = float(np_smooth2_loss(image1, preds, **one)[0][0])
    parts = sum(float(np_smooth2_loss(image1, [p], **one)[0][0]) for p in preds)
    assert abs(total - parts) <= 1e-6 * abs(parts)


# ------------------------------------------------------------------ the C entries
def test_the_entries_are_declared_exported_and_typed():
    from tf_raft_amd import build
    assert 'smooth2_loss.hip' in build.SOURCES
    P, I, L, F, D = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double
    assert _ffi._SIGNATURES['raft_smooth2_loss_workspace_doubles'] == (L, [])
    assert _ffi._SIGNATURES['raft_smooth2_loss_f32'] == (I, [P, P, L, I, I, I, I, D, F, F, F, F, P, P, P, I, P, P])
    assert {'raft_smooth2_loss_workspace_doubles', 'raft_smooth2_loss_f32'} <= set(_ffi.EXPORTED_SYMBOLS)
    assert _ffi.ABI_VERSION == 222                                   # entries were added, no signature changed
    lib = _ffi.load_library()
    assert lib.raft_smooth2_loss_workspace_doubles() > 0
    assert len(lib.raft_smooth2_loss_f32.argtypes) == 18


def test_argument_errors_are_returned_before_any_device_work():
    """tests/windowed_loss.py ``check_argument_errors`` for this argument list.  No GPU here: a call that got past its checks would
    fail in the launch (a positive hipError_t) or crash."""
    fn = _ffi.load_library().raft_smooth2_loss_f32
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off = C.c_void_p(p.value + 4)
    nan, inf = float('nan'), float('inf')
    #       0 image1 1 preds 2 stride 3 n 4 B 5 H 6 W 7 gamma 8 smooth2_weight 9 edge_weight 10 eps 11 upstream 12 add_to 13 out2
    #       14 d_preds 15 accumulate 16 workspace 17 stream
    good = [p, p, 2 * 20, 3, 1, 4, 5, 0.8, 1.0, 10.0, 0.01, 1.0, p, p, p, 0, p, None]

    def call(**changes):
        args = list(good)
        for k, v in changes.items():
            args[int(k[1:])] = v
        return fn(*args)
    for k in (0, 1, 13, 16):                                                # (add_to and d_preds may be NULL)
        assert call(**{f'a{k}': None}) == -1, k
    for k in (3, 4, 5, 6):
        for v in (0, -3):
            assert call(**{f'a{k}': v}) == -2, (k, v)
    for bad in ((1, 1 << 15, 1 << 15), (1 << 10, 1 << 10, 1 << 10), (1, 1, 1 << 30), (1, 26755, 26755)):   # B*H*W*3 reaches 2^31
        assert call(a4=bad[0], a5=bad[1], a6=bad[2], a2=1 << 40) == -2, bad
    assert call(a2=2 * 20 - 2) == -2                                        # predictions would overlap
    assert call(a2=2 * 20 + 1) == -3                                        # read as float2
    assert call(a3=65) == -3
    for k in (7, 8, 9):
        for v in (-1e-3, nan, inf, -inf):
            assert call(**{f'a{k}': v}) == -2, (k, v)
    for v in (0.0, -0.01, 1e-30, 1e30, nan, inf):                           # (1e-30, 1e30: eps * eps is 0 / infinite in float32)
        assert call(a10=v) == -2, v
    for v in (nan, inf, -inf):
        assert call(a11=v) == -2, v
    for v in (-1, 2):
        assert call(a15=v) == -2, v
    for k in (1, 14, 16):
        assert call(**{f'a{k}': off}) == -4, k
    for a, d in ((None, None), (p, None), (None, p)):                       # no error of their own when NULL
        assert call(a12=a, a14=d, a3=65) == -3, (a, d)
    # precedence: NULL, then every shape check, then unsupported, then alignment
    assert call(a0=None, a5=0, a3=65, a16=off) == -1
    assert call(a5=0, a3=65, a16=off) == -2
    assert call(a15=7, a3=65, a16=off) == -2
    assert call(a11=nan, a2=2 * 20 + 1, a16=off) == -2
    assert call(a3=65, a16=off) == -3
    assert call(a16=off) == -4


# ------------------------------------------------------------------ the Python layers, nothing reaches the device
def test_the_weight_is_checked_and_carried_without_a_gpu():
    """``smooth2_weight`` is the last keyword of ``Smooth2SequenceLoss`` and of the two ``grad.smooth2_*`` helpers; the parents keep
    the signatures tests/test_census_loss.py and tests/test_ssim_loss.py pin, as ``SSIMSequenceLoss`` kept its parent's."""
    import inspect
    from tf_raft_amd import grad, losses
    cls = losses.Smooth2SequenceLoss
    loss = cls()
    assert isinstance(loss, losses.SSIMSequenceLoss) and isinstance(loss, losses.PhotometricSequenceLoss)
    assert loss._params()['smooth2_weight'] == 0.0 and loss.smooth2_weight == 0.0
    assert loss._params() == dict(losses.SSIMSequenceLoss()._params(), smooth2_weight=0.0)
    assert losses.SSIMSequenceLoss()._params() == dict(losses.PhotometricSequenceLoss()._params(), ssim_weight=0.0)
    assert cls(smooth2_weight=np.float32(0.5))._params()['smooth2_weight'] == 0.5
    both = cls(0.8, 0.1, 10.0, 0.01, 2, 3, 4)
    assert (both.census_weight, both.ssim_weight, both.smooth2_weight) == (2.0, 3.0, 4.0)
    assert cls(smooth_weight=0, smooth2_weight=2).smooth_weight == 0.0                       # the second-order term alone
    for bad in (-0.1, float('nan'), float('inf'), -float('inf'), 1e39, True, False, 'x', b'1', None, 1j, (1.0,)):
        with pytest.raises(ValueError, match='smooth2_weight'):
            cls(smooth2_weight=bad)
    with pytest.raises(ValueError, match='ssim_weight'):
        cls(ssim_weight=-1.0, smooth2_weight=1.0)
    fns = (cls.__init__, grad.smooth2_sequence_loss_value_and_grad, grad.smooth2_sequence_loss_grad, losses.smooth2_sequence_loss)
    for fn in fns:                                                          # the last keyword, off by default
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert (last.name, last.default) == ('smooth2_weight', 0.0), fn
    want = ['y_true', 'y_pred', 'gamma', 'smooth_weight', 'edge_weight', 'eps', 'upstream', 'census_weight', 'ssim_weight', 'smooth2_weight']
    for fn in fns[1:3]:
        sig = inspect.signature(fn).parameters
        assert list(sig) == want and [sig[k].default for k in want[2:]] == [0.8, 0.1, 10.0, 0.01, 1.0, 0.0, 0.0, 0.0], fn
    assert inspect.signature(losses._photometric_launch).parameters['smooth2_weight'].default == 0.0
    i1 = np.zeros((2, 4, 5, 3), np.float32)
    p = np.zeros((2, 4, 5, 2), np.float32)
    assert list(inspect.signature(losses.smooth2_sequence_loss).parameters) == want[:6] + want[7:]       # (no upstream)
    for fn in fns[1:]:
        for bad in (-1.0, float('nan'), float('inf'), True, 'x'):
            with pytest.raises(ValueError, match='smooth2_weight'):
                fn((i1, i1), [p], smooth2_weight=bad)
    for fn in fns[1:3]:
        with pytest.raises(ValueError, match='upstream'):
            fn((i1, i1), [p], upstream=float('inf'), smooth2_weight=1.0)
    for fn in fns[1:]:
        with pytest.raises(ValueError, match='prediction'):                  # the shape checks still come before the device
            fn((i1, i1), [p[:, :3]], smooth2_weight=1.0)
    with pytest.raises(ValueError, match='prediction'):
        cls(smooth2_weight=1.0).terms((i1, i1), [p[:, :3]])


def test_compile_reports_the_key_behind_smoothness():
    from tf_raft_amd import losses
    from tf_raft_amd.model import RAFT, SmallRAFT
    for cls in (RAFT, SmallRAFT):
        model = cls.__new__(cls)
        model.compile(optimizer=None, loss=losses.Smooth2SequenceLoss(smooth2_weight=1.0))
        assert model._unlabelled_keys() == ('loss', 'photometric', 'smoothness', 'smoothness2')
        assert isinstance(model.flow_metrics['smoothness2'], losses.Mean) and model.flow_metrics['smoothness2'].name == 'smoothness2'
        assert list(model.flow_metrics) == ['loss', 'epe', 'u1', 'u3', 'u5', 'photometric', 'smoothness', 'smoothness2']
        model.compile(optimizer=None, loss=losses.Smooth2SequenceLoss(census_weight=0.5, ssim_weight=0.5, smooth2_weight=0.25),
                      bidirectional=True)
        assert model._unlabelled_keys() == ('loss', 'photometric', 'census', 'ssim', 'smoothness', 'smoothness2', 'occluded')
        assert 'smoothness2' in model.flow_metrics
        # weight 0: today's tuples
        for loss in (losses.PhotometricSequenceLoss(), losses.Smooth2SequenceLoss(), losses.Smooth2SequenceLoss(smooth2_weight=0.0)):
            model.compile(optimizer=None, loss=loss)
            assert model._unlabelled_keys() == ('loss', 'photometric', 'smoothness') and 'smoothness2' not in model.flow_metrics
        model.compile(optimizer=None, loss=losses.Smooth2SequenceLoss(census_weight=0.5, ssim_weight=0.5), bidirectional=True)
        assert model._unlabelled_keys() == ('loss', 'photometric', 'census', 'ssim', 'smoothness', 'occluded')
        model.compile(optimizer=None, loss=losses.Smooth2SequenceLoss(smooth2_weight=1.0), bidirectional=True, selfsup_crop=(8, 8))
        assert model._unlabelled_keys() == ('loss', 'photometric', 'smoothness', 'smoothness2', 'occluded', 'selfsup', 'selfsup_used')

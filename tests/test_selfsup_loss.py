"""Self-supervision term, host side (no GPU): the float64 yardstick of ``raft_selfsup_loss_f32`` with its
autograd gradient checked against central differences, the float32 NumPy restatement in the kernel's operation order and its
distance to the yardstick per case (the tolerances of tests/test_gpu_selfsup_loss.py), known answers, the C entry's declaration
and argument checks, ``compile``'s and ``train_step``'s validation, and the float64 oracle of the two-pass update-block step with
the check that its masks are stable against float32 arithmetic for the inputs and the ``beta`` the GPU test uses.

Measured distances of the restatement to the yardstick (loss relative, last distance relative, gradient absolute and over max|g|;
with both masks, weight 0.3, eps 0.001; `pytest -s` prints them for every case):

    student in teacher at origin, n          loss rel   last rel   gradient abs / over max|g|
    (1,1,1) in (1,3,3) at (1,1), 1           8.1e-08    4.1e-08    8.2e-09 / 5.5e-08
    (1,5,7) in (1,5,7) at (0,0), 3           5.5e-10    2.9e-08    4.4e-10 / 1.0e-07
    (2,37,53) in (2,45,69) at (3,11), 3      1.8e-08    7.8e-09    8.3e-12 / 2.2e-07
    (2,37,53) in (2,45,69) at (3,11), 12     3.9e-08    1.2e-08    8.7e-12 / 2.3e-07
    (2,368,496) in (2,380,512) at (5,9), 2   1.7e-08    4.2e-08    7.4e-14 / 1.8e-07
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from tf_raft_amd import _ffi
from test_bidirectional_step import np_flow_visibility, np_visibility_f64
from test_photometric_loss import DEFAULTS, pred_weights, torch_photometric_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = dict(gamma=0.8, weight=0.3, eps=0.001)

# (student (B, H, W), teacher (B, Ht, Wt), origin (oy, ox))
SMALL = [((1, 1, 1), (1, 3, 3), (1, 1)),
         ((1, 5, 7), (1, 5, 7), (0, 0)),
         ((2, 37, 53), (2, 45, 69), (3, 11))]          # odd sizes: the tail of any paired path, window rows not aligned
BIG = ((2, 368, 496), (2, 380, 512), (5, 9))           # more 256-pixel runs than records
MASKS = ('none', 'teacher', 'student', 'both')
# (geometry, n, masks): n in {1, 3} everywhere, 12 once, the large picture once
CASES = [(g, n, m) for g in SMALL for n in (1, 3) for m in MASKS] + [(SMALL[2], 12, 'both'), (BIG, 2, 'both')]


def case_id(case):
    (s, t, o), n, m = case
    return f"{'x'.join(map(str, s))}in{'x'.join(map(str, t[1:]))}at{o[0]}_{o[1]}-n{n}-{m}"


CASE_IDS = [case_id(c) for c in CASES]


@functools.lru_cache(maxsize=None)
def selfsup_case(case):
    """``(teacher, teacher_visible or None, origin, student_visible or None, [preds])`` as NumPy: a teacher of a few pixels'
    magnitude, predictions around its window (some exactly on it), masks with 70 % nonzero bytes of several values, and -- where
    the window has room -- three teacher vectors that are not finite.  Treat as read-only: the tests share it."""
    (B, H, W), (_, Ht, Wt), (oy, ox) = case[0]
    n, masks = case[1], case[2]
    rng = np.random.default_rng(1000 * H + W + n)
    teacher = rng.normal(0.0, 3.0, (B, Ht, Wt, 2)).astype(np.float32)
    window = teacher[:, oy:oy + H, ox:ox + W].copy()
    preds = []
    for i in range(n):
        p = (window + rng.normal(0.0, 2.0 / (i + 1), window.shape)).astype(np.float32)
        same = rng.uniform(size=(B, H, W)) < 0.1                      # d = 0 exactly: rho = sqrtf(eps2), gradient 0
        p[same] = window[same]
        preds.append(p)
    if H * W >= 35:
        teacher[0, oy, ox] = (np.nan, 1.0)
        teacher[-1, oy + H - 1, ox + W - 1] = (1.0, np.inf)
        teacher[0, oy + H // 2, ox + W // 2] = (-np.inf, np.nan)
    tv = sv = None
    if masks in ('teacher', 'both'):
        tv = ((rng.uniform(size=(B, Ht, Wt)) < 0.7) * rng.integers(1, 256, (B, Ht, Wt))).astype(np.uint8)
    if masks in ('student', 'both'):
        sv = ((rng.uniform(size=(B, H, W)) < 0.3) * rng.integers(1, 256, (B, H, W))).astype(np.uint8)
    if H * W == 1:                                                     # the one pixel is used
        tv = None if tv is None else np.full_like(tv, 7)
        sv = None if sv is None else np.zeros_like(sv)
    for a in (teacher, tv, sv, *preds):
        if a is not None:
            a.setflags(write=False)
    return teacher, tv, (oy, ox), sv, preds


def used_pixels(teacher, teacher_visible, origin, student_visible, shape):
    B, H, W = shape
    oy, ox = origin
    t = np.asarray(teacher)[:, oy:oy + H, ox:ox + W]
    used = np.isfinite(t).all(-1)
    if teacher_visible is not None:
        used &= np.asarray(teacher_visible)[:, oy:oy + H, ox:ox + W] != 0
    if student_visible is not None:
        used &= np.asarray(student_visible) == 0
    return used


# ------------------------------------------------------------------ the yardstick
def torch_selfsup_loss(teacher, teacher_visible, origin, student_visible, preds, gamma=0.8, weight=0.3, eps=0.001, add_to=0.0):
    """``(loss, dist_last, used_share)`` by the definition in include/raft_hip.h in float64: ``preds`` float64 tensors (B, H, W, 2)
    that may require grad; the teacher (NumPy or a detached tensor) and the masks are constants.  ``eps2`` and the ``w_i`` are
    the float32 numbers the definition names, ``weight`` the float32 the entry receives."""
    B, H, W, _ = preds[0].shape
    t_full = teacher.detach().double() if isinstance(teacher, torch.Tensor) else torch.tensor(np.array(teacher), dtype=torch.float64)
    used_np = used_pixels(t_full.numpy(), teacher_visible, origin, student_visible, (B, H, W))
    used = torch.as_tensor(used_np)
    oy, ox = origin
    t = t_full[:, oy:oy + H, ox:ox + W]
    t = torch.where(used[..., None], t, torch.zeros_like(t))          # (a vector that is not finite is not used: keep NaN out of autograd)
    eps2 = float(np.float32(eps) * np.float32(eps))
    total, dist = 0.0, None
    for w_i, p in zip(pred_weights(gamma, len(preds)), preds):
        d = p - t
        dist = (used[..., None].double() * torch.sqrt(d * d + eps2)).sum() / (B * H * W * 2)
        total = total + w_i * dist
    return add_to + float(np.float32(weight)) * total, dist, float(used_np.sum()) / (B * H * W)


def selfsup_yardstick(case, upstream=1.0, add_to=0.0, **params):
    """``(loss, dist_last, used_share, [gradients])`` as float64 NumPy."""
    teacher, tv, origin, sv, preds = selfsup_case(case) if not isinstance(case[0], np.ndarray) else case
    ps = [torch.tensor(np.asarray(p), dtype=torch.float64, requires_grad=True) for p in preds]
    loss, dist, share = torch_selfsup_loss(teacher, tv, origin, sv, ps, add_to=add_to, **dict(PARAMS, **params))
    (float(np.float32(upstream)) * loss).backward()
    return float(loss.detach()), float(dist.detach()), share, [p.grad.numpy() for p in ps]


# ------------------------------------------------------------------ the restatement
def np_selfsup_loss(teacher, teacher_visible, origin, student_visible, preds, gamma=0.8, weight=0.3, eps=0.001, upstream=1.0,
                    add_to=None):
    """csrc/selfsup_loss.hip operation for operation in float32 (the sums over pixels in float64, as the kernel's, associated
    differently): ``(out3 float32 (3,), d_preds float32 (n, B, H, W, 2))``."""
    f = np.float32
    B, H, W, _ = preds[0].shape
    n, npix = len(preds), B * H * W
    oy, ox = origin
    used = used_pixels(teacher, teacher_visible, origin, student_visible, (B, H, W))
    t = np.where(used[..., None], np.asarray(teacher, f)[:, oy:oy + H, ox:ox + W], f(0))
    eps2 = f(eps) * f(eps)
    inv2 = 1.0 / (npix * 2.0)
    scale0 = f(upstream) * f(weight)
    tot, last = 0.0, 0.0
    d_preds = np.zeros((n, B, H, W, 2), f)
    for i, (w_i, p) in enumerate(zip(pred_weights(gamma, n), preds)):
        d = np.asarray(p, f) - t
        r = np.sqrt(d * d + eps2)
        assert r.dtype == f
        pair = (r[..., 0] + r[..., 1])[used]                          # float32 sum of the two components
        s = float(pair.astype(np.float64).sum())
        tot += float(f(w_i)) * s
        last = s
        g = (scale0 * f(w_i)) * ((d / r) * f(inv2))
        assert g.dtype == f
        d_preds[i] = np.where(used[..., None], g, f(0))
    before = 0.0 if add_to is None else float(f(add_to))
    out3 = np.array([before + float(f(weight)) * (tot * inv2), last * inv2, float(used.sum()) / npix]).astype(f)
    return out3, d_preds


@functools.lru_cache(maxsize=None)
def restatement_distance(case):
    """What the float32 restatement is away from the yardstick on ``case``: ``(loss rel, last rel, gradient abs, max|g|)``."""
    want_loss, want_last, _, want_g = selfsup_yardstick(case)
    out3, d = np_selfsup_loss(*selfsup_case(case), **PARAMS)
    rel = lambda got, want: abs(float(got) - want) / abs(want) if want else abs(float(got))
    diff = max(float(np.abs(d[i].astype(np.float64) - g).max()) for i, g in enumerate(want_g))
    return rel(out3[0], want_loss), rel(out3[1], want_last), diff, max(float(np.abs(g).max()) for g in want_g)


# ------------------------------------------------------------------ yardstick and restatement
def test_the_yardstick_gradient_matches_central_differences():
    case = (SMALL[1], 3, 'both')
    teacher, tv, origin, sv, preds = selfsup_case(case)
    _, _, _, grads = selfsup_yardstick(case)
    rng = np.random.default_rng(3)
    h, worst = 1e-6, 0.0
    value = lambda ps: float(torch_selfsup_loss(teacher, tv, origin, sv, [torch.tensor(p, dtype=torch.float64) for p in ps], **PARAMS)[0])
    for _ in range(24):
        i = int(rng.integers(len(preds)))
        idx = tuple(int(rng.integers(s)) for s in preds[0].shape)
        if np.asarray(preds[i])[idx] == teacher[(idx[0], idx[1] + origin[0], idx[2] + origin[1], idx[3])]:
            continue                                                   # (d = 0 with eps = 1e-3: the second derivative is 1 / eps)
        up = [np.array(p, np.float64) for p in preds]
        dn = [np.array(p, np.float64) for p in preds]
        up[i][idx] += h
        dn[i][idx] -= h
        numeric = (value(up) - value(dn)) / (2 * h)
        worst = max(worst, abs(numeric - grads[i][idx]))
    print(f'[selfsup] autograd against central differences: largest difference {worst:.3e}')
    assert worst <= 1e-8
    assert all(np.abs(g).max() > 1e-4 for g in grads)


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_the_restatement_and_its_distance_to_the_yardstick(case):
    """The distances are the GPU test's tolerances (times 4); here they are bounded by what float32 can do: the loss is one
    rounding of a float64 sum of float32 terms, each within 3 roundings of its value, and a gradient element goes through six
    float32 operations."""
    loss_rel, last_rel, g_abs, g_max = restatement_distance(case)
    want = selfsup_yardstick(case)
    out3, d = np_selfsup_loss(*selfsup_case(case), **PARAMS)
    print(f'[selfsup] restatement {case_id(case)}: loss rel {loss_rel:.3e} last rel {last_rel:.3e} gradient abs {g_abs:.3e} '
          f'over max|g| {g_abs / g_max if g_max else 0.0:.3e} used {want[2]:.4f}')
    U = 2.0 ** -24
    assert loss_rel <= 4 * U and last_rel <= 4 * U
    assert g_abs <= 8 * U * g_max
    assert out3[2] == np.float32(want[2])                              # the count is exact
    used = used_pixels(*selfsup_case(case)[:4], d.shape[1:4])
    assert not d[:, ~used].any()


# ------------------------------------------------------------------ known answers
def _known(teacher, preds, origin=(0, 0), tv=None, sv=None, **params):
    params = dict(PARAMS, **params)
    out3, d = np_selfsup_loss(teacher, tv, origin, sv, preds, **params)
    ps = [torch.tensor(np.asarray(p), dtype=torch.float64, requires_grad=True) for p in preds]
    loss, dist, share = torch_selfsup_loss(teacher, tv, origin, sv, ps, **params)
    loss.backward()
    return out3, d, float(loss.detach()), float(dist.detach()), share, [p.grad.numpy() for p in ps]


def equal_case():
    """Student equal to the windowed teacher, with a teacher mask: ``(teacher, tv, origin, [preds], used share)``."""
    rng = np.random.default_rng(5)
    teacher = rng.normal(0, 2, (2, 9, 11, 2)).astype(np.float32)
    tv = (rng.uniform(size=(2, 9, 11)) < 0.6).astype(np.uint8)
    origin, (H, W) = (2, 3), (6, 7)
    window = teacher[:, 2:2 + H, 3:3 + W].copy()
    share = float((tv[:, 2:2 + H, 3:3 + W] != 0).sum()) / (2 * H * W)
    return teacher, tv, origin, [window.copy(), window.copy()], share


def ramp_case():
    """Teacher ``t(y, x) = (x, y)``, a constant student ``(cu, cv)`` at origin ``(oy, ox)``: ``d = (cu - ox - x, cv - oy - y)``."""
    Ht, Wt, H, W, oy, ox = 9, 12, 4, 6, 3, 5
    ys, xs = np.meshgrid(np.arange(Ht, dtype=np.float32), np.arange(Wt, dtype=np.float32), indexing='ij')
    teacher = np.stack([xs, ys], -1)[None]
    cu, cv = 7.25, 1.5                                                 # (d_u changes sign inside the window)
    pred = np.broadcast_to(np.array([cu, cv], np.float32), (1, H, W, 2)).copy()
    eps2 = float(np.float32(PARAMS['eps']) * np.float32(PARAMS['eps']))
    total = sum(np.sqrt((cu - ox - x) ** 2 + eps2) + np.sqrt((cv - oy - y) ** 2 + eps2) for y in range(H) for x in range(W))
    return teacher, (oy, ox), [pred], total / (H * W * 2)


def test_student_equal_to_the_windowed_teacher():
    teacher, tv, origin, preds, share = equal_case()
    out3, d, loss, dist, got_share, grads = _known(teacher, preds, origin, tv)
    root = np.sqrt(np.float32(PARAMS['eps']) * np.float32(PARAMS['eps']))            # sqrtf(eps2)
    assert got_share == share and out3[2] == np.float32(share)
    np.testing.assert_allclose(dist, float(np.sqrt(np.float64(root.dtype.type(PARAMS['eps']) ** 2))) * share, rtol=1e-12)   # (sqrt in float64)
    np.testing.assert_allclose(out3[1], float(root) * share, rtol=2e-7)
    np.testing.assert_allclose(out3[0], float(np.float32(0.3)) * (0.8 + 1.0) * float(root) * share, rtol=3e-7)
    assert not d.any() and not any(g.any() for g in grads)             # exactly 0


def test_masks_that_leave_nothing_give_exactly_zero():
    teacher, _, origin, preds, _ = equal_case()
    preds = [p + np.float32(0.5) for p in preds]
    for tv, sv in ((np.zeros(teacher.shape[:3], np.uint8), None), (None, np.full(preds[0].shape[:3], 3, np.uint8))):
        out3, d, loss, dist, share, grads = _known(teacher, preds, origin, tv, sv)
        assert out3.tolist() == [0.0, 0.0, 0.0] and (loss, dist, share) == (0.0, 0.0, 0.0)
        assert not d.any() and not any(g.any() for g in grads)


def test_the_ramp_teacher_pins_the_window_offset():
    teacher, origin, preds, want = ramp_case()
    out3, d, loss, dist, share, _ = _known(teacher, preds, origin, gamma=0.8, weight=1.0)
    np.testing.assert_allclose(dist, want, rtol=1e-12)
    np.testing.assert_allclose(out3[1], want, rtol=2e-7)
    assert share == 1.0
    # a swapped or a dropped offset gives another number
    for wrong in ((origin[1], origin[0]), (0, 0)):
        assert abs(_known(teacher, preds, wrong, weight=1.0)[3] - want) > 0.1
    # d_u > 0 left of x = cu - ox, < 0 right of it: the sign of the gradient follows the window
    assert (np.sign(d[0, 0, 0, :, 0]) == np.sign(7.25 - 5 - np.arange(6))).all()


def test_teacher_vectors_that_are_not_finite_are_left_out_and_counted_as_unused():
    case = (SMALL[2], 3, 'none')
    teacher, tv, origin, sv, preds = selfsup_case(case)
    B, H, W = case[0][0]
    assert (~np.isfinite(teacher)).any(-1).sum() == 3
    out3, d = np_selfsup_loss(teacher, tv, origin, sv, preds, **PARAMS)
    assert out3[2] == np.float32((B * H * W - 3) / (B * H * W)) and np.isfinite(out3).all() and np.isfinite(d).all()
    assert not d[:, 0, 0, 0].any() and not d[:, -1, -1, -1].any() and not d[:, 0, H // 2, W // 2].any()
    assert selfsup_yardstick(case)[2] == (B * H * W - 3) / (B * H * W)


# ------------------------------------------------------------------ the C entry
def test_the_header_declares_and_the_library_exports_the_entries():
    with open(os.path.join(ROOT, 'include', 'raft_hip.h')) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    assert re.search(r'int64_t\s+raft_selfsup_loss_workspace_doubles\s*\(\s*void\s*\)', header)
    assert re.search(r'int\s+raft_selfsup_loss_f32\s*\(', header)
    sigs = _ffi.header_signatures(header)
    P, I, L, F, D = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double
    assert sigs['raft_selfsup_loss_workspace_doubles'] == (L, [])
    assert sigs['raft_selfsup_loss_f32'] == (I, [P, P, I, I, I, I, P, P, L, I, I, I, I, D, F, F, F, P, P, P, I, P, P])
    assert _ffi.ABI_VERSION == 222                                   # entries were added, no signature changed
    lib = _ffi.load_library()
    assert lib.raft_selfsup_loss_workspace_doubles() >= 3
    assert len(lib.raft_selfsup_loss_f32.argtypes) == 23


def test_argument_errors_are_returned_in_the_stated_order_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    fn = _ffi.load_library().raft_selfsup_loss_f32
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off = C.c_void_p(p.value + 4)
    nan, inf = float('nan'), float('inf')
    #       0 teacher 1 tvis 2 Ht 3 Wt 4 oy 5 ox 6 svis 7 preds 8 stride 9 n 10 B 11 H 12 W 13 gamma 14 weight 15 eps 16 upstream
    #       17 add_to 18 out3 19 d_preds 20 accumulate 21 workspace 22 stream
    good = [p, p, 6, 8, 1, 2, p, p, 2 * 4 * 5, 2, 1, 4, 5, 0.8, 0.3, 1e-3, 1.0, p, p, p, 0, p, None]

    def call(**changes):
        args = list(good)
        for k, v in changes.items():
            args[int(k[1:])] = v
        return fn(*args)
    for k in (0, 7, 18, 21):                                               # (the masks, add_to and d_preds may be NULL)
        assert call(**{f'a{k}': None}) == -1, k
    assert call(a1=None, a6=None, a17=None, a19=None) > 0                   # past the checks: the launch fails without a device
    for k in (2, 3, 9, 10, 11, 12):
        for v in (0, -3):
            assert call(**{f'a{k}': v}) == -2, (k, v)
    for changes in (dict(a4=-1), dict(a5=-1), dict(a4=3), dict(a5=4), dict(a11=6, a8=2 * 6 * 5, a4=1), dict(a12=8, a8=2 * 4 * 8, a5=1)):
        assert call(**changes) == -2, changes                               # the window does not lie inside the teacher
    assert call(a4=2, a5=3) > 0                                             # flush with the far corner: allowed
    assert call(a8=2 * 4 * 5 - 2) == -2                                     # pred_stride < 2*B*H*W
    assert call(a2=1 << 15, a3=1 << 15) == -2                               # B*Ht*Wt*3 reaches 2^31 (raft_loss_shape_ok on the teacher)
    for k in (13, 14):
        for v in (-1e-3, nan, inf):
            assert call(**{f'a{k}': v}) == -2, (k, v)
    for v in (0.0, -1e-3, nan, inf, 1e-30, 1e30):                           # eps, or eps * eps in float32, not positive and finite
        assert call(a15=v) == -2, v
    for v in (nan, inf, -inf):
        assert call(a16=v) == -2, v
    for v in (-1, 2):
        assert call(a20=v) == -2, v
    assert call(a9=65) == -3 and call(a8=2 * 4 * 5 + 1) == -3
    for k in (0, 7, 19, 21):
        assert call(**{f'a{k}': off}) == -4, k
    assert call(a1=off, a6=off, a17=off, a18=off) > 0                       # bytes and float scalars need no 8-byte alignment
    # precedence: NULL, then every shape check, then unsupported, then alignment
    assert call(a0=None, a11=0, a9=65, a21=off) == -1
    assert call(a11=0, a9=65, a21=off) == -2
    assert call(a20=7, a9=65, a21=off) == -2
    assert call(a16=nan, a8=2 * 4 * 5 + 1, a21=off) == -2
    assert call(a9=65, a21=off) == -3
    assert call(a21=off) == -4


# ------------------------------------------------------------------ the Python layers, nothing reaches the device
def test_the_loss_object_validates_its_parameters_and_shapes():
    from tf_raft_amd import grad, losses
    loss = losses.SelfSupervisionLoss()
    assert (loss.gamma, loss.weight, loss.eps) == (0.8, 0.3, 0.001)
    for kw in (dict(gamma=-1), dict(weight=-0.1), dict(weight=float('nan')), dict(weight='x'), dict(weight=True), dict(eps=0),
               dict(eps=1e-30), dict(eps=float('inf')), dict(gamma=float('inf'))):
        with pytest.raises(ValueError):
            losses.SelfSupervisionLoss(**kw)
    t = np.zeros((2, 9, 11, 2), np.float32)
    p = np.zeros((2, 6, 7, 2), np.float32)
    bad = [dict(teacher=t[..., :1]), dict(teacher=t[0]), dict(preds=[]), dict(preds=[p] * 65), dict(preds=[p, p[:, :5]]), dict(preds=[p[:1]]),
           dict(origin=(4, 0)), dict(origin=(0, 5)), dict(origin=(-1, 0)), dict(origin=(0.0, 0)), dict(origin=3), dict(origin=(True, 0)),
           dict(teacher_visible=np.zeros((2, 6, 7), np.uint8)), dict(student_visible=np.zeros((2, 9, 11), np.uint8))]
    for kw in bad:                                                     # (with no device, anything that got further would fail otherwise)
        args = dict(dict(teacher=t, preds=[p, p], origin=(3, 4)), **kw)
        with pytest.raises(ValueError):
            loss.terms(**args)
        with pytest.raises(ValueError):
            loss.value_and_grad(**args)
        with pytest.raises(ValueError):
            grad.selfsup_loss_value_and_grad(**args)
    with pytest.raises(ValueError, match='upstream'):
        loss.value_and_grad(t, [p], upstream=float('nan'))


def test_compile_validates_the_selfsup_arguments():
    import inspect
    from tf_raft_amd import losses
    from tf_raft_amd.model import RAFT, SmallRAFT
    sig = inspect.signature(RAFT.compile).parameters
    assert sig['selfsup_crop'].default is None and sig['selfsup_mask'].default == 'teacher'
    assert (sig['selfsup_weight'].default, sig['selfsup_eps'].default) == (0.3, 0.001)
    ph = losses.PhotometricSequenceLoss
    for cls in (RAFT, SmallRAFT):
        model = cls.__new__(cls)
        for kw in ({}, {'bidirectional': False}):
            with pytest.raises(ValueError, match='bidirectional'):
                model.compile(optimizer=None, loss=ph(), selfsup_crop=(8, 8), **kw)
        for bad in ((0, 0), (-8, 8), (8, -8), (8,), (8, 8, 8), (8.0, 8), ('8', 8), (True, 8), 8, 'ab'):
            with pytest.raises(ValueError, match='selfsup_crop'):
                model.compile(optimizer=None, loss=ph(), bidirectional=True, selfsup_crop=bad)
        for bad in ('student', None, 1, 'Teacher'):
            with pytest.raises(ValueError, match='selfsup_mask'):
                model.compile(optimizer=None, loss=ph(), bidirectional=True, selfsup_crop=(8, 8), selfsup_mask=bad)
        for kw in (dict(selfsup_weight=-1.0), dict(selfsup_weight=float('nan')), dict(selfsup_eps=0.0), dict(selfsup_weight='x')):
            with pytest.raises(ValueError):
                model.compile(optimizer=None, loss=ph(), bidirectional=True, selfsup_crop=(8, 8), **kw)
        model.compile(optimizer=None, loss=ph(), bidirectional=True, selfsup_crop=(np.int64(8), 0), selfsup_weight=0.5, selfsup_eps=0.01,
                      selfsup_mask='occluded')
        assert model.selfsup_crop == (8, 0) and (model.selfsup_weight, model.selfsup_eps, model.selfsup_mask) == (0.5, 0.01, 'occluded')
        assert model.last_student_visibility is None
        assert model._unlabelled_keys() == ('loss', 'photometric', 'smoothness', 'occluded', 'selfsup', 'selfsup_used')
        assert 'selfsup' in model.flow_metrics and 'selfsup_used' in model.flow_metrics
        # the default stays what it was
        model.compile(optimizer=None, loss=ph(), bidirectional=True)
        assert model.selfsup_crop is None and model._unlabelled_keys() == ('loss', 'photometric', 'smoothness', 'occluded')
        assert 'selfsup' not in model.flow_metrics
        model.compile(optimizer=None)
        assert list(model.flow_metrics) == ['loss', 'epe', 'u1', 'u3', 'u5'] and model.selfsup_crop is None


def test_train_step_names_the_sizes_before_any_device_work():
    from tf_raft_amd import losses
    from tf_raft_amd.model import RAFT, SmallRAFT
    for cls in (RAFT, SmallRAFT):
        model = cls.__new__(cls)                                             # (no device: anything enqueued would fail)
        for crop, shape, sizes in (((8, 8), (2, 64, 96), '48 x 80'), ((3, 8), (1, 80, 112), '74 x 96'), ((8, 2), (1, 80, 112), '64 x 108'),
                                   ((0, 32), (1, 80, 120), '80 x 56')):
            model.compile(optimizer=None, loss=losses.PhotometricSequenceLoss(), bidirectional=True, selfsup_crop=crop)
            x = np.zeros(shape + (3,), np.float32)
            with pytest.raises(ValueError, match=f'selfsup_crop.*{sizes}.*{shape[1]} x {shape[2]}'):
                model.train_step((x, x))
        model.selfsup_weight = -1.0                                          # a weight changed to something the entry refuses
        with pytest.raises(ValueError, match='weight'):
            model.train_step((np.zeros((1, 80, 160, 3), np.float32),) * 2)


# ------------------------------------------------------------------ the float64 oracle of the two-pass update-block step
# Frames 80 x 112, crop (8, 8), student 64 x 96.  alpha = 0 and beta chosen as tests/test_bidirectional_step.py chose its own: in
# the valley of the float64 oracle's |f + s|^2 at step 0 (`PYTHONPATH=. python tests/test_selfsup_loss.py` prints the quantiles for
# the teacher and the student pass); test_the_oracle_masks_are_stable_in_float32 keeps the choice honest.
ORACLE_ALPHA, ORACLE_BETA = 0.0, 1.4
ORACLE_SHAPE, ORACLE_CROP, ORACLE_ITERS, ORACLE_STEPS = (1, 80, 112), (8, 8), 3, 2
ORACLE_LR0, ORACLE_WD, ORACLE_CLIP = 4e-4, 1e-4, 1.0
ORACLE_SELFSUP = dict(weight=0.3, eps=0.001)
# model.occlusion per step: off.  With these weights and noise frames the forward-backward test passes only in the outer ring of
# eight pixels of a pass's own frame (29 % of the teacher's pixels, 35 % of the student's), which the crop of (8, 8) removes: with
# the teacher's test applied, 12 of the window's 12288 pixels would be left for the term.  So the teacher's mask is the user's
# (step 0: 80 %; step 1: none, all ones), read through the window, and in 'occluded' mode the student's own test, always applied,
# leaves the 65 % it marks at step 0 and everything at step 1.
ORACLE_OCCLUSION = (False, False)


@functools.lru_cache(maxsize=None)
def oracle_case():
    """Weights and the two batches of the update-block test: step 0 carries a mask pair, step 1 none."""
    from tf_raft_amd import weights as wm
    N, H, W = ORACLE_SHAPE
    rng = np.random.default_rng(22)
    wts = wm.condition_weights('raft', wm.init_weights('raft', seed=5))
    batches = []
    for step in range(ORACLE_STEPS):
        i1 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
        i2 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
        masks = tuple((rng.uniform(size=(N, H, W)) < 0.8).astype(np.uint8) for _ in range(2))
        batches.append((i1, i2, masks) if step == 0 else (i1, i2))
    return wts, batches


def oracle_schedule():
    from tf_raft_amd import training
    return training.CyclicalLearningRate(ORACLE_LR0, 2 * ORACLE_LR0, step_size=1000, scale_fn=training.first_cycle_scaler, scale_mode='cycle')


def reference_selfsup_train_steps(wts, batches, iters, lr_fn, wd, clip_norm, n_steps, params, alpha, beta, crop, selfsup, mode,
                                  teacher_masks=None, student_masks=None, occlusion=None, dtype=torch.float64):
    """tests/test_bidirectional_step.py::reference_bidirectional_train_steps extended with the student pass: per step the update
    block runs on the doubled batch of the full frames and again on the doubled batch of their centre crops, and
    ``loss1 + weight * selfsup(student predictions, teacher.detach())`` is differentiated by autograd, then clip_by_global_norm
    and AdamW.  Every step computes its own visibility of both passes' last predictions (``np_visibility_f64``).  The masks the
    losses take are ``teacher_masks[step]`` (visible1: nonzero = use) and, in ``mode='occluded'``, ``student_masks[step]`` (nonzero
    = the student sees the pixel: left out) when given -- the device's, so that a pixel on the threshold cannot move the loss --
    else the oracle's own (``occlusion[step]`` false: the teacher's own mask is the user's alone, as with ``model.occlusion = False``).
    Returns (losses, [(loss1, selfsup_last, used share)], updated weights, [teacher occluded], [student
    occluded], and the float64 margins of both)."""
    import oracle
    from oracle.layers import W, basic_update_block, encoder
    from oracle.model import upsample_flow
    names = sorted(k for k in wts if k.startswith('update_block'))
    var = {k: torch.tensor(wts[k], dtype=dtype) for k in names}
    m = {k: torch.zeros_like(v) for k, v in var.items()}
    v2 = {k: torch.zeros_like(v) for k, v in var.items()}
    frozen = W({k: val for k, val in wts.items() if not k.startswith('update_block')}, dtype)
    cy, cx = crop
    losses, parts, occs1, occs2 = [], [], [], []

    margins1, margins2 = [], []

    def visibility(last, N, margins):
        if dtype == torch.float64:
            occ, margin = np_visibility_f64(last.detach().numpy(), N, alpha, beta)
            margins.append(margin)
            return occ
        return np_flow_visibility(last.detach().numpy(), N, None, alpha, beta)[2]       # (the stability check)

    for step in range(n_steps):
        N, H, Wd = batches[step][0].shape[:3]
        i1 = np.concatenate([batches[step][0], batches[step][1]])
        i2 = np.concatenate([batches[step][1], batches[step][0]])
        user = np.concatenate(batches[step][2]) != 0 if len(batches[step]) == 3 else np.ones(i1.shape[:3], bool)
        ow = W({}, dtype)
        ow.t = {k: val.clone().requires_grad_(True) for k, val in var.items()}

        def run(a, b):
            with torch.no_grad():
                x1 = 2 * (torch.tensor(a, dtype=dtype) / 255.0) - 1.0
                x2 = 2 * (torch.tensor(b, dtype=dtype) / 255.0) - 1.0
                f1, f2 = encoder(frozen, 'fnet', [x1, x2])
                corr_blk = oracle.CorrBlock(f1, f2, 4, 4)
                cnet = encoder(frozen, 'cnet', x1)
                net, inp = torch.tanh(cnet[..., :128]), torch.relu(cnet[..., 128:])
            B, h, w, _ = net.shape
            coords0 = oracle.coords_grid(B, h, w, dtype)
            coords1, preds = coords0.clone(), []
            for _ in range(iters):
                corr = corr_blk.retrieve(coords1)
                net, up_mask, delta = basic_update_block(ow, 'update_block', net, inp, corr, coords1 - coords0)
                coords1 = coords1 + delta
                preds.append(upsample_flow(coords1 - coords0, up_mask))
            return preds

        preds1 = run(i1, i2)
        occ1 = visibility(preds1[-1], N, margins1)
        occs1.append(occ1)
        mask1 = np.asarray(teacher_masks[step]) != 0 if teacher_masks is not None else (user & ~(occ1 & bool(occlusion is None or occlusion[step])))
        loss1 = torch_photometric_loss(i1, i2, mask1, [p.double() for p in preds1], **params)[0]
        preds2 = run(np.ascontiguousarray(i1[:, cy:H - cy, cx:Wd - cx]), np.ascontiguousarray(i2[:, cy:H - cy, cx:Wd - cx]))
        occ2 = visibility(preds2[-1], N, margins2)
        occs2.append(occ2)
        sv = None
        if mode == 'occluded':
            sv = np.asarray(student_masks[step]) != 0 if student_masks is not None else ~occ2
        loss, dist, share = torch_selfsup_loss(preds1[-1].detach(), mask1.astype(np.uint8), crop, None if sv is None else sv.astype(np.uint8),
                                               [p.double() for p in preds2], gamma=params['gamma'], add_to=loss1, **selfsup)
        loss.backward()
        losses.append(float(loss.detach()))
        parts.append((float(loss1.detach()), float(dist.detach()), share))
        g = {k: ow.t[k].grad for k in names}
        gnorm = torch.sqrt(sum((gg ** 2).sum() for gg in g.values()))
        scale = clip_norm / max(float(gnorm), clip_norm)
        t = step + 1
        lr = lr_fn(step)
        lr_t = lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        for k in names:
            gk = g[k] * scale
            w_ = var[k] - wd * var[k]
            m[k] = 0.9 * m[k] + 0.1 * gk
            v2[k] = 0.999 * v2[k] + 0.001 * gk * gk
            var[k] = w_ - lr_t * m[k] / (torch.sqrt(v2[k]) + 1e-7)
    return losses, parts, {k: v.detach().numpy() for k, v in var.items()}, occs1, occs2, margins1, margins2


@functools.lru_cache(maxsize=None)
def _oracle_run(dtype, mode='occluded'):
    wts, batches = oracle_case()
    return reference_selfsup_train_steps(wts, batches, ORACLE_ITERS, oracle_schedule(), ORACLE_WD, ORACLE_CLIP, ORACLE_STEPS, DEFAULTS,
                                         ORACLE_ALPHA, ORACLE_BETA, ORACLE_CROP, ORACLE_SELFSUP, mode, occlusion=ORACLE_OCCLUSION,
                                         dtype=dtype)


def test_the_oracle_masks_are_stable_in_float32():
    """The condition the GPU test's cap rests on: with the committed inputs and ``beta`` the float64 oracle alone marks between
    20 % and 80 % of the teacher pass's pixels at step 0, and the same procedure in float32 disagrees with it on at most 1e-3 of
    the pixels of either pass at either step."""
    _, parts, _, occ1_64, occ2_64, _, _ = _oracle_run(torch.float64)
    _, _, _, occ1_32, occ2_32, _, _ = _oracle_run(torch.float32)
    share1, share2 = [float(o.mean()) for o in occ1_64], [float(o.mean()) for o in occ2_64]
    differ = [float((a != b).mean()) for a, b in zip(occ1_64 + occ2_64, occ1_32 + occ2_32)]
    print(f'[selfsup] oracle occluded share per step: teacher {share1}, student {share2}; float32 against float64 disagreement {differ}; '
          f'(loss1, selfsup, used) per step {parts}')
    assert 0.2 <= share1[0] <= 0.8
    assert 0.2 <= share2[0] <= 0.8
    assert max(differ) <= 1e-3
    for mode in ('teacher', 'occluded'):                                   # the term has pixels to work on at both steps
        parts = _oracle_run(torch.float64, mode)[1]
        print(f'[selfsup] oracle, selfsup_mask={mode!r}: (loss1, selfsup, used) per step {parts}')
        assert all(p[2] > 0.2 and p[1] > 0 for p in parts)


# ------------------------------------------------------------------ the float64 oracle of the full two-pass step
@functools.lru_cache(maxsize=None)
def full_step_oracle():
    """One step at (2, 80, 112), crop (8, 8), iters = 2, ALL weights, occlusion off, no masks: ``oracle.RAFT`` run twice in float64
    under autograd, on the doubled batch of the frames and on the doubled batch of their centre crops, with the yardstick
    losses, clip_by_global_norm and AdamW's first step; and Keras' update of the batch-norm layers' moving statistics with the
    first pass's batch statistics and then the second's (momentum 0.99, the unbiased batch variance).  Returns ``(weights,
    (image1, image2), crop, iters, (lr, wd, clip), updated weights, moving statistics after both updates, after the first alone,
    (loss, loss1, selfsup_last, used share, global norm))``."""
    import oracle
    import oracle.layers as olayers
    from tf_raft_amd import weights as wm
    N, H, W, iters, (cy, cx) = 2, 80, 112, 2, (8, 8)
    rng = np.random.default_rng(1234)
    wts = wm.condition_weights('raft', wm.init_weights('raft', seed=6, perturb=True))
    i1 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
    i2 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
    lr, wd, clip = 4e-4, 1e-4, 1.0
    a, b = np.concatenate([i1, i2]), np.concatenate([i2, i1])
    seen = []                                                                 # (layer, mean, biased variance, count) per batch-norm call
    plain = olayers.normalization

    def recording(w, p, x, training):
        if training and w.has(f'{p}/moving_mean'):
            xd = x.detach()
            mean = xd.mean(dim=(0, 1, 2))
            seen.append((p, mean.numpy(), ((xd - mean) ** 2).mean(dim=(0, 1, 2)).numpy(), float(xd.numel() // xd.shape[-1])))
        return plain(w, p, x, training)
    olayers.normalization = recording
    try:
        om = oracle.RAFT(wts, iters=iters, dtype=torch.float64)
        names = sorted(k for k in wts if 'moving' not in k)
        for k in names:
            om.w.t[k].requires_grad_(True)
        preds1 = om([a, b], training=True, return_numpy=False)
        first = len(seen)
        loss1 = torch_photometric_loss(a, b, None, preds1, **DEFAULTS)[0]
        preds2 = om([np.ascontiguousarray(a[:, cy:H - cy, cx:W - cx]), np.ascontiguousarray(b[:, cy:H - cy, cx:W - cx])], training=True,
                    return_numpy=False)
    finally:
        olayers.normalization = plain
    assert first == 15 and len(seen) == 30                                    # every batch-norm layer of cnet, once per pass
    loss, dist, share = torch_selfsup_loss(preds1[-1].detach(), None, (cy, cx), None, preds2, gamma=DEFAULTS['gamma'], add_to=loss1,
                                           **ORACLE_SELFSUP)
    loss.backward()
    g = {k: om.w.t[k].grad for k in names}
    gnorm = float(torch.sqrt(sum((v ** 2).sum() for v in g.values())))
    scale = clip / max(gnorm, clip)
    lr_t = lr * np.sqrt(1 - 0.999) / (1 - 0.9)
    want = {}
    for k in names:
        gk = g[k] * scale
        v0 = torch.tensor(wts[k], dtype=torch.float64)
        want[k] = ((v0 - wd * v0) - lr_t * (0.1 * gk) / (torch.sqrt(0.001 * gk * gk) + 1e-7)).numpy()
    moving = {k: wts[k].astype(np.float64) for k in wts if 'moving' in k}
    once = None
    for idx, (p, mean, var, cnt) in enumerate(seen):
        if idx == first:
            once = dict(moving)
        moving[f'{p}/moving_mean'] = 0.99 * moving[f'{p}/moving_mean'] + 0.01 * mean
        moving[f'{p}/moving_variance'] = 0.99 * moving[f'{p}/moving_variance'] + 0.01 * cnt / (cnt - 1.0) * var
    scalars = (float(loss.detach()), float(loss1.detach()), float(dist.detach()), share, gnorm)
    return wts, (i1, i2), (cy, cx), iters, (lr, wd, clip), want, moving, once, scalars


def test_the_full_step_oracle_tells_one_update_of_the_moving_statistics_from_two():
    """The GPU test bounds the moving statistics by rtol 1e-4 + atol 2e-5; in every one of the 30 tensors the second update moves
    some element by at least ten times that, so a step that updated once, or twice with the same statistics, cannot pass."""
    *_, moving, once, scalars = full_step_oracle()
    gaps = {k: float((np.abs(once[k] - ref) / (2e-5 + 1e-4 * np.abs(ref))).max()) for k, ref in moving.items()}
    print(f'[selfsup] full-step oracle: (loss, loss1, selfsup, used, norm) {scalars}; the second update over the bound, smallest over the '
          f'tensors {min(gaps.values()):.1f}')
    assert len(gaps) == 30 and min(gaps.values()) >= 10.0
    assert scalars[3] == 1.0 and scalars[2] > 0


if __name__ == '__main__':      # how ORACLE_BETA was derived
    ORACLE_BETA = 1.0
    run = _oracle_run(torch.float64)
    for name, margins in (('teacher', run[5]), ('student', run[6])):
        for step, marg in enumerate(margins):
            lhs = marg + ORACLE_BETA                                       # (alpha = 0: margin = |f + s|^2 - beta)
            print(f'{name} step {step}: quantiles of |f + s|^2 at 10/25/50/75/90 %:',
                  np.quantile(lhs[np.isfinite(lhs)], [0.1, 0.25, 0.5, 0.75, 0.9]))

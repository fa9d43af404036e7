"""Backward warp and forward-backward consistency check, host side (no GPU): the float64 restatements ``np_warp`` /
``np_flow_consistency`` of the definitions in DESIGN.md section 15, an analytic case with a known answer (a square that moves by
an integer vector over a static background), the three C entries' declarations and argument checks, and the model's check of
``alpha`` / ``beta``.  tests/test_gpu_consistency.py compares the kernels with the restatements and builds its flows with
``analytic_case`` / ``parity_flows``.

The definitions: for the pixel at integer ``(x, y)`` with vector ``(u, v)`` the sample position is ``sx = float32(x) + u``,
``sy = float32(y) + v`` (ONE float32 addition each); the pixel is in frame iff ``0 <= sx <= W - 1`` and ``0 <= sy <= H - 1``
(a NaN is not); a map is sampled there with ``x0 = floor(sx)``, ``x1 = min(x0 + 1, W - 1)``, ``a = sx - x0`` (same for y) as
``(1 - b) * ((1 - a) * g[y0, x0] + a * g[y0, x1]) + b * ((1 - a) * g[y1, x0] + a * g[y1, x1])``.  Everything after the sample
position is float64 here.
"""
import ctypes as C

import numpy as np
import pytest

from tf_raft_amd import _ffi

U = 2.0 ** -24


# ------------------------------------------------------------------ the restatements
def np_sample_positions(flow):
    """(N, H, W, 2) float32 -> sx, sy (float32, one addition each) and the in-frame map."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 4 and flow.shape[-1] == 2
    _, H, W, _ = flow.shape
    with np.errstate(invalid='ignore'):
        sx = np.arange(W, dtype=np.float32)[None, None, :] + flow[..., 0]
        sy = np.arange(H, dtype=np.float32)[None, :, None] + flow[..., 1]
        assert sx.dtype == sy.dtype == np.float32
        inside = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
    return sx, sy, inside


def np_bilinear(g, sx, sy, inside):
    """(N, H, W, C) sampled at the in-frame positions in float64; anything at the others."""
    g = np.asarray(g, np.float64)
    N, H, W, _ = g.shape
    px, py = np.where(inside, sx, 0).astype(np.float64), np.where(inside, sy, 0).astype(np.float64)
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    a, b = (px - x0)[..., None], (py - y0)[..., None]
    n = np.arange(N)[:, None, None]
    with np.errstate(invalid='ignore'):
        return (1 - b) * ((1 - a) * g[n, y0, x0] + a * g[n, y0, x1]) + b * ((1 - a) * g[n, y1, x0] + a * g[n, y1, x1])


def np_warp(src, flow):
    """float64 ``(N, H, W, C)`` and the bool in-frame map ``(N, H, W)``; 0 in every channel out of frame."""
    sx, sy, inside = np_sample_positions(flow)
    return np.where(inside[..., None], np_bilinear(src, sx, sy, inside), 0.0), inside


def np_flow_consistency(flow_a, flow_b, alpha=0.01, beta=0.5):
    """Direction a: ``(occluded, inside, margin)`` with ``margin = lhs - rhs`` in float64 (NaN where a vector is not finite)."""
    sx, sy, inside = np_sample_positions(flow_a)
    f = np.asarray(flow_a, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        s = np_bilinear(flow_b, sx, sy, inside)
        lhs = ((f + s) ** 2).sum(-1)
        rhs = alpha * ((f ** 2).sum(-1) + (s ** 2).sum(-1)) + beta
        margin = lhs - rhs
        ok = inside & (lhs <= rhs)
    return ~ok, inside, margin


# ------------------------------------------------------------------ the flows both test files use
def analytic_case(H, W, N=1, d=(7, -4), seed=0):
    """A square of side min(H, W) // 3 at (H // 3, W // 4) that moves by the integer vector ``d`` = (u, v) over a static background:
    frames (N, H, W, 3) uint8, both flows, and the two squares as bool maps."""
    rng = np.random.default_rng(seed)
    side, top, left = min(H, W) // 3, H // 3, W // 4
    u, v = d
    bg = rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    tex = rng.integers(0, 256, size=(N, side, side, 3), dtype=np.uint8)
    sq1, sq2 = np.zeros((H, W), bool), np.zeros((H, W), bool)
    sq1[top:top + side, left:left + side] = True
    sq2[top + v:top + v + side, left + u:left + u + side] = True
    assert sq1.sum() == sq2.sum() == side * side, 'the moved square leaves the frame'
    f1, f2 = bg.copy(), bg.copy()
    f1[:, top:top + side, left:left + side] = tex
    f2[:, top + v:top + v + side, left + u:left + u + side] = tex
    fwd, bwd = np.zeros((N, H, W, 2), np.float32), np.zeros((N, H, W, 2), np.float32)
    fwd[:, sq1] = (u, v)
    bwd[:, sq2] = (-u, -v)
    return f1, f2, fwd, bwd, sq1, sq2


def push_past_borders(flow):
    """A copy with vectors that end just outside each border, exactly on each border, and well outside; returns it with the map
    of the pixels that must be out of frame because of it (the rest of the flow is untouched)."""
    f = np.array(flow, np.float32, order='C')
    _, H, W, _ = f.shape
    out = np.zeros(f.shape[:3], bool)
    ys = slice(0, H)
    if H >= 12:                                                    # (a frame of few rows keeps its rows: only columns are pushed)
        f[:, 1, :, :] = (0, -1.5); out[:, 1] = True                # half a pixel above the top row
        f[:, 2, :, :] = (0, -2.0)                                  # exactly on the top row: in frame
        f[:, H - 2, :, :] = (0, 1.25); out[:, H - 2] = True        # a quarter past the bottom row
        f[:, H - 3, :, :] = (0, 2.0)                               # exactly on the bottom row
        ys = slice(4, H - 4)
    f[:, ys, 0, :] = (-0.5, 0); out[:, ys, 0] = True
    f[:, ys, 3, :] = (-3.0, 0)                                     # exactly on the left column
    f[:, ys, W - 1, :] = (2.0 ** -10, 0); out[:, ys, W - 1] = True
    f[:, ys, W - 4, :] = (3.0, 0)                                  # exactly on the right column
    f[:, ys, 5, :] = (-7.5, 0.0); out[:, ys, 5] = True             # well outside (kept small: the band grows with the largest component)
    return f, out


def smooth_noise(rng, N, H, W, amp):
    """(N, H, W, 2) float64: coarse normal noise (one knot per 8 pixels) interpolated bilinearly, about ``amp`` pixels."""
    gh, gw = H // 8 + 2, W // 8 + 2
    knots = rng.normal(size=(N, gh, gw, 2)) * amp
    y, x = np.arange(H) / 8.0, np.arange(W) / 8.0
    y0, x0 = y.astype(int), x.astype(int)
    b, a = (y - y0)[None, :, None, None], (x - x0)[None, None, :, None]
    k = lambda dy, dx: knots[:, y0 + dy][:, :, x0 + dx]
    return (1 - b) * ((1 - a) * k(0, 0) + a * k(0, 1)) + b * ((1 - a) * k(1, 0) + a * k(1, 1))


def parity_flows(H, W, N, seed, borders=True):
    """The flows of the parity tests: smooth noise of a few pixels (the backward flow roughly its negative), plus the square moved
    by (7.3, -4.6), plus -- ``borders`` -- vectors that cross every border."""
    rng = np.random.default_rng(seed)
    noise = smooth_noise(rng, N, H, W, 1.0)
    fwd = noise + smooth_noise(rng, N, H, W, 0.2)
    bwd = -noise + smooth_noise(rng, N, H, W, 0.2)
    side, top, left = min(H, W) // 3, H // 3, W // 4
    if side >= 3 and top - 5 >= 0 and left + 8 + side <= W:
        fwd[:, top:top + side, left:left + side] = (7.3, -4.6)
        bwd[:, top - 5:top - 5 + side, left + 7:left + 7 + side] = (-7.3, 4.6)
    fwd, bwd = np.ascontiguousarray(fwd, np.float32), np.ascontiguousarray(bwd, np.float32)
    if borders and W >= 12:
        fwd, bwd = push_past_borders(fwd)[0], push_past_borders(bwd)[0]
    return fwd, bwd


def consistency_band(flow_a, flow_b):
    """|margin| within which either answer passes: 128 * 2^-24 * (1 + M)^2, M the largest (finite) flow component of either input."""
    both = np.concatenate([np.ravel(flow_a), np.ravel(flow_b)])
    M = float(np.abs(both[np.isfinite(both)]).max())
    return 128 * U * (1 + M) ** 2


# ------------------------------------------------------------------ the analytic case
@pytest.mark.parametrize('H,W', [(37, 53), (64, 96)])
def test_a_moving_square_has_the_known_occlusions_and_warp(H, W):
    f1, f2, fwd, bwd, sq1, sq2 = analytic_case(H, W, N=2)
    occ_f, in_f, _ = np_flow_consistency(fwd, bwd)
    occ_b, in_b, _ = np_flow_consistency(bwd, fwd)
    assert in_f.all() and in_b.all()
    covered, uncovered = sq2 & ~sq1, sq1 & ~sq2
    assert covered.any() and uncovered.any()
    for n in range(2):
        np.testing.assert_array_equal(occ_f[n], covered)           # the background the moved square covers
        np.testing.assert_array_equal(occ_b[n], uncovered)         # the background the square uncovered
    got, inside = np_warp(f2, fwd)
    assert inside.all()
    np.testing.assert_array_equal(got[~occ_f], f1[~occ_f].astype(np.float64))      # frame 1 again, bit for bit, off the occluded set
    assert (got[occ_f] != f1[occ_f]).any()
    back, _ = np_warp(f1, bwd)
    np.testing.assert_array_equal(back[~occ_b], f2[~occ_b].astype(np.float64))
    # zero flow is the identity
    zero = np.zeros_like(fwd)
    np.testing.assert_array_equal(np_warp(f1, zero)[0], f1.astype(np.float64))
    assert not np_flow_consistency(zero, zero)[0].any()


@pytest.mark.parametrize('H,W', [(37, 53), (64, 96)])
def test_vectors_pushed_past_a_border_are_out_of_frame(H, W):
    f1, f2, fwd, bwd, sq1, sq2 = analytic_case(H, W)
    pushed, out = push_past_borders(fwd)
    got, inside = np_warp(f2, pushed)
    touched = (pushed != fwd).any(-1)
    np.testing.assert_array_equal(~inside, out)                    # exactly the vectors that end outside, not those that end ON a border
    assert (touched & ~out).any()
    assert not got[out].any()
    occ, in_c, margin = np_flow_consistency(pushed, bwd)
    np.testing.assert_array_equal(in_c, inside)
    assert occ[out].all()
    # a vector that ends exactly on the last column / row samples that column / row itself
    ys = slice(4, H - 4)
    np.testing.assert_array_equal(got[0, ys, W - 4], f2[0, ys, W - 1].astype(np.float64))
    np.testing.assert_array_equal(got[0, H - 3, 6:W - 6], f2[0, H - 1, 6:W - 6].astype(np.float64))
    # non-finite vectors: out of frame, zero, occluded
    bad = fwd.copy()
    bad[0, 5, 7] = (np.nan, 0)
    bad[0, 6, 7] = (0, np.inf)
    bad[0, 7, 7] = (-np.inf, np.nan)
    got, inside = np_warp(f2, bad)
    occ = np_flow_consistency(bad, bwd)[0]
    for y in (5, 6, 7):
        assert not inside[0, y, 7] and not got[0, y, 7].any() and occ[0, y, 7]
    # ... and a finite vector whose sample touches a non-finite one is occluded too
    assert np_flow_consistency(bwd, bad)[0][0, 5, 7]


def test_the_restatement_leaves_few_pixels_to_the_band():
    """On the parity flows the float64 margin lies within the band 128 * 2^-24 * (1 + M)^2 on far fewer than 0.5 % of the pixels
    (the GPU test asserts that share), and the flows do exercise occlusions, borders and fractional taps."""
    worst = 0.0
    for (H, W) in ((37, 53), (64, 96), (100, 150), (3, 2051)):
        for N in (1, 3):
            fwd, bwd = parity_flows(H, W, N, seed=H + N)
            band = consistency_band(fwd, bwd)
            for a, b in ((fwd, bwd), (bwd, fwd)):
                occ, inside, margin = np_flow_consistency(a, b)
                share = float((inside & (np.abs(margin) <= band)).mean())
                worst = max(worst, share)
                assert share <= 0.005, ((H, W), N, share)
                if H >= 37:
                    assert (~inside).any() and occ[inside].any() and (~occ).mean() > 0.5
    print(f'[consistency] largest share of pixels inside the band: {100 * worst:.3f} %')


# ------------------------------------------------------------------ the C entries
def test_flow_check_entries_are_declared_exported_and_mirrored():
    """The unit is built (the prototypes: tests/test_host_logic.py test_the_binding_is_the_header)."""
    from tf_raft_amd import build
    assert 'flow_check.hip' in build.SOURCES


def test_flow_check_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    off = C.c_void_p(p.value + 4)
    for name in ('raft_warp_f32', 'raft_warp_u8_f32'):
        fn = getattr(lib, name)
        good = [p, p, p, None, 1, 4, 5, 3, None]                            # (inside may be NULL)
        for k in (0, 1, 2):
            args = list(good)
            args[k] = None
            assert fn(*args) == -1, (name, k)
        for k in range(4, 8):
            for v in (0, -3):
                args = list(good)
                args[k] = v
                assert fn(*args) == -2, (name, k, v)
        for bad in ((1, 4, 1 << 30, 3),                                     # W * C does not fit an int
                    (1, 1 << 15, 1 << 15, 2), (2, 1 << 15, 1 << 15, 1), (1, 1 << 14, 1 << 15, 4), (1 << 10, 1 << 10, 1 << 10, 2),
                    (1 << 20, 1 << 20, 1 << 20, 1)):                        # N * H * W * max(C, 2) reaches 2^31
            args = list(good)
            args[4:8] = bad
            assert fn(*args) == -2, (name, bad)
        args = list(good)
        args[1] = off                                                       # a flow is read as float2
        assert fn(*args) == -4, name
        args[3] = p
        assert fn(*args) == -4, name
    fn = lib.raft_flow_consistency_f32
    good = [p, p, p, p, 1, 4, 5, 0.01, 0.5, None]
    for k in (0, 1, 2):
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    for k in (4, 5, 6):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for bad in ((1, 1 << 15, 1 << 15), (1 << 10, 1 << 10, 1 << 10), (1, 1, 1 << 30)):
        args = list(good)
        args[4:7] = bad
        assert fn(*args) == -2, bad
    for k in (7, 8):
        for v in (-1e-3, float('nan'), float('inf'), -float('inf')):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for k in (0, 1):
        for second in (p, None):                                            # (occluded_b may be NULL)
            args = list(good)
            args[k], args[3] = off, second
            assert fn(*args) == -4, (k, second)


# ------------------------------------------------------------------ the public ops and the model check
def test_alpha_and_beta_are_checked_without_a_gpu():
    from tf_raft_amd import image_ops
    from tf_raft_amd.model import RAFT, SmallRAFT, BidirectionalFlow
    assert BidirectionalFlow._fields == ('forward', 'backward', 'occluded_forward', 'occluded_backward')
    for cls in (RAFT, SmallRAFT):
        assert cls._check_consistency(0.01, 0.5) == (0.01, 0.5)
        assert cls._check_consistency(0, np.float32(2)) == (0.0, 2.0)
        for bad in (-0.01, float('nan'), float('inf'), -float('inf'), 1e39, 'x', None, (0.01,), True, 1j):
            with pytest.raises(ValueError, match='alpha'):
                cls._check_consistency(bad, 0.5)
            with pytest.raises(ValueError, match='beta'):
                cls._check_consistency(0.01, bad)
    for bad in (-1.0, float('nan'), 'x'):
        with pytest.raises(ValueError, match='alpha'):
            image_ops.flow_consistency(np.zeros((4, 5, 2), np.float32), np.zeros((4, 5, 2), np.float32), alpha=bad)
    assert (image_ops.CONSISTENCY_ALPHA, image_ops.CONSISTENCY_BETA) == (0.01, 0.5)

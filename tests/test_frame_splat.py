"""The forward splat of frames and the frame in between, host side (no GPU): the NumPy restatement of DESIGN.md section 25 with
its known answers, the C entries' declarations and argument checks, and the errors of the Python layer.
tests/test_gpu_frame_splat.py compares the kernels with the restatement BIT FOR BIT: everything behind the float32 landing
position, the float32 fraction and the float32 quantisation is integer arithmetic up to one float64 division, so there is no
tolerance anywhere.

The definition: the source pixel at integer ``(x, y)`` of slice ``n`` with vector ``(u, v)`` and time ``t`` (float32) lands on
``sx = float32(x) + t * u``, ``sy = float32(y) + t * v`` (a float32 product, then a float32 sum); it contributes iff
``-1 < sx < float32(W)`` and ``-1 < sy < float32(H)`` and, under a mask, ``mask[n, y, x] != 0``; the corners and their integer
weights ``w`` are the range map's (``np_range_weights``).  Every destination pixel holds ``C + 1`` uint64 sums, ``W += w`` and
``S_c += w * q_c``, with ``q_c`` the byte of a uint8 frame or ``rint(fmin(fmax(value, 0), 255) * 256)`` of a float32 one.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tf_raft_amd import _ffi
from test_consistency import analytic_case, np_flow_consistency
from test_range_occlusion import ONE, all_to_one, np_range_acc, np_range_weights, range_flows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 1, 1), (1, 3, 1), (1, 5, 7), (2, 37, 53), (2, 97, 203)]          # what tests/test_gpu_frame_splat.py runs
TIMES = (0.0, 0.25, 0.3, 1.0)


# ------------------------------------------------------------------ the restatement
def np_quantise(frames):
    """uint8 -> the byte; float32 on 0 .. 255 -> rint(clamp * 256), a NaN gives 0.  int64."""
    frames = np.asarray(frames)
    if frames.dtype == np.uint8:
        return frames.astype(np.int64)
    assert frames.dtype == np.float32
    with np.errstate(invalid='ignore'):
        q = np.rint(np.fmin(np.fmax(frames, np.float32(0)), np.float32(255)) * np.float32(256))
    assert q.dtype == np.float32
    return q.astype(np.int64)


def np_frame_splat_acc(frames, flow, t, mask=None):
    """(N, H, W, C) uint8 / float32, (N, H, W, 2) float32, a time -> the uint64 sums (N, H, W, C + 1): W in front of the S_c."""
    frames, flow = np.asarray(frames), np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 4 and flow.shape == frames.shape[:3] + (2,)
    N, H, W, Cn = frames.shape
    t = np.float32(t)
    q = np_quantise(frames)
    acc = np.zeros((N, H, W, Cn + 1), np.uint64)
    with np.errstate(invalid='ignore', over='ignore'):
        sx = np.arange(W, dtype=np.float32)[None, None, :] + t * flow[..., 0]
        sy = np.arange(H, dtype=np.float32)[None, :, None] + t * flow[..., 1]
        assert sx.dtype == sy.dtype == np.float32
        ok = (sx > np.float32(-1)) & (sx < np.float32(W)) & (sy > np.float32(-1)) & (sy < np.float32(H))
    if mask is not None:
        ok &= np.asarray(mask) != 0
    n = np.nonzero(ok)[0]
    sx, sy, q = sx[ok], sy[ok], q[ok]
    fx, fy = np.floor(sx), np.floor(sy)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    w = np_range_weights(sx - fx, sy - fy)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        cx, cy = x0 + dx, y0 + dy
        keep = (w[k] > 0) & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        wk = w[k][keep]
        np.add.at(acc[..., 0], (n[keep], cy[keep], cx[keep]), wk.astype(np.uint64))
        for c in range(Cn):
            np.add.at(acc[..., 1 + c], (n[keep], cy[keep], cx[keep]), (wk * q[keep, c]).astype(np.uint64))
    return acc


def _scale(frames):
    return 1.0 if np.asarray(frames).dtype == np.uint8 else 0.00390625


def np_splat(frames, flow, t=1.0, mask=None, acc=None):
    """-> (dst float32 (N, H, W, C), weight float32 (N, H, W)).  ``acc``: the sums where the caller has them already."""
    acc = np_frame_splat_acc(frames, flow, t, mask) if acc is None else acc
    Wd, S = acc[..., :1].astype(np.float64), acc[..., 1:].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        dst = np.where(Wd > 0, S / Wd, 0.0) * _scale(frames)
    return dst.astype(np.float32), (acc[..., 0].astype(np.float64) * 2.0 ** -24).astype(np.float32)


def np_interpolate(image1, image2, flow_forward, flow_backward, t=0.5, mask1=None, mask2=None, dtype=np.float32, acc1=None, acc2=None):
    """-> (frame of ``dtype`` (N, H, W, C), holes uint8 (N, H, W))."""
    t = np.float32(t)
    s = np.float32(1) - t
    acc1 = np_frame_splat_acc(image1, flow_forward, t, mask1) if acc1 is None else acc1
    acc2 = np_frame_splat_acc(image2, flow_backward, s, mask2) if acc2 is None else acc2
    td = np.float64(t)
    a, b = (1.0 - td) * acc1[..., :1].astype(np.float64), td * acc2[..., :1].astype(np.float64)
    den = a + b
    landed = den > 0
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = ((1.0 - td) * acc1[..., 1:].astype(np.float64) + td * acc2[..., 1:].astype(np.float64)) / den
    fade = (1.0 - td) * np_quantise(image1).astype(np.float64) + td * np_quantise(image2).astype(np.float64)
    out = np.where(landed, mean, fade) * _scale(image1)
    holes = (~landed[..., 0]).astype(np.uint8)
    if dtype == np.uint8:
        assert np.asarray(image1).dtype == np.uint8
        return np.fmin(np.rint(out), 255.0).astype(np.uint8), holes
    return out.astype(np.float32), holes


# ------------------------------------------------------------------ the inputs both test files use
def splat_flows(N, H, W):
    """``range_flows(N, H, W, seed=H + W)`` and, where the frame has room (H >= 37), in sample 0: a 10 x 12 block in BOTH
    directions whose vectors leave the frame (nothing lands inside it: the neighbours move 1.5 px at most), and in each direction
    a block of vectors of 25 to 36 px per axis, beyond any LDS window."""
    f = range_flows(N, H, W, seed=H + W)
    if H >= 37:
        rng = np.random.default_rng(1000 + H + W)
        f[0, 6:16, 8:20] = (-(W + 100.0), 0.0)
        f[N, 6:16, 8:20] = (0.0, H + 100.0)
        far = rng.uniform(25, 36, size=(2, 6, 6, 2)).astype(np.float32)
        f[0, 20:26, 4:10] = far[0]
        f[N, 28:34, 30:36] = far[1] * np.float32([1, -1])
    return np.ascontiguousarray(f)


def splat_frames(N, H, W, Cn, kind, seed=0):
    """Two frame batches (2, N, H, W, C): uint8, or float32 that leaves 0 .. 255 on both sides and holds a NaN and infinities."""
    rng = np.random.default_rng(seed + 31 * H + W + 7 * Cn)
    if kind == 'u8':
        return rng.integers(0, 256, size=(2, N, H, W, Cn), dtype=np.uint8)
    x = rng.uniform(-20.0, 280.0, size=(2, N, H, W, Cn)).astype(np.float32)
    if H * W > 1:
        x[0, 0, 0, 0, 0], x[1, 0, -1, -1, 0], x[0, -1, -1, 0, -1] = np.nan, np.inf, -np.inf
        x[1, 0, 0, 0, -1] = 127.998046875                                   # a tie of the quantiser: 32767.5
    return x


def splat_masks(N, H, W):
    """(2N, H, W) uint8, non-zero = the pixel is splatted (values other than 1 on purpose)."""
    return (np.random.default_rng(11 + H * W).uniform(size=(2 * N, H, W)) < 0.7).astype(np.uint8) * 3


def classes(acc1, acc2):
    """The four classes of a destination pixel: both splats land, only frame 1's, only frame 2's, neither (a hole at 0 < t < 1)."""
    l1, l2 = acc1[..., 0] > 0, acc2[..., 0] > 0
    return l1 & l2, l1 & ~l2, ~l1 & l2, ~l1 & ~l2


# ------------------------------------------------------------------ known answers
H0, W0 = 37, 53


def _u8(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def test_zero_flow_gives_the_frame_itself_and_weight_one():
    zero = np.zeros((2, H0, W0, 2), np.float32)
    for frames in (_u8(0, 2, H0, W0, 3), (_u8(1, 2, H0, W0, 3).astype(np.float32) * np.float32(0.5))):
        for t in TIMES:
            dst, weight = np_splat(frames, zero, t)
            np.testing.assert_array_equal(dst, frames.astype(np.float32))
            np.testing.assert_array_equal(weight, np.ones((2, H0, W0), np.float32))
            acc = np_frame_splat_acc(frames, zero, t)
            assert acc.dtype == np.uint64 and (acc[..., 0] == ONE).all()


def test_an_integer_shift_moves_the_window_and_leaves_a_band_of_holes():
    frames = _u8(2, 1, H0, W0, 3)
    f = np.zeros((1, H0, W0, 2), np.float32)
    f[...] = (3, -2)
    dst, weight = np_splat(frames, f, 1.0)
    want = np.zeros((1, H0, W0, 3), np.float32)
    want[:, :H0 - 2, 3:] = frames[:, 2:, :W0 - 3]
    np.testing.assert_array_equal(dst, want)
    landed = np.zeros((1, H0, W0), np.float32)
    landed[:, :H0 - 2, 3:] = 1
    np.testing.assert_array_equal(weight, landed)
    f[...] = (6, -4)                                                        # ... and the same window at t = 0.5
    np.testing.assert_array_equal(np_splat(frames, f, 0.5)[0], want)
    _, holes = np_interpolate(frames, frames, f, f, 0.5, mask2=np.zeros((1, H0, W0), np.uint8))
    np.testing.assert_array_equal(holes, 1 - landed.astype(np.uint8))


@pytest.mark.parametrize('shape', SHAPES)
def test_interpolate_at_the_ends_returns_the_frames_for_any_flows(shape):
    """t = 0: frame 1 stays where it is (0 * u = 0; a non-finite vector gives a NaN and is skipped, its pixel is a hole unless a
    neighbour stayed too -- none moves -- and a hole's fallback at t = 0 is frame 1's own value); frame 2's share has weight 0."""
    N, H, W = shape
    flows = splat_flows(N, H, W)
    i1, i2 = splat_frames(N, H, W, 3, 'u8')
    masks = splat_masks(N, H, W)
    for m1, m2 in ((None, None), (masks[:N], masks[N:])):
        for dtype in (np.float32, np.uint8):
            got0, holes0 = np_interpolate(i1, i2, flows[:N], flows[N:], 0.0, m1, m2, dtype)
            got1, holes1 = np_interpolate(i1, i2, flows[:N], flows[N:], 1.0, m1, m2, dtype)
            np.testing.assert_array_equal(got0, i1.astype(dtype))
            np.testing.assert_array_equal(got1, i2.astype(dtype))
            if H >= 5:
                assert holes0.any()                                         # the non-finite vectors, the masked pixels
            if m1 is not None:
                np.testing.assert_array_equal(holes0 != 0, (m1 == 0) | ~np.isfinite(flows[:N]).all(-1))


def test_the_weight_plane_at_t_1_is_the_range_map_accumulator():
    for shape in SHAPES:
        N, H, W = shape
        flows = splat_flows(N, H, W)
        frames = np.concatenate(splat_frames(N, H, W, 3, 'f32'))
        np.testing.assert_array_equal(np_frame_splat_acc(frames, flows, 1.0)[..., 0], np_range_acc(flows))


def test_the_moving_square_has_its_closed_form_picture():
    """tests/test_consistency.py's square, moved by the even vector (8, -4), at t = 0.5 with the occluded pixels skipped: the
    square's texture half way; the background wherever neither square is; where the half-way square covers background that no
    square touches, the mean of both; and the rest of the two squares' footprints -- nothing lands there -- cross-faded."""
    f1, f2, fwd, bwd, sq1, sq2 = analytic_case(H0, W0, N=2, d=(8, -4))
    occ_f, occ_b = np_flow_consistency(fwd, bwd)[0], np_flow_consistency(bwd, fwd)[0]
    np.testing.assert_array_equal(occ_f, np.broadcast_to(sq2 & ~sq1, occ_f.shape))
    np.testing.assert_array_equal(occ_b, np.broadcast_to(sq1 & ~sq2, occ_b.shape))
    got, holes = np_interpolate(f1, f2, fwd, bwd, 0.5, (~occ_f).astype(np.uint8), (~occ_b).astype(np.uint8))
    sqm = np.roll(sq1, (-2, 4), axis=(0, 1))
    tex = np.roll(f1, (-2, 4), axis=(1, 2)).astype(np.float64)             # the texture half way (read inside sqm only)
    either = sq1 | sq2
    assert (sqm & ~either).any() and (either & ~sqm).any() and (sqm & either).any()
    bg = f1.astype(np.float64)                                              # (outside sq1: the background, the same in both frames)
    want = np.where((sqm & either)[None, :, :, None], tex, bg)
    want = np.where((sqm & ~either)[None, :, :, None], (tex + bg) / 2, want)
    want = np.where((either & ~sqm)[None, :, :, None], 0.5 * f1.astype(np.float64) + 0.5 * f2.astype(np.float64), want)
    np.testing.assert_array_equal(got, want.astype(np.float32))
    np.testing.assert_array_equal(holes, np.broadcast_to(either & ~sqm, holes.shape).astype(np.uint8))
    as_bytes, _ = np_interpolate(f1, f2, fwd, bwd, 0.5, (~occ_f).astype(np.uint8), (~occ_b).astype(np.uint8), np.uint8)
    np.testing.assert_array_equal(as_bytes, np.rint(want).astype(np.uint8))           # (ties to even, as rint does)


def test_a_float_frame_in_steps_of_1_256_round_trips_exactly():
    rng = np.random.default_rng(3)
    frames = (rng.integers(0, 65281, size=(1, H0, W0, 3)).astype(np.float32) / np.float32(256))
    assert frames.max() <= 255 and (frames * 256 == np.rint(frames * 256)).all()
    zero = np.zeros((1, H0, W0, 2), np.float32)
    np.testing.assert_array_equal(np_splat(frames, zero, 0.3)[0], frames)
    np.testing.assert_array_equal(np_interpolate(frames, frames, zero, zero, 0.3)[0], frames)
    f = np.zeros((1, H0, W0, 2), np.float32)
    f[..., 0] = 0.5                                                         # every interior pixel: the exact mean of two
    dst, _ = np_splat(frames, f, 1.0)
    np.testing.assert_array_equal(dst[:, :, 1:], ((frames[:, :, 1:].astype(np.float64) + frames[:, :, :-1]) / 2).astype(np.float32))


def test_float_values_are_clamped_and_a_nan_is_zero():
    v = np.float32([-3.0, 0.0, 0.001953125, 127.998046875, 255.0, 300.0, np.nan, np.inf, -np.inf]).reshape(1, 1, 9, 1)
    np.testing.assert_array_equal(np_quantise(v).ravel(), [0, 0, 0, 32768, 65280, 65280, 0, 65280, 0])       # (ties to even)
    dst, _ = np_splat(v, np.zeros((1, 1, 9, 2), np.float32), 1.0)
    np.testing.assert_array_equal(dst.ravel(), np.float32([0, 0, 0, 128.0, 255, 255, 0, 255, 0]))


def test_every_vector_on_one_pixel_drives_the_sums_past_32_bits():
    frames = _u8(4, 1, H0, W0, 3)
    acc = np_frame_splat_acc(frames, all_to_one(H0, W0, 11, 17)[None], 1.0)[0]
    assert int(acc[11, 17, 0]) == H0 * W0 * ONE > 1 << 32
    for c in range(3):
        assert int(acc[11, 17, 1 + c]) == ONE * int(frames[..., c].sum()) > 1 << 40
    assert np.count_nonzero(acc[..., 0]) == 1
    dst, weight = np_splat(frames, all_to_one(H0, W0, 11, 17)[None], 1.0)
    np.testing.assert_array_equal(dst[0, 11, 17], (frames.reshape(-1, 3).sum(0).astype(np.float64) / (H0 * W0)).astype(np.float32))
    assert weight[0, 11, 17] == np.float32(H0 * W0)
    # at t = 0.5 every vector goes half way: the frame shrinks to half its size around the pixel
    half = np_frame_splat_acc(frames, all_to_one(H0, W0, 11, 17)[None], 0.5)[0]
    assert int(half[..., 0].sum()) == H0 * W0 * ONE and np.count_nonzero(half[..., 0]) < H0 * W0 // 3


@pytest.mark.parametrize('shape', [s for s in SHAPES if s[1] >= 37])
def test_the_test_flows_exercise_every_branch(shape):
    N, H, W = shape
    flows = splat_flows(N, H, W)
    assert flows.shape == (2 * N, H, W, 2) and flows.dtype == np.float32
    assert np.isnan(flows).any() and np.isinf(flows).any() and (np.abs(flows) == np.float32(1e30)).any()
    big = np.abs(flows[[0, N]]).min(-1)
    with np.errstate(invalid='ignore'):
        assert ((big >= 25) & (big <= 36)).sum() == 72                      # the two far blocks
    i1, i2 = splat_frames(N, H, W, 3, 'u8')
    for t in (0.25, 0.3):
        acc1 = np_frame_splat_acc(i1, flows[:N], t)
        acc2 = np_frame_splat_acc(i2, flows[N:], np.float32(1) - np.float32(t))
        both, only1, only2, none = classes(acc1, acc2)
        assert both.any() and only1.any() and only2.any() and none.any()
        # the block nothing lands in: a neighbour moves 1.5 * 0.75 px at most and its footprint reaches one pixel further
        assert 6 * 8 <= int(none[0, 6:16, 8:20].sum()) <= 10 * 12
        _, holes = np_interpolate(i1, i2, flows[:N], flows[N:], t, acc1=acc1, acc2=acc2)
        np.testing.assert_array_equal(holes != 0, none)
        assert (acc1[..., 0] > ONE).any() and ((acc1[..., 0] > 0) & (acc1[..., 0] < ONE)).any()


def test_the_time_takes_the_float32_product_rule():
    """0.3 is no binary fraction: float32(0.3) * u, rounded, then added to x, rounded -- not x + 0.3 * u in one rounding."""
    t = np.float32(0.3)
    f = np.zeros((1, 1, 64, 2), np.float32)
    f[0, 0, :, 0] = np.random.default_rng(9).uniform(-0.9, 0.9, 64).astype(np.float32)
    u = f[0, 0, :, 0]
    frames = _u8(5, 1, 1, 64, 1)
    acc = np_frame_splat_acc(frames, f, 0.3)
    sx = np.arange(64, dtype=np.float32) + t * u
    assert sx.dtype == np.float32
    fused = (np.arange(64, dtype=np.float64) + np.float64(t) * u.astype(np.float64)).astype(np.float32)
    assert (sx != fused).any()                                              # the two rules differ on this row
    want = np.zeros((64,), np.uint64)
    x0 = np.floor(sx).astype(np.int64)
    qa = np.rint((sx - np.floor(sx)) * np.float32(4096)).astype(np.int64)
    for x in range(64):
        for cx, w in ((x0[x], (4096 - qa[x]) * 4096), (x0[x] + 1, qa[x] * 4096)):
            if 0 <= cx < 64:
                want[cx] += np.uint64(w)
    np.testing.assert_array_equal(acc[0, 0, :, 0], want)


# ------------------------------------------------------------------ the C entries
SPLAT_ENTRIES = ('raft_splat_frames_f32', 'raft_splat_frames_u8_f32')
INTERPOLATE_ENTRIES = ('raft_interpolate_frames_f32', 'raft_interpolate_frames_u8_f32', 'raft_interpolate_frames_u8')


def test_the_header_declares_and_the_library_exports_the_entries():
    from tf_raft_amd import build
    assert 'frame_splat.hip' in build.SOURCES and 'flow_splat.hip' in build.SOURCES and 'splat_geometry.h' in build.HEADERS
    with open(os.path.join(ROOT, 'include', 'raft_hip.h')) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    assert re.search(r'int64_t\s+raft_frame_splat_workspace_bytes\s*\(\s*int slices,\s*int H,\s*int W,\s*int C\s*\)', header)
    for name in SPLAT_ENTRIES + INTERPOLATE_ENTRIES:
        assert re.search(r'int\s+' + name + r'\s*\(', header), name
    sigs = _ffi.header_signatures(header)
    P, I, F = C.c_void_p, C.c_int, C.c_float
    assert sigs['raft_frame_splat_workspace_bytes'] == (C.c_int64, [I, I, I, I])
    for name in SPLAT_ENTRIES:          # src flow mask t dst weight N H W C workspace stream
        assert sigs[name] == (I, [P, P, P, F, P, P, I, I, I, I, P, P]), name
    for name in INTERPOLATE_ENTRIES:    # image1 image2 flow_forward flow_backward mask1 mask2 t dst holes N H W C workspace stream
        assert sigs[name] == (I, [P, P, P, P, P, P, F, P, P, I, I, I, I, P, P]), name
    assert _ffi.ABI_VERSION == 222                                   # entries were added, no signature changed
    lib = _ffi.load_library()
    assert lib.raft_version() == 222
    assert lib.raft_interpolate_frames_u8.argtypes == sigs['raft_interpolate_frames_u8'][1]
    assert lib.raft_frame_splat_workspace_bytes(3, 37, 53, 3) == 3 * 37 * 53 * 4 * 8
    assert lib.raft_frame_splat_workspace_bytes(8, 1080, 1920, 3) == 8 * 1080 * 1920 * 4 * 8
    assert lib.raft_frame_splat_workspace_bytes(1, 1 << 12, 1 << 12, 4) == (1 << 24) * 5 * 8
    for bad in ((0, 4, 5, 3), (1, 0, 5, 3), (1, 4, -1, 3), (1, 4, 5, 0), (1, 4, 5, 5), (1, 1 << 12, (1 << 12) + 1, 3),
                (1 << 10, 1 << 10, 1 << 10, 1)):
        assert lib.raft_frame_splat_workspace_bytes(*bad) == 0, bad


SIZES_REFUSED = ((1, 4, 5, 0), (1, 4, 5, 5), (1, 4, 5, -1),                                    # C outside 1 .. 4
                 (1, 1 << 12, (1 << 12) + 1, 3), (1, 1, (1 << 24) + 1, 1), (1, 1 << 15, 1 << 15, 3),      # H * W > 2^24
                 (1 << 10, 1 << 10, 1 << 10, 3), (32, 1 << 12, 1 << 12, 1))                      # slices * H * W * 4 >= 2^31


def _buffers():
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    return buf, p, C.c_void_p(p.value + 4)


@pytest.mark.parametrize('name', SPLAT_ENTRIES)
def test_splat_argument_errors_are_returned_before_any_device_work(name):
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    fn = getattr(_ffi.load_library(), name)
    _keep, p, off = _buffers()
    #       src flow mask t   dst weight N H  W  C  ws stream
    good = [p, p, p, 0.5, p, p, 1, 4, 5, 3, p, None]
    for k in (0, 1, 4, 10):                                         # (mask and weight may be NULL)
        for opt in (p, None):
            args = list(good)
            args[k], args[2], args[5] = None, opt, opt
            assert fn(*args) == -1, k
    for k in (6, 7, 8, 9):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for bad in SIZES_REFUSED:
        args = list(good)
        args[6:10] = bad
        assert fn(*args) == -2, bad
    for t in (float('nan'), float('inf'), -float('inf')):
        args = list(good)
        args[3] = t
        assert fn(*args) == -2, t
    for k in (1, 10):
        args = list(good)
        args[k] = off
        assert fn(*args) == -4, k
    args = list(good)                                               # precedence: NULL before shape before alignment
    args[4], args[9], args[1] = None, 0, off
    assert fn(*args) == -1
    args[4] = p
    assert fn(*args) == -2
    args[9], args[3] = 4, float('nan')
    assert fn(*args) == -2
    args[3] = -2.5                                                  # (any finite time is allowed)
    assert fn(*args) == -4


@pytest.mark.parametrize('name', INTERPOLATE_ENTRIES)
def test_interpolate_argument_errors_are_returned_before_any_device_work(name):
    fn = getattr(_ffi.load_library(), name)
    _keep, p, off = _buffers()
    #       image1 image2 fwd bwd mask1 mask2 t  dst holes N H  W  C  ws stream
    good = [p, p, p, p, p, p, 0.5, p, p, 1, 4, 5, 3, p, None]
    for k in (0, 1, 2, 3, 7, 13):                                   # (the masks and holes may be NULL)
        for opt in (p, None):
            args = list(good)
            args[k], args[4], args[5], args[8] = None, opt, opt, opt
            assert fn(*args) == -1, k
    for k in (9, 10, 11, 12):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for bad in SIZES_REFUSED + ((16, 1 << 12, 1 << 12, 1), (1 << 29, 1, 1, 1), (1 << 30, 1, 1, 1)):       # 2N slices
        args = list(good)
        args[9:13] = bad
        assert fn(*args) == -2, bad
    for t in (float('nan'), float('inf'), -float('inf'), -2.0 ** -20, 1.0 + 2.0 ** -20, 2.0):
        args = list(good)
        args[6] = t
        assert fn(*args) == -2, t
    for k in (2, 3, 13):
        args = list(good)
        args[k] = off
        assert fn(*args) == -4, k
    args = list(good)                                               # precedence: NULL before shape before alignment
    args[1], args[6], args[3] = None, 2.0, off
    assert fn(*args) == -1
    args[1] = p
    assert fn(*args) == -2
    for t in (0.0, 1.0):                                            # (both ends are allowed)
        args[6] = t
        assert fn(*args) == -4


# ------------------------------------------------------------------ the Python layer, nothing reaches the device
BAD_TIMES = (float('nan'), float('inf'), -float('inf'), 10 ** 400, 'x', None, True, 1j)
BAD_UNIT_TIMES = BAD_TIMES + (-0.25, 1.5, -1e-30 - 1e-9, 2)


def test_the_time_is_checked_without_a_gpu():
    from tf_raft_amd import image_ops
    assert image_ops.check_splat_time(0.3) == float(np.float32(0.3))          # what the entry will see
    assert image_ops.check_splat_time(-2) == -2.0 and image_ops.check_splat_time(np.float32(1.5)) == 1.5
    assert image_ops.check_splat_time(0, unit=True) == 0.0 and image_ops.check_splat_time(1, unit=True) == 1.0
    u8 = np.zeros((4, 5, 3), np.uint8)
    zero = np.zeros((4, 5, 2), np.float32)
    for bad in BAD_TIMES:
        with pytest.raises(ValueError, match='t must'):
            image_ops.check_splat_time(bad)
        with pytest.raises(ValueError, match='t must'):
            image_ops.splat(u8, zero, t=bad)
    for bad in BAD_UNIT_TIMES:
        with pytest.raises(ValueError, match='t must'):
            image_ops.interpolate(u8, u8, zero, zero, t=bad)
        with pytest.raises(ValueError, match='t must'):
            image_ops.interpolate(u8, u8, zero, zero, t=[0.5, bad])
    with pytest.raises(ValueError, match='empty'):
        image_ops.interpolate(u8, u8, zero, zero, t=[])


def test_shapes_and_types_are_checked_without_a_gpu():
    import torch
    from tf_raft_amd import image_ops
    u8, f32 = np.zeros((2, 4, 5, 3), np.uint8), np.zeros((2, 4, 5, 3), np.float32)
    zero = np.zeros((2, 4, 5, 2), np.float32)
    mask = np.ones((2, 4, 5), np.uint8)
    with pytest.raises(ValueError, match=r'\(H, W, C\) or \(N, H, W, C\)'):
        image_ops.splat(np.zeros((4, 5), np.uint8), zero)
    with pytest.raises(ValueError, match='empty'):
        image_ops.splat(np.zeros((0, 4, 5, 3), np.uint8), zero)
    with pytest.raises(TypeError, match='uint8 or float32'):
        image_ops.splat(np.zeros((2, 4, 5, 3), bool), zero)
    with pytest.raises(TypeError):
        image_ops.splat(np.zeros((2, 4, 5, 3), np.int32), zero)
    with pytest.raises(ValueError, match='expects a flow'):
        image_ops.splat(u8, zero[:1])
    with pytest.raises(TypeError, match='a flow is float32'):
        image_ops.splat(u8, zero.astype(np.uint8))
    with pytest.raises(ValueError, match='expects a mask'):
        image_ops.splat(u8, zero, mask=mask[..., None])
    with pytest.raises(TypeError, match='a mask is uint8 or bool'):
        image_ops.splat(u8, zero, mask=mask.astype(np.float32))
    with pytest.raises(ValueError, match='1 to 4 channels'):
        image_ops.splat(np.zeros((2, 4, 5, 5), np.uint8), zero)
    with pytest.raises(ValueError, match='too large'):
        image_ops.splat(torch.empty((1, 4097, 4096, 1), dtype=torch.uint8, device='meta'),
                        torch.empty((1, 4097, 4096, 2), dtype=torch.float32, device='meta'))
    # interpolate: the same, for both frames, both flows and both masks
    with pytest.raises(ValueError, match='one shape and type'):
        image_ops.interpolate(u8, f32, zero, zero)
    with pytest.raises(ValueError, match='one shape and type'):
        image_ops.interpolate(u8, u8[:1], zero, zero)
    with pytest.raises(ValueError, match='expects a flow'):
        image_ops.interpolate(u8, u8, zero, zero[..., :1])
    with pytest.raises(ValueError, match='expects a flow'):
        image_ops.interpolate(u8, u8, zero[0], zero)
    with pytest.raises(ValueError, match='expects a mask'):
        image_ops.interpolate(u8, u8, zero, zero, mask2=mask[:1])
    with pytest.raises(ValueError, match='expects a mask'):
        image_ops.interpolate(u8, u8, zero, zero, mask1=mask[0])
    with pytest.raises(TypeError, match='uint8 for uint8 frames'):
        image_ops.interpolate(f32, f32, zero, zero, dtype=torch.uint8)          # uint8 results for uint8 frames only
    with pytest.raises(TypeError, match='uint8 for uint8 frames'):
        image_ops.interpolate(u8, u8, zero, zero, dtype=torch.float16)
    with pytest.raises(ValueError, match='too large'):
        image_ops.interpolate(*[torch.empty((1, 4097, 4096, 1), dtype=torch.uint8, device='meta')] * 2,
                              *[torch.empty((1, 4097, 4096, 2), dtype=torch.float32, device='meta')] * 2)


def test_the_model_checks_its_arguments_before_any_device_work():
    import inspect
    from tf_raft_amd.model import RAFT, SmallRAFT
    x = np.zeros((1, 64, 96, 3), np.float32)
    for cls in (RAFT, SmallRAFT):
        sig = inspect.signature(cls.interpolate_step).parameters
        assert sig['t'].default == 0.5 and sig['skip_occluded'].default is False         # every pixel is splatted: a choice
        assert inspect.signature(cls.predict_interpolated).parameters['t'].default == 0.5
        assert inspect.signature(cls.interpolate_video).parameters['factor'].default == 2
        model = cls.__new__(cls)                                             # (no device: anything enqueued would fail)
        for bad in BAD_UNIT_TIMES:
            with pytest.raises(ValueError, match='t must'):
                model.interpolate_step((x, x), t=bad)
            with pytest.raises(ValueError, match='t must'):
                model.predict_interpolated([x, x], t=[0.25, bad])
        with pytest.raises(TypeError, match='unexpected keyword'):
            model.interpolate_step((x, x), gamma=1.0)
        with pytest.raises(ValueError, match='one type'):
            model.interpolate_step((x, x.astype(np.uint8)))
        with pytest.raises(ValueError, match='one type'):
            model.interpolate_step((x, x[:, :32]))
        with pytest.raises(ValueError, match=r'\(T, H, W, 3\)'):
            model.interpolate_video(x[0])
        with pytest.raises(ValueError, match='at least two frames'):
            model.interpolate_video(x)
        for bad in (0, -1, 1.5, True, None, '2'):
            with pytest.raises(ValueError, match='factor'):
                model.interpolate_video(np.zeros((3, 64, 96, 3), np.uint8), factor=bad)

"""Motion-compensated temporal filtering without a GPU: ``np_fuse_frames``, the float32 NumPy restatement of
csrc/frame_fuse.hip in exactly its operation order, with its known answers, the denoising and ghosting conditions, the inputs
tests/test_gpu_frame_fuse.py runs and what they cover, and the argument checks of every entry, C and Python, none of which may
reach a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tf_raft_amd import _ffi, image_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

# (K, N, H, W, C, r): what tests/test_gpu_frame_fuse.py runs.  The kernel's tile is 32 x 8: (9, 33) and (19, 70) cross a tile edge
# on each axis and leave partial tiles, (17, 64) has whole tiles along x.
SHAPES = [(1, 1, 1, 1, 1, 0), (1, 1, 1, 1, 3, 3), (2, 2, 5, 7, 3, 1), (3, 1, 9, 33, 3, 2), (4, 2, 19, 70, 4, 3), (16, 1, 8, 40, 1, 1),
          (3, 2, 17, 64, 2, 1)]
IDS = ['x'.join(map(str, s)) for s in SHAPES]


# ------------------------------------------------------------------ the restatement
def np_taps(sx, sy, H, W):
    """csrc/flow_sample.h sample_taps on float32 arrays: ``(in, x0, x1, y0, y1, a, b)``."""
    with np.errstate(invalid='ignore'):
        inn = (sx >= 0) & (sx <= f32(W - 1)) & (sy >= 0) & (sy <= f32(H - 1))
    px, py = np.where(inn, sx, f32(0)).astype(f32), np.where(inn, sy, f32(0)).astype(f32)
    fx, fy = np.floor(px), np.floor(py)
    x0, y0 = np.clip(fx.astype(np.int64), 0, W - 1), np.clip(fy.astype(np.int64), 0, H - 1)
    return inn, x0, np.minimum(x0 + 1, W - 1), y0, np.minimum(y0 + 1, H - 1), px - fx, py - fy


def np_fuse_frames(center, neighbours, vectors, skip=None, absolute=False, sigma=image_ops.FUSE_SIGMA,
                   center_weight=image_ops.FUSE_CENTER_WEIGHT, patch_radius=image_ops.FUSE_PATCH_RADIUS, out_uint8=False, info=None):
    """csrc/frame_fuse.hip restated: ``center`` (N, H, W, C) uint8 / float32, ``neighbours`` (K, N, H, W, C), ``vectors``
    (K, N, H, W, 2) float32, ``skip`` uint8 (K, N, H, W) or None -> ``(dst (N, H, W, C), weight (N, H, W))``.  Every product, sum and
    quotient is one float32 operation, in the kernel's order.  ``info``: a dict that receives ``vis`` and ``cnt`` (K, N, H, W)."""
    center, neighbours, vectors = np.asarray(center), np.asarray(neighbours), np.asarray(vectors, f32)
    K, N, H, W, Cn = neighbours.shape
    r = int(patch_radius)
    assert center.shape == (N, H, W, Cn) and vectors.shape == (K, N, H, W, 2) and center.dtype == neighbours.dtype
    cen = center.astype(f32)
    ys, xs = np.mgrid[0:H, 0:W]
    s2 = f32(sigma) * f32(sigma)
    cw = f32(center_weight)
    num = (cw * cen).astype(f32)
    den = np.full((N, H, W), cw, f32)
    all_vis, all_cnt = np.zeros((K, N, H, W), bool), np.zeros((K, N, H, W), np.int32)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for k in range(K):
            for n in range(N):
                u, v = vectors[k, n, ..., 0], vectors[k, n, ..., 1]
                sx, sy = (u, v) if absolute else (xs.astype(f32) + u, ys.astype(f32) + v)
                inn, x0, x1, y0, y1, a, b = np_taps(sx, sy, H, W)
                vis = inn & (True if skip is None else skip[k, n] == 0)
                g = neighbours[k, n].astype(f32)
                a, b = a[..., None], b[..., None]
                na, nb = f32(1) - a, f32(1) - b
                c = nb * (na * g[y0, x0] + a * g[y0, x1]) + b * (na * g[y1, x0] + a * g[y1, x1])
                assert c.dtype == f32
                q = None
                for ch in range(Cn):
                    d = cen[n, ..., ch] - c[..., ch]
                    q = d * d if q is None else q + d * d
                qp, vp = np.pad(np.where(vis, q, f32(0)).astype(f32), r), np.pad(vis.astype(np.int32), r)
                total, cnt = np.zeros((H, W), f32), np.zeros((H, W), np.int32)
                for dy in range(2 * r + 1):
                    for dx in range(2 * r + 1):
                        total = total + qp[dy:dy + H, dx:dx + W]
                        cnt = cnt + vp[dy:dy + H, dx:dx + W]
                m = total / (cnt * Cn).astype(f32)
                w = np.where(vis, s2 / (s2 + m), f32(0)).astype(f32)
                num[n] = num[n] + w[..., None] * c
                den[n] = den[n] + w
                all_vis[k, n], all_cnt[k, n] = vis, cnt
        dst = num / den[..., None]
    assert dst.dtype == f32 and den.dtype == f32
    if info is not None:
        info.update(vis=all_vis, cnt=all_cnt)
    if out_uint8:
        dst = np.clip(np.rint(dst), 0, 255).astype(np.uint8)
    return dst, den


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def assert_same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    np.testing.assert_array_equal(bits(got), bits(want))


def grid_of(H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs, ys], axis=-1).astype(f32)


# ------------------------------------------------------------------ the inputs of the GPU tests
def fuse_case(shape, seed=1):
    """Inputs for one shape: a dict with uint8 ``center`` / ``neighbours``, their float32 twins ``center_f`` / ``neighbours_f``
    (off the integers), ``flows`` with zero, sub-pixel, border-landing, leaving and non-finite vectors, ``positions`` (grid + flow
    in float32, so both forms sample the same points) and ``skip``.  About one pixel in eight sees no neighbour at all."""
    K, N, H, W, Cn, r = shape
    rng = np.random.default_rng(seed * 1000 + K * 131 + H * 17 + W)
    ys, xs = np.mgrid[0:H, 0:W]
    base = 128 + 60 * np.sin(xs / 5.0) * np.cos(ys / 7.0) + 40 * np.sin((xs + ys) / 3.0)
    frames = base[None, None, ..., None] + rng.normal(0, 12, (K + 1, N, H, W, Cn)) + 10 * np.arange(Cn)
    frames_f = np.clip(frames, 0, 255).astype(f32)
    frames_u = np.clip(np.rint(frames), 0, 255).astype(np.uint8)
    flows = rng.normal(0, 1.5, (K, N, H, W, 2)).astype(f32)
    kind = rng.integers(0, 16, (K, N, H, W))
    flows[kind == 0] = 0                                                             # zero
    flows[kind == 1] = np.rint(flows[kind == 1])                                     # whole pixels
    land_x, land_y = kind == 2, kind == 3                                            # taps exactly on W - 1 / H - 1
    flows[..., 0][land_x] = np.broadcast_to((W - 1 - xs).astype(f32), kind.shape)[land_x]
    flows[..., 1][land_x] = 0
    flows[..., 1][land_y] = np.broadcast_to((H - 1 - ys).astype(f32), kind.shape)[land_y]
    flows[..., 0][land_y] = 0
    flows[kind == 4] += f32(2 * max(H, W))                                           # leaving
    flows[kind == 5] -= f32(2 * max(H, W))
    flows[..., 0][kind == 6] = np.nan
    flows[..., 1][kind == 7] = np.inf
    flows[..., 0][kind == 8] = -np.inf
    blind = np.broadcast_to(rng.integers(0, 8, (1, N, H, W)) == 0, kind.shape)      # no neighbour is seen here
    half = np.arange(K)[:, None, None, None] % 2 == 0
    flows[..., 0][blind & half] = np.nan
    skip = (rng.integers(0, 6, (K, N, H, W)) == 0).astype(np.uint8) * rng.integers(1, 3, (K, N, H, W)).astype(np.uint8)
    skip[blind & ~half] = 2
    positions = (grid_of(H, W)[None, None] + flows).astype(f32)
    return dict(center=frames_u[0], neighbours=np.ascontiguousarray(frames_u[1:]), center_f=frames_f[0],
                neighbours_f=np.ascontiguousarray(frames_f[1:]), flows=flows, positions=positions, skip=skip, blind=blind[0],
                sigma=10.0, center_weight=1.0 if K % 2 else 0.75, patch_radius=r)


_EXPECTED = {}


def expected(shape, frames='u8', out_uint8=False, with_skip=True, absolute=False):
    """``np_fuse_frames`` on ``fuse_case(shape)``, computed once per variant and shared (never written to)."""
    key = (tuple(shape), frames, out_uint8, with_skip, absolute)
    if key not in _EXPECTED:
        c = fuse_case(shape)
        f = '' if frames == 'u8' else '_f'
        dst, weight = np_fuse_frames(c['center' + f], c['neighbours' + f], c['positions'] if absolute else c['flows'],
                                     c['skip'] if with_skip else None, absolute, c['sigma'], c['center_weight'], c['patch_radius'],
                                     out_uint8)
        dst.setflags(write=False)
        weight.setflags(write=False)
        _EXPECTED[key] = (dst, weight)
    return _EXPECTED[key]


def test_the_test_inputs_cover_what_the_kernel_can_meet():
    seen = dict(land_x=0, land_y=0, leaving=0, nan=0, inf=0, short_window=0, blind=0, skipped=0, partial_tile=0)
    for shape in SHAPES:
        K, N, H, W, Cn, r = shape
        c = fuse_case(shape)
        info = {}
        dst, weight = np_fuse_frames(c['center'], c['neighbours'], c['flows'], c['skip'], False, c['sigma'], c['center_weight'], r, info=info)
        g = grid_of(H, W)
        sx, sy = g[..., 0] + c['flows'][..., 0], g[..., 1] + c['flows'][..., 1]
        with np.errstate(invalid='ignore'):
            fin = np.isfinite(sx) & np.isfinite(sy)
            if W > 1:
                seen['land_x'] += int(np.sum(fin & (sx == W - 1) & (g[..., 0] < W - 1) & info['vis']))
            if H > 1:
                seen['land_y'] += int(np.sum(fin & (sy == H - 1) & (g[..., 1] < H - 1) & info['vis']))
            seen['leaving'] += int(np.sum(fin & ((sx < 0) | (sx > W - 1) | (sy < 0) | (sy > H - 1))))
        seen['nan'] += int(np.sum(np.isnan(c['flows'])))
        seen['inf'] += int(np.sum(np.isinf(c['flows'])))
        seen['skipped'] += int(np.sum(c['skip'] != 0))
        # the positions form samples the very same points
        with np.errstate(invalid='ignore'):
            assert np.array_equal(c['positions'][..., 0], sx, equal_nan=True) and np.array_equal(c['positions'][..., 1], sy, equal_nan=True)
        none = ~info['vis'].any(axis=0)
        seen['blind'] += int(none.sum())
        assert np.array_equal(bits(weight[none]), bits(np.full(int(none.sum()), c['center_weight'], f32)))
        if H > 2 * r and W > 2 * r and r > 0:
            inner = np.zeros((H, W), bool)
            inner[r:H - r, r:W - r] = True
            seen['short_window'] += int(np.sum((info['cnt'] < (2 * r + 1) ** 2) & info['vis'] & inner))
            for edge in (info['cnt'][..., 0, :], info['cnt'][..., -1, :], info['cnt'][..., :, 0], info['cnt'][..., :, -1]):
                assert edge.max() <= (2 * r + 1) * (r + 1)                                   # windows cut by every border
        seen['partial_tile'] += int(W % 32 != 0 and W > 32) + int(H % 8 != 0 and H > 8)
        assert np.isfinite(dst).all() and np.isfinite(weight).all()
    assert all(v > 0 for v in seen.values()), seen
    assert {s[5] for s in SHAPES} == {0, 1, 2, 3} and {s[4] for s in SHAPES} == {1, 2, 3, 4}
    assert max(s[0] for s in SHAPES) == 16 and min(s[0] for s in SHAPES) == 1


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('r', [0, 1, 3])
def test_identical_frames_under_zero_flow_return_the_centre_exactly(K, r):
    rng = np.random.default_rng(K)
    centre = rng.uniform(0, 255, (2, 6, 9, 3)).astype(f32)
    dst, weight = np_fuse_frames(centre, np.stack([centre] * K), np.zeros((K, 2, 6, 9, 2), f32), None, False, 10.0, 1.0, r)
    assert_same(dst, centre)                       # (K + 1 a power of two: (c + c + c) / 3 is not exact in float32)
    assert_same(weight, np.full((2, 6, 9), K + 1, f32))
    u8 = rng.integers(0, 256, (1, 6, 9, 2)).astype(np.uint8)
    dst, _ = np_fuse_frames(u8, np.stack([u8] * K), np.zeros((K, 1, 6, 9, 2), f32), None, False, 10.0, 1.0, r, out_uint8=True)
    assert_same(dst, u8)


def test_a_pixel_without_a_visible_neighbour_keeps_the_centre():
    rng = np.random.default_rng(3)
    centre = rng.uniform(0, 255, (1, 7, 8, 3)).astype(f32)
    neighbours = rng.uniform(0, 255, (3, 1, 7, 8, 3)).astype(f32)
    flows = np.zeros((3, 1, 7, 8, 2), f32)
    skip = np.zeros((3, 1, 7, 8), np.uint8)
    flows[0, 0, 2, 3], flows[1, 0, 2, 3], skip[2, 0, 2, 3] = (np.nan, 0), (100, 0), 1         # NaN, out of frame, skipped
    flows[:, 0, 4, 4, 1] = -np.inf
    for cw in (1.0, 0.3, 7.0):
        for r in (0, 2):
            dst, weight = np_fuse_frames(centre, neighbours, flows, skip, False, 10.0, cw, r)
            for y, x in ((2, 3), (4, 4)):
                assert_same(dst[0, y, x], (f32(cw) * centre[0, y, x]) / f32(cw))
                assert bits(weight[0, y, x]) == bits(f32(cw))
            assert (weight[0, 0, 0] > f32(cw)) and np.isfinite(dst).all()


@pytest.mark.parametrize('r', [0, 1, 2])
def test_a_whole_pixel_flow_undoes_a_whole_pixel_shift(r):
    rng = np.random.default_rng(5)
    centre = rng.uniform(0, 255, (1, 20, 24, 3)).astype(f32)
    neighbour = (centre + rng.normal(0, 8, centre.shape)).astype(f32)[None]
    plain, w_plain = np_fuse_frames(centre, neighbour, np.zeros((1, 1, 20, 24, 2), f32), None, False, 10.0, 1.0, r)
    for dx, dy in ((3, 0), (-2, 1), (0, -4)):
        moved = np.roll(neighbour, (dy, dx), axis=(2, 3))                  # the scene of the neighbour, (dx, dy) further on
        flow = np.broadcast_to(np.array([dx, dy], f32), (1, 1, 20, 24, 2))
        got, w_got = np_fuse_frames(centre, moved, flow, None, False, 10.0, 1.0, r)
        b = max(abs(dx), abs(dy)) + r
        assert_same(got[:, b:-b, b:-b], plain[:, b:-b, b:-b])
        assert_same(w_got[:, b:-b, b:-b], w_plain[:, b:-b, b:-b])


def test_a_larger_sigma_increases_every_weight():
    c = fuse_case(SHAPES[4])
    flows = np.where(np.isfinite(c['flows']), c['flows'], 0).astype(f32) * f32(0.1)
    info = {}
    weights = [np_fuse_frames(c['center_f'], c['neighbours_f'], flows, None, False, s, 1.0, 1, info=info)[1] for s in (2.0, 10.0, 50.0)]
    seen = info['vis'].any(axis=0)                 # (a vector at the border may still leave the frame: the weight stays 1 there)
    assert seen.mean() > 0.9 and not seen.all()
    assert (weights[0][seen] < weights[1][seen]).all() and (weights[1][seen] < weights[2][seen]).all()
    assert (weights[2] <= f32(1 + 4)).all() and (weights[0][seen] > f32(1)).all()
    for w in weights:
        assert_same(w[~seen], np.ones(int((~seen).sum()), f32))


@pytest.mark.parametrize('shape', SHAPES[2:5], ids=IDS[2:5])
def test_positions_are_the_flow_form_at_grid_plus_flow(shape):
    c = fuse_case(shape)
    for with_skip in (True, False):
        for a, b in zip(expected(shape, 'f32', False, with_skip, False), expected(shape, 'f32', False, with_skip, True)):
            assert_same(a, b)


# ------------------------------------------------------------------ it denoises and does not ghost
def _scene(ox, oy, H=48, W=64):
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    x, y = xs + ox, ys + oy
    g = 128 + 60 * np.sin(x / 5.0) * np.cos(y / 7.0) + 40 * np.sin((x + y) / 3.0)
    return np.stack([g, 0.8 * g + 20, 255 - g], -1)


SHIFTS = [(-2.5, 1.25), (-1.0, 0.5), (1.5, -0.75), (3.25, 2.0)]


@pytest.mark.parametrize('r', [0, 1, 2])
def test_it_denoises_under_the_true_flows_and_does_not_ghost_under_wrong_ones(r):
    """Conditions, not measurements: (1) with the true flows the fused frame's MSE against the clean centre is below 0.5 of the
    noisy centre's (the ideal five-frame average would reach 0.2); (2) with zero flows, every neighbour misaligned, it is below
    the plain five-frame average's.  Both on the interior, 6 pixels from the border."""
    rng = np.random.default_rng(0)
    H, W = 48, 64
    clean = _scene(0, 0)
    centre = (clean + rng.normal(0, 10, clean.shape)).clip(0, 255).astype(f32)[None]
    # neighbour k shows the scene shifted by o: neighbour(x) = clean(x + o), so the centre's pixel x is found at x - o
    neighbours = np.stack([(_scene(ox, oy) + rng.normal(0, 10, clean.shape)).clip(0, 255).astype(f32)[None] for ox, oy in SHIFTS])
    true = np.stack([np.broadcast_to(np.array([-ox, -oy], f32), (1, H, W, 2)) for ox, oy in SHIFTS])
    i = slice(6, -6)
    mse = lambda x: float(((x[0].astype(np.float64) - clean)[i, i] ** 2).mean())       # noqa: E731
    fused, _ = np_fuse_frames(centre, neighbours, true, None, False, 10.0, 1.0, r)
    print(f'r={r}: noisy {mse(centre):.2f} fused {mse(fused):.2f} ratio {mse(fused) / mse(centre):.3f}')
    assert mse(fused) < 0.5 * mse(centre)
    ghost, _ = np_fuse_frames(centre, neighbours, np.zeros_like(true), None, False, 10.0, 1.0, r)
    average = (centre + neighbours.sum(axis=0)) / 5
    print(f'r={r}: misaligned fused {mse(ghost):.2f} plain average {mse(average):.2f}')
    assert mse(ghost) < mse(average)


# ------------------------------------------------------------------ the C entries
ENTRIES = ('raft_fuse_frames_f32', 'raft_fuse_frames_u8_f32', 'raft_fuse_frames_u8')


def test_the_header_declares_and_the_library_exports_the_entries():
    from tf_raft_amd import build
    assert 'frame_fuse.hip' in build.SOURCES and 'flow_sample.h' in build.HEADERS
    with open(os.path.join(ROOT, 'include', 'raft_hip.h')) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    sigs = _ffi.header_signatures(header)
    P, I, F = C.c_void_p, C.c_int, C.c_float
    lib = _ffi.load_library()
    for name in ENTRIES:
        assert sigs[name] == (I, [P, P, C.POINTER(C.c_int64), P, P, I, F, F, I, P, P, I, I, I, I, I, P]), name
        assert getattr(lib, name).argtypes == sigs[name][1] and len(sigs[name][1]) == 17
    assert _ffi.ABI_VERSION == 222 and lib.raft_version() == 222             # entries were added, no signature changed
    with open(os.path.join(ROOT, 'tf_raft_amd', 'csrc', 'frame_fuse.hip')) as f:
        src = f.read()
    assert '#pragma clang fp contract(off)' in src and '#include "flow_sample.h"' in src
    assert src.index('#pragma clang fp contract(off)') < src.index('#include "flow_sample.h"')
    assert 'atomic' not in src.split('namespace {', 1)[1] and 'hipMemset' not in src


@pytest.mark.parametrize('name', ENTRIES)
def test_argument_errors_are_returned_before_any_device_work(name):
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    fn = getattr(_ffi.load_library(), name)
    size = 4 if name == 'raft_fuse_frames_f32' else 1
    buf = (C.c_double * 4096)()
    base = C.cast(buf, C.c_void_p).value
    at = lambda n: C.c_void_p(base + n)                   # noqa: E731
    idx = (C.c_int64 * 16)(*range(16))
    K, N, H, W, Cn = 3, 1, 4, 5, 3
    frame = N * H * W * Cn * size
    #       center  neighbours index vectors    skip       abs sigma cw  r  dst         weight      K  N  H  W  C  stream
    good = [at(0), at(512), idx, at(4096), at(8192), 0, 10.0, 1.0, 1, at(12288), at(16384), K, N, H, W, Cn, None]
    for k in (0, 1, 3, 9):
        for opt in ((idx, at(8192), at(16384)), (None, None, None)):             # (index, skip and weight may be NULL)
            args = list(good)
            args[k], (args[2], args[4], args[10]) = None, opt
            assert fn(*args) == -1, k
    for k, values in ((11, (0, -1, 17)), (12, (0, -2)), (13, (0, -2)), (14, (0, -2)), (15, (0, 5, -1)), (8, (-1, 4)), (5, (2, -1))):
        for v in values:
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for k in (6, 7):
        for v in (0.0, -1.0, float('nan'), float('inf'), -float('inf')):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for v in (1e30, 1e-30):                                                          # sigma * sigma leaves float32
        args = list(good)
        args[6] = v
        assert fn(*args) == -2, v
    for bad in ((1, 1 << 14, 1 << 13), (1 << 10, 1 << 9, 1 << 8), (1 << 27, 1, 1), (1, 1 << 30, 4)):      # N * H * W above 2^26
        args = list(good)
        args[12:15] = bad
        assert fn(*args) == -2, bad
    for bad in ((0, -1, 2), (0, 1, 1 << 61)):
        args = list(good)
        args[2] = (C.c_int64 * 3)(*bad)
        assert fn(*args) == -2, bad
    args = list(good)
    args[3] = at(4100)                                                                # vectors are read as float2
    assert fn(*args) == -4
    if size == 4:
        for k in (0, 1, 9):
            args = list(good)
            args[k] = at(args[k].value - base + 2)
            assert fn(*args) == -4, k
    args = list(good)
    args[10] = at(16386)
    assert fn(*args) == -4
    # an output on an input (windows read the neighbours' pixels), or on the other output
    for k, where in ((9, 0), (9, (frame - 1) // 4 * 4), (9, 512 + 2 * frame), (9, 4096 + 8), (9, 8192 + 4), (10, 0),
                     (10, 512 + frame), (10, 4096), (10, 8192 + 56), (10, 12288)):
        args = list(good)
        args[k] = at(where)
        assert fn(*args) == -2, (k, where)
    args = list(good)
    args[2], args[1] = (C.c_int64 * 3)(0, 0, 2), at(12288 - 2 * frame - 4)            # a repeated index is fine; block 2 ends on dst
    assert fn(*args) == -2
    args = list(good)                                                                  # precedence: NULL, shape, alignment, overlap
    args[9], args[11], args[3], args[10] = None, 0, at(4100), at(0)
    assert fn(*args) == -1
    args[9] = at(12288)
    assert fn(*args) == -2
    args[11] = K
    assert fn(*args) == -4
    args[3] = at(4096)
    assert fn(*args) == -2


# ------------------------------------------------------------------ the Python layer, nothing reaches the device
BAD_POSITIVE = (0, -1, float('nan'), float('inf'), 1e39, True, None, 'x')


def test_shapes_types_and_arguments_are_checked_without_a_gpu():
    import torch
    from tf_raft_amd import image_ops
    assert (image_ops.FUSE_SIGMA, image_ops.FUSE_PATCH_RADIUS, image_ops.FUSE_CENTER_WEIGHT) == (10.0, 1, 1.0)
    c = np.zeros((2, 4, 5, 3), np.uint8)
    nb = np.zeros((3, 2, 4, 5, 3), np.uint8)
    fl = np.zeros((3, 2, 4, 5, 2), np.float32)
    for bad in BAD_POSITIVE:
        with pytest.raises(ValueError, match='sigma must'):
            image_ops.fuse_frames(c, nb, fl, sigma=bad)
        with pytest.raises(ValueError, match='center_weight must'):
            image_ops.fuse_frames(c, nb, positions=fl, center_weight=bad)
    for bad in (1e30, 1e-30):
        with pytest.raises(ValueError, match='sigma \\* sigma'):
            image_ops.fuse_frames(c, nb, fl, sigma=bad)
    for bad in (-1, 4, 1.0, True, None):
        with pytest.raises(ValueError, match='patch_radius must'):
            image_ops.fuse_frames(c, nb, fl, patch_radius=bad)
    with pytest.raises(ValueError, match='exactly one of flows and positions'):
        image_ops.fuse_frames(c, nb)
    with pytest.raises(ValueError, match='exactly one of flows and positions'):
        image_ops.fuse_frames(c, nb, fl, fl)
    with pytest.raises(ValueError, match='1 to 16 neighbours'):
        image_ops.fuse_frames(c, np.zeros((17, 2, 4, 5, 3), np.uint8), np.zeros((17, 2, 4, 5, 2), np.float32))
    with pytest.raises(ValueError, match='1 to 16 neighbours'):
        image_ops.fuse_frames(c, nb[:0], fl[:0])
    with pytest.raises(ValueError, match='1 to 4 channels'):
        image_ops.fuse_frames(np.zeros((4, 5, 5), np.uint8), np.zeros((3, 4, 5, 5), np.uint8), np.zeros((3, 4, 5, 2), np.float32))
    with pytest.raises(ValueError, match='expects neighbours'):
        image_ops.fuse_frames(c, nb[0], fl)
    with pytest.raises(ValueError, match='expects neighbours'):
        image_ops.fuse_frames(c, nb[:, :1], fl)
    with pytest.raises(ValueError, match='expects neighbours'):
        image_ops.fuse_frames(c, nb.astype(np.float32), fl)
    with pytest.raises(ValueError, match=r'\(H, W, C\) or \(N, H, W, C\)'):
        image_ops.fuse_frames(c[None], nb[:, None], fl[:, None])
    with pytest.raises(TypeError, match='unsupported type'):
        image_ops.fuse_frames(c.astype(np.int32), nb.astype(np.int32), fl)
    with pytest.raises(TypeError, match='uint8 or float32 frames'):
        image_ops.fuse_frames(torch.zeros((2, 4, 5, 3), dtype=torch.int32), torch.zeros((3, 2, 4, 5, 3), dtype=torch.int32), fl)
    with pytest.raises(ValueError, match='expects a flow'):
        image_ops.fuse_frames(c, nb, fl[:2])
    with pytest.raises(ValueError, match='expects a flow'):
        image_ops.fuse_frames(c, nb, positions=fl[..., :1])
    with pytest.raises(TypeError, match='a flow is float32'):
        image_ops.fuse_frames(c, nb, fl.astype(np.uint8))
    with pytest.raises(ValueError, match='expects a mask'):
        image_ops.fuse_frames(c, nb, fl, skip=np.zeros((2, 4, 5), np.uint8))
    with pytest.raises(TypeError, match='a mask is uint8 or bool'):
        image_ops.fuse_frames(c, nb, fl, skip=np.zeros((3, 2, 4, 5), np.float32))
    with pytest.raises(TypeError, match='returns float32, or uint8 for uint8 frames'):
        image_ops.fuse_frames(c.astype(np.float32), nb.astype(np.float32), fl, dtype=torch.uint8)
    with pytest.raises(TypeError, match='returns float32, or uint8 for uint8 frames'):
        image_ops.fuse_frames(c, nb, fl, dtype=torch.float16)
    with pytest.raises(ValueError, match='too large'):
        image_ops.fuse_frames(torch.empty((1 << 10, 1 << 9, 1 << 8, 3), dtype=torch.uint8, device='meta'),
                              torch.empty((1, 1 << 10, 1 << 9, 1 << 8, 3), dtype=torch.uint8, device='meta'),
                              torch.empty((1, 1 << 10, 1 << 9, 1 << 8, 2), dtype=torch.float32, device='meta'))
    # a list of frames is a stack
    with pytest.raises(ValueError, match='expects a flow'):
        image_ops.fuse_frames(c, [c, c], fl)
    # the launch form checks what it is handed, too
    dc, ds, dv = torch.zeros((2, 4, 5, 3), dtype=torch.uint8), torch.zeros((5, 2, 4, 5, 3), dtype=torch.uint8), torch.zeros((3, 2, 4, 5, 2))
    with pytest.raises(ValueError, match='sigma must'):
        image_ops.fuse_frames_launch(dc, ds, dv, [0, 1, 3], sigma=-1)
    with pytest.raises(ValueError, match='contiguous centre'):
        image_ops.fuse_frames_launch(dc[0], ds, dv, [0, 1, 3])
    with pytest.raises(ValueError, match='needs a contiguous stack'):
        image_ops.fuse_frames_launch(dc, ds[0], dv, [0, 1, 3])
    with pytest.raises(ValueError, match='needs a contiguous stack'):
        image_ops.fuse_frames_launch(dc, ds.float(), dv, [0, 1, 3])
    for bad in ([0, 5, 1], [0, -1, 1], [0, 1.0, 2], [True, 1, 2], 3, 'ab'):
        with pytest.raises(ValueError, match='index'):
            image_ops.fuse_frames_launch(dc, ds, dv, bad)
    with pytest.raises(ValueError, match='need vectors'):
        image_ops.fuse_frames_launch(dc, ds, dv)                                  # index None: all 5 blocks
    with pytest.raises(ValueError, match='need vectors'):
        image_ops.fuse_frames_launch(dc, ds, dv, [0, 1])
    with pytest.raises(ValueError, match='1 to 16 neighbours'):
        image_ops.fuse_frames_launch(dc, ds, dv, [])
    with pytest.raises(ValueError, match='out must be a contiguous'):
        image_ops.fuse_frames_launch(dc, ds, dv, [0, 4, 4], skip=torch.zeros((3, 2, 4, 5)))
    with pytest.raises(ValueError, match='out must be a contiguous'):
        image_ops.fuse_frames_launch(dc, ds, dv, [0, 4, 4], out=torch.zeros((2, 4, 5, 3)))
    with pytest.raises(ValueError, match='out must be a contiguous'):
        image_ops.fuse_frames_launch(dc, ds, dv, [0, 4, 4], weight=torch.zeros((2, 4, 5, 1)))


def test_the_model_checks_its_arguments_before_any_device_work():
    import inspect
    from tf_raft_amd import video
    from tf_raft_amd.model import RAFT, SmallRAFT
    c = np.zeros((1, 64, 96, 3), np.uint8)
    nb = np.zeros((2, 1, 64, 96, 3), np.uint8)
    clip = np.zeros((3, 64, 96, 3), np.uint8)
    for cls in (RAFT, SmallRAFT):
        sig = inspect.signature(cls.fuse_step).parameters
        assert (sig['sigma'].default, sig['patch_radius'].default, sig['center_weight'].default) == (10.0, 1, 1.0)
        assert sig['occlusion_test'].default == 'consistency'
        sig = inspect.signature(cls.denoise_video).parameters
        assert (sig['radius'].default, sig['sigma'].default, sig['patch_radius'].default, sig['center_weight'].default,
                sig['batch_size'].default) == (2, 10.0, 1, 1.0, 4)
        model = cls.__new__(cls)                                             # (no device: anything enqueued would fail)
        for bad in BAD_POSITIVE:
            with pytest.raises(ValueError, match='sigma must'):
                model.fuse_step((c, nb), sigma=bad)
            with pytest.raises(ValueError, match='center_weight must'):
                model.denoise_video(clip, center_weight=bad)
        with pytest.raises(ValueError, match='patch_radius must'):
            model.fuse_step((c, nb), patch_radius=4)
        with pytest.raises(ValueError, match='patch_radius must'):
            model.denoise_video(clip, patch_radius=-1)
        with pytest.raises(ValueError, match='occlusion_test'):
            model.fuse_step((c, nb), occlusion_test='nope')
        with pytest.raises(TypeError, match='unexpected keyword'):
            model.fuse_step((c, nb), gamma=1)
        with pytest.raises(ValueError, match=r'neighbours \(K, N, H, W, 3\)'):
            model.fuse_step((c, nb[0]))
        with pytest.raises(ValueError, match=r'neighbours \(K, N, H, W, 3\)'):
            model.fuse_step((c[0], nb[:, 0]))
        with pytest.raises(ValueError, match=r'neighbours \(K, N, H, W, 3\)'):
            model.fuse_step((c, nb.astype(np.float32)))
        with pytest.raises(ValueError, match=r'neighbours \(K, N, H, W, 3\)'):
            model.fuse_step((c[..., :2], nb[..., :2]))
        with pytest.raises(ValueError, match='1 to 16 neighbours'):
            model.fuse_step((c, np.zeros((17, 1, 64, 96, 3), np.uint8)))
        # the denoise_video validator
        for bad in (clip[0], clip[..., :2], clip[None]):
            with pytest.raises(ValueError, match=r'one video \(T, H, W, 3\)'):
                model.denoise_video(bad)
        with pytest.raises(TypeError, match='unsupported type'):
            model.denoise_video(clip.astype(np.int16))
        with pytest.raises(TypeError, match='uint8 or float32 frames'):
            model.denoise_video(clip.astype(bool))
        with pytest.raises(ValueError, match='empty'):
            model.denoise_video(clip[:0])
        for bad in (0, -1, 9, 2.0, True, None):
            with pytest.raises(ValueError, match='radius must'):
                model.denoise_video(clip, radius=bad)
        for bad in (0, -1, 2.0, True, None):
            with pytest.raises(ValueError, match='batch_size must'):
                model.denoise_video(clip, batch_size=bad)
        # one frame has no neighbour: it is returned, without a device
        for one in (clip[:1] + 7, (clip[:1] + 0.5).astype(np.float32)):
            got = model.denoise_video(one)
            assert got.dtype == one.dtype and got is not one and np.array_equal(got, one)
    assert video.denoise_neighbours(0, 5, 2) == [1, 2] and video.denoise_neighbours(2, 5, 2) == [1, 0, 3, 4]
    assert video.denoise_neighbours(4, 5, 2) == [3, 2] and video.denoise_neighbours(1, 2, 8) == [0]
    for T in (2, 3, 9):
        for radius in (1, 2, 8):
            for t in range(T):
                nbs = video.denoise_neighbours(t, T, radius)
                assert sorted(nbs) == [s for s in range(T) if s != t and abs(s - t) <= radius] and 1 <= len(nbs) <= 16

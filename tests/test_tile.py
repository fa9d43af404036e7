"""Tiled inference, host side (no GPU): the tiling rule of ``tf_raft_amd.image_ops`` (``tile_origins`` / ``tile_taps``) against its
stated properties and against an independent float64 restatement of the blend that never uses separability -- it accumulates the
2-D tent weight of every tile over the frame and divides -- plus the argument checks of the model option, of the public
functions and of the three C entries.  tests/test_gpu_tile.py compares the kernels with ``np_tile_gather`` / ``np_tile_blend``.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tf_raft_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement
def np_origins(L, T, o):
    """The rule as DESIGN.md section 14 states it, with exact rationals: n tiles spread evenly over [0, L - T], rounded half up."""
    from fractions import Fraction
    if L <= T:
        return [-((T - L) // 2)]
    n = 1
    while (n - 1) * (T - o) < L - T:          # the fewest tiles whose strides of at most T - o reach L - T
        n += 1
    return [int(np.floor(Fraction(i * (L - T), n - 1) + Fraction(1, 2))) for i in range(n)]


def np_tile_gather(x, Ht, Wt, oy, ox):
    """(N, H, W, C) -> (N * ny * nx, Ht, Wt, C) float32 by slicing, zero outside the frame."""
    x = np.asarray(x)
    N, H, W, Cn = x.shape
    out = np.zeros((N, len(oy), len(ox), Ht, Wt, Cn), np.float32)
    for ky, y0 in enumerate(oy):
        for kx, x0 in enumerate(ox):
            ya, yb, xa, xb = max(y0, 0), min(y0 + Ht, H), max(x0, 0), min(x0 + Wt, W)
            out[:, ky, kx, ya - y0:yb - y0, xa - x0:xb - x0] = x[:, ya:yb, xa:xb]
    return out.reshape(N * len(oy) * len(ox), Ht, Wt, Cn)


def np_tent2d(Ht, Wt):
    ty, tx = np.arange(Ht, dtype=np.float64), np.arange(Wt, dtype=np.float64)
    return np.minimum(ty + 1, Ht - ty)[:, None] * np.minimum(tx + 1, Wt - tx)[None, :]


def np_weights2d(H, W, Ht, Wt, oy, ox):
    """(ny, nx, H, W) float64: the normalised 2-D tent weight of every tile at every frame pixel (0 where it does not reach)."""
    w = np.zeros((len(oy), len(ox), H, W))
    tent = np_tent2d(Ht, Wt)
    for ky, y0 in enumerate(oy):
        for kx, x0 in enumerate(ox):
            ya, yb, xa, xb = max(y0, 0), min(y0 + Ht, H), max(x0, 0), min(x0 + Wt, W)
            w[ky, kx, ya:yb, xa:xb] = tent[ya - y0:yb - y0, xa - x0:xb - x0]
    total = w.sum(axis=(0, 1))
    assert (total > 0).all(), 'a frame pixel no tile covers'
    return w / total


def np_tile_blend(tiles, H, W, oy, ox):
    """(..., N * ny * nx, Ht, Wt, 2) -> (..., N, H, W, 2) in float64: sum over every tile of weight * value, never separated."""
    tiles = np.asarray(tiles, np.float64)
    Ht, Wt = tiles.shape[-3:-1]
    ny, nx = len(oy), len(ox)
    lead = tiles.shape[:-4]
    t = tiles.reshape(lead + (-1, ny, nx, Ht, Wt, 2))
    w = np_weights2d(H, W, Ht, Wt, oy, ox)
    out = np.zeros(lead + (t.shape[len(lead)], H, W, 2))
    for ky, y0 in enumerate(oy):
        for kx, x0 in enumerate(ox):
            ya, yb, xa, xb = max(y0, 0), min(y0 + Ht, H), max(x0, 0), min(x0 + Wt, W)
            out[..., ya:yb, xa:xb, :] += w[ky, kx, ya:yb, xa:xb, None] * t[..., ky, kx, ya - y0:yb - y0, xa - x0:xb - x0, :]
    return out


def np_max_cover(L, T, org):
    p = np.arange(L)[:, None] - np.asarray(org)[None, :]
    return int(((p >= 0) & (p < T)).sum(axis=1).max())


# ------------------------------------------------------------------ the rule
def test_tile_origins_have_the_stated_properties():
    """Every T in {64, 96}, every overlap a multiple of 4 up to T // 2, every L in T + 1 .. 5 T: first origin 0, last L - T,
    consecutive origins 1 .. T - o apart, the fewest tiles that allow it, the stated formula, and at most 3 tiles per coordinate."""
    from tf_raft_amd.image_ops import tile_origins
    for T in (64, 96):
        for o in range(0, T // 2 + 1, 4):
            for L in range(T + 1, 5 * T + 1):
                org = tile_origins(L, T, o)
                assert all(isinstance(v, int) for v in org)
                n = len(org)
                assert n == -(-(L - T) // (T - o)) + 1 >= 2
                assert org[0] == 0 and org[-1] == L - T, (L, T, o, org)
                d = np.diff(org)
                assert d.min() >= 1 and d.max() <= T - o, (L, T, o, org)
                assert org == [(2 * i * (L - T) + (n - 1)) // (2 * (n - 1)) for i in range(n)] == np_origins(L, T, o)
                assert np_max_cover(L, T, org) <= 3, (L, T, o, org)


def test_a_frame_no_longer_than_the_tile_takes_the_crop_or_pad_offset_and_weight_one():
    from tf_raft_amd.image_ops import crop_or_pad_offsets, tile_origins, tile_taps
    for T in (64, 96):
        for L in list(range(1, 12)) + list(range(T - 9, T + 1)):
            for o in (0, 16, T // 2):
                org = tile_origins(L, T, o)
                crop, pad, ext = crop_or_pad_offsets(L, T)
                assert org == [-pad] and crop == 0 and ext == L
                first, count, w = tile_taps(L, T, org)
                assert first.dtype == count.dtype == np.int32 and w.dtype == np.float64 and w.shape == (L, 1)
                assert not first.any() and (count == 1).all() and (w == 1.0).all()
                assert (w.astype(np.float32) == np.float32(1.0)).all()


SIZES = [((100, 150), (64, 96), (16, 16)), ((60, 200), (64, 96), (32, 32)), ((170, 96), (64, 96), (8, 8)), ((65, 97), (64, 96), (0, 32)),
         ((40, 70), (64, 96), (16, 0)), ((64, 96), (64, 96), (32, 48)), ((1080, 1920), (448, 1024), (64, 64)), ((301, 333), (64, 96), (32, 48))]


@pytest.mark.parametrize('frame,tile,overlap', SIZES, ids=[f'{f[0]}x{f[1]}_o{o[0]}_{o[1]}' for f, _, o in SIZES])
def test_tile_taps_equal_the_two_dimensional_restatement(frame, tile, overlap):
    from tf_raft_amd.image_ops import tile_origins, tile_taps
    (H, W), (Ht, Wt) = frame, tile
    oy, ox = tile_origins(H, Ht, overlap[0]), tile_origins(W, Wt, overlap[1])
    (fy, cy, wy), (fx, cx, wx) = tile_taps(H, Ht, oy), tile_taps(W, Wt, ox)
    assert fy.shape == cy.shape == (H,) and fx.shape == cx.shape == (W,) and wy.dtype == wx.dtype == np.float64
    assert wy.shape == (H, cy.max()) and wx.shape == (W, cx.max()) and max(cy.max(), cx.max()) <= 3
    assert cy.min() >= 1 and cx.min() >= 1                                 # every frame pixel is covered
    assert (wy >= 0).all() and (wx >= 0).all()
    assert np.abs(wy.sum(axis=1) - 1.0).max() <= 1e-15 and np.abs(wx.sum(axis=1) - 1.0).max() <= 1e-15
    # the tables as dense (tiles, coordinates) matrices: zero outside [first, first + count)
    a, b = np.zeros((len(oy), H)), np.zeros((len(ox), W))
    for dense, first, count, w in ((a, fy, cy, wy), (b, fx, cx, wx)):
        for p in range(dense.shape[1]):
            assert first[p] >= 0 and first[p] + count[p] <= dense.shape[0] and not w[p, count[p]:].any()
            dense[first[p]:first[p] + count[p], p] = w[p, :count[p]]
    want = np_weights2d(H, W, Ht, Wt, oy, ox)                               # accumulated over every tile, then divided
    got = a[:, None, :, None] * b[None, :, None, :]
    assert np.abs(got - want).max() <= 1e-15
    assert np.abs(got.sum(axis=(0, 1)) - 1.0).max() <= 1e-15
    assert ((got > 0) == (want > 0)).all()                                  # exactly the tiles that reach a pixel weigh in


def test_restated_blend_undoes_the_restated_gather():
    """The yardsticks themselves: tiles cut from a field blend back to the field (a convex combination of equal values)."""
    from tf_raft_amd.image_ops import tile_origins
    rng = np.random.default_rng(0)
    f = rng.normal(size=(2, 60, 200, 2))
    oy, ox = tile_origins(60, 64, 32), tile_origins(200, 96, 32)
    assert (len(oy), len(ox)) == (1, 3) and oy == [-2] and ox == [0, 52, 104]
    tiles = np_tile_gather(f, 64, 96, oy, ox)
    assert tiles.shape == (6, 64, 96, 2) and tiles.dtype == np.float32
    np.testing.assert_array_equal(tiles[4, 2:62, :, :], f[1, :, 52:148].astype(np.float32))
    assert not tiles[:, :2].any() and not tiles[:, 62:].any()
    assert np.abs(np_tile_blend(tiles, 60, 200, oy, ox) - f.astype(np.float32)).max() <= 1e-14


def test_three_tiles_over_one_coordinate_where_the_strides_are_short():
    """Of the GPU tests' shapes it is 170 rows under 64-row tiles at overlap 32 that has coordinates under three tiles (five tiles
    26 or 27 rows apart); 200 columns under 96-column tiles at overlap 32 take three tiles 52 apart, never more than two deep."""
    from tf_raft_amd.image_ops import tile_origins, tile_taps
    org = tile_origins(170, 64, 32)
    assert org == [0, 27, 53, 80, 106] and np_max_cover(170, 64, org) == 3 == tile_taps(170, 64, org)[2].shape[1]
    assert np_max_cover(200, 96, tile_origins(200, 96, 32)) == 2


def test_tile_functions_reject_bad_arguments():
    from tf_raft_amd import image_ops
    for bad in ((0, 64, 0), (100, 0, 0), (100, 64, 33), (100, 64, -1), (100, 64, 1.5), (100, 64, None), (100, 64, True)):
        with pytest.raises(ValueError):
            image_ops.tile_origins(*bad)
    assert image_ops.tile_origins(100, 64, 32) == [0, 18, 36]
    assert image_ops.tile_origins(128, 64, 0) == [0, 64]
    with pytest.raises(ValueError):
        image_ops.tile_taps(100, 64, [])
    with pytest.raises(ValueError):
        image_ops.tile_taps(100, 64, [0, 0, 36])                           # origins must increase
    with pytest.raises(ValueError, match='cover'):
        image_ops.tile_taps(200, 64, [0, 136])                             # a gap
    with pytest.raises(ValueError):
        image_ops.tile_taps(0, 64, [0])
    # what the kernels cannot take is refused before anything touches a device (there is none here)
    with pytest.raises(ValueError, match='per axis'):
        image_ops.TilePlan(torch.device('cuda', 0), 64, 64 * 40, 64, 64, 0)                    # 40 tiles on one axis
    for bad in (33, (16, 49), (1, 2, 3), -1, 'x', None, 2.0):
        with pytest.raises(ValueError, match='overlap'):
            image_ops.TilePlan(torch.device('cuda', 0), 100, 150, 64, 96, bad)
        with pytest.raises(ValueError, match='overlap'):
            image_ops.tile_gather(np.zeros((100, 150, 3), np.float32), 64, 96, overlap=bad)
        with pytest.raises(ValueError, match='overlap'):
            image_ops.tile_blend(np.zeros((4, 64, 96, 2), np.float32), 100, 150, overlap=bad)
    with pytest.raises(ValueError):
        image_ops.tile_gather(np.zeros((100, 150, 3), np.float32), 0, 96, overlap=0)
    with pytest.raises(ValueError):
        image_ops.tile_blend(np.zeros((4, 64, 96, 2), np.float32), 100, 0, overlap=0)


def test_the_tile_option_is_validated_at_construction():
    """The checks run before anything needs a device; a valid combination then fails like every model does without a GPU."""
    from tf_raft_amd.model import RAFT, SmallRAFT
    for cls in (RAFT, SmallRAFT):
        for size in (None, 'auto'):
            with pytest.raises(ValueError, match='target_size'):
                cls(fit='tile', target_size=size)
        with pytest.raises(ValueError, match='target_size'):
            cls(fit='tile', target_size=(60, 96))
        for fit, size in (('crop_or_pad', (64, 96)), ('resize', (64, 96)), ('crop_or_pad', None), ('resize', 'auto')):
            with pytest.raises(ValueError, match='tile_overlap'):
                cls(fit=fit, target_size=size, tile_overlap=16)
        for bad in (33, -1, (16, 49), (40, 16), (1, 2, 3), 'wide', 1.5, True):
            with pytest.raises(ValueError, match='overlap'):
                cls(fit='tile', target_size=(64, 96), tile_overlap=bad)
        with pytest.raises(ValueError, match='overlap'):
            cls(fit='tile', target_size=(64, 96))                           # the default of 64 is more than half such a tile
        assert cls._check_tile_overlap('tile', None, (448, 1024)) == (64, 64)
        assert cls._check_tile_overlap('tile', 32, (64, 96)) == (32, 32)
        assert cls._check_tile_overlap('tile', (0, 48), (64, 96)) == (0, 48)
        assert cls._check_tile_overlap('crop_or_pad', None, (64, 96)) is None
        assert cls._check_fit('tile', True, (64, 96)) == ('tile', True)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            RAFT(fit='tile', target_size=(448, 1024))


# ------------------------------------------------------------------ the C entries
def test_tile_entries_are_declared_exported_and_mirrored():
    """The constants and the by-value struct (the prototypes: tests/test_host_logic.py test_the_binding_is_the_header)."""
    with open(os.path.join(ROOT, 'include', 'raft_hip.h')) as f:
        header = f.read()
    assert int(re.search(r'#define RAFT_TILE_MAX_PER_AXIS (\d+)', header).group(1)) == _ffi.TILE_MAX_PER_AXIS == 32
    assert int(re.search(r'#define RAFT_TILE_MAX_TAPS (\d+)', header).group(1)) == _ffi.TILE_MAX_TAPS == 4
    assert C.sizeof(_ffi.TileOrigins) == 4 * (2 + 2 * 32)


def _origins(oy, ox, ny=None, nx=None):
    o = _ffi.TileOrigins(len(oy) if ny is None else ny, len(ox) if nx is None else nx)
    o.oy[:len(oy)] = oy
    o.ox[:len(ox)] = ox
    return o


def test_tile_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    org = _origins([0, 36], [0, 54])
    for name in ('raft_tile_gather_f32', 'raft_tile_gather_u8_f32'):
        fn = getattr(lib, name)
        good = [p, p, 1, 100, 150, 64, 96, 3, org, None]
        for k in (0, 1):
            args = list(good)
            args[k] = None
            assert fn(*args) == -1, (name, k)
        for k in range(2, 8):
            for v in (0, -3):
                args = list(good)
                args[k] = v
                assert fn(*args) == -2, (name, k, v)
        for bad in ((1, 4, 1 << 30, 64, 96, 3), (1, 100, 150, 64, 1 << 30, 3)):       # W * C does not fit an int
            args = list(good)
            args[2:8] = bad
            assert fn(*args) == -2, (name, bad)
        for bad in (_origins([0], [0], ny=0), _origins([0], [0], nx=0), _origins([0], [0], ny=33), _origins([0], [0], nx=-1),
                    _origins([0, 100], [0, 54]), _origins([-64, 36], [0, 54]), _origins([0, 36], [0, 150]), _origins([0, 36], [-96, 54])):
            args = list(good)
            args[8] = bad                                                   # too many tiles, or a tile wholly outside the frame
            assert fn(*args) == -2, (name, bad.ny, bad.nx)
    fn = lib.raft_tile_blend_f32
    good = [p, p, 1, 1, 100, 150, 64, 96, org, p, p, p, 2, p, p, p, 2, None]
    for k in (0, 1, 9, 10, 11, 13, 14, 15):
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    for k in range(2, 8):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for k, taps in ((12, 0), (12, 5), (12, -1), (16, 0), (16, 5), (16, 1 << 20)):
        args = list(good)
        args[k] = taps
        assert fn(*args) == -2, (k, taps)
    for bad in (_origins([0], [0], ny=0), _origins([0], [0], nx=33)):
        args = list(good)
        args[8] = bad
        assert fn(*args) == -2
    args = list(good)
    args[6:8] = (1 << 16, 1 << 16)                                          # Ht * Wt beyond an int
    assert fn(*args) == -2
    args = list(good)
    args[2:4] = (1 << 40, 1 << 20)                                          # more rows than one grid
    assert fn(*args) == -2
    for k in (0, 1):
        args = list(good)
        args[k] = C.c_void_p(p.value + 4)                                   # a flow is read and written as float2
        assert fn(*args) == -4, k

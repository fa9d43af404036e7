"""The range map and its occlusion test, host side (no GPU): the NumPy restatement of DESIGN.md section 21 with its known
answers, the C entries' declarations and argument checks, and the ``ValueError``s of the Python layer.
tests/test_gpu_range_occlusion.py compares the kernels with the restatement BIT FOR BIT: everything behind the float32 sample
position and the float32 fraction is integer arithmetic, so there is no tolerance anywhere.

The definition: the source pixel at integer ``(x, y)`` with vector ``(u, v)`` has ``sx = float32(x) + u``, ``sy = float32(y) + v``;
it contributes iff ``-1 < sx < float32(W)`` and ``-1 < sy < float32(H)``; ``x0 = floor(sx)``, ``a = sx - x0`` in float32,
``qa = rint(a * 4096)``, likewise ``y0``, ``b``, ``qb``; the corner ``(x0 + dx, y0 + dy)`` receives the integer weight
``(dx ? qa : 4096 - qa) * (dy ? qb : 4096 - qb)`` if it lies in the frame and the weight is not 0; ``acc`` is the uint64 sum.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tf_raft_amd import _ffi
from test_consistency import analytic_case, np_flow_consistency, np_sample_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 24           # the four weights of one vector


# ------------------------------------------------------------------ the restatement
def np_range_weights(a, b):
    """float32 fractions -> the four integer weights, order (dy, dx) = (0, 0), (0, 1), (1, 0), (1, 1)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype == np.float32
    qa = np.rint(a * np.float32(4096)).astype(np.int64)
    qb = np.rint(b * np.float32(4096)).astype(np.int64)
    return [(qa if dx else 4096 - qa) * (qb if dy else 4096 - qb) for dy in (0, 1) for dx in (0, 1)]


def np_range_acc(flow):
    """(N, H, W, 2) float32 -> the uint64 accumulator (N, H, W)."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 4 and flow.shape[-1] == 2
    N, H, W, _ = flow.shape
    acc = np.zeros((N, H, W), np.uint64)
    with np.errstate(invalid='ignore', over='ignore'):
        sx = np.arange(W, dtype=np.float32)[None, None, :] + flow[..., 0]
        sy = np.arange(H, dtype=np.float32)[None, :, None] + flow[..., 1]
        assert sx.dtype == sy.dtype == np.float32
        ok = (sx > np.float32(-1)) & (sx < np.float32(W)) & (sy > np.float32(-1)) & (sy < np.float32(H))
    n = np.nonzero(ok)[0]
    sx, sy = sx[ok], sy[ok]
    fx, fy = np.floor(sx), np.floor(sy)
    assert fx.dtype == np.float32
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    w = np_range_weights(sx - fx, sy - fy)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        cx, cy = x0 + dx, y0 + dy
        keep = (w[k] > 0) & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        np.add.at(acc, (n[keep], cy[keep], cx[keep]), w[k][keep].astype(np.uint64))
    return acc


def np_range_map(flow):
    return (np_range_acc(flow).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def range_threshold_sum(threshold):
    """T = (uint64)ceil(double(float32 t) * 2^24)."""
    return int(math.ceil(float(np.float32(threshold)) * 2.0 ** 24))


def np_range_occlusion(flow_a, flow_b, threshold=0.5, acc_b=None):
    """Direction a: occluded = acc(flow_b) < T or flow_a's pixel out of frame (bool (N, H, W)).  ``acc_b``: ``np_range_acc(flow_b)``
    where the caller has it already."""
    inside = np_sample_positions(flow_a)[2]
    acc_b = np_range_acc(flow_b) if acc_b is None else acc_b
    return (acc_b < np.uint64(range_threshold_sum(threshold))) | ~inside


def np_range_visibility(flows, N, mask=None, threshold=0.5, apply=True, acc=None):
    """(2N, H, W, 2) -> (visible uint8, float32 share, occluded bool), as raft_flow_range_visibility_f32 defines them.  ``acc``:
    ``np_range_acc(flows)`` where the caller has it already."""
    flows = np.asarray(flows)
    acc = np_range_acc(flows) if acc is None else acc
    occ = np.concatenate([np_range_occlusion(flows[:N], flows[N:], threshold, acc[N:]),
                          np_range_occlusion(flows[N:], flows[:N], threshold, acc[:N])])
    use = np.ones(occ.shape, bool) if mask is None else np.asarray(mask) != 0
    visible = (use & ~(occ & bool(apply))).astype(np.uint8)
    return visible, np.float32(np.float64(int(occ.sum())) / np.float64(occ.size)), occ


# ------------------------------------------------------------------ the flows both test files use
def all_to_one(H, W, ty, tx):
    """Every vector of the frame ends exactly on (tx, ty)."""
    f = np.zeros((H, W, 2), np.float32)
    f[..., 0] = tx - np.arange(W, dtype=np.float32)[None, :]
    f[..., 1] = ty - np.arange(H, dtype=np.float32)[:, None]
    return f


def range_flows(N, H, W, seed):
    """(2N, H, W, 2): the N forward flows in front of the N backward ones.  Sub-pixel vectors everywhere, a block of whole-pixel
    shifts, vectors that end within [-1, 0) and (W - 1, W) (they still give a share to the border), vectors far out of frame, 1e30,
    an infinity and a NaN, and -- in the last backward image -- every vector on one pixel."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(-1.5, 1.5, size=(2 * N, H, W, 2)).astype(np.float32)
    f[:, H // 2:, W // 2:] = np.rint(f[:, H // 2:, W // 2:])                  # whole pixels
    f[:, :, 0, 0] = rng.uniform(-0.99, -0.01, size=(2 * N, H)).astype(np.float32)     # ends in [-1, 0)
    f[:, :, W - 1, 0] = rng.uniform(0.01, 0.99, size=(2 * N, H)).astype(np.float32)   # ends in (W - 1, W)
    f[:, 0, :, 1] = rng.uniform(-0.99, -0.01, size=(2 * N, W)).astype(np.float32)
    if H >= 5 and W >= 7:
        f[:, 1, 1] = (-(W + 40.0), 3.0)
        f[:, 1, 2] = (2.5, H + 1000.0)
        f[:, 2, 1] = (1e30, 0.0)
        f[:, 2, 2] = (0.0, -np.inf)
        f[:, 3, 3] = (np.nan, 0.25)
        f[:, 3, 4] = (-5.0, 0.0)                                              # ends exactly on -1: contributes nothing
        f[-1] = all_to_one(H, W, H // 2, W // 3)
    elif H * W > 1:
        f[0, -1, -1] = (np.nan, 0.0)
        f[-1, 0, 0] = (1e30, np.inf)
    return np.ascontiguousarray(f)


# ------------------------------------------------------------------ known answers
H0, W0 = 37, 53


def test_zero_flow_is_one_everywhere():
    acc = np_range_acc(np.zeros((2, H0, W0, 2), np.float32))
    assert acc.dtype == np.uint64 and (acc == ONE).all()
    np.testing.assert_array_equal(np_range_map(np.zeros((1, H0, W0, 2), np.float32)), np.ones((1, H0, W0), np.float32))


def test_an_integer_shift_moves_the_window():
    f = np.zeros((1, H0, W0, 2), np.float32)
    f[...] = (3, -2)
    acc = np_range_acc(f)[0]
    want = np.zeros((H0, W0), np.uint64)
    want[:H0 - 2, 3:] = ONE
    np.testing.assert_array_equal(acc, want)


def test_a_sub_pixel_shift_is_exactly_one_inside():
    f = np.zeros((1, H0, W0, 2), np.float32)
    f[...] = (0.3, 0.7)
    acc = np_range_acc(f)[0]
    assert (acc[1:, 1:] == ONE).all()                               # every interior pixel, exactly
    assert (acc[0, :] < ONE).all() and (acc[:, 0] < ONE).all() and (acc[0, :] > 0).all()


def test_the_moving_square_has_the_known_occlusions():
    """A 10 x 10 square that moved by (4, 3): the backward flow is (-4, -3) on the moved square and zero elsewhere.  Nothing of
    frame 2 comes from the 58 background pixels the moved square covers; everything else receives at least one whole vector."""
    top, left, side = 12, 13, 10
    sq1, sq2 = np.zeros((H0, W0), bool), np.zeros((H0, W0), bool)
    sq1[top:top + side, left:left + side] = True
    sq2[top + 3:top + 3 + side, left + 4:left + 4 + side] = True
    bwd = np.zeros((1, H0, W0, 2), np.float32)
    bwd[0, sq2] = (-4, -3)
    acc = np_range_acc(bwd)[0]
    covered = sq2 & ~sq1
    assert covered.sum() == 58
    np.testing.assert_array_equal(acc < (1 << 23), covered)
    doubled = sq1 & ~sq2                                            # the static background there AND the square land on it
    assert (acc[covered] == 0).all() and (acc[doubled] == 2 * ONE).all() and (acc[~covered & ~doubled] == ONE).all()
    fwd = np.zeros((1, H0, W0, 2), np.float32)
    fwd[0, sq1] = (4, 3)
    np.testing.assert_array_equal(np_range_occlusion(fwd, bwd)[0], covered)
    np.testing.assert_array_equal(np_range_occlusion(bwd, fwd)[0], sq1 & ~sq2)          # what the square uncovered


@pytest.mark.parametrize('H,W', [(37, 53), (64, 96)])
def test_on_the_consistency_tests_square_both_methods_agree(H, W):
    """tests/test_consistency.py's moving square: the range test marks exactly what the forward-backward test marks."""
    _, _, fwd, bwd, _, _ = analytic_case(H, W, N=2)
    np.testing.assert_array_equal(np_range_occlusion(fwd, bwd), np_flow_consistency(fwd, bwd)[0])
    np.testing.assert_array_equal(np_range_occlusion(bwd, fwd), np_flow_consistency(bwd, fwd)[0])


def test_the_four_weights_sum_to_two_to_the_24():
    rng = np.random.default_rng(0)
    a = rng.uniform(0, 1, 100000).astype(np.float32)
    b = rng.uniform(0, 1, 100000).astype(np.float32)
    a[:4], b[:4] = (0.0, 0.5, np.float32(1 - 2.0 ** -24), 2.0 ** -13), (np.float32(1 - 2.0 ** -24), 0.0, 0.5, 2.0 ** -13)
    w = np_range_weights(a, b)
    assert all((k >= 0).all() and (k <= ONE).all() for k in w)
    assert (sum(w) == ONE).all()


def test_a_fraction_just_below_one_rounds_to_the_far_corner():
    a = np.array([1 - 2.0 ** -24], np.float32)
    assert a[0] < 1 and np_range_weights(a, np.zeros(1, np.float32))[1][0] == ONE      # qa = 4096
    f = np.zeros((1, 3, 4, 2), np.float32)
    f[0, 1, 1, 0] = -2.0 ** -24                                     # sx = 1 - 2^-24: x0 = 0, all of the weight on x0 + 1
    acc = np_range_acc(f)[0]
    assert (acc == ONE).all()
    f[0, 1, 1, 0] = -2.0 ** -30                                     # float32(1 - 2^-30) is 1: no fraction at all
    assert (np_range_acc(f)[0] == ONE).all()


def test_every_vector_on_one_pixel_needs_more_than_32_bits():
    acc = np_range_acc(all_to_one(H0, W0, 11, 17)[None])[0]
    assert int(acc[11, 17]) == H0 * W0 * ONE > 1 << 32
    assert int(acc.sum()) == H0 * W0 * ONE and np.count_nonzero(acc) == 1
    assert np_range_map(all_to_one(H0, W0, 11, 17)[None])[0, 11, 17] == np.float32(H0 * W0)


def test_vectors_out_of_range_contribute_nothing():
    f = np.zeros((1, 5, 7, 2), np.float32)
    f[0, 2, 3] = (1e30, 0)
    f[0, 2, 4] = (0, np.inf)
    f[0, 2, 5] = (np.nan, np.nan)
    f[0, 1, 0] = (-1.0, 0)                                          # sx = -1 exactly: out
    f[0, 1, 6] = (1.0, 0)                                           # sx = W exactly: out
    f[0, 0, 2] = (0, -0.25)                                         # sy = -0.25: three quarters of it reach row 0
    acc = np_range_acc(f)[0]
    want = np.full((5, 7), ONE, np.uint64)
    want[2, 3:6] = 0
    want[1, 0] = want[1, 6] = 0
    want[0, 2] = 3 * ONE // 4
    np.testing.assert_array_equal(acc, want)


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 3, 1), (1, 5, 7), (2, 37, 53)])
def test_the_test_flows_exercise_every_branch(shape):
    N, H, W = shape
    flows = range_flows(N, H, W, seed=H + W)
    assert flows.shape == (2 * N, H, W, 2) and flows.dtype == np.float32
    vis, frac, occ = np_range_visibility(flows, N)
    assert vis.shape == (2 * N, H, W) and 0.0 <= float(frac) <= 1.0
    if H >= 5:
        acc = np_range_acc(flows)
        assert np.isnan(flows).any() and np.isinf(flows).any() and (np.abs(flows) == np.float32(1e30)).any()
        assert int(acc[-1].max()) >= (H * W - 8) * ONE // 2          # the all-to-one image
        assert occ.any() and not occ.all()
        assert ((acc > 0) & (acc < ONE)).any() and (acc > ONE).any()
    if shape == (2, 37, 53):
        assert int(np_range_acc(flows)[-1].max()) > 1 << 32
        assert 0.05 < float(frac) < 0.95


def test_the_threshold_is_compared_on_the_integers():
    assert range_threshold_sum(0.5) == 1 << 23 and range_threshold_sum(1.0) == ONE
    assert range_threshold_sum(2.0 ** -30) == 1 and range_threshold_sum(np.float32(0.3)) == math.ceil(float(np.float32(0.3)) * ONE)
    f = np.zeros((2, 4, 4, 2), np.float32)
    f[1, :, :, 0] = 0.5                                             # column 0 of the other frame receives exactly half
    occ = np_range_occlusion(f[:1], f[1:], 0.5)[0]
    assert not occ.any()                                            # 2^23 < 2^23 is false
    occ = np_range_occlusion(f[:1], f[1:], np.float32(0.5) + np.float32(2.0 ** -24))[0]
    np.testing.assert_array_equal(occ[:, 0], True)
    assert not occ[:, 1:].any()


# ------------------------------------------------------------------ the C entries
def test_the_header_declares_and_the_library_exports_the_entries():
    from tf_raft_amd import build
    assert 'flow_splat.hip' in build.SOURCES
    with open(os.path.join(ROOT, 'include', 'raft_hip.h')) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    assert re.search(r'int64_t\s+raft_flow_range_workspace_bytes\s*\(\s*int slices,\s*int H,\s*int W\s*\)', header)
    for name in ('raft_flow_range_map_f32', 'raft_flow_range_occlusion_f32', 'raft_flow_range_visibility_f32'):
        assert re.search(r'int\s+' + name + r'\s*\(', header), name
    sigs = _ffi.header_signatures(header)
    P, I, F = C.c_void_p, C.c_int, C.c_float
    assert sigs['raft_flow_range_workspace_bytes'] == (C.c_int64, [I, I, I])
    assert sigs['raft_flow_range_map_f32'] == (I, [P, P, I, I, I, P, P])
    assert sigs['raft_flow_range_occlusion_f32'] == (I, [P, P, P, P, I, I, I, F, P, P])
    assert sigs['raft_flow_range_visibility_f32'] == (I, [P, P, P, P, I, I, I, F, I, P, P, P])
    assert _ffi.ABI_VERSION == 222                                   # entries were added, no signature changed
    lib = _ffi.load_library()
    assert lib.raft_version() == 222
    assert lib.raft_flow_range_visibility_f32.argtypes == sigs['raft_flow_range_visibility_f32'][1]
    assert lib.raft_flow_range_workspace_bytes(3, 37, 53) == 3 * 37 * 53 * 8
    assert lib.raft_flow_range_workspace_bytes(8, 1080, 1920) == 8 * 1080 * 1920 * 8
    for bad in ((0, 4, 5), (1, 0, 5), (1, 4, -1), (1, 1 << 14, (1 << 14) + 1), (1 << 10, 1 << 10, 1 << 10)):
        assert lib.raft_flow_range_workspace_bytes(*bad) == 0, bad
    assert lib.raft_flow_range_workspace_bytes(1, 1 << 14, 1 << 14) == 8 << 28


SIZES_REFUSED = ((1, 1 << 15, 1 << 15), (1 << 10, 1 << 10, 1 << 10), (1, 1, 1 << 30),      # what flow_check_sizes refuses
                 (1, 1 << 14, (1 << 14) + 1), (1, 1, (1 << 28) + 1))                         # H * W > 2^28
THRESHOLDS_REFUSED = (0.0, -0.5, 1.0 + 2.0 ** -20, 2.0, float('nan'), float('inf'), -float('inf'))


def _buffers():
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    return buf, p, C.c_void_p(p.value + 4)


def test_range_map_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    fn = _ffi.load_library().raft_flow_range_map_f32
    _keep, p, off = _buffers()
    #       flow range N  H  W  ws stream
    good = [p, p, 1, 4, 5, p, None]
    for k in (0, 1, 5):
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    for k in (2, 3, 4):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for bad in SIZES_REFUSED:
        args = list(good)
        args[2:5] = bad
        assert fn(*args) == -2, bad
    for k in (0, 5):
        args = list(good)
        args[k] = off
        assert fn(*args) == -4, k
    args = list(good)                                               # precedence: NULL before shape before alignment
    args[1], args[2], args[0] = None, 0, off
    assert fn(*args) == -1
    args[1] = p
    assert fn(*args) == -2
    args[2] = 1
    assert fn(*args) == -4


def test_range_occlusion_argument_errors_are_returned_before_any_device_work():
    fn = _ffi.load_library().raft_flow_range_occlusion_f32
    _keep, p, off = _buffers()
    #       flow_a flow_b occ_a occ_b N  H  W  t    ws stream
    good = [p, p, p, p, 1, 4, 5, 0.5, p, None]
    for k in (0, 1, 2, 8):                                          # (occluded_b may be NULL)
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    for k in (4, 5, 6):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for bad in SIZES_REFUSED:
        args = list(good)
        args[4:7] = bad
        assert fn(*args) == -2, bad
    for t in THRESHOLDS_REFUSED:
        args = list(good)
        args[7] = t
        assert fn(*args) == -2, t
    for k in (0, 1, 8):
        for second in (p, None):
            args = list(good)
            args[k], args[3] = off, second
            assert fn(*args) == -4, (k, second)
    args = list(good)                                               # precedence
    args[2], args[7], args[8] = None, 0.0, off
    assert fn(*args) == -1
    args[2] = p
    assert fn(*args) == -2
    args[7] = 1.0                                                   # (1 is allowed)
    assert fn(*args) == -4


def test_range_visibility_argument_errors_are_returned_before_any_device_work():
    fn = _ffi.load_library().raft_flow_range_visibility_f32
    _keep, p, off = _buffers()
    #       flows mask visible fraction N  H  W  t    apply ws records stream
    good = [p, p, p, p, 1, 4, 5, 0.5, 1, p, p, None]
    for k in (0, 3, 9, 10):                                         # (mask and visible may be NULL)
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    for k in (4, 5, 6):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for bad in ((1, 1 << 14, 1 << 15), (1 << 9, 1 << 10, 1 << 10), (1, 1, 1 << 29), ((1 << 30) + 1, 1, 1), (1 << 29, 1, 1),   # 2N*H*W*2 reaches 2^31
                (1, 1 << 14, (1 << 14) + 1)):
        args = list(good)
        args[4:7] = bad
        assert fn(*args) == -2, bad
    for t in THRESHOLDS_REFUSED:
        args = list(good)
        args[7] = t
        assert fn(*args) == -2, t
    for v in (-1, 2):
        args = list(good)
        args[8] = v
        assert fn(*args) == -2, v
    for k in (0, 9, 10):
        for m, vis in ((p, p), (None, None)):
            args = list(good)
            args[k], args[1], args[2] = off, m, vis
            assert fn(*args) == -4, (k, m)
    args = list(good)                                               # precedence: NULL before shape before alignment
    args[0], args[4], args[9] = None, 0, off
    assert fn(*args) == -1
    args[0] = off
    assert fn(*args) == -2
    args[4], args[8] = 1, 7
    assert fn(*args) == -2
    args[8], args[7] = 0, float('nan')
    assert fn(*args) == -2
    args[7] = 2.0 ** -20
    assert fn(*args) == -4


# ------------------------------------------------------------------ the Python layer, nothing reaches the device
BAD_THRESHOLDS = (0, 0.0, -0.5, 1.5, float('nan'), float('inf'), 1e-60, 10 ** 400, 'x', None, True, (0.5,), 1j)


def test_the_threshold_is_checked_without_a_gpu():
    from tf_raft_amd import image_ops
    assert image_ops.RANGE_THRESHOLD == 0.5
    assert image_ops.check_range_threshold(0.5) == 0.5 and image_ops.check_range_threshold(1) == 1.0
    assert image_ops.check_range_threshold(np.float32(0.3)) == float(np.float32(0.3))
    assert image_ops.check_range_threshold(0.3) == float(np.float32(0.3))          # what the entry will see
    zero = np.zeros((4, 5, 2), np.float32)
    for bad in BAD_THRESHOLDS:
        with pytest.raises(ValueError, match='threshold'):
            image_ops.check_range_threshold(bad)
        with pytest.raises(ValueError, match='threshold'):
            image_ops.range_occlusion(zero, zero, threshold=bad)
    with pytest.raises(ValueError, match=r'\(\.\.\., H, W, 2\)'):
        image_ops.range_map(np.zeros((4, 5, 3), np.float32))
    with pytest.raises(ValueError, match='empty'):
        image_ops.range_map(np.zeros((0, 5, 2), np.float32))


def test_predict_step_bidirectional_checks_the_occlusion_test_before_any_device_work():
    import inspect
    from tf_raft_amd import image_ops
    from tf_raft_amd.model import RAFT, SmallRAFT
    x = np.zeros((1, 64, 96, 3), np.float32)
    for cls in (RAFT, SmallRAFT):
        for fn in (cls.predict_step_bidirectional, cls.predict_bidirectional):
            sig = inspect.signature(fn).parameters
            assert sig['occlusion_test'].default == 'consistency' and sig['range_threshold'].default == image_ops.RANGE_THRESHOLD
            assert (sig['alpha'].default, sig['beta'].default) == (0.01, 0.5)
        model = cls.__new__(cls)                                             # (no device: anything enqueued would fail)
        for bad in ('Range', 'unflow', '', None, 1, True, ('range',)):
            with pytest.raises(ValueError, match='occlusion_test'):
                model.predict_step_bidirectional((x, x), occlusion_test=bad)
            with pytest.raises(ValueError, match='occlusion_test'):
                model.predict_bidirectional([x, x], occlusion_test=bad)
        for bad in BAD_THRESHOLDS:
            with pytest.raises(ValueError, match='threshold'):
                model.predict_step_bidirectional((x, x), occlusion_test='range', range_threshold=bad)
            with pytest.raises(ValueError, match='threshold'):
                model.predict_bidirectional([x, x], occlusion_test='range', range_threshold=bad)


def test_compile_validates_the_occlusion_test():
    import inspect
    from tf_raft_amd import image_ops, losses
    from tf_raft_amd.model import RAFT, SmallRAFT
    sig = inspect.signature(RAFT.compile).parameters
    assert sig['occlusion_test'].default == 'consistency' and sig['range_threshold'].default == image_ops.RANGE_THRESHOLD == 0.5
    for cls in (RAFT, SmallRAFT):
        model = cls.__new__(cls)
        loss = losses.PhotometricSequenceLoss()
        for bad in ('Range', 'unflow', '', None, 1, True):
            with pytest.raises(ValueError, match='occlusion_test'):
                model.compile(optimizer=None, loss=loss, bidirectional=True, occlusion_test=bad)
        for bad in BAD_THRESHOLDS:
            with pytest.raises(ValueError, match='threshold'):
                model.compile(optimizer=None, loss=loss, bidirectional=True, occlusion_test='range', range_threshold=bad)
        for kw in ({}, {'bidirectional': False}):                            # 'range' is the mask of a bidirectional step
            with pytest.raises(ValueError, match='bidirectional=True'):
                model.compile(optimizer=None, loss=loss, occlusion_test='range', **kw)
            with pytest.raises(ValueError, match='bidirectional=True'):
                model.compile(optimizer=None, occlusion_test='range', **kw)
        model.compile(optimizer=None, loss=loss, bidirectional=True, occlusion_test='range', range_threshold=np.float32(0.25))
        assert model.occlusion_test == 'range' and model.range_threshold == 0.25 and model.bidirectional is True
        assert model._unlabelled_keys() == ('loss', 'photometric', 'smoothness', 'occluded') and model.last_visibility is None
        for kw in ({}, {'occlusion_test': 'consistency'}):                   # the default stays what it was
            model.compile(optimizer=None, loss=loss, bidirectional=True, **kw)
            assert model.occlusion_test == 'consistency' and model.consistency == (0.01, 0.5) and model.range_threshold == 0.5
        model.compile(optimizer=None)
        assert model.occlusion_test == 'consistency' and model.bidirectional is False

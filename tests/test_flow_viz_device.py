"""Device-side flow colour coding (CPU side): the C ABI of the two entries, their argument checks, and the fixtures.

tests/golden/flow_viz_device_golden.npz is made by tests/golden/make_flow_viz_device_golden.py from the reference's own
flow_viz.py.  ``tf_raft_amd.io.flow_to_image`` is pinned to that NumPy bit for bit (tests/test_io.py), so recomputing every
fixture with it here pins the file: a fixture that drifted from its generator fails without a GPU.
tests/test_gpu_flow_viz.py holds the kernels to these fixtures and imports ``load_golden`` / ``assert_parity`` from here.
"""
import ctypes as C
import json
import os

import numpy as np

from conftest import GOLDEN
from test_any_size import np_crop_or_pad

from tf_raft_amd import _ffi, io


def load_golden():
    """``(checks, arrays)``: the manifest's entries and the npz's arrays (``flow/<name>``, ``img/<check>``, ``rad/<check>``)."""
    with np.load(os.path.join(GOLDEN, 'flow_viz_device_golden.npz')) as z:
        arrays = {k: z[k] for k in z.files}
    return json.loads(str(arrays.pop('manifest'))), arrays


def assert_parity(got, want, what=''):
    """The parity condition of DESIGN.md section 13: the one source of difference is the rounding of atan2, which can move
    floor(255 * col) by one level where the value lies within about 1e-4 of an integer.  So every channel value is within one
    level, and at most max(2, 1e-5 * values) of them differ at all."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    differing = int((diff != 0).sum())
    print(f'[parity] flow_viz {what}: {differing} of {want.size} values differ, largest difference {int(diff.max())}')
    assert diff.max() <= 1, (what, int(diff.max()))
    assert differing <= max(2, 1e-5 * want.size), (what, differing, want.size)


def test_flow_viz_entries_are_declared_exported_and_mirrored():
    """The workspace rule (the prototypes: tests/test_host_logic.py test_the_binding_is_the_header)."""
    lib = _ffi.load_library()
    k = lib.raft_flow_to_image_workspace_floats(1)
    assert k >= 1 and lib.raft_flow_to_image_workspace_floats(5) == 5 * k and lib.raft_flow_to_image_workspace_floats(0) == 0


def test_flow_viz_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    buf = (C.c_double * 64)()                                      # (8-byte aligned)
    p = C.cast(buf, C.c_void_p)
    calls = {'raft_flow_rad_max_f32': ([p, p, 1, 4, 4, 8, 8, -1.0, None], (0, 1)),
             'raft_flow_to_image_u8': ([p, p, p, 1, 4, 4, 8, 8, -1.0, 0, 0.0, None], (0, 1, 2))}
    for name, (good, pointers) in calls.items():
        fn = getattr(lib, name)
        first = len(pointers)                                      # index of N
        for k in pointers:
            args = list(good)
            args[k] = None
            assert fn(*args) == -1, (name, k)
        for bad in ((0, 4, 4, 8, 8), (1, 0, 4, 8, 8), (1, 4, 0, 8, 8), (1, 4, 4, 0, 8), (1, 4, 4, 8, 0), (-1, 4, 4, 8, 8), (1, 4, 4, 8, -8)):
            args = list(good)
            args[first:first + 5] = bad
            assert fn(*args) == -2, (name, bad)
        # a row's elements (Ws * 2, Wt * 3) and the pixels of one picture do not fit an int
        for bad in ((1, 4, 1 << 30, 8, 8), (1, 4, 4, 8, 1 << 30), (1, 4, 4, 1 << 16, 1 << 16)):
            args = list(good)
            args[first:first + 5] = bad
            assert fn(*args) == -2, (name, bad)
        args = list(good)
        args[0] = C.c_void_p(p.value + 4)                          # the flow is read as float2
        assert fn(*args) == -4, name
    # only a fixed radius > 0 makes the maxima optional (tests/test_gpu_flow_viz.py passes none with one)
    for fixed in (0.0, -1.0, float('nan')):
        args = list(calls['raft_flow_to_image_u8'][0])
        args[1], args[10] = None, fixed
        assert lib.raft_flow_to_image_u8(*args) == -1, fixed


def test_python_argument_checks_need_no_device():
    import pytest
    from tf_raft_amd import image_ops
    assert image_ops._viz_args(None, None) == (-1.0, 0.0)
    assert image_ops._viz_args(2, 3) == (2.0, 3.0)
    for clip in (-1.0, float('nan')):
        with pytest.raises(ValueError, match='clip_flow'):
            image_ops._viz_args(clip, None)
    for rad in (0.0, -2.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='rad_max'):
            image_ops._viz_args(None, rad)


def test_fixtures_are_what_the_host_colour_coding_gives():
    checks, arrays = load_golden()
    names = [c['name'] for c in checks]
    assert len(set(names)) == len(names) >= 18
    eps = np.float32(1e-5)
    for c in checks:
        flows = arrays['flow/' + c['flow']]
        assert flows.dtype == np.float32 and flows.ndim == 4
        want = arrays['img/' + c['name']]
        for n, f in enumerate(flows):
            if c['size'] is not None:
                f = np_crop_or_pad(f[None], *c['size'])[0]
            if c['rad_max'] is None:
                img = io.flow_to_image(f, clip_flow=c['clip'], convert_to_bgr=c['bgr'])
                g = f if c['clip'] is None else np.clip(f, 0, c['clip'])
                rad = np.max(np.sqrt(np.square(g[..., 0]) + np.square(g[..., 1])))
                assert rad.dtype == np.float32 and rad == arrays['rad/' + c['name']][n], (c['name'], n)
            else:
                d = np.float32(c['rad_max']) + eps
                img = io.flow_uv_to_colors(f[..., 0] / d, f[..., 1] / d, c['bgr'])
            np.testing.assert_array_equal(img, want[n], err_msg=c['name'])
    # what the cases are there for
    assert (arrays['img/zeros'] == 255).all()
    assert [round(float(r), 3) for r in arrays['rad/batch3']] == [0.5, 3.0, 40.0]
    assert arrays['rad/lastpix'][0] == 50.0 and arrays['rad/window_pad'].tolist() == [50.0, 50.0]
    assert (arrays['rad/window_crop'] < 12).all() and (arrays['rad/window_mixed'] < 12).all()      # the 50 px vector is cut away
    axes = arrays['flow/axes'].reshape(-1, 2)
    assert np.signbit(axes[1, 1]) and not np.signbit(axes[0, 1])
    red = arrays['img/axes'].reshape(-1, 3)
    # (1, +0.0): fk = 0, the wheel's first entry (red); (1, -0.0): fk = 54, its last entry (towards magenta) with weight 1 and
    # k1 = 55 wrapped to entry 0 with weight 0
    assert red[0][0] == 255 and red[0][1] == red[0][2] < 255
    assert red[1][0] == 255 and red[1][1] == red[0][1] < red[1][2] < 255
    # a fixed radius below the image's own maximum: some pixels take the darkened out-of-range branch
    d = np.float32(2.0) + eps
    assert (np.sqrt(((arrays['flow/odd'][0] / d) ** 2).sum(-1)) > 1).any()

"""The forward projection of a flow and the warm start, without a GPU: the float32 rule of include/raft_hip.h
(``np_forward_interpolate`` in tests/golden/make_flow_init_golden.py) against SciPy's ``griddata(method='nearest')`` applied the way
the RAFT authors' ``forward_interpolate`` applies it (tests/golden/flow_init_golden.npz holds SciPy's outputs), the rule's edge
cases, the C entries' declarations and argument checks, and the public op's argument errors.

The two computations agree in every cell of the six cases and the float32 rule has no distance tie on them (the make script
asserts both before it writes the fixture), so equality is exact and no cell is left out.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from tf_raft_amd import _ffi

sys.path.insert(0, GOLDEN)
from make_flow_init_golden import CASES, case_flow, np_forward_interpolate      # noqa: E402

# the rule restated and pinned below is the contract of this entry: on a tree without it the file has nothing to speak about
ENTRY = _ffi._SIGNATURES['raft_forward_interpolate_f32']


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'flow_init_golden.npz')) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize('case', CASES, ids=[f'seed{c[0]}_{c[1]}x{c[2]}' for c in CASES])
def test_the_float32_rule_is_scipy_nearest_in_every_cell(golden, case):
    seed, h, w, scale = case
    flow = golden[f'flow_{seed}']
    np.testing.assert_array_equal(flow, case_flow(seed, h, w, scale))                    # the fixture's input is the stated one
    got, ties = np_forward_interpolate(flow, return_ties=True)
    assert got.dtype == np.float32 and got.shape == (h, w, 2)
    assert ties == 0, 'the case has a float32 distance tie: SciPy does not promise which source it returns'
    np.testing.assert_array_equal(got, golden[f'scipy_{seed}'])
    assert got.any()


def test_zero_flow_gives_zero_and_no_valid_source_gives_zero():
    for h, w in ((1, 1), (1, 7), (8, 12), (9, 13)):
        np.testing.assert_array_equal(np_forward_interpolate(np.zeros((h, w, 2), np.float32)), np.zeros((h, w, 2), np.float32))
        for vec in ((-w, 0), (w, 0), (0, h), (0, -h), (3 * w, -2 * h), (np.nan, 0)):
            flow = np.empty((h, w, 2), np.float32)
            flow[...] = vec
            got = np_forward_interpolate(flow)
            assert not got.any() and not np.isnan(got).any(), (h, w, vec)
    # row 0 and column 0 are no sources (the inequalities are strict): a flow that lives there alone leaves nothing
    flow = np.zeros((8, 12, 2), np.float32)
    flow[0, :, 1], flow[:, 0, 0] = -0.25, -0.25
    assert not np_forward_interpolate(flow)[1:, 1:].any()
    # ... and a batch is its images one by one
    both = np.stack([case_flow(0, 8, 12, 2), np.full((8, 12, 2), 100, np.float32)])
    got = np_forward_interpolate(both)
    np.testing.assert_array_equal(got[0], np_forward_interpolate(both[0]))
    assert not got[1].any()


def shifted_flow(h, w):
    """u = 1 with a small v that names its source: target (tx, ty) must take the vector of source (max(tx - 1, 0), ty)."""
    flow = np.empty((h, w, 2), np.float32)
    flow[..., 0] = 1
    flow[..., 1] = (1 + np.arange(h * w, dtype=np.float32).reshape(h, w)) * np.float32(2.0 ** -12)
    return flow


def tied_flow(h, w, tagged):
    """u = +0.5 everywhere: every target with a column to its left lies exactly half a cell from two end points.  ``tagged``: v is
    +0.25 in even and -0.25 in odd columns, which keeps the two distances equal (0.25 + 0.0625) and shows which source won."""
    flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0] = 0.5
    if tagged:
        flow[:, 0::2, 1], flow[:, 1::2, 1] = 0.25, -0.25
    return flow


def test_an_integer_shift_moves_the_field_and_a_half_cell_tie_goes_to_the_lowest_index():
    h, w = 6, 9
    flow = shifted_flow(h, w)
    got, ties = np_forward_interpolate(flow, return_ties=True)
    assert ties == 0
    np.testing.assert_array_equal(got[:, 1:], flow[:, :-1])
    np.testing.assert_array_equal(got[:, 0], flow[:, 0])
    plain = tied_flow(h, w, False)
    got, ties = np_forward_interpolate(plain, return_ties=True)
    assert ties >= (h - 1) * (w - 1)
    np.testing.assert_array_equal(got, plain)                       # (a constant field projects onto itself)
    tagged = tied_flow(h, w, True)
    got, ties = np_forward_interpolate(tagged, return_ties=True)
    assert ties >= (h - 2) * (w - 1)
    np.testing.assert_array_equal(got[1:-1, 1:], tagged[1:-1, :-1])   # the LEFT source, index y * w + x - 1, wins every tie


def test_flow_init_entries_are_declared_exported_and_mirrored():
    """The unit is built (the prototypes: tests/test_host_logic.py test_the_binding_is_the_header)."""
    from tf_raft_amd import build
    assert 'flow_init.hip' in build.SOURCES


def test_flow_init_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    a, b = (C.c_float * 256)(), (C.c_float * 256)()
    pa, pb = C.cast(a, C.c_void_p), C.cast(b, C.c_void_p)
    fn = lib.raft_forward_interpolate_f32
    good = [pa, 1, 4, 5, pb, None]
    for k in (0, 4):
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    for k in (1, 2, 3):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for bad in ((1, 1 << 15, 1 << 15), (1 << 10, 1 << 10, 1 << 10), (1, 1, 1 << 30), (1 << 20, 1 << 20, 1 << 20)):
        args = list(good)
        args[1:4] = bad
        assert fn(*args) == -2, bad
    for k in (0, 4):
        args = list(good)
        args[k] = C.c_void_p(args[k].value + 4)                             # read and written as float2
        assert fn(*args) == -4, k
    assert fn(pa, 1, 4, 5, pa, None) == -3                                  # in place
    assert fn(pa, 1, 4, 5, C.c_void_p(pa.value + 8), None) == -3            # overlapping
    for name in ('raft_warm_start_f32', 'raft_warm_start_small_f32'):
        fn = getattr(lib, name)
        st = _ffi.State(**{f: pb for f, _ in _ffi.State._fields_})
        assert fn(None, 1, 4, 5, C.byref(st), None) == -1, name
        assert fn(pa, 1, 4, 5, None, None) == -1, name
        for field in ('x', 'coords1', 'flow'):
            broken = _ffi.State(**{f: (None if f == field else pb) for f, _ in _ffi.State._fields_})
            assert fn(pa, 1, 4, 5, C.byref(broken), None) == -1, (name, field)
        for bad in ((0, 4, 5), (1, -1, 5), (1, 4, 0), (1 << 10, 1 << 10, 1 << 10)):
            assert fn(pa, *bad, C.byref(st), None) == -2, (name, bad)
        assert fn(C.c_void_p(pa.value + 4), 1, 4, 5, C.byref(st), None) == -4, name
        for field in ('x', 'coords1', 'flow'):
            skew = _ffi.State(**{f: (C.c_void_p(pb.value + 4) if f == field else pb) for f, _ in _ffi.State._fields_})
            assert fn(pa, 1, 4, 5, C.byref(skew), None) == -4, (name, field)


def test_the_public_op_rejects_bad_arguments_without_a_gpu():
    import torch
    from tf_raft_amd import image_ops
    for bad in (np.zeros((4, 2), np.float32), np.zeros((2,), np.float32), np.zeros((4, 5, 3), np.float32), np.zeros((2, 4, 5, 1), np.float32),
                np.zeros((0, 5, 2), np.float32), np.zeros((3, 0, 5, 2), np.float32), torch.zeros((4, 5, 3))):
        with pytest.raises(ValueError):
            image_ops.forward_interpolate(bad)
    for bad in (np.zeros((4, 5, 2), np.int32), np.zeros((4, 5, 2), np.float16), np.zeros((4, 5, 2), np.uint8),
                torch.zeros((4, 5, 2), dtype=torch.float16), torch.zeros((4, 5, 2), dtype=torch.int64)):
        with pytest.raises(TypeError):
            image_ops.forward_interpolate(bad)


def test_the_model_has_the_video_entry_points_and_predict_video_checks_its_frames_first():
    from tf_raft_amd import video
    from tf_raft_amd.model import RAFT, SmallRAFT
    for cls in (RAFT, SmallRAFT):
        assert callable(cls.video) and callable(cls.predict_video)
    for bad in (np.zeros((1, 64, 96, 3), np.uint8), np.zeros((0, 64, 96, 3), np.uint8)):
        with pytest.raises(ValueError, match='two frames'):
            video.predict_video(None, bad)
    for bad in (np.zeros((64, 96, 3), np.uint8), np.zeros((3, 64, 96, 1), np.uint8)):
        with pytest.raises(ValueError, match='one video'):
            video.predict_video(None, bad)

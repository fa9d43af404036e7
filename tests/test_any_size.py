"""Frames of any size (CPU side): the crop-or-pad rule, the C ABI of the window-copy entries, the reference's names
(CropOrPadder / ShapeSetter / VisFlowCallback / flow_viz) and the PNG writer.

The yardstick of the rule is ``np_crop_or_pad`` below: tf.image.resize_with_crop_or_pad restated in NumPy from TensorFlow's
published source (TensorFlow is not available to the tests), pinned by worked cases.  tests/test_gpu_any_size.py imports it.
"""
import ctypes as C
import importlib
import os
import struct
import sys
import zlib

import numpy as np
import pytest

from conftest import GOLDEN

from tf_raft_amd import _ffi


def np_axis(source, target):
    """(first source index kept, first target index written, length) of one axis."""
    d = target - source
    return max(-d // 2, 0), max(d // 2, 0), min(source, target)


def np_crop_or_pad(x, th, tw):
    """tf.image.resize_with_crop_or_pad(x, th, tw) on (..., H, W, C): centred crop where the source is larger, centred zero
    padding where it is smaller, independently per axis; an odd surplus goes to the bottom / right."""
    x = np.asarray(x)
    out = np.zeros(x.shape[:-3] + (th, tw, x.shape[-1]), x.dtype)
    cy, py, ey = np_axis(x.shape[-3], th)
    cx, px, ex = np_axis(x.shape[-2], tw)
    out[..., py:py + ey, px:px + ex, :] = x[..., cy:cy + ey, cx:cx + ex, :]
    return out


# (source, target) -> (rows / columns of padding before, after) or (dropped before, dropped after): worked cases of the rule
PAD_CASES = {(436, 448): (6, 6), (1242, 1248): (3, 3), (375, 376): (0, 1), (5, 8): (1, 2)}
CROP_CASES = {(7, 4): (1, 2), (70, 64): (3, 3)}


def test_the_numpy_restatement_gives_the_worked_cases():
    for (s, t), (before, after) in PAD_CASES.items():
        got = np_crop_or_pad(np.arange(1, s + 1, dtype=np.float32).reshape(s, 1, 1), t, 1)[:, 0, 0]
        assert list(got[:before]) == [0] * before and list(got[t - after:]) == [0] * after
        np.testing.assert_array_equal(got[before:t - after], np.arange(1, s + 1))
    for (s, t), (before, after) in CROP_CASES.items():
        got = np_crop_or_pad(np.arange(s, dtype=np.float32).reshape(1, s, 1), 1, t)[0, :, 0]
        np.testing.assert_array_equal(got, np.arange(before, s - after))
    np.testing.assert_array_equal(np_crop_or_pad(np.arange(7).reshape(1, 7, 1), 1, 4)[0, :, 0], [1, 2, 3, 4])    # 7 -> 4 keeps columns 1..4


def test_crop_or_pad_offsets_follow_the_rule():
    from tf_raft_amd.image_ops import crop_or_pad_offsets
    for (s, t), (before, after) in PAD_CASES.items():
        assert crop_or_pad_offsets(s, t) == (0, before, s) and t - before - s == after
    for (s, t), (before, after) in CROP_CASES.items():
        assert crop_or_pad_offsets(s, t) == (before, 0, t) and s - before - t == after
    for s in range(1, 21):
        for t in range(1, 21):
            crop, pad, ext = crop_or_pad_offsets(s, t)
            assert (crop, pad, ext) == np_axis(s, t)
            want = np_crop_or_pad(np.arange(1, s + 1).reshape(s, 1, 1), t, 1)[:, 0, 0]
            got = np.zeros(t, want.dtype)
            got[pad:pad + ext] = np.arange(1, s + 1)[crop:crop + ext]
            np.testing.assert_array_equal(got, want)
            if t >= s:       # padding, then cropping back to the source size, is the identity
                back = crop_or_pad_offsets(t, s)
                assert back == (pad, 0, s)
                np.testing.assert_array_equal(np_crop_or_pad(want.reshape(t, 1, 1), s, 1)[:, 0, 0], np.arange(1, s + 1))
    for bad in ((0, 4), (4, 0), (-1, 3)):
        with pytest.raises(ValueError):
            crop_or_pad_offsets(*bad)


def test_the_fixture_generator_restates_the_same_rule(rng):
    sys.path.insert(0, GOLDEN)
    mk = importlib.import_module('make_conditioning_any_size')
    x = rng.normal(size=(2, 7, 10, 3)).astype(np.float32)
    for th, tw in ((8, 16), (4, 5), (9, 6), (7, 10), (1, 1)):
        np.testing.assert_array_equal(mk.np_crop_or_pad(x, th, tw), np_crop_or_pad(x, th, tw))


NEW_ENTRIES = ('raft_crop_or_pad_f32', 'raft_crop_or_pad_u8_f32', 'raft_crop_or_pad_u8')


def test_window_copy_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for name in NEW_ENTRIES:
        fn = getattr(lib, name)
        assert fn(None, p, 1, 4, 4, 8, 8, 3, None) == -1
        assert fn(p, None, 1, 4, 4, 8, 8, 3, None) == -1
        for bad in ((0, 4, 4, 8, 8, 3), (1, 0, 4, 8, 8, 3), (1, 4, 0, 8, 8, 3), (1, 4, 4, 0, 8, 3), (1, 4, 4, 8, 0, 3),
                    (1, 4, 4, 8, 8, 0), (-2, 4, 4, 8, 8, 3), (1, 4, 4, 8, -8, 3)):
            assert fn(p, p, *bad, None) == -2, (name, bad)
        assert fn(p, p, 1, 4, 1 << 30, 8, 8, 3, None) == -2            # W * C does not fit an int


def test_reference_import_lines_resolve():
    from tf_raft.datasets import ShapeSetter, CropOrPadder              # train_sintel.py:9
    from tf_raft.datasets.flow_viz import flow_to_image                 # tf_raft/training.py:7
    from tf_raft.training import VisFlowCallback, first_cycle_scaler    # train_sintel.py:11
    import tf_raft_amd.datasets
    import tf_raft_amd.io
    import tf_raft_amd.training
    assert CropOrPadder is tf_raft_amd.datasets.CropOrPadder and ShapeSetter is tf_raft_amd.datasets.ShapeSetter
    assert flow_to_image is tf_raft_amd.io.flow_to_image
    assert VisFlowCallback is tf_raft_amd.training.VisFlowCallback and first_cycle_scaler(1) == 1.0
    assert 'out of scope' not in tf_raft_amd.training.__doc__


def test_shape_setter_checks_the_four_shapes():
    from tf_raft_amd.datasets import ShapeSetter
    f = ShapeSetter(2, (8, 16))
    good = (np.zeros((2, 8, 16, 3)), np.zeros((2, 8, 16, 3)), np.zeros((2, 8, 16, 2)), np.zeros((2, 8, 16)))
    out = f(*good)
    assert all(a is b for a, b in zip(out, good))
    for k, wrong in enumerate((np.zeros((2, 8, 15, 3)), np.zeros((1, 8, 16, 3)), np.zeros((2, 8, 16, 3)), np.zeros((2, 8, 16, 1)))):
        args = list(good)
        args[k] = wrong
        with pytest.raises(ValueError):
            f(*args)


def test_target_size_is_validated_at_construction():
    """The check runs before anything needs a device; a valid value then fails like every model does without a GPU."""
    import torch
    from tf_raft_amd.model import RAFT, SmallRAFT
    for cls in (RAFT, SmallRAFT):
        for bad in ((450, 1024), (448, 1020), (56, 1024), (448, 32), 'nearest', (448,), 448):
            with pytest.raises(ValueError, match='target_size'):
                cls(target_size=bad)
        assert cls._check_target_size((448, 1024)) == (448, 1024)
        assert cls._check_target_size('auto') == 'auto' and cls._check_target_size(None) is None
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            RAFT(target_size=(448, 1024))
    probe = RAFT.__new__(RAFT)
    for target, cases in (('auto', {(436, 1024): (440, 1024), (375, 1242): (376, 1248), (60, 90): (64, 96), (59, 155): (64, 160),
                                   (40, 90): (64, 96), (1, 1): (64, 64), (64, 96): (64, 96)}),
                          ((64, 96), {(70, 100): (64, 96), (10, 300): (64, 96)})):
        probe.target_size = target
        for frame, want in cases.items():
            assert probe._model_size(*frame) == want


def _decode_png(path):
    with open(path, 'rb') as f:
        data = f.read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff
        chunks.append((kind, body))
        pos += 12 + n
    assert [k for k, _ in chunks][0] == b'IHDR' and chunks[-1] == (b'IEND', b'')
    w, h, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b''.join(b for k, b in chunks if k == b'IDAT')), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()                                          # filter type 0 on every scanline
    return raw[:, 1:].reshape(h, w, 3)


def test_write_png_round_trips(tmp_path, rng):
    from tf_raft_amd.io import write_png
    for shape in ((5, 7, 3), (1, 1, 3), (33, 64, 3)):
        image = rng.integers(0, 256, size=shape, dtype=np.uint8)
        path = str(tmp_path / f'x{shape[0]}.png')
        write_png(path, image)
        np.testing.assert_array_equal(_decode_png(path), image)
        try:
            from PIL import Image
        except ImportError:
            continue
        with Image.open(path) as im:
            assert im.mode == 'RGB'
            np.testing.assert_array_equal(np.asarray(im), image)
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            write_png(str(tmp_path / 'bad.png'), bad)


def test_vis_flow_callback_surface(tmp_path):
    from tf_raft_amd.training import VisFlowCallback
    logdir = str(tmp_path / 'flows' / 'run')
    cb = VisFlowCallback([], target_size=(448, 1024), num_visualize=2, logdir=logdir)
    assert os.path.isdir(logdir) and cb.model is None and cb.target_size == (448, 1024) and not cb.choose_random
    with pytest.raises(RuntimeError):
        cb.on_epoch_end(0)
    sentinel = object()
    cb.set_model(sentinel)
    assert cb.model is sentinel
    cb.dataset = [(np.zeros((1, 8, 8, 3), np.uint8), np.zeros((1, 8, 8, 3), np.uint8))]
    with pytest.raises(ValueError, match='batched'):
        cb.on_epoch_end(0)

"""Frames of any size by interpolation (CPU side): the resize rule, the host tap tables, the C ABI of the resize entries and
the constructor's checks.

The yardstick of the rule is ``np_resize`` below: the separable bilinear resize with half-pixel centres (and the widened
triangle of ``antialias`` on a shrinking axis) restated in NumPy float64, pinned here against what can be EXECUTED --
``torch.nn.functional.interpolate(mode='bilinear', align_corners=False, antialias=...)`` on CPU float64.  TensorFlow's
``tf.image.resize(method='bilinear', antialias=...)`` is recalled to compute the same; it is not available to the tests.
tests/test_gpu_resize.py imports the restatement; it does not use the product's ``resize_taps``.

One detail of float64 itself shows at rows of 1242 pixels.  The rule's ``center = scale * (i + 0.5)`` is rounded once as a product;
torch's two-tap path (``antialias=False``) forms ``scale * (i + 0.5) - 0.5`` with ONE rounding (a fused multiply-add), its
antialias path rounds the product as the rule is written.  Half an ulp of a coordinate near 1242 is 1.1e-13, times a step of up to
255 between neighbouring samples: measured here, the rule as written and torch's two-tap path differ by 0.9e-11 .. 1.3e-11 at
(9, 1242) -> (8, 1248) depending on the random frame (2.8e-12 at (45, 200) -> (64, 96), under 1e-13 elsewhere), which straddles the
1e-11 asked of the comparison -- and an exact rational evaluation of the rule sits 2.5e-11 from torch in both modes, torch's own
rounding of ``scale``.  So ``np_taps(..., fused=True)`` evaluates the same rule with the centre rounded the way torch's two-tap path
rounds it (exact product, one rounding, through ``fractions``); it is used for the ``antialias=False`` comparison with torch only,
where it agrees to 1e-13, and ``test_fused_and_written_evaluations_are_one_rule`` ties it to the rule as written within the
rounding of one coordinate.  The rule as written (``fused=False``) is what the product's ``resize_taps`` and the kernels are held to.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from tf_raft_amd import _ffi

# (Hs, Ws) -> (Ht, Wt): what each exercises is listed in tests/test_gpu_resize.py
SHAPES = [((37, 53), (64, 72)), ((150, 201), (64, 88)), ((45, 200), (64, 96)), ((131, 67), (64, 64)), ((1, 5), (64, 64)),
          ((3, 5), (1, 1)), ((530, 70), (64, 64)), ((9, 1242), (8, 1248)), ((64, 96), (45, 200)), ((64, 88), (150, 201))]


def np_taps(n_in, n_out, antialias, fused=False):
    """One axis, output by output, in float64: [(first, weights)].  ``fused``: ``center - 0.5`` is the exactly computed
    ``scale * (i + 0.5) - 0.5`` rounded once, as a fused multiply-add gives it (the module's docstring)."""
    scale = n_in / n_out
    support = max(scale, 1.0) if antialias else 1.0
    inv = 1.0 / support
    taps = []
    for i in range(n_out):
        center = scale * (i + 0.5)
        first = max(int(center - support + 0.5), 0)
        last = min(int(center + support + 0.5), n_in)
        if fused:
            below = float(Fraction(scale) * Fraction(i + 0.5) - Fraction(1, 2))
            w = np.array([max(0.0, 1.0 - abs((j - below) * inv)) for j in range(first, last)], np.float64)
        else:
            w = np.array([max(0.0, 1.0 - abs((j - center + 0.5) * inv)) for j in range(first, last)], np.float64)
        taps.append((first, w / w.sum()))
    return taps


def np_axis_matrix(n_in, n_out, antialias, fused=False):
    m = np.zeros((n_out, n_in), np.float64)
    for i, (first, w) in enumerate(np_taps(n_in, n_out, antialias, fused)):
        m[i, first:first + len(w)] = w
    return m


def np_resize(x, ht, wt, antialias, factors=None, fused=False):
    """(..., H, W, C) -> (..., ht, wt, C) in float64; ``factors``: one multiplier per channel."""
    x = np.asarray(x, np.float64)
    my, mx = np_axis_matrix(x.shape[-3], ht, antialias, fused), np_axis_matrix(x.shape[-2], wt, antialias, fused)
    out = np.einsum('yh,...hwc->...ywc', my, x)
    out = np.einsum('xw,...ywc->...yxc', mx, out)
    return out if factors is None else out * np.asarray(factors, np.float64)


def np_max_taps(n_in, n_out, antialias):
    return max(len(w) for _, w in np_taps(n_in, n_out, antialias))


def _torch64(x, ht, wt, antialias):
    t = torch.from_numpy(np.asarray(x, np.float64)).permute(0, 3, 1, 2)
    out = torch.nn.functional.interpolate(t, size=(ht, wt), mode='bilinear', align_corners=False, antialias=antialias)
    return out.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize('antialias', [False, True])
def test_the_numpy_restatement_is_torch_float64_interpolate(antialias, rng):
    fused = not antialias                       # the rounding of the centre in torch's two-tap path (the module's docstring)
    worst = 0.0
    for n_in in range(1, 25):
        # one axis at a time, the other one two samples long and left alone (torch's antialias path does not take a width of 1)
        x = rng.uniform(0, 255, size=(1, n_in, 2, 1))
        xt = np.ascontiguousarray(x.transpose(0, 2, 1, 3))
        for n_out in range(1, 25):
            for f in {False, fused}:            # at these sizes the rule as written agrees as well
                worst = max(worst, np.abs(np_resize(x, n_out, 2, antialias, fused=f) - _torch64(x, n_out, 2, antialias)).max())
                worst = max(worst, np.abs(np_resize(xt, 2, n_out, antialias, fused=f) - _torch64(xt, 2, n_out, antialias)).max())
    assert worst <= 1e-11, worst
    for (hs, ws), (ht, wt) in SHAPES:
        x = rng.uniform(0, 255, size=(2, hs, ws, 3))
        want = _torch64(x, ht, wt, antialias)
        err = np.abs(np_resize(x, ht, wt, antialias, fused=fused) - want).max()
        written = np.abs(np_resize(x, ht, wt, antialias) - want).max()
        print(f'[resize] restatement vs torch float64 {(hs, ws)} -> {(ht, wt)} antialias={antialias}: {err:.2e} (centre rounded as written: {written:.2e})')
        assert err <= 1e-11, ((hs, ws), (ht, wt), err)
        # as written: within the rounding of one coordinate (half an ulp of the largest index) times the data's range, per axis
        assert written <= 1e-11 + 255 * 2.0 ** -52 * (hs + ws), ((hs, ws), (ht, wt), written)


def test_fused_and_written_evaluations_are_one_rule():
    """The two evaluations of the centre differ by one rounding of a number below n_in: at most 2^-53 n_in, so a triangle weight
    moves by at most that (the slope is at most 1) and a normalised row by at most three times it."""
    for antialias in (False, True):
        for n_in, n_out in [(s[k], t[k]) for s, t in SHAPES for k in (0, 1)] + [(24, 7), (7, 24), (1920, 1024), (448, 1080)]:
            d = np.abs(np_axis_matrix(n_in, n_out, antialias) - np_axis_matrix(n_in, n_out, antialias, fused=True)).max()
            assert d <= 3 * n_in * 2.0 ** -53, (n_in, n_out, antialias, d)


def test_plain_bilinear_is_two_taps_and_antialias_differs_only_where_an_axis_shrinks():
    for n_in, n_out in ((5, 9), (7, 7), (64, 150), (1, 4)):
        assert all(len(w) <= 2 for _, w in np_taps(n_in, n_out, False))
        for (f0, w0), (f1, w1) in zip(np_taps(n_in, n_out, False), np_taps(n_in, n_out, True)):
            assert f0 == f1 and np.array_equal(w0, w1)
    first, w = np_taps(5, 9, False)[0]
    assert first == 0 and list(w) == [1.0]                                # the clamped border: one tap of weight 1
    assert np_max_taps(150, 64, True) == 5 and np_max_taps(201, 88, True) == 5
    assert np_max_taps(530, 64, True) == 17
    assert np_max_taps(16 * 64, 64, True) <= 34                            # a shrink ratio of 16


def test_resize_taps_equal_the_restatement():
    from tf_raft_amd.image_ops import resize_taps
    pairs = [(a, b) for a in range(1, 25) for b in range(1, 25)]
    pairs += [(s[k], t[k]) for s, t in SHAPES for k in (0, 1)] + [(2160, 448), (3840, 1024), (1080, 448), (1920, 1024), (448, 1080), (1024, 64)]
    for antialias in (False, True):
        for n_in, n_out in pairs:
            first, count, w = resize_taps(n_in, n_out, antialias)
            want = np_taps(n_in, n_out, antialias)
            assert first.shape == count.shape == (n_out,) and w.shape == (n_out, max(len(v) for _, v in want)) and w.dtype == np.float64
            assert (w >= 0).all()
            for i, (f, v) in enumerate(want):
                assert (first[i], count[i]) == (f, len(v)), (n_in, n_out, antialias, i)
                assert np.abs(w[i, :len(v)] - v).max() <= 1e-15 and not w[i, len(v):].any()
                assert f + len(v) <= n_in
            # each quotient and each addition of a row's sum is rounded once: count roundings of at most eps / 2 each way
            assert (np.abs(w.sum(axis=1) - 1.0) <= count * np.finfo(np.float64).eps).all()
    for bad in ((0, 4), (4, 0), (-3, 2)):
        with pytest.raises(ValueError):
            resize_taps(*bad)


NEW_ENTRIES = ('raft_resize_f32', 'raft_resize_u8_f32')


def test_resize_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    good = [p, p, 1, 4, 4, 8, 8, 3, p, p, p, 2, p, p, p, 2, None, None]
    for name in NEW_ENTRIES:
        fn = getattr(lib, name)
        for k in (0, 1, 8, 9, 10, 12, 13, 14):                            # every pointer but the optional channel factors
            args = list(good)
            args[k] = None
            assert fn(*args) == -1, (name, k)
        for bad in ((0, 4, 4, 8, 8, 3), (1, 0, 4, 8, 8, 3), (1, 4, 0, 8, 8, 3), (1, 4, 4, 0, 8, 3), (1, 4, 4, 8, 0, 3),
                    (1, 4, 4, 8, 8, 0), (-2, 4, 4, 8, 8, 3), (1, 4, 4, 8, -8, 3)):
            args = list(good)
            args[2:8] = bad
            assert fn(*args) == -2, (name, bad)
        for bad in ((1, 4, 1 << 30, 8, 8, 3), (1, 4, 4, 8, 1 << 30, 3)):    # W * C does not fit an int
            args = list(good)
            args[2:8] = bad
            assert fn(*args) == -2, (name, bad)
        for k, taps in ((11, 0), (11, -1), (11, 65), (15, 0), (15, 65), (15, 1 << 20)):      # a tap count the kernel cannot take
            args = list(good)
            args[k] = taps
            assert fn(*args) == -2, (name, k, taps)
        args = list(good)
        args[7], args[15] = 64, 34                                       # 34 taps of 64 channels do not fit a wave's share of LDS
        assert fn(*args) == -2, name


def test_fit_is_validated_at_construction():
    """The checks run before anything needs a device; a valid combination then fails like every model does without a GPU."""
    from tf_raft_amd.model import RAFT, SmallRAFT
    for cls in (RAFT, SmallRAFT):
        for kw in ({'fit': 'bilinear', 'target_size': 'auto'}, {'fit': None, 'target_size': 'auto'}, {'fit': 'RESIZE', 'target_size': (64, 96)},
                   {'fit': 'nearest'}):
            with pytest.raises(ValueError, match='fit'):
                cls(**kw)
        with pytest.raises(ValueError, match='target_size'):
            cls(fit='resize')                                            # nothing to resize to
        with pytest.raises(ValueError, match='target_size'):
            cls(fit='resize', target_size=(60, 96))
        for bad in (None, 'yes', 2, 0.5):
            with pytest.raises(ValueError, match='antialias'):
                cls(fit='resize', target_size='auto', antialias=bad)
        assert cls._check_fit('crop_or_pad', True, None) == ('crop_or_pad', True)
        assert cls._check_fit('resize', False, (64, 96)) == ('resize', False)
        assert cls._check_fit('resize', np.True_, 'auto') == ('resize', True)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            RAFT(fit='resize', target_size=(448, 1024))

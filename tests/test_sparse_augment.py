"""SparseFlowAugmentor, host side (no GPU): the random draws against the reference's, the fixture's coverage, the collision rule of
the reference's scatter restated as a gather, the argument checks and the C ABI of the new entry.

The reference's augmentor.py runs UNMODIFIED under the stand-in cv2 / albumentations of tests/augstub
(tests/golden/make_sparse_augment_golden.py); what it did on the fixture's seeds is committed in
tests/golden/sparse_augment_golden.npz.  Where the reference tree is present the same is checked live, on more seeds; elsewhere
those tests skip and the fixture stands in.
"""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from tf_raft_amd import _ffi
from tf_raft_amd.augment import FlowAugmentor, SparseFlowAugmentor

sys.path.insert(0, GOLDEN)
import make_augment_golden as mk                                   # noqa: E402
import make_sparse_augment_golden as ms                            # noqa: E402

needs_reference = pytest.mark.skipif(not mk.reference_available(), reason='reference tree not present on this machine')

# the factors of the issue: downscales with hundreds of collisions, upscales with holes, 0.5 and 1.5 for the halves to even
FACTORS = (0.3333, 0.45, 0.5, 0.7071, 0.87, 0.9348, 1.0054, 1.2317, 1.4142, 1.5, 2.0)


def plain(rec):
    """A record as JSON holds it (tuples become lists; floats survive exactly)."""
    return json.loads(json.dumps(rec))


def product_draw(seed, H, W, do_flip, n=1):
    """``draw`` the way the fixture's cases were made: global np.random seeded, colour parameters from their own generator."""
    np.random.seed(seed)
    aug = SparseFlowAugmentor(ms.CROP, do_flip=do_flip, photo_rng=np.random.RandomState(seed + mk.PHOTO_SEED_OFFSET))
    return [plain(r) for r in aug.draw(H, W, n)], np.random.get_state()


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


def same_outputs(got, want, what):
    """By value, no tolerance; the reference's flow is float64 where it was multiplied by a list, `valid` int32 where resized."""
    for name in ms.NAMES:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape, (what, name)
        np.testing.assert_array_equal(g, w, err_msg=f'{name} {what}')


# ------------------------------------------------------------------ draws
def test_draw_reproduces_the_recorded_parameters_and_generator_state():
    cases = ms.load_fixture()
    assert [tuple(c[:4]) for c in cases] == [tuple(c) for c in ms.CASES]
    for H, W, seed, do_flip, rec, _, state in cases:
        got, got_state = product_draw(seed, H, W, do_flip)
        assert got == [rec], (H, W, seed)
        assert same_state(got_state, state), f'np.random is not where the reference left it (case {H}x{W} seed {seed})'


@needs_reference
def test_draw_and_the_numpy_chain_against_the_live_reference():
    """150 seeds per source size, with and without do_flip: parameters, generator state, and the step-by-step chain on the stand-ins
    against the reference's own outputs (so that tests/test_gpu_sparse_augment.py may use the chain where the reference is absent)."""
    for H, W in ms.SIZES:
        for seed in range(500, 650):
            do_flip = bool(seed % 2)
            outs, rec, state = ms.run_reference(seed, H, W, do_flip)
            got, got_state = product_draw(seed, H, W, do_flip)
            assert got == [plain(rec)], (H, W, seed)
            assert same_state(got_state, state)
            chain = ms.sparse_numpy_chain(rec, *ms.sparse_case_inputs(seed, H, W))
            for name in ms.NAMES:
                assert chain[name].dtype == outs[name].dtype, (name, H, W, seed)
            same_outputs(chain, outs, f'{H}x{W} seed {seed}')


@needs_reference
def test_the_fixture_is_what_the_reference_computes():
    for H, W, seed, do_flip, rec, outs, state in ms.load_fixture():
        live, live_rec, live_state = ms.run_reference(seed, H, W, do_flip)
        assert plain(live_rec) == rec and same_state(live_state, state)
        for name in ms.NAMES:
            assert live[name].dtype == outs[name].dtype
        same_outputs(live, outs, f'{H}x{W} seed {seed}')
    assert 'cv2' not in sys.modules and 'albumentations' not in sys.modules       # nobody else sees the stand-ins


def test_the_numpy_chain_reproduces_the_fixture():
    for H, W, seed, do_flip, rec, outs, _ in ms.load_fixture():
        same_outputs(ms.sparse_numpy_chain(rec, *ms.sparse_case_inputs(seed, H, W)), outs, f'{H}x{W} seed {seed}')


def test_fixture_coverage():
    """Asserted on what the reference did: its decoded records and its outputs."""
    cases = ms.load_fixture()
    cov = ms.coverage([ms.case_properties(rec, do_flip, outs, seed) for _, _, seed, do_flip, rec, outs, _ in cases])
    assert all(v > 0 for v in cov.values()), cov
    assert os.path.getsize(ms.FIXTURE) <= os.path.getsize(mk.FIXTURE)
    for _, _, _, _, rec, outs, _ in cases:
        assert outs['image1'].shape == (*ms.CROP, 3) and outs['image1'].dtype == np.uint8 and outs['image2'].dtype == np.uint8
        assert outs['flow'].shape == (*ms.CROP, 2) and outs['valid'].shape == ms.CROP
        assert outs['flow'].dtype == (np.float64 if rec['flip_h'] else np.float32)
        assert outs['valid'].dtype == (np.int32 if rec['resize'] else np.float32)
        assert set(np.unique(outs['valid']).tolist()) == {0, 1}
        if rec['resize']:
            assert not (outs['flow'][outs['valid'] == 0] != 0).any()         # zero flow where nothing landed
        assert (np.abs(outs['flow'][outs['valid'] == 1]) < 100).all()        # the -512 of invalid sources reaches no valid pixel
    # the strict `> 0`: a crop that holds resized column 0 has it invalid from top to bottom although valid sources land there
    shown = 0
    for H, W, seed, _, rec, outs, _ in cases:
        if rec['resize'] and rec['x0'] == 0 and not rec['flip_h']:
            valid = ms.sparse_case_inputs(seed, H, W)[3]
            lands = ms.landing(rec['scale_x'], W) == 0
            assert valid[:, lands].any() and not outs['valid'][:, 0].any()
            shown += 1
    assert shown


def test_a_batch_draw_equals_single_draws():
    H, W, n = 120, 160, 5
    batch, state = product_draw(31, H, W, True, n)
    np.random.seed(31)
    aug = SparseFlowAugmentor(ms.CROP, do_flip=True, photo_rng=np.random.RandomState(31 + mk.PHOTO_SEED_OFFSET))
    singles = [plain(aug.draw(H, W)[0]) for _ in range(n)]
    assert batch == singles and same_state(state, np.random.get_state())
    assert len({json.dumps(r) for r in batch}) == n                     # and the samples differ
    np.random.seed(5)
    before = np.random.get_state()
    own = SparseFlowAugmentor(ms.CROP, do_flip=True, rng=np.random.RandomState(31), photo_rng=np.random.RandomState(31 + mk.PHOTO_SEED_OFFSET))
    assert [plain(r) for r in own.draw(H, W, n)] == batch
    assert same_state(before, np.random.get_state())                    # a RandomState of its own leaves the global generator alone


def test_draw_keeps_the_drawn_origin_next_to_the_clipped_one():
    aug = SparseFlowAugmentor(ms.CROP, rng=np.random.RandomState(2))
    recs = aug.draw(120, 160, 300)
    for r in recs:
        H1, W1 = r['size']
        assert -50 <= r['x0_drawn'] < W1 - 96 + 50 and 0 <= r['y0_drawn'] < H1 - 64 + 20
        assert r['x0'] == min(max(r['x0_drawn'], 0), W1 - 96) and r['y0'] == min(max(r['y0_drawn'], 0), H1 - 64)
        assert r['scale_x'] == r['scale_y'] and not r['flip_h'] and not r['flip_v'] and r['photo'][0] is r['photo'][1]
        assert (H1, W1) == ((int(round(120 * r['scale_y'])), int(round(160 * r['scale_x']))) if r['resize'] else (120, 160))
    assert any(r['x0_drawn'] < 0 for r in recs) and any(r['x0_drawn'] > r['size'][1] - 96 for r in recs)
    assert any(r['y0_drawn'] > r['size'][0] - 64 for r in recs)


def test_constructor_carries_the_reference_attributes():
    aug = SparseFlowAugmentor((288, 960))
    want = dict(crop_size=(288, 960), min_scale=-0.2, max_scale=0.5, spatial_aug_prob=0.8, stretch_prob=0.8, max_stretch=0.2,
                do_flip=False, h_flip_prob=0.5, v_flip_prob=0.1, asymmetric_color_aug_prob=0.2, eraser_aug_prob=0.5)
    for k, v in want.items():
        assert getattr(aug, k) == v, k
    pa = aug.photo_aug
    assert (pa.brightness_limit, pa.contrast_limit, pa.hue_shift_limit, pa.sat_shift_limit, pa.val_shift_limit, pa.p) == (0.3, 0.3, 17, 76, 0, 0.5)
    flip = SparseFlowAugmentor((64, 96), do_flip=True, rng=np.random.RandomState(0)).draw(120, 160, 40)
    assert any(r['flip_h'] for r in flip) and not all(r['flip_h'] for r in flip) and not any(r['flip_v'] for r in flip)


@needs_reference
def test_constructor_attributes_equal_the_reference_objects():
    ref = mk.load_reference().augmentor.SparseFlowAugmentor((288, 960))
    aug = SparseFlowAugmentor((288, 960))
    for k, v in vars(ref).items():
        if k == 'photo_aug':
            bc, hsv = v.transforms
            assert bc.brightness_limit == (-aug.photo_aug.brightness_limit, aug.photo_aug.brightness_limit)
            assert bc.contrast_limit == (-aug.photo_aug.contrast_limit, aug.photo_aug.contrast_limit)
            assert [hi for _, hi in hsv.limits] == [aug.photo_aug.hue_shift_limit, aug.photo_aug.sat_shift_limit, aug.photo_aug.val_shift_limit]
        else:
            assert getattr(aug, k) == v, k


# ------------------------------------------------------------------ the collision rule
def gather(flow, valid, f):
    """The scatter of ``resize_sparse_flow_map`` as a gather, the way the kernel computes it: per target the
    candidate sources ``floor(X / f) - r .. ceil(X / f) + r``, ``r = ceil(0.5 / f) + 1``, each tested with the forward formula; of the
    valid sources in the rectangle the one with the largest row, then the largest column."""
    H, W = valid.shape
    f = np.float64(f)
    H1, W1 = int(round(H * f)), int(round(W * f))
    r = int(math.ceil(0.5 / f)) + 1

    def sources(target, size):
        lo, hi = int(math.floor(target / f)) - r, int(math.ceil(target / f)) + r
        return [s for s in range(max(lo, 0), min(hi, size - 1) + 1) if int(np.rint(np.float64(np.float32(s)) * f)) == target]

    cols = [sources(X, W) for X in range(W1)]
    rows = [sources(Y, H) for Y in range(H1)]
    out_flow, out_valid = np.zeros((H1, W1, 2), np.float32), np.zeros((H1, W1), np.int32)
    for Y in range(1, H1):
        for X in range(1, W1):
            win = next(((y, x) for y in reversed(rows[Y]) for x in reversed(cols[X]) if valid[y, x] >= 1), None)
            if win is not None:
                out_flow[Y, X] = (flow[win].astype(np.float64) * f).astype(np.float32)
                out_valid[Y, X] = 1
    return out_flow, out_valid


@pytest.mark.parametrize('f', FACTORS)
def test_the_gather_equals_the_scatter_of_the_installed_numpy(f):
    """Which of several sources on one target stays is NumPy's assignment order in ``flow_img[yy, xx] = flow1``: the last one.  This
    pins the rule the kernel restates to the NumPy that is installed."""
    rs = np.random.RandomState(int(f * 10000))
    H, W = 46, 61
    flow = rs.normal(scale=20, size=(H, W, 2)).astype(np.float32)
    valid = (rs.rand(H, W) < 0.6).astype(np.float32)
    valid[rs.rand(H, W) < 0.05] = 0.5                                    # below 1: not valid
    valid[rs.rand(H, W) < 0.05] = 2.0                                    # above 1: valid
    flow[valid < 1] = np.nan                                             # nothing of an invalid source may arrive
    want_flow, want_valid = ms.scatter(flow, valid, np.float64(f))
    got_flow, got_valid = gather(flow, valid, f)
    np.testing.assert_array_equal(got_valid, want_valid)
    assert got_flow.tobytes() == want_flow.tobytes()
    assert not np.isnan(want_flow).any()
    # the case is not empty: collisions below 1, holes above
    tx, ty = ms.landing(f, W), ms.landing(f, H)
    keys = (ty[:, None] * 100000 + tx[None, :])[valid >= 1]
    if f < 1:
        assert len(keys) - len(np.unique(keys)) >= (100 if f < 0.9 else 10)
    if f > 1.2:
        assert (want_valid[1:, 1:] == 0).sum() >= 100


@needs_reference
@pytest.mark.parametrize('f', FACTORS)
def test_the_scatter_helper_is_the_reference_method(f):
    rs = np.random.RandomState(7)
    flow = rs.normal(scale=20, size=(46, 61, 2)).astype(np.float32)
    valid = (rs.rand(46, 61) < 0.6).astype(np.float32)
    ref = mk.load_reference().augmentor.SparseFlowAugmentor((8, 8))
    want = ref.resize_sparse_flow_map(flow, valid, fx=np.float64(f), fy=np.float64(f))
    got = ms.scatter(flow, valid, np.float64(f))
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()


# ------------------------------------------------------------------ arguments
def test_bad_arguments_raise_value_error_before_any_launch():
    """No GPU here: anything that got past the checks would fail for want of a device, with another exception."""
    aug = SparseFlowAugmentor((64, 96), rng=np.random.RandomState(0))
    i = np.zeros((2, 120, 160, 3), np.uint8)
    f = np.zeros((2, 120, 160, 2), np.float32)
    v = np.ones((2, 120, 160), np.float32)
    state = aug.rng.get_state()
    for H, W in ((63, 160), (120, 95), (60, 90)):                       # the source is smaller than the crop
        with pytest.raises(ValueError):
            aug.draw(H, W)
        with pytest.raises(ValueError):
            aug(np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 2), np.float32), np.ones((H, W), np.float32))
    bad = [(i.astype(np.float32), i, f, v), (i, i, f.astype(np.float64), v), (i, i, f, v.astype(np.float64)), (i, i, f, v > 0),     # dtypes
           (i, i, f, v[..., None]), (i, i, f, v[:, :100]), (i, i, f, v[0]), (i[0], i[0], f[0], v), (i, i[:, :100], f, v)]          # shapes
    for args in bad:
        with pytest.raises(ValueError):
            aug.batch(*args)
        with pytest.raises(ValueError):
            aug.apply(aug.draw(120, 160, 2), *args)
    with pytest.raises(TypeError):
        aug.batch(i, i, f)                                              # the validity map is not optional
    with pytest.raises(ValueError):
        aug.apply(aug.draw(120, 160, 3), i, i, f, v)                    # three records for two samples
    with pytest.raises(ValueError):
        aug.apply(aug.draw(100, 160, 2), i, i, f, v)                    # records drawn for another source size
    # records the sparse kernel cannot serve
    rec = aug.draw(120, 160)[0]
    for change in ({'scale_y': rec['scale_x'] * 1.5}, {'flip_v': True}, {'resize': True, 'scale_x': 0.12, 'scale_y': 0.12},
                   {'photo': (rec['photo'][0], {'bc': (1.1, 0.0), 'hsv': None})}, {'x0': -1}):
        with pytest.raises(ValueError):
            aug.apply([{**rec, **change}], i[0], i[0], f[0], v[0])
    aug.rng.set_state(state)
    with pytest.raises(ValueError):
        aug.draw(63, 96)
    # a factor below 1/8 is refused before anything is drawn: 2 ** -3.5 on a source whose size lets it through
    low = SparseFlowAugmentor((8, 8), min_scale=-3.5, max_scale=0.0, rng=aug.rng)
    with pytest.raises(ValueError):
        low.draw(400, 400)
    with pytest.raises(ValueError):
        low.batch(np.zeros((400, 400, 3), np.uint8), np.zeros((400, 400, 3), np.uint8), np.zeros((400, 400, 2), np.float32), np.ones((400, 400), np.float32))
    assert same_state(aug.rng.get_state(), state)                       # a refused call draws nothing
    assert len(low.draw(60, 60)) == 1                                   # there (8 + 1) / 60 keeps the factor above 1/8
    # a source of the crop's own size is legal: every resize enlarges it, and the origin is clipped to 0
    for r in SparseFlowAugmentor((64, 96), rng=np.random.RandomState(1)).draw(64, 96, 50):
        assert (r['y0'], r['x0']) == (0, 0) or r['resize']
        assert r['size'][0] >= 64 and r['size'][1] >= 96


def test_the_dense_augmentor_is_untouched_by_the_shared_host_code():
    """The same records, byte for byte, for both classes where they mean the same, and the dense class takes no validity map."""
    dense = FlowAugmentor((64, 96), rng=np.random.RandomState(3), photo_rng=np.random.RandomState(4))
    sparse = SparseFlowAugmentor((64, 96), rng=np.random.RandomState(3), photo_rng=np.random.RandomState(4))
    rec = sparse.draw(120, 160)[0]
    assert dense._records([rec], 120, 160) == sparse._records([rec], 120, 160)
    assert len(dense._records([rec], 120, 160)) == C.sizeof(_ffi.AugmentParams) == 168
    with pytest.raises(TypeError):
        dense.apply([rec], None, None, None, None)


# ------------------------------------------------------------------ C ABI
def test_the_sparse_entry_is_declared_exported_and_mirrored():
    """The sparse entry shares the dense one's record (its prototype: tests/test_host_logic.py test_the_binding_is_the_header)."""
    assert _ffi.load_library().raft_augment_params_bytes() == C.sizeof(_ffi.AugmentParams) == 168


def test_sparse_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    for k in range(10):
        args = [p] * 10
        args[k] = None
        assert lib.raft_augment_gather_sparse_u8(*args, 1, 8, 8, 4, 4, None) == -1, k
    for bad in ((0, 8, 8, 4, 4), (1, 0, 8, 4, 4), (1, 8, 0, 4, 4), (1, 8, 8, 0, 4), (1, 8, 8, 4, 0), (1, 8, 8, -4, 4), (1, 4097, 4096, 4, 4),
                (1, 8, 8, 4097, 4096), (70000, 8, 8, 4, 4)):
        assert lib.raft_augment_gather_sparse_u8(*([p] * 10), *bad, None) == -2, bad


def test_the_sparse_kernel_is_in_the_unit_the_disassembly_test_reads_and_uses_no_scratch_and_no_atomics(tmp_path):
    from tf_raft_amd import build
    asm = str(tmp_path / 'augment.s')
    subprocess.run([build._hipcc(), *build.FLAGS, '--cuda-device-only', '-S', '-x', 'hip', os.path.join(build.CSRC, 'augment.hip'), '-o', asm],
                   check=True, capture_output=True)
    with open(asm) as f:
        text = f.read()
    assert 'augment_gather_sparse_kernel' in text
    assert not re.findall(r'^\s*\w*atomic\w*', text, flags=re.M)
    scratch = re.findall(r'\.private_segment_fixed_size:\s+(\d+)', text[text.index('amdhsa.kernels'):])
    assert len(scratch) == 3 and all(int(s) == 0 for s in scratch), scratch          # the sums kernel and the two gathers


# ------------------------------------------------------------------ names
def test_reference_import_line_resolves_and_the_product_needs_no_stand_in():
    from tf_raft.datasets.augmentor import FlowAugmentor as dense, SparseFlowAugmentor as shim      # reference dataset.py:11
    from tf_raft.datasets import SparseFlowAugmentor as exported
    assert shim is SparseFlowAugmentor and exported is SparseFlowAugmentor and dense is FlowAugmentor
    code = ('import sys; from tf_raft.datasets.augmentor import FlowAugmentor, SparseFlowAugmentor; '
            'assert "cv2" not in sys.modules and "albumentations" not in sys.modules; print("clean")')
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and 'clean' in out.stdout, out.stderr

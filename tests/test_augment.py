"""FlowAugmentor, host side (no GPU): the random draws against the reference's, the fixture's coverage, the argument checks and
the C ABI of the two kernels.

The reference's augmentor.py runs UNMODIFIED under the stand-in cv2 / albumentations of tests/augstub
(tests/golden/make_augment_golden.py); what it did on the fixture's seeds is committed in tests/golden/augment_golden.npz.
Where the reference tree is present the same is checked live, on more seeds; elsewhere those tests skip and the fixture stands in.
What the stand-ins compute is the restatement of DESIGN.md section 10 -- agreement with the real OpenCV is not claimed here.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from tf_raft_amd import _ffi
from tf_raft_amd.augment import FlowAugmentor

sys.path.insert(0, GOLDEN)
import make_augment_golden as mk                                   # noqa: E402

needs_reference = pytest.mark.skipif(not mk.reference_available(), reason='reference tree not present on this machine')


def plain(rec):
    """A record as JSON holds it (tuples become lists; floats survive exactly)."""
    return json.loads(json.dumps(rec))


def product_draw(seed, H, W, n=1):
    """``draw`` the way the fixture's cases were made: global np.random seeded, colour parameters from their own generator."""
    np.random.seed(seed)
    aug = FlowAugmentor(mk.CROP, photo_rng=np.random.RandomState(seed + mk.PHOTO_SEED_OFFSET))
    return [plain(r) for r in aug.draw(H, W, n)], np.random.get_state()


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


# ------------------------------------------------------------------ draws
def test_draw_reproduces_the_recorded_parameters_and_generator_state():
    cases = mk.load_fixture()
    assert [tuple(c[:3]) for c in cases] == [tuple(c) for c in mk.CASES]
    for H, W, seed, rec, _, state in cases:
        got, got_state = product_draw(seed, H, W)
        assert got == [rec], (H, W, seed)
        assert same_state(got_state, state), f'np.random is not where the reference left it (case {H}x{W} seed {seed})'


@needs_reference
def test_draw_and_the_numpy_chain_against_the_live_reference():
    """24 seeds per source size: parameters, generator state, and the step-by-step chain on the stand-ins against the reference's
    own outputs (so that tests/test_gpu_augment.py may use the chain where the reference tree is absent)."""
    for H, W in ((120, 160), (96, 128)):
        for seed in range(200, 224):
            outs, rec, state = mk.run_reference(seed, H, W)
            got, got_state = product_draw(seed, H, W)
            assert got == [plain(rec)], (H, W, seed)
            assert same_state(got_state, state)
            chain = mk.numpy_chain(rec, *mk.case_inputs(seed, H, W))
            for name in ('image1', 'image2', 'flow', 'valid'):
                assert chain[name].dtype == outs[name].dtype
                np.testing.assert_array_equal(chain[name], outs[name], err_msg=f'{name} {H}x{W} seed {seed}')


@needs_reference
def test_the_fixture_is_what_the_reference_computes():
    for H, W, seed, rec, outs, state in mk.load_fixture():
        live, live_rec, live_state = mk.run_reference(seed, H, W)
        assert plain(live_rec) == rec and same_state(live_state, state)
        for name in ('image1', 'image2', 'flow', 'valid'):
            assert live[name].dtype == outs[name].dtype
            np.testing.assert_array_equal(live[name], outs[name])
        assert os.path.realpath(mk.load_reference().augmentor.__file__).startswith(os.path.realpath(mk.reference_root()))
    assert 'cv2' not in sys.modules and 'albumentations' not in sys.modules       # nobody else sees the stand-ins


def test_the_numpy_chain_reproduces_the_fixture():
    for H, W, seed, rec, outs, _ in mk.load_fixture():
        chain = mk.numpy_chain(rec, *mk.case_inputs(seed, H, W))
        for name in ('image1', 'image2', 'flow', 'valid'):
            np.testing.assert_array_equal(chain[name], outs[name], err_msg=f'{name} {H}x{W} seed {seed}')


def test_fixture_coverage():
    cases = mk.load_fixture()
    cov = mk.coverage([c[3] for c in cases])
    assert all(v > 0 for v in cov.values()), cov
    assert os.path.getsize(mk.FIXTURE) <= os.path.getsize(os.path.join(GOLDEN, 'reference_forward_golden.npz'))
    for _, _, _, rec, outs, _ in cases:
        assert outs['image1'].shape == (*mk.CROP, 3) and outs['image1'].dtype == np.uint8 and outs['image2'].dtype == np.uint8
        assert outs['flow'].shape == (*mk.CROP, 2) and outs['valid'].shape == mk.CROP
        # the reference's flow is float64 whenever it was multiplied by a list (resize or flip), float32 otherwise
        assert outs['flow'].dtype == (np.float64 if rec['resize'] or rec['flip_h'] or rec['flip_v'] else np.float32)
    assert any(0 < c[4]['valid'].mean() < 1 for c in cases)            # `valid` is exercised with both values


def test_a_batch_draw_equals_single_draws():
    H, W, n = 120, 160, 5
    batch, state = product_draw(31, H, W, n)
    np.random.seed(31)
    aug = FlowAugmentor(mk.CROP, photo_rng=np.random.RandomState(31 + mk.PHOTO_SEED_OFFSET))
    singles = [plain(aug.draw(H, W)[0]) for _ in range(n)]
    assert batch == singles and same_state(state, np.random.get_state())
    assert len({json.dumps(r) for r in batch}) == n                     # and the samples differ
    # a RandomState of its own leaves the global generator alone
    np.random.seed(5)
    before = np.random.get_state()
    own = FlowAugmentor(mk.CROP, rng=np.random.RandomState(31), photo_rng=np.random.RandomState(31 + mk.PHOTO_SEED_OFFSET))
    assert [plain(r) for r in own.draw(H, W, n)] == batch
    assert same_state(before, np.random.get_state())


def test_constructor_carries_the_reference_attributes():
    aug = FlowAugmentor((368, 496))
    want = dict(crop_size=(368, 496), min_scale=-0.2, max_scale=0.5, spatial_aug_prob=0.8, stretch_prob=0.8, max_stretch=0.2,
                do_flip=True, h_flip_prob=0.5, v_flip_prob=0.1, asymmetric_color_aug_prob=0.2, eraser_aug_prob=0.5)
    for k, v in want.items():
        assert getattr(aug, k) == v, k
    pa = aug.photo_aug
    assert (pa.brightness_limit, pa.contrast_limit, pa.hue_shift_limit, pa.sat_shift_limit, pa.val_shift_limit, pa.p) == (0.4, 0.4, 28, 102, 0, 0.5)
    no_flip = FlowAugmentor((64, 96), do_flip=False, rng=np.random.RandomState(0))
    assert not any(r['flip_h'] or r['flip_v'] for r in no_flip.draw(120, 160, 40))


def test_bad_arguments_raise_value_error_before_any_launch():
    """No GPU here: anything that got past the checks would fail for want of a device, with another exception."""
    aug = FlowAugmentor((64, 96), rng=np.random.RandomState(0))
    i = np.zeros((2, 120, 160, 3), np.uint8)
    f = np.zeros((2, 120, 160, 2), np.float32)
    state = aug.rng.get_state()
    for H, W in ((64, 160), (120, 96), (60, 90)):                       # the crop does not fit the source
        with pytest.raises(ValueError):
            aug.draw(H, W)
        with pytest.raises(ValueError):
            aug(np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 2), np.float32))
    bad = [(i.astype(np.float32), i, f), (i, i.astype(np.int32), f), (i, i, f.astype(np.float64)),        # dtypes
           (i[..., :2], i[..., :2], f), (i, i, f[..., :1]), (i[0, 0], i[0, 0], f[0, 0]), (i[:, :0], i[:, :0], f[:, :0]),   # shapes
           (i, i[:, :100], f), (i, i, f[:, :, :150]), (i, i[:1], f), (i[0], i[0], f)]                       # mixed sizes
    for args in bad:
        with pytest.raises(ValueError):
            aug.batch(*args)
        with pytest.raises(ValueError):
            aug.apply(aug.draw(120, 160, 2), *args)
    import torch
    with pytest.raises(ValueError):
        aug.batch(torch.zeros((120, 160, 3)), torch.zeros((120, 160, 3), dtype=torch.uint8), torch.zeros((120, 160, 2)))
    with pytest.raises(ValueError):
        aug.apply(aug.draw(120, 160, 3), i, i, f)                       # three records for two samples
    with pytest.raises(ValueError):
        aug.apply(aug.draw(100, 160, 2), i, i, f)                       # records drawn for another source size
    with pytest.raises(ValueError):
        aug.draw(120, 160, 0)
    with pytest.raises(ValueError):
        FlowAugmentor((64,))
    aug.rng.set_state(state)
    with pytest.raises(ValueError):
        aug.draw(64, 96)
    assert same_state(aug.rng.get_state(), state)                       # a refused call draws nothing


# ------------------------------------------------------------------ C ABI
def test_augment_entries_are_declared_exported_and_mirrored():
    """The record: same fields in the same order, same size (the prototypes: tests/test_host_logic.py test_the_binding_is_the_header)."""
    with open(os.path.join(ROOT, 'include', 'raft_hip.h')) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    lib = _ffi.load_library()
    body = re.search(r'typedef struct \{(.*?)\} RaftAugmentParams;', header, flags=re.S).group(1)
    fields = [re.sub(r'\[.*', '', n.strip()) for line in body.split(';') if line.strip()
              for n in line.strip().split(None, 1)[1].split(',')]
    assert fields == [n for n, _ in _ffi.AugmentParams._fields_]
    assert lib.raft_augment_params_bytes() == C.sizeof(_ffi.AugmentParams) == 168
    assert int(re.search(r'#define RAFT_AUGMENT_SUM_BLOCKS (\d+)', header).group(1)) == _ffi.AUGMENT_SUM_BLOCKS


def test_augment_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    for k in range(3):
        args = [p, p, p]
        args[k] = None
        assert lib.raft_augment_sums_u8(*args, 1, 8, 8, None) == -1
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, 8, -8), (1, 4097, 4096), (70000, 8, 8)):
        assert lib.raft_augment_sums_u8(p, p, p, *bad, None) == -2, bad
    for k in range(9):
        args = [p] * 9
        args[k] = None
        assert lib.raft_augment_gather_u8(*args, 1, 8, 8, 4, 4, None) == -1, k
    for bad in ((0, 8, 8, 4, 4), (1, 0, 8, 4, 4), (1, 8, 0, 4, 4), (1, 8, 8, 0, 4), (1, 8, 8, 4, 0), (1, 8, 8, -4, 4), (1, 4097, 4096, 4, 4),
                (1, 8, 8, 4097, 4096), (70000, 8, 8, 4, 4)):
        assert lib.raft_augment_gather_u8(*([p] * 9), *bad, None) == -2, bad


def test_the_kernels_contract_nothing_into_fused_multiply_adds(tmp_path):
    """Every result is to be reproducible with individually rounded operations: the only fused operations allowed in the code
    object are the double-precision ones of the correctly rounded division that fills the colour tables."""
    from tf_raft_amd import build
    hipcc = build._hipcc()
    asm = str(tmp_path / 'augment.s')
    subprocess.run([hipcc, *build.FLAGS, '--cuda-device-only', '-S', '-x', 'hip', os.path.join(build.CSRC, 'augment.hip'), '-o', asm],
                   check=True, capture_output=True)
    with open(asm) as f:
        text = f.read()
    assert 'augment_gather_kernel' in text and 'augment_sums_kernel' in text
    fused = re.findall(r'^\s*(v_(?:pk_)?(?:fma|fmac|mad|mac)\w*f(?:16|32)\w*|v_dot\w*)', text, flags=re.M)
    assert not fused, sorted(set(fused))
    fused64 = len(re.findall(r'^\s*v_(?:fma|fmac)_f64', text, flags=re.M))
    divisions = len(re.findall(r'^\s*v_div_fmas_f64', text, flags=re.M))
    assert divisions > 0 and fused64 == 5 * divisions, (fused64, divisions)      # five per division, nothing else


# ------------------------------------------------------------------ names
def test_reference_import_line_resolves_and_the_product_needs_no_stand_in():
    from tf_raft.datasets.augmentor import FlowAugmentor as shim      # reference tf_raft/datasets/dataset.py:11
    from tf_raft.datasets import FlowAugmentor as exported
    assert shim is FlowAugmentor and exported is FlowAugmentor
    code = ('import sys; import tf_raft_amd.augment, tf_raft.datasets.augmentor; '
            'assert "cv2" not in sys.modules and "albumentations" not in sys.modules; print("clean")')
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and 'clean' in out.stdout, out.stderr
    for path in ('tf_raft_amd/augment.py', 'tf_raft/datasets/augmentor.py'):
        with open(os.path.join(ROOT, path)) as f:
            assert not re.search(r'^\s*(import|from)\s+(cv2|albumentations)\b', f.read(), flags=re.M)

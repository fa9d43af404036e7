"""Generates tests/golden/augment_golden.npz: the REFERENCE's own FlowAugmentor (tf_raft/datasets/augmentor.py, loaded unmodified
under the stand-in cv2 / albumentations of tests/augstub) run on seeded samples, with the parameters it used.
Run where the reference tree is present:
    python tests/golden/make_augment_golden.py

Per case: the outputs (two uint8 crops, the flow as the float64 array the reference returns, `valid` by dataset.py:102), the
parameter record decoded from the reference's own np.random calls, and np.random's final state.  The inputs are regenerated from
the seed (`case_inputs`), not stored.  tests/test_augment.py and tests/test_gpu_augment.py import the helpers below.
"""
import contextlib
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
STUB_DIR = os.path.join(ROOT, 'tests', 'augstub')
FIXTURE = os.path.join(HERE, 'augment_golden.npz')
CROP = (64, 96)
# (source height, width, seed).  Chosen by `python tests/golden/make_augment_golden.py --scan` to cover the list in `coverage`
# with few cases; on 96 x 128 frames the minimum scale (crop + 8) / source = 0.8125 clips most draws.
CASES = ((96, 128, 63), (96, 128, 1134), (120, 160, 11), (120, 160, 76), (120, 160, 2), (120, 160, 3))
PHOTO_SEED_OFFSET = 7919        # the colour parameters of case `seed` come from RandomState(seed + PHOTO_SEED_OFFSET)
_STUB_MODULES = ('cv2', 'albumentations')


def reference_root():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import reference_runner
    return reference_runner.REFERENCE_ROOT


def reference_available():
    # the reference's file imports PIL as well (unused by FlowAugmentor): the real one, where it is installed
    return os.path.isfile(os.path.join(reference_root(), 'tf_raft', 'datasets', 'augmentor.py')) and importlib.util.find_spec('PIL') is not None


@contextlib.contextmanager
def _stub_on_path():
    saved = {k: v for k, v in sys.modules.items() if k.split('.')[0] in _STUB_MODULES}
    for k in saved:
        del sys.modules[k]
    dont_write = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    sys.path.insert(0, STUB_DIR)
    try:
        yield
    finally:
        sys.path.remove(STUB_DIR)
        sys.dont_write_bytecode = dont_write
        for k in [k for k in sys.modules if k.split('.')[0] in _STUB_MODULES]:
            del sys.modules[k]
        sys.modules.update(saved)


_loaded = None
_stubs = None


def load_reference():
    """-> namespace: .augmentor (the reference's module, its source untouched), .cv2 and .albumentations (the stand-ins it runs on)."""
    global _loaded
    if _loaded is None:
        path = os.path.join(reference_root(), 'tf_raft', 'datasets', 'augmentor.py')
        with _stub_on_path():
            spec = importlib.util.spec_from_file_location('_reference_augmentor', path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            _loaded = types.SimpleNamespace(augmentor=mod, cv2=sys.modules['cv2'], albumentations=sys.modules['albumentations'])
        assert os.path.realpath(mod.__file__) == os.path.realpath(path)
    return _loaded


def load_stubs():
    """The stand-in (cv2, albumentations) modules alone -- no reference tree needed."""
    global _stubs
    if _loaded is not None:
        return _loaded.cv2, _loaded.albumentations
    if _stubs is None:
        with _stub_on_path():
            import albumentations
            import cv2
            _stubs = (cv2, albumentations)
    return _stubs


def numpy_chain(rec, img1, img2, flow, crop=CROP):
    """The reference's chain for GIVEN parameters, step by step on the stand-ins: colour map, erase on the source, resize, flips,
    crop, flow factors (augmentor.py:42-129) and `valid` (dataset.py:102).  tests/test_augment.py pins it to the reference's own
    run; tests/test_gpu_augment.py uses it as the yardstick for cases beyond the fixture (the reference tree does not travel)."""
    cv2, A = load_stubs()
    bc, hsv = A.RandomBrightnessContrast(), A.HueSaturationValue()
    frames = []
    for img, ph in zip((img1, img2), rec['photo']):
        img = img.copy()
        if ph['bc'] is not None:
            img = bc.apply(img, *ph['bc'])
        if ph['hsv'] is not None:
            img = hsv.apply(img, *ph['hsv'])
        frames.append(img)
    img1, img2 = frames
    if rec['rects']:
        mean_color = np.mean(img2.reshape(-1, 3), axis=0)
        for x0, y0, dx, dy in rec['rects']:
            img2[y0:y0 + dy, x0:x0 + dx, :] = mean_color
    if rec['resize']:
        fx, fy = rec['scale_x'], rec['scale_y']
        img1, img2, flow = (cv2.resize(a, None, fx=fx, fy=fy, interpolation=cv2.INTER_LINEAR) for a in (img1, img2, flow))
        flow = flow * [fx, fy]
    if rec['flip_h']:
        img1, img2, flow = img1[:, ::-1], img2[:, ::-1], flow[:, ::-1] * [-1.0, 1.0]
    if rec['flip_v']:
        img1, img2, flow = img1[::-1, :], img2[::-1, :], flow[::-1, :] * [1.0, -1.0]
    y0, x0 = rec['y0'], rec['x0']
    img1, img2, flow = (np.ascontiguousarray(a[y0:y0 + crop[0], x0:x0 + crop[1]]) for a in (img1, img2, flow))
    valid = (np.abs(flow[:, :, 0]) < 1000) * (np.abs(flow[:, :, 1]) < 1000)
    return {'image1': img1, 'image2': img2, 'flow': flow, 'valid': valid.astype(np.float32)}


class _RecordingRandom:
    """``np.random`` as the reference module sees it while a case runs: every call goes to the real global generator and is noted."""

    def __init__(self):
        self.trace = []

    def __getattr__(self, name):
        fn = getattr(np.random, name)

        def call(*args):
            out = fn(*args)
            self.trace.append((name, args, out))
            return out
        return call


class _NumpyProxy:
    def __init__(self, random):
        self.random = random

    def __getattr__(self, name):
        return getattr(np, name)


def case_inputs(seed, H, W):
    """Smooth frames with detail, a smooth flow with a block of invalid (> 1000) vectors: regenerated, never stored."""
    rs = np.random.RandomState(100000 + seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')

    def frame():
        ph = rs.uniform(0, 6.28, (3, 3))
        fr = rs.uniform(0.02, 0.25, (3, 3))
        chans = [127.5 + 70 * np.sin(fr[c, 0] * xx + ph[c, 0]) * np.cos(fr[c, 1] * yy + ph[c, 1]) + 50 * np.sin(fr[c, 2] * (xx + yy) + ph[c, 2])
                 for c in range(3)]
        img = np.stack(chans, -1) + rs.randint(-3, 4, (H, W, 3))
        return np.clip(np.rint(img), 0, 255).astype(np.uint8)

    img1, img2 = frame(), frame()
    flow = np.stack([12 * np.sin(0.05 * xx + 0.03 * yy), 9 * np.cos(0.04 * yy - 0.02 * xx)], -1) + rs.normal(scale=0.5, size=(H, W, 2))
    flow = flow.astype(np.float32)
    by, bx = rs.randint(0, H - 24), rs.randint(0, W - 32)
    flow[by:by + 24, bx:bx + 32] = (1.5e3, -2.5e3)
    flow[by + 4:by + 8, bx:bx + 32, 1] = 3.0
    return img1, img2, flow


def decode(trace, photo, H, W, crop):
    """The reference's np.random calls of one sample (augmentor.py:42-118, in order) -> the record ``FlowAugmentor.draw`` returns."""
    t = list(trace)

    def take(name, *args):
        got_name, got_args, value = t.pop(0)
        assert got_name == name and (not args or tuple(got_args) == args), (got_name, got_args, name, args)
        return value

    ch, cw = crop
    rec = {'asymmetric': bool(take('rand') < 0.2), 'rects': []}
    assert len(photo) == (2 if rec['asymmetric'] else 1)
    rec['photo'] = [photo[0], photo[-1]]
    if take('rand') < 0.5:
        for _ in range(take('randint', 1, 3)):
            x0, y0 = take('randint', 0, W), take('randint', 0, H)
            rec['rects'].append([int(x0), int(y0), int(take('randint', 50, 100)), int(take('randint', 50, 100))])
    min_scale = max((ch + 8) / float(H), (cw + 8) / float(W))
    sx = sy = 2 ** take('uniform', -0.2, 0.5)
    rec['stretch'] = bool(take('rand') < 0.8)
    if rec['stretch']:
        sx = sx * 2 ** take('uniform', -0.2, 0.2)
        sy = sy * 2 ** take('uniform', -0.2, 0.2)
    rec['clipped'] = bool(sx < min_scale or sy < min_scale)
    rec['scale_x'], rec['scale_y'] = float(max(sx, min_scale)), float(max(sy, min_scale))
    rec['resize'] = bool(take('rand') < 0.8)
    rec['flip_h'] = bool(take('rand') < 0.5)
    rec['flip_v'] = bool(take('rand') < 0.1)
    H1, W1 = (int(np.rint(H * rec['scale_y'])), int(np.rint(W * rec['scale_x']))) if rec['resize'] else (H, W)
    rec['y0'] = int(take('randint', 0, H1 - ch))
    rec['x0'] = int(take('randint', 0, W1 - cw))
    rec['size'], rec['source'] = [H1, W1], [H, W]
    assert not t, t
    return rec


def run_reference(seed, H, W, crop=CROP):
    """One sample through the reference -> (outputs, record, final np.random state).  Seeds the GLOBAL np.random, as a user of the
    reference would, and hands the stand-in albumentations its own generator."""
    ref = load_reference()
    img1, img2, flow = case_inputs(seed, H, W)
    aug = ref.augmentor.FlowAugmentor(crop_size=list(crop))
    ref.albumentations.set_photo_rng(np.random.RandomState(seed + PHOTO_SEED_OFFSET))
    del ref.albumentations.applied[:], ref.cv2.resized[:]
    rec_random = _RecordingRandom()
    np.random.seed(seed)
    real_np = ref.augmentor.np
    ref.augmentor.np = _NumpyProxy(rec_random)
    try:
        o1, o2, oflow = aug(img1.copy(), img2.copy(), flow.copy())
    finally:
        ref.augmentor.np = real_np
    state = np.random.get_state()
    valid = (np.abs(oflow[:, :, 0]) < 1000) * (np.abs(oflow[:, :, 1]) < 1000)                   # dataset.py:102
    photo = [{k: (None if v is None else [float(x) for x in v]) for k, v in a.items()} for a in ref.albumentations.applied]
    rec = decode(rec_random.trace, photo, H, W, crop)
    # what the stand-in cv2 was asked agrees with the decoded record
    if rec['resize']:
        assert len(ref.cv2.resized) == 3 and all(r[:2] == (rec['scale_x'], rec['scale_y']) for r in ref.cv2.resized)
        assert tuple(ref.cv2.resized[0][2][:2]) == tuple(rec['size'])
    else:
        assert not ref.cv2.resized
    assert o1.shape == (*crop, 3) and o1.dtype == np.uint8 and oflow.shape == (*crop, 2)
    return {'image1': o1, 'image2': o2, 'flow': np.asarray(oflow), 'valid': valid.astype(np.float32)}, rec, state


def crosses_crop(rec, crop=CROP):
    """True when an eraser rectangle's edge runs through the crop (the crop holds erased and kept pixels of frame 2): decided on
    the resized, flipped frame from the rectangle's corners, conservatively (a margin of two pixels)."""
    H, W = rec['source']
    H1, W1 = rec['size']
    for x0, y0, dx, dy in rec['rects']:
        xs = sorted(np.array([x0, min(x0 + dx, W)]) * (W1 / W))
        ys = sorted(np.array([y0, min(y0 + dy, H)]) * (H1 / H))
        if rec['flip_h']:
            xs = sorted(W1 - v for v in xs)
        if rec['flip_v']:
            ys = sorted(H1 - v for v in ys)
        cx0, cy0 = rec['x0'], rec['y0']
        inside_x = [v for v in xs if cx0 + 2 < v < cx0 + crop[1] - 2]
        inside_y = [v for v in ys if cy0 + 2 < v < cy0 + crop[0] - 2]
        overlap_x = xs[0] < cx0 + crop[1] - 2 and xs[1] > cx0 + 2
        overlap_y = ys[0] < cy0 + crop[0] - 2 and ys[1] > cy0 + 2
        if (inside_x and overlap_y) or (inside_y and overlap_x):
            return True
    return False


def coverage(recs):
    """name -> number of cases of the set that show the property; every one must be > 0 (tests/test_augment.py asserts it)."""
    def count(pred):
        return sum(1 for r in recs if pred(r))
    on = lambda r, k: any(p[k] is not None for p in r['photo'])       # noqa: E731
    off = lambda r, k: any(p[k] is None for p in r['photo'])          # noqa: E731
    return {
        'resized': count(lambda r: r['resize']), 'not_resized': count(lambda r: not r['resize']),
        'stretched': count(lambda r: r['resize'] and r['stretch'] and r['scale_x'] != r['scale_y']),
        'clipped_to_min_scale': count(lambda r: r['resize'] and r['clipped']),
        'h_flip_only': count(lambda r: r['flip_h'] and not r['flip_v']), 'v_flip_only': count(lambda r: r['flip_v'] and not r['flip_h']),
        'both_flips': count(lambda r: r['flip_h'] and r['flip_v']), 'no_flip': count(lambda r: not r['flip_h'] and not r['flip_v']),
        'no_rectangle': count(lambda r: len(r['rects']) == 0), 'one_rectangle': count(lambda r: len(r['rects']) == 1),
        'two_rectangles': count(lambda r: len(r['rects']) == 2), 'rectangle_crosses_crop': count(crosses_crop),
        'symmetric_colour': count(lambda r: not r['asymmetric']), 'asymmetric_colour': count(lambda r: r['asymmetric']),
        'brightness_contrast_on': count(lambda r: on(r, 'bc')), 'brightness_contrast_off': count(lambda r: off(r, 'bc')),
        'hue_saturation_on': count(lambda r: on(r, 'hsv')), 'hue_saturation_off': count(lambda r: off(r, 'hsv')),
        'small_source_set': count(lambda r: tuple(r['source']) == (96, 128)), 'large_source_set': count(lambda r: tuple(r['source']) == (120, 160)),
    }


def load_fixture():
    """-> list of (H, W, seed, record, outputs dict, final np.random state)."""
    with np.load(FIXTURE) as z:
        index = json.loads(str(z['index']))
        cases = []
        for k, (H, W, seed) in enumerate(index['cases']):
            outs = {name: z[f'{k}_{name}'] for name in ('image1', 'image2', 'flow', 'valid')}
            state = ('MT19937', z[f'{k}_state_keys'], *index['state_tail'][k])
            cases.append((H, W, seed, index['records'][k], outs, state))
    return cases


def scan(seeds=1500):
    """Greedy cover of `coverage` preferring cheap cases (a resized case stores 98 KB of incompressible float64 flow).  Candidates
    are drawn with the product's host draw, which is fast; `main` then runs the reference on the chosen seeds and asserts the
    coverage on what the reference did."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from tf_raft_amd.augment import FlowAugmentor
    need = set(coverage([]))
    chosen, pool = [], []
    for H, W in ((96, 128), (120, 160)):
        for seed in range(seeds):
            np.random.seed(seed)
            rec = FlowAugmentor(CROP, photo_rng=np.random.RandomState(seed + PHOTO_SEED_OFFSET)).draw(H, W)[0]
            pool.append(((H, W, seed), rec, {k for k, v in coverage([rec]).items() if v}))
    while need:
        best = max(pool, key=lambda c: (len(c[2] & need) - (0.9 if c[1]['resize'] else 0.0), -c[0][2]))
        if not best[2] & need:
            raise SystemExit(f'cannot cover {need}')
        chosen.append(best[0])
        need -= best[2]
    print('CASES =', tuple(sorted(chosen)))


def main():
    if '--scan' in sys.argv:
        return scan()
    out, records, tails = {}, [], []
    for k, (H, W, seed) in enumerate(CASES):
        outs, rec, state = run_reference(seed, H, W)
        for name, a in outs.items():
            out[f'{k}_{name}'] = a
        assert state[0] == 'MT19937'
        out[f'{k}_state_keys'] = state[1]
        tails.append([int(state[2]), int(state[3]), float(state[4])])
        records.append(rec)
    cov = coverage(records)
    assert all(cov.values()), cov
    out['index'] = np.array(json.dumps({'cases': [list(c) for c in CASES], 'records': records, 'state_tail': tails, 'crop': list(CROP)}))
    np.savez_compressed(FIXTURE, **out)
    print('wrote', FIXTURE, os.path.getsize(FIXTURE), 'bytes;', cov)


if __name__ == '__main__':
    main()

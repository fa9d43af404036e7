"""Generates tests/golden/sparse_augment_golden.npz: the REFERENCE's own SparseFlowAugmentor (tf_raft/datasets/augmentor.py:132-267,
loaded unmodified under the stand-in cv2 / albumentations of tests/augstub) run on seeded samples, with the parameters it used.
Run where the reference tree is present:
    python tests/golden/make_sparse_augment_golden.py            (--scan: choose the cases)

Per case: the four outputs as the reference returns them (two uint8 crops; the flow float64 where it was multiplied by a list;
`valid` int32 where the sample was resized, the input's float32 otherwise), the parameter record decoded from the reference's own
np.random calls, and np.random's final state.  The inputs are regenerated from the seed (`sparse_case_inputs`), not stored.
tests/test_sparse_augment.py and tests/test_gpu_sparse_augment.py import the helpers below; those of the dense generator
(make_augment_golden) are reused, not copied.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_augment_golden as mk                                   # noqa: E402
from make_augment_golden import ROOT, PHOTO_SEED_OFFSET, load_reference, load_stubs, case_inputs, _RecordingRandom, _NumpyProxy  # noqa: E402

FIXTURE = os.path.join(HERE, 'sparse_augment_golden.npz')
CROP = mk.CROP
SIZES = ((72, 108), (120, 160))
# (source height, width, seed, do_flip).  Chosen by `--scan` to cover the list in `coverage` with few cases.
CASES = ((72, 108, 107, True), (120, 160, 24, False), (120, 160, 34, True))
NAMES = ('image1', 'image2', 'flow', 'valid')
VALID_DENSITY = 0.6


def sparse_case_inputs(seed, H, W):
    """The dense generator's frames and flow (its block of huge vectors clipped away), a seeded validity mask with values in {0, 1}
    at about 60 % density, and -512 (what the KITTI reader stores) in the flow wherever the mask is 0."""
    img1, img2, flow = case_inputs(seed, H, W)
    flow = np.clip(flow, -40, 40)
    rs = np.random.RandomState(200000 + seed)
    valid = (rs.rand(H, W) < VALID_DENSITY).astype(np.float32)
    flow[valid == 0] = -512.0
    return img1, img2, flow, valid


def _photo(ph):
    return {k: (None if v is None else [float(x) for x in v]) for k, v in ph.items()}


def decode(trace, photo, H, W, crop, do_flip):
    """The reference's np.random calls of one sample (augmentor.py:170-255, in order) -> the record ``SparseFlowAugmentor.draw``
    returns."""
    t = list(trace)

    def take(name, *args):
        got_name, got_args, value = t.pop(0)
        assert got_name == name and (not args or tuple(got_args) == args), (got_name, got_args, name, args)
        return value

    ch, cw = crop
    assert len(photo) == 1
    rec = {'photo': [photo[0], photo[0]], 'rects': []}
    if take('rand') < 0.5:
        for _ in range(take('randint', 1, 3)):
            x0, y0 = take('randint', 0, W), take('randint', 0, H)
            rec['rects'].append([int(x0), int(y0), int(take('randint', 50, 100)), int(take('randint', 50, 100))])
    min_scale = max((ch + 1) / float(H), (cw + 1) / float(W))
    s = 2 ** take('uniform', -0.2, 0.5)
    rec['clipped'] = bool(s < min_scale)
    rec['scale_x'] = rec['scale_y'] = float(max(s, min_scale))
    rec['resize'] = bool(take('rand') < 0.8)
    rec['flip_h'] = bool(take('rand') < 0.5) if do_flip else False
    rec['flip_v'] = False
    H1, W1 = (int(np.rint(H * rec['scale_y'])), int(np.rint(W * rec['scale_x']))) if rec['resize'] else (H, W)
    rec['y0_drawn'] = int(take('randint', 0, H1 - ch + 20))
    rec['x0_drawn'] = int(take('randint', -50, W1 - cw + 50))
    rec['y0'], rec['x0'] = min(max(rec['y0_drawn'], 0), H1 - ch), min(max(rec['x0_drawn'], 0), W1 - cw)
    rec['size'], rec['source'] = [H1, W1], [H, W]
    assert not t, t
    return rec


def run_reference(seed, H, W, do_flip, crop=CROP):
    """One sample through the reference -> (outputs, record, final np.random state).  Seeds the
    GLOBAL np.random, as a user of the reference would, and hands the stand-in albumentations its own generator."""
    ref = load_reference()
    img1, img2, flow, valid = sparse_case_inputs(seed, H, W)
    aug = ref.augmentor.SparseFlowAugmentor(crop_size=list(crop), do_flip=do_flip)
    ref.albumentations.set_photo_rng(np.random.RandomState(seed + PHOTO_SEED_OFFSET))
    del ref.albumentations.applied[:], ref.cv2.resized[:]
    rec_random = _RecordingRandom()
    np.random.seed(seed)
    real_np = ref.augmentor.np
    ref.augmentor.np = _NumpyProxy(rec_random)
    try:
        o1, o2, oflow, ovalid = aug(img1.copy(), img2.copy(), flow.copy(), valid.copy())
    finally:
        ref.augmentor.np = real_np
    state = np.random.get_state()
    rec = decode(rec_random.trace, [_photo(a) for a in ref.albumentations.applied], H, W, crop, do_flip)
    if rec['resize']:                       # the two frames went through the stand-in cv2, the flow did not
        assert len(ref.cv2.resized) == 2 and all(r[:2] == (rec['scale_x'], rec['scale_y']) for r in ref.cv2.resized)
        assert tuple(ref.cv2.resized[0][2][:2]) == tuple(rec['size'])
    else:
        assert not ref.cv2.resized
    assert o1.shape == (*crop, 3) and o1.dtype == np.uint8 and oflow.shape == (*crop, 2) and ovalid.shape == tuple(crop)
    return {'image1': o1, 'image2': o2, 'flow': np.asarray(oflow), 'valid': np.asarray(ovalid)}, rec, state


def landing(f, size):
    """Target index of every source index of one axis: ``rint(double(float(s)) * f)``, halves to even."""
    return np.rint(np.arange(size).astype(np.float32) * np.float64(f)).astype(np.int64)


def scatter(flow, valid, f):
    """The sparse resize as a SCATTER (what augmentor.py:183-215 computes), written on the per-axis landing tables: every source with
    ``valid >= 1`` whose target lies strictly inside ``0 < X < W1``, ``0 < Y < H1`` is assigned, in row-major source order, in ONE fancy
    assignment -- so which of several sources on a target stays is decided by NumPy, exactly as in the reference.
    tests/test_sparse_augment.py pins this helper to the reference's own method where the reference tree is present."""
    H, W = valid.shape
    f = np.float64(f)
    H1, W1 = int(np.rint(H * f)), int(np.rint(W * f))
    row_of, col_of = landing(f, H), landing(f, W)
    rows_ok, cols_ok = (row_of > 0) & (row_of < H1), (col_of > 0) & (col_of < W1)
    src_y, src_x = np.nonzero((np.asarray(valid, np.float32) >= 1) & rows_ok[:, None] & cols_ok[None, :])      # row-major
    out_flow = np.zeros((H1, W1, 2), np.float32)
    out_valid = np.zeros((H1, W1), np.int32)
    out_flow[row_of[src_y], col_of[src_x]] = np.asarray(flow, np.float32)[src_y, src_x].astype(np.float64) * f
    out_valid[row_of[src_y], col_of[src_x]] = 1
    return out_flow, out_valid


def sparse_numpy_chain(rec, img1, img2, flow, valid, crop=CROP):
    """The reference's chain for GIVEN parameters, step by step on the stand-ins (augmentor.py:163-267): colour map, erase on the
    source, resize of the frames, the scatter of flow and validity (`scatter`), flip, crop.  tests/test_sparse_augment.py pins it to the
    reference's own run; tests/test_gpu_sparse_augment.py uses it as the yardstick beyond the fixture."""
    cv2, A = load_stubs()
    img = np.concatenate([img1, img2], axis=0)
    ph = rec['photo'][0]
    if ph['bc'] is not None:
        img = A.RandomBrightnessContrast().apply(img, *ph['bc'])
    if ph['hsv'] is not None:
        img = A.HueSaturationValue().apply(img, *ph['hsv'])
    img1, img2 = (a.copy() for a in np.split(img, 2, axis=0))
    if rec['rects']:
        mean_color = np.mean(img2.reshape(-1, 3), axis=0)
        for x0, y0, dx, dy in rec['rects']:
            img2[y0:y0 + dy, x0:x0 + dx, :] = mean_color
    if rec['resize']:
        f = rec['scale_x']
        img1, img2 = (cv2.resize(a, None, fx=f, fy=f, interpolation=cv2.INTER_LINEAR) for a in (img1, img2))
        flow, valid = scatter(flow, valid, np.float64(f))
    if rec['flip_h']:
        img1, img2, flow, valid = img1[:, ::-1], img2[:, ::-1], flow[:, ::-1] * [-1.0, 1.0], valid[:, ::-1]
    y0, x0 = rec['y0'], rec['x0']
    return dict(zip(NAMES, (np.ascontiguousarray(a[y0:y0 + crop[0], x0:x0 + crop[1]]) for a in (img1, img2, flow, valid))))


# ------------------------------------------------------------------ what a case shows
def crop_targets(rec, crop=CROP):
    """Resized-frame coordinates (Y, X) of the crop's pixels, the flip undone: arrays of shape crop."""
    H1, W1 = rec['size']
    X = rec['x0'] + np.arange(crop[1])
    if rec['flip_h']:
        X = W1 - 1 - X
    Y = rec['y0'] + np.arange(crop[0])
    return np.broadcast_to(Y[:, None], crop), np.broadcast_to(X[None, :], crop)


def collisions_with_different_flow(rec, flow, valid, crop=CROP):
    """Number of crop pixels on which two or more VALID sources with different flow vectors land: a first-wins or any-wins kernel
    gets these wrong."""
    if not rec['resize']:
        return 0
    H, W = rec['source']
    f = rec['scale_x']
    tx, ty = landing(f, W), landing(f, H)
    Y, X = crop_targets(rec, crop)
    inside = set(zip(Y.ravel().tolist(), X.ravel().tolist()))
    seen, differing = {}, set()
    ys, xs = np.nonzero(valid >= 1)
    for y, x in zip(ys.tolist(), xs.tolist()):
        key = (int(ty[y]), int(tx[x]))
        if key[0] <= 0 or key[1] <= 0 or key not in inside:
            continue
        vec = tuple(flow[y, x].tolist())
        if key in seen and seen[key] != vec:
            differing.add(key)
        seen.setdefault(key, vec)
    return len(differing)


def holes(rec, outs):
    """Crop pixels of a resized sample that no valid source reaches, away from row / column 0 of the resized frame."""
    if not rec['resize']:
        return 0
    Y, X = crop_targets(rec, outs['valid'].shape)
    return int(((np.asarray(outs['valid']) == 0) & (Y > 0) & (X > 0)).sum())


def coverage(cases):
    """name -> number of cases that show the property; ``cases``: (record, do_flip, collisions, holes).  Every one must be > 0
    (tests/test_sparse_augment.py asserts it on what the reference did)."""
    def count(pred):
        return sum(1 for c in cases if pred(*c))
    H1 = lambda r: r['size'][0] - CROP[0]      # noqa: E731
    W1 = lambda r: r['size'][1] - CROP[1]      # noqa: E731
    out = {
        'resized_below_1_with_differing_collisions': count(lambda r, d, c, h: r['resize'] and r['scale_x'] < 1 and c > 0),
        'resized_above_1_with_holes': count(lambda r, d, c, h: r['resize'] and r['scale_x'] > 1 and h > 0),
        'not_resized': count(lambda r, d, c, h: not r['resize']),
        'clipped_to_min_scale': count(lambda r, d, c, h: r['resize'] and r['clipped']),
        'do_flip_flipped': count(lambda r, d, c, h: d and r['flip_h']), 'do_flip_not_flipped': count(lambda r, d, c, h: d and not r['flip_h']),
        'no_do_flip': count(lambda r, d, c, h: not d),
        'resized_and_flipped': count(lambda r, d, c, h: r['resize'] and r['flip_h']),
        'origin_clipped_left_resized': count(lambda r, d, c, h: r['resize'] and not r['flip_h'] and r['x0_drawn'] < 0),
        'origin_clipped_right': count(lambda r, d, c, h: r['x0_drawn'] > W1(r)),
        'origin_clipped_bottom': count(lambda r, d, c, h: r['y0_drawn'] > H1(r)),
        'origin_unclipped': count(lambda r, d, c, h: r['y0_drawn'] == r['y0'] and r['x0_drawn'] == r['x0']),
        'no_rectangle': count(lambda r, d, c, h: len(r['rects']) == 0), 'one_rectangle': count(lambda r, d, c, h: len(r['rects']) == 1),
        'two_rectangles': count(lambda r, d, c, h: len(r['rects']) == 2),
        'brightness_contrast_on': count(lambda r, d, c, h: r['photo'][0]['bc'] is not None),
        'brightness_contrast_off': count(lambda r, d, c, h: r['photo'][0]['bc'] is None),
        'hue_saturation_on': count(lambda r, d, c, h: r['photo'][0]['hsv'] is not None),
        'hue_saturation_off': count(lambda r, d, c, h: r['photo'][0]['hsv'] is None),
    }
    for H, W in SIZES:
        out[f'source_{H}x{W}'] = count(lambda r, d, c, h: tuple(r['source']) == (H, W))
    return out


def case_properties(rec, do_flip, outs, seed):
    H, W = rec['source']
    _, _, flow, valid = sparse_case_inputs(seed, H, W)
    return rec, bool(do_flip), collisions_with_different_flow(rec, flow, valid), holes(rec, outs)


def load_fixture():
    """-> list of (H, W, seed, do_flip, record, outputs dict, final np.random state)."""
    with np.load(FIXTURE) as z:
        index = json.loads(str(z['index']))
        cases = []
        for k, (H, W, seed, do_flip) in enumerate(index['cases']):
            outs = {name: z[f'{k}_{name}'] for name in NAMES}
            state = ('MT19937', z[f'{k}_state_keys'], *index['state_tail'][k])
            cases.append((H, W, seed, bool(do_flip), index['records'][k], outs, state))
    return cases


def scan(seeds=400):
    """Greedy cover of `coverage`.  Candidates are drawn with the product's host draw and judged on the chain's outputs; `main` then
    runs the reference on the chosen seeds and asserts the coverage on what the reference did."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from tf_raft_amd.augment import SparseFlowAugmentor
    need = set(coverage([]))
    chosen, pool = [], []
    for H, W in SIZES:
        for seed in range(seeds):
            do_flip = bool(seed % 3)
            np.random.seed(seed)
            rec = SparseFlowAugmentor(CROP, do_flip=do_flip, photo_rng=np.random.RandomState(seed + PHOTO_SEED_OFFSET)).draw(H, W)[0]
            rec = json.loads(json.dumps(rec))
            outs = sparse_numpy_chain(rec, *sparse_case_inputs(seed, H, W))
            props = case_properties(rec, do_flip, outs, seed)
            pool.append(((H, W, seed, do_flip), {k for k, v in coverage([props]).items() if v}))
    while need:
        best = max(pool, key=lambda c: (len(c[1] & need), -c[0][2]))
        if not best[1] & need:
            raise SystemExit(f'cannot cover {need}')
        chosen.append(best[0])
        need -= best[1]
    print('CASES =', tuple(sorted(chosen)))


def main():
    if '--scan' in sys.argv:
        return scan()
    out, records, tails, props = {}, [], [], []
    for k, (H, W, seed, do_flip) in enumerate(CASES):
        outs, rec, state = run_reference(seed, H, W, do_flip)
        for name, a in outs.items():
            out[f'{k}_{name}'] = a
        assert state[0] == 'MT19937'
        out[f'{k}_state_keys'] = state[1]
        tails.append([int(state[2]), int(state[3]), float(state[4])])
        records.append(rec)
        props.append(case_properties(rec, do_flip, outs, seed))
    cov = coverage(props)
    assert all(cov.values()), cov
    out['index'] = np.array(json.dumps({'cases': [list(c) for c in CASES], 'records': records, 'state_tail': tails, 'crop': list(CROP)}))
    np.savez_compressed(FIXTURE, **out)
    print('wrote', FIXTURE, os.path.getsize(FIXTURE), 'bytes;', cov)


if __name__ == '__main__':
    main()

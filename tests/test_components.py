"""Connected components and their statistics, the part that needs no GPU: the NumPy restatements of
``raft_label_components``, ``raft_find_objects`` and ``raft_remove_small_components`` -- a breadth-first fill in raster order, which
shares nothing with the kernel's union-find over tiles --, the fixed cases of tests/test_gpu_components.py with the property each was
chosen for ASSERTED here, known answers written out by hand, the header / binding / build list, the C entries' error codes (every
check precedes the first launch, so NULL and dummy pointers do) and the argument checks of the Python layer.
"""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

from tf_raft_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_W, TILE_H = 32, 16                  # csrc/components.hip kTileW, kTileH (asserted below)
FLOW_LIMIT = np.float32(2.0 ** 20)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the restatements
def _foreground(mask, exclude):
    fg = np.asarray(mask) != 0
    if exclude is not None:
        fg &= np.asarray(exclude) == 0
    return fg


_NEIGHBOURS = {4: ((0, -1), (0, 1), (-1, 0), (1, 0)),
               8: ((0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))}


def np_label_components(mask, exclude=None, connectivity=8):
    """labels (N, H, W) int32: 0 for background, 1 + the smallest raster index of its component for a foreground pixel.  Pixels are
    visited in raster order; the first pixel of a component that is met is its smallest index, and a breadth-first fill labels
    the rest."""
    fg = _foreground(mask, exclude)
    N, H, W = fg.shape
    labels = np.zeros((N, H, W), np.int32)
    steps = _NEIGHBOURS[connectivity]
    for n in range(N):
        f, lab = fg[n], labels[n]
        for y0, x0 in zip(*np.nonzero(f)):                 # (raster order)
            if lab[y0, x0]:
                continue
            name = int(y0) * W + int(x0) + 1
            lab[y0, x0] = name
            queue = collections.deque([(int(y0), int(x0))])
            while queue:
                y, x = queue.popleft()
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and f[yy, xx] and not lab[yy, xx]:
                        lab[yy, xx] = name
                        queue.append((yy, xx))
    return labels


def np_find_objects(mask, max_objects, min_area=64, connectivity=8, exclude=None, flow=None):
    """(labels, count, area, boxes, centroid, mean_flow or None) as include/raft_hip.h defines raft_find_objects."""
    full = np_label_components(mask, exclude, connectivity)
    N, H, W = full.shape
    K = int(max_objects)
    labels = np.zeros((N, H, W), np.int32)
    count = np.zeros((N,), np.int32)
    area = np.zeros((N, K), np.int32)
    boxes = np.tile(np.array([0, 0, -1, -1], np.int32), (N, K, 1))
    centroid = np.full((N, K, 2), -1, np.float32)
    mean_flow = None if flow is None else np.zeros((N, K, 2), np.float32)
    for n in range(N):
        names, areas = np.unique(full[n][full[n] > 0], return_counts=True)
        keys = sorted(((int(a) << 32) | (0xFFFFFFFF - (int(r) - 1)) for r, a in zip(names, areas) if a >= min_area), reverse=True)
        count[n] = min(len(keys), K)
        for slot, key in enumerate(keys[:K]):
            name = 0xFFFFFFFF - (key & 0xFFFFFFFF) + 1
            ys, xs = np.nonzero(full[n] == name)
            assert len(ys) == key >> 32
            labels[n][ys, xs] = slot + 1
            area[n, slot] = len(ys)
            boxes[n, slot] = (xs.min(), ys.min(), xs.max(), ys.max())
            sx, sy = int(xs.astype(np.int64).sum()), int(ys.astype(np.int64).sum())
            centroid[n, slot] = (np.float32(np.float64(sx) / np.float64(len(ys))), np.float32(np.float64(sy) / np.float64(len(ys))))
            if flow is not None:
                vec = np.asarray(flow, np.float32)[n][ys, xs]
                with np.errstate(invalid='ignore'):
                    ok = ((vec >= -FLOW_LIMIT) & (vec <= FLOW_LIMIT)).all(axis=1)          # (a NaN fails)
                q = np.rint(vec[ok] * np.float32(256)).astype(np.int64)                    # float32 product, ties to even
                cnt = int(ok.sum())
                if cnt:
                    for c in (0, 1):
                        mean_flow[n, slot, c] = np.float32(np.float64(int(q[:, c].sum())) / (256.0 * np.float64(cnt)))
    return labels, count, area, boxes, centroid, mean_flow


def np_remove_small(mask, min_area, connectivity=8, exclude=None):
    full = np_label_components(mask, exclude, connectivity)
    out = np.zeros(full.shape, np.uint8)
    for n in range(full.shape[0]):
        names, areas = np.unique(full[n][full[n] > 0], return_counts=True)
        out[n] = np.isin(full[n], names[areas >= min_area])
    return out


def component_areas(labels_n):
    """{root index: area} of one image's labels."""
    names, areas = np.unique(labels_n[labels_n > 0], return_counts=True)
    return {int(r) - 1: int(a) for r, a in zip(names, areas)}


def tiles_touched(labels_n, name):
    ys, xs = np.nonzero(labels_n == name)
    return len(set(zip((ys // TILE_H).tolist(), (xs // TILE_W).tolist())))


# ------------------------------------------------------------------ the fixed cases
def _spiral(H, W):
    """A one-pixel path that winds inwards from (0, 0), one background pixel between its turns."""
    g = np.zeros((H, W), np.uint8)
    y = x = 0
    g[0, 0] = 1
    dy, dx, turns = 0, 1, 0
    inside = lambda a, b: 0 <= a < H and 0 <= b < W       # noqa: E731
    while turns < 2:
        ny, nx = y + dy, x + dx
        if inside(ny, nx) and not g[ny, nx] and not (inside(ny + dy, nx + dx) and g[ny + dy, nx + dx]):
            y, x, turns = ny, nx, 0
            g[y, x] = 1
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return g


def _comb(H, W):
    """Full rows at even y, joined at the right end after rows 0, 4, ... and at the left end after rows 2, 6, ...: one serpentine."""
    g = np.zeros((H, W), np.uint8)
    g[0::2] = 1
    g[1::4, W - 1] = 1
    g[3::4, 0] = 1
    return g


def _flow_for(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape + (2,)) * 6).astype(np.float32)


def _case_background():
    return dict(mask=np.zeros((3, 5, 3), np.uint8), components={4: [0, 0, 0], 8: [0, 0, 0]})


def _case_foreground():
    m = np.full((2, 37, 70), 7, np.uint8)
    m[1, 17, :] = 0                                        # the second image: two halves
    return dict(mask=m, components={4: [1, 2], 8: [1, 2]}, crosses={4, 8})


def _case_last_pixel():
    m = np.zeros((2, 37, 70), np.uint8)
    m[0, 36, 69] = 1
    m[1, 0, 0] = 255
    m[1, 36, 0] = 1
    return dict(mask=m, components={4: [1, 2], 8: [1, 2]}, min_area=1)


def _case_checkerboard():
    yy, xx = np.mgrid[0:37, 0:70]
    m = np.stack([(yy + xx) % 2 == 0, (yy + xx) % 2 == 1]).astype(np.uint8)
    # 4-connectivity: the exact maximum ceil(H W / 2) = the whole candidate list; every area is 1: ties all the way, overflow
    return dict(mask=m, components={4: [1295, 1295], 8: [1, 1]}, min_area=1, max_objects=16, crosses={8}, ties={4}, overflow={4})


def _case_tiny_checkerboard():
    yy, xx = np.mgrid[0:5, 0:3]
    m = np.stack([(yy + xx) % 2 == 0, (yy + xx) % 2 == 1, np.ones((5, 3), bool)]).astype(np.uint8)
    return dict(mask=m, components={4: [8, 7, 1], 8: [1, 1, 1]}, min_area=1, max_objects=8, ties={4})


def _case_dots():
    m = np.zeros((2, 37, 70), np.uint8)
    m[0, 0::2, 0::2] = 1                                   # 8-connectivity: the exact maximum ceil(H / 2) * ceil(W / 2)
    m[1, 1::2, 1::2] = 1
    return dict(mask=m, components={4: [19 * 35, 18 * 35], 8: [19 * 35, 18 * 35]}, min_area=1, max_objects=1024, ties={4, 8})


def _case_spiral():
    m = np.stack([_spiral(61, 93)])
    return dict(mask=m, components={4: [1], 8: [1]}, crosses={4, 8}, every_tile=True)


def _case_comb():
    m = np.stack([_comb(37, 70), _comb(37, 70)[::-1].copy()])
    return dict(mask=m, components={4: [1, 1], 8: [1, 1]}, crosses={4, 8}, every_tile=True)


def _case_diagonal_touch():
    m = np.zeros((2, 37, 70), np.uint8)
    m[0, 12:16, 28:32] = 1                                 # the corner shared by four tiles at (y, x) = (16, 32): a diagonal
    m[0, 16:20, 32:36] = 1
    m[0, 12:16, 64:68] = 1                                 # the corner at (16, 64): the other diagonal
    m[0, 16:20, 60:64] = 1
    m[1, 2:5, 2:5] = 1                                     # the same inside one tile
    m[1, 5:8, 5:8] = 1
    m[1, 5:8, 40:43] = 1
    m[1, 8:11, 37:40] = 1
    return dict(mask=m, components={4: [4, 4], 8: [2, 2]}, min_area=1, max_objects=8, crosses={8}, ties={4, 8})


def _noise(density, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((2, 97, 131)) < density).astype(np.uint8)


def _case_noise30():
    return dict(mask=_noise(0.30, 30), min_area=3, max_objects=32, overflow={4, 8}, ties={4, 8}, drops={4, 8})


def _case_noise60():
    return dict(mask=_noise(0.60, 60), min_area=2, max_objects=48, crosses={4, 8}, overflow={4}, ties={4, 8}, drops={4, 8})


def _case_blobs():
    m = np.zeros((2, 37, 70), np.uint8)
    m[0, 1:5, 1:5] = 1          # 16
    m[0, 20:22, 30:38] = 1      # 16, crosses x = 32: a tie, the earlier one first
    m[0, 8:12, 50:54] = 1       # 16
    m[0, 14:19, 10:15] = 1      # 25, crosses y = 16
    m[0, 30, 60:63] = 1         # 3: dropped
    m[0, 34, 5] = 1             # 1: dropped
    m[1, 10:30, 20:60] = 1      # 800
    m[1, 0:3, 0:3] = 1          # 9: dropped
    return dict(mask=m, components={4: [6, 2], 8: [6, 2]}, min_area=10, max_objects=8, crosses={4, 8}, ties={4, 8}, drops={4, 8},
                empty_slots=True)


def _case_exclude_cut():
    m = np.zeros((2, 37, 70), np.uint8)
    m[0, 15:18, 3:67] = 1
    m[1, 3:34, 33:36] = 1
    e = np.zeros((2, 37, 70), np.uint8)
    e[0, :, 31:33] = 9                                     # cuts the bar in two at the tile border
    e[1, 16, :] = 1
    return dict(mask=m, exclude=e, components={4: [2, 2], 8: [2, 2]}, components_without_exclude=[1, 1], min_area=4, max_objects=4,
                crosses={4, 8})


def _case_flow_specials():
    m = np.zeros((2, 37, 70), np.uint8)
    m[0, 2:10, 2:12] = 1        # object A: a NaN, an Inf, a vector beyond 2^20 and one exactly at it inside
    m[0, 20:30, 28:40] = 1      # object B: ties of the quantisation
    m[1, 5:9, 40:50] = 1        # object C: no vector counts at all: mean flow 0
    m[1, 20:25, 5:9] = 1        # object D: plain
    flow = _flow_for((2, 37, 70), 77)
    flow[0, 3, 3] = (np.nan, 1.0)
    flow[0, 4, 4] = (1.0, np.inf)
    flow[0, 5, 5] = (-np.inf, np.nan)
    flow[0, 6, 6] = (2.0 ** 20 + 1, 0.0)
    flow[0, 7, 7] = (2.0 ** 20, -2.0 ** 20)                # counts
    flow[0, 20:30, 28:40] = (0.5 / 256, 1.5 / 256)         # 0.5 -> 0 and 1.5 -> 2: ties to even
    flow[0, 21, 30] = (-2.5 / 256, 0.49 / 256)
    flow[1, 5:9, 40:50, 0] = np.nan
    return dict(mask=m, flow=flow, components={4: [2, 2], 8: [2, 2]}, min_area=8, max_objects=3, empty_slots=True)


CASES = collections.OrderedDict([
    # name: (why it is here, the builder)
    ('background', ('no foreground at all: nothing to merge, every slot empty', _case_background)),
    ('foreground', ('one component over every tile, the deepest chains; nonzero values other than 1', _case_foreground)),
    ('last_pixel', ('a single pixel in the last row and column: the partial tile at both ends', _case_last_pixel)),
    ('checkerboard', ('4: exactly ceil(HW/2) components, the whole candidate list, all areas tied, more than max_objects -> the '
                      'radix select; 8: exactly one component made of diagonals only', _case_checkerboard)),
    ('tiny_checkerboard', ('the smallest shape, one partial tile, known answers by hand', _case_tiny_checkerboard)),
    ('dots', ('8: exactly ceil(H/2) ceil(W/2) components, the whole candidate list; max_objects = the limit', _case_dots)),
    ('spiral', ('one one-pixel path through every tile, its smallest index far from most of its pixels', _case_spiral)),
    ('comb', ('one serpentine over all tiles: every tile holds several pieces whose local minima are not the global one', _case_comb)),
    ('diagonal_touch', ('squares that touch only diagonally, across a corner of four tiles and inside a tile: two components '
                        'under 4, one under 8', _case_diagonal_touch)),
    ('noise30', ('random 30 %: many small components, min_area drops some, more than max_objects remain', _case_noise30)),
    ('noise60', ('random 60 %: large ragged components across many tiles next to specks', _case_noise60)),
    ('blobs', ('equal areas for the tie rule, fewer components than slots, min_area drops some', _case_blobs)),
    ('exclude_cut', ('an exclude mask cuts a component in two at a tile border', _case_exclude_cut)),
    ('flow_specials', ('NaN, Inf and a value above 2^20 inside an object; ties of the quantisation; an object without any '
                       'counted vector', _case_flow_specials)),
])
IDS = list(CASES)
_BUILT = {}


def case_args(name):
    """The inputs of one case (built once, read-only): dict(mask, exclude, flow, min_area, max_objects, ...properties)."""
    if name not in _BUILT:
        case = dict(exclude=None, min_area=1, max_objects=8)
        case.update(CASES[name][1]())
        if case.get('flow') is None:
            case['flow'] = _flow_for(case['mask'].shape, len(name))
        for k in ('mask', 'exclude', 'flow'):
            if case[k] is not None:
                case[k].setflags(write=False)
        _BUILT[name] = case
    return _BUILT[name]


_WANT = {}


def want(name, connectivity):
    """What the restatements say about one case: (labels, objects with the flow, small-component mask), computed once."""
    key = (name, connectivity)
    if key not in _WANT:
        c = case_args(name)
        labels = np_label_components(c['mask'], c['exclude'], connectivity)
        objects = np_find_objects(c['mask'], c['max_objects'], c['min_area'], connectivity, c['exclude'], c['flow'])
        small = np_remove_small(c['mask'], c['min_area'], connectivity, c['exclude'])
        for a in (labels, small) + objects:
            a.setflags(write=False)
        _WANT[key] = (labels, objects, small)
    return _WANT[key]


def assert_same_objects(got, wanted, what=''):
    """labels, count, area, boxes as integers; centroid and mean flow as bit patterns.  No tolerance."""
    for name, g, w in zip(('labels', 'count', 'area', 'boxes'), got[:4], wanted[:4]):
        if g is None and name == 'labels':
            continue
        np.testing.assert_array_equal(np.asarray(g), w, err_msg=f'{what} {name}')
    np.testing.assert_array_equal(bits(got[4]), bits(wanted[4]), err_msg=f'{what} centroid')
    if wanted[5] is not None and got[5] is not None:
        np.testing.assert_array_equal(bits(got[5]), bits(wanted[5]), err_msg=f'{what} mean_flow')


# ------------------------------------------------------------------ the cases have the properties they were chosen for
def test_the_tile_of_the_kernel_is_the_tile_of_these_cases():
    src = open(os.path.join(ROOT, 'tf_raft_amd', 'csrc', 'components.hip')).read()
    assert f'kTileW = {TILE_W}, kTileH = {TILE_H}' in src
    shapes = {case_args(n)['mask'].shape for n in IDS}
    assert all(H % TILE_H and W % TILE_W for _, H, W in shapes)                      # never a multiple of the tile
    assert any(H > 2 * TILE_H and W > 2 * TILE_W for _, H, W in shapes)              # more than two tiles along each axis
    assert any(N > 1 for N, _, _ in shapes) and any(H < TILE_H and W < TILE_W for _, H, W in shapes)
    for n in IDS:
        m = case_args(n)['mask']
        if m.shape[0] > 1 and n != 'background':
            assert not (m[0] == m[1]).all(), n                                       # different content per image


@pytest.mark.parametrize('connectivity', (4, 8))
@pytest.mark.parametrize('name', IDS)
def test_the_fixed_cases_meet_the_conditions_the_gpu_tests_rely_on(name, connectivity):
    c = case_args(name)
    labels, (slots, count, area, boxes, centroid, mean_flow), small = want(name, connectivity)
    N, H, W = labels.shape
    per_image = [component_areas(labels[n]) for n in range(N)]
    if 'components' in c:
        assert [len(p) for p in per_image] == c['components'][connectivity]
    fg = _foreground(c['mask'], c['exclude'])
    np.testing.assert_array_equal(labels > 0, fg)
    for n in range(N):                                                               # the label IS the smallest index
        for root in per_image[n]:
            ys, xs = np.nonzero(labels[n] == root + 1)
            assert int((ys * W + xs).min()) == root
    if connectivity in c.get('crosses', ()):
        assert any(tiles_touched(labels[n], r + 1) > 1 for n in range(N) for r in per_image[n])
    if c.get('every_tile'):
        tiles = -(-H // TILE_H) * -(-W // TILE_W)
        assert all(tiles_touched(labels[n], next(iter(per_image[n])) + 1) == tiles for n in range(N))
        assert all(next(iter(per_image[n])) < W for n in range(N))                   # the root lies in the first row
    qualifying = [[a for a in p.values() if a >= c['min_area']] for p in per_image]
    if connectivity in c.get('ties', ()):
        assert any(len(set(q[:])) < len(q) for q in qualifying)
        assert any(len(set(area[n, :count[n]].tolist())) < count[n] for n in range(N))          # ... among the chosen ones
    if connectivity in c.get('overflow', ()):
        assert any(len(q) > c['max_objects'] for q in qualifying) and (count == c['max_objects']).any()
    if connectivity in c.get('drops', ()):
        assert any(len(q) < len(p) for q, p in zip(qualifying, per_image))
        assert (small != fg).any()
    if c.get('empty_slots'):
        assert (count < c['max_objects']).any()
    # the exact bound of the candidate list
    bound = min(H * W // c['min_area'], -(-H // 2) * -(-W // 2) if connectivity == 8 else -(-H * W // 2))
    assert all(len(q) <= bound for q in qualifying)
    if name == 'checkerboard' and connectivity == 4 or name == 'dots' and connectivity == 8:
        assert max(len(q) for q in qualifying) == bound                              # reached
    # slots: sorted by the key, labels consistent with areas
    for n in range(N):
        keys = [(int(area[n, k]) << 32) | (0xFFFFFFFF - int(np.flatnonzero(slots[n].ravel() == k + 1)[0])) for k in range(count[n])]
        assert keys == sorted(keys, reverse=True)
        assert all(int((slots[n] == k + 1).sum()) == area[n, k] for k in range(count[n]))
        assert (area[n, count[n]:] == 0).all() and (centroid[n, count[n]:] == -1).all() and (mean_flow[n, count[n]:] == 0).all()
        assert (boxes[n, count[n]:] == (0, 0, -1, -1)).all()
    if all(len(q) <= c['max_objects'] for q in qualifying):
        np.testing.assert_array_equal(small, (slots > 0).astype(np.uint8))


def test_an_exclude_mask_cuts_and_special_flows_are_left_out():
    c = case_args('exclude_cut')
    whole = np_label_components(c['mask'], None, 8)
    assert [len(component_areas(whole[n])) for n in range(2)] == c['components_without_exclude']
    c = case_args('flow_specials')
    flow = c['flow']
    inside = c['mask'][0, 2:10, 2:12] != 0
    assert inside.all() and np.isnan(flow[0, 2:10, 2:12]).any() and np.isinf(flow[0, 2:10, 2:12]).any()
    assert (np.abs(np.nan_to_num(flow[0, 2:10, 2:12], posinf=0, neginf=0)) > 2.0 ** 20).any()
    _, count, area, _, _, mean = want('flow_specials', 8)[1]
    assert count.tolist() == [2, 2] and np.isfinite(mean).all()
    # object B (120 pixels, the larger of image 0): 119 vectors quantise to (0, 2), one to (-2, 0)
    assert area[0, 0] == 120
    assert mean[0, 0, 0] == np.float32(-2.0 / (256.0 * 120)) and mean[0, 0, 1] == np.float32(2.0 * 119 / (256.0 * 120))
    # object A: 80 pixels, 4 left out (NaN, Inf, both, beyond the limit); the one AT the limit counts
    plain = np.ones((8, 10), bool)
    plain[[1, 2, 3, 4], [1, 2, 3, 4]] = False
    q = np.rint(flow[0, 2:10, 2:12][plain] * np.float32(256)).astype(np.int64)
    assert len(q) == 76 and (np.abs(q) == 2 ** 28).any()
    assert mean[0, 1, 0] == np.float32(float(q[:, 0].sum()) / (256.0 * 76))
    # object C of image 1: nothing counts
    k = int(np.flatnonzero(area[1] == 40)[0])
    assert (mean[1, k] == 0).all()


def test_scipy_agrees_on_the_partition_when_it_is_there():
    ndimage = pytest.importorskip('scipy.ndimage')
    for name in ('noise30', 'noise60', 'diagonal_touch', 'comb'):
        c = case_args(name)
        for conn, structure in ((4, None), (8, np.ones((3, 3), int))):
            mine = want(name, conn)[0]
            for n in range(mine.shape[0]):
                theirs, k = ndimage.label(c['mask'][n] != 0, structure=structure)
                assert k == len(component_areas(mine[n]))
                pairs = set(zip(mine[n].ravel().tolist(), theirs.ravel().tolist()))
                assert len(pairs) == k + 1                                               # a bijection of the names


# ------------------------------------------------------------------ known answers, by hand
def test_known_answers():
    m = np.array([[[1, 0, 1],
                   [0, 1, 0],
                   [1, 0, 0],
                   [0, 0, 1],
                   [0, 1, 1]]], np.uint8)
    np.testing.assert_array_equal(np_label_components(m, None, 4)[0], [[1, 0, 3], [0, 5, 0], [7, 0, 0], [0, 0, 12], [0, 12, 12]])
    np.testing.assert_array_equal(np_label_components(m, None, 8)[0], [[1, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 12], [0, 12, 12]])
    flow = np.zeros((1, 5, 3, 2), np.float32)
    flow[0, ..., 0] = 1.0
    flow[0, 4, 1] = (4.0, -3.0)
    labels, count, area, boxes, centroid, mean = np_find_objects(m, 3, 1, 8, None, flow)
    assert count.tolist() == [2] and area.tolist() == [[4, 3, 0]]
    np.testing.assert_array_equal(labels[0], [[1, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 2], [0, 2, 2]])
    assert boxes.tolist() == [[[0, 0, 2, 2], [1, 3, 2, 4], [0, 0, -1, -1]]]
    assert centroid.tolist() == [[[0.75, 0.75], [np.float32(5 / 3), np.float32(11 / 3)], [-1.0, -1.0]]]
    assert mean.tolist() == [[[1.0, 0.0], [2.0, -1.0], [0.0, 0.0]]]
    # 4-connectivity: five single pixels tie; the earlier one comes first, behind the one larger component
    labels, count, area, boxes, centroid, _ = np_find_objects(m, 4, 1, 4)
    assert count.tolist() == [4] and area.tolist() == [[3, 1, 1, 1]]
    np.testing.assert_array_equal(labels[0], [[2, 0, 3], [0, 4, 0], [0, 0, 0], [0, 0, 1], [0, 1, 1]])
    assert boxes[0, 1:].tolist() == [[0, 0, 0, 0], [2, 0, 2, 0], [1, 1, 1, 1]]
    # min_area
    assert np_find_objects(m, 4, 2, 4)[1].tolist() == [1]
    np.testing.assert_array_equal(np_remove_small(m, 2, 4)[0], [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 1], [0, 1, 1]])
    np.testing.assert_array_equal(np_remove_small(m, 4, 8)[0], [[1, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0]])
    # exclude
    e = np.zeros_like(m)
    e[0, 1, 1] = 1
    np.testing.assert_array_equal(np_label_components(m, e, 8)[0], [[1, 0, 3], [0, 0, 0], [7, 0, 0], [0, 0, 12], [0, 12, 12]])
    labels = want('tiny_checkerboard', 8)[0]
    assert labels[0].max() == 1 and labels[1].max() == 2 and (labels[2] == 1).all()
    assert want('tiny_checkerboard', 4)[1][1].tolist() == [8, 7, 1]


# ------------------------------------------------------------------ the C entries
ENTRIES = ('raft_components_workspace_bytes', 'raft_label_components', 'raft_find_objects', 'raft_remove_small_components')


def test_the_header_declares_and_the_library_exports_the_entries():
    from tf_raft_amd import build, image_ops
    assert 'components.hip' in build.SOURCES
    with open(os.path.join(ROOT, 'include', 'raft_hip.h')) as f:
        text = f.read()
    header = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    sigs = _ffi.header_signatures(text)
    P, I, L = C.c_void_p, C.c_int, C.c_int64
    assert sigs['raft_components_workspace_bytes'] == (L, [I, I, I, I, I])
    assert sigs['raft_label_components'] == (I, [P, P, P, I, I, I, I, P, P])
    assert sigs['raft_find_objects'] == (I, [P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, P, P])
    assert sigs['raft_remove_small_components'] == (I, [P, P, P, I, I, I, I, I, P, P])
    assert set(ENTRIES) <= set(_ffi.EXPORTED_SYMBOLS)
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, header)
    assert _ffi.ABI_VERSION == 222                                   # entries were added, no signature changed
    lib = _ffi.load_library()
    assert lib.raft_version() == 222
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == sigs[name][1] and getattr(lib, name).restype is sigs[name][0]
    consts = _ffi.header_constants(text)
    assert consts['RAFT_OBJECTS_MAX'] == image_ops.OBJECTS_MAX == 1024
    assert image_ops.OBJECTS_MIN_AREA == 64 and image_ops.OBJECTS_CONNECTIVITY == 8
    src = open(os.path.join(ROOT, 'tf_raft_amd', 'csrc', 'components.hip')).read()
    assert 'no thread ever waits for another' in src and 'atomicMin(p, kNoLabel)' in src
    assert not re.search(r'atomic\w*\s*\(\s*\(?\s*float', src)        # no float atomic


def test_the_workspace_size():
    fn = _ffi.load_library().raft_components_workspace_bytes
    up8 = lambda v: (v + 7) // 8 * 8                                           # noqa: E731
    for (N, H, W, conn, a) in [(3, 5, 3, 4, 1), (3, 5, 3, 8, 1), (2, 37, 70, 8, 64), (2, 97, 131, 4, 3), (4, 1080, 1920, 8, 64),
                               (1, 1, 1, 8, 1), (1, 7, 9, 4, 1000)]:
        bound = min(H * W // a, -(-H // 2) * -(-W // 2) if conn == 8 else -(-H * W // 2))
        assert fn(N, H, W, conn, a) == 2 * up8(N * H * W * 4) + up8((N * H * W + N) * 4) + N * bound * 8 + N * 1024 * 8 * 56
    for bad in [(0, 5, 3, 8, 1), (1, 0, 3, 8, 1), (1, 5, -1, 8, 1), (1, 5, 3, 6, 1), (1, 5, 3, 0, 1), (1, 5, 3, 8, 0), (1, 5, 3, 8, -4),
                (1, 1 << 16, 1 << 15, 8, 1), (2, 1 << 15, 1 << 15, 8, 1), (1 << 20, 1 << 6, 1 << 6, 8, 1)]:
        assert fn(*bad) == 0, bad
    assert fn(1, (1 << 31) - 2, 1, 8, 1 << 20) > 0                             # H * W = 2^31 - 2 is the largest image


def test_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off4, off1 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 1)
    sizes = ((0, 5, 3), (1, -5, 3), (1, 5, 0), (1, 1 << 16, 1 << 15), (2, 1 << 15, 1 << 15), (1 << 20, 1 << 6, 1 << 6))
    # ---- labelling
    #       mask exclude labels N  H   W  conn ws stream
    good = [p, p, p, 2, 37, 70, 8, p, None]
    fn = lib.raft_label_components
    for k in (0, 2, 7):
        for opt in (p, None):                                                # (exclude may be NULL)
            args = list(good)
            args[k], args[1] = None, opt
            assert fn(*args) == -1, k
    for bad in sizes:
        args = list(good)
        args[3:6] = bad
        assert fn(*args) == -2, bad
    for v in (0, 6, -8, 16):
        args = list(good)
        args[6] = v
        assert fn(*args) == -2, v
    for k, off in ((7, off4), (7, off1), (2, off1)):
        args = list(good)
        args[k] = off
        assert fn(*args) == -4, k
    args = list(good)
    args[0], args[1] = off1, off1                                            # (bytes may lie at any address)
    args[2], args[6], args[7] = None, 5, off1                               # precedence: NULL before shape before alignment
    assert fn(*args) == -1
    args[2] = p
    assert fn(*args) == -2
    args[6] = 4
    assert fn(*args) == -4
    # ---- the objects
    #       mask excl flow labels count area boxes centroid mean N  H   W  conn min_area K  ws stream
    good = [p, p, p, p, p, p, p, p, p, 2, 37, 70, 8, 64, 16, p, None]
    fn = lib.raft_find_objects
    for k in (0, 4, 5, 6, 7, 15):
        for opt in (p, None):                                                # (exclude, flow, labels and mean_flow may be NULL)
            args = list(good)
            args[k], args[1], args[2], args[3], args[8] = None, opt, opt, opt, opt
            assert fn(*args) == -1, k
    for bad in sizes:
        args = list(good)
        args[9:12] = bad
        assert fn(*args) == -2, bad
    for k, values in {12: (0, 6, -4), 13: (0, -1), 14: (0, -1, 1025, 1 << 20)}.items():
        for v in values:
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for k, off in ((15, off4), (15, off1), (2, off1), (3, off1), (4, off1), (5, off1), (6, off1), (7, off1), (8, off1)):
        args = list(good)
        args[k] = off
        assert fn(*args) == -4, k
    args = list(good)
    args[4], args[14], args[15] = None, 0, off4
    assert fn(*args) == -1
    args[4] = p
    assert fn(*args) == -2
    args[14] = 1024
    assert fn(*args) == -4
    # ---- the small components
    #       mask excl out N  H   W  conn min_area ws stream
    good = [p, p, p, 2, 37, 70, 4, 64, p, None]
    fn = lib.raft_remove_small_components
    for k in (0, 2, 8):
        for opt in (p, None):
            args = list(good)
            args[k], args[1] = None, opt
            assert fn(*args) == -1, k
    for bad in sizes:
        args = list(good)
        args[3:6] = bad
        assert fn(*args) == -2, bad
    for k, values in {6: (0, 6, 2), 7: (0, -64)}.items():
        for v in values:
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for off in (off4, off1):
        args = list(good)
        args[8] = off
        assert fn(*args) == -4
    args = list(good)
    args[2], args[7], args[8] = None, 0, off4
    assert fn(*args) == -1
    args[2] = p
    assert fn(*args) == -2


# ------------------------------------------------------------------ the Python layer, nothing reaches the device
def test_the_public_functions_check_their_arguments_without_a_gpu():
    import torch
    from tf_raft_amd import image_ops
    mask = np.zeros((2, 40, 50), np.uint8)
    calls = (lambda **kw: image_ops.find_objects(mask, **{'max_objects': 4, **kw}),
             lambda **kw: image_ops.label_components(mask, **{k: v for k, v in kw.items() if k in ('connectivity', 'exclude')}),
             lambda **kw: image_ops.remove_small_components(mask, **{'min_area': 4, **{k: v for k, v in kw.items() if k != 'max_objects'}}))
    for fn in calls:
        for bad in (0, 6, 16, 8.0, True, None, '8'):
            with pytest.raises(ValueError, match='connectivity must be 4 or 8'):
                fn(connectivity=bad)
        with pytest.raises(ValueError, match='expects a mask'):
            fn(exclude=np.zeros((2, 40, 51), np.uint8))
        with pytest.raises(TypeError, match='a mask is uint8 or bool'):
            fn(exclude=np.zeros((2, 40, 50), np.float32))
    for bad in (0, -1, 1025, 4.0, True, None):
        with pytest.raises(ValueError, match='max_objects must be an integer in 1 .. 1024'):
            image_ops.find_objects(mask, bad)
    for bad in (0, -64, 1 << 31, 64.0, False, None):
        with pytest.raises(ValueError, match='min_area must be an integer'):
            image_ops.find_objects(mask, 4, min_area=bad)
        with pytest.raises(ValueError, match='min_area must be an integer'):
            image_ops.remove_small_components(mask, bad)
    for fn in (lambda m: image_ops.label_components(m), lambda m: image_ops.find_objects(m, 4),
               lambda m: image_ops.remove_small_components(m, 4)):
        with pytest.raises(TypeError, match='a mask is uint8 or bool'):
            fn(np.zeros((2, 40, 50), np.float32))
        with pytest.raises(TypeError):
            fn(np.zeros((2, 40, 50), np.int32))
        with pytest.raises(ValueError, match='expects a mask'):
            fn(np.zeros((40,), np.uint8))
        with pytest.raises(ValueError, match='empty input'):
            fn(np.zeros((2, 0, 50), np.uint8))
        with pytest.raises(ValueError, match='too large'):
            fn(np.broadcast_to(np.uint8(0), (1 << 16, 1 << 15)))
        with pytest.raises(ValueError, match='too large'):
            fn(torch.empty((1 << 11, 1 << 10, 1 << 10), dtype=torch.uint8, device='meta'))
    with pytest.raises(ValueError, match='expects a flow'):
        image_ops.find_objects(mask, 4, flow=np.zeros((2, 40, 50, 3), np.float32))
    with pytest.raises(ValueError, match='expects a flow'):
        image_ops.find_objects(mask, 4, flow=np.zeros((40, 50, 2), np.float32))
    with pytest.raises(TypeError, match='a flow is float32'):
        image_ops.find_objects(mask, 4, flow=np.zeros((2, 40, 50, 2), np.uint8))
    assert image_ops.check_objects_args(1024, 1, 4) == (1024, 1, 4)
    assert image_ops.check_objects_args(np.int64(3), np.int32(64), np.int8(8)) == (3, 64, 8)
    assert image_ops.components_workspace_bytes(4, 1080, 1920, 8, 64) == \
        _ffi.load_library().raft_components_workspace_bytes(4, 1080, 1920, 8, 64)
    with pytest.raises(ValueError, match='too large'):
        image_ops.components_workspace_bytes(2, 1 << 15, 1 << 15)
    assert image_ops.Objects._fields == ('labels', 'count', 'area', 'boxes', 'centroid', 'mean_flow')


def test_the_launch_functions_check_their_tensors_without_a_gpu():
    import torch
    from tf_raft_amd import image_ops
    mask = torch.zeros((2, 40, 50), dtype=torch.uint8)
    for fn in (lambda m, **kw: image_ops.label_components_launch(m, **kw), lambda m, **kw: image_ops.find_objects_launch(m, 4, **kw),
               lambda m, **kw: image_ops.remove_small_components_launch(m, 4, **kw)):
        with pytest.raises(ValueError, match='expected a contiguous uint8 mask'):
            fn(np.zeros((2, 40, 50), np.uint8))
        with pytest.raises(ValueError, match='expected a contiguous uint8 mask'):
            fn(mask[0])
        with pytest.raises(ValueError):
            fn(mask.to(torch.int32))
        with pytest.raises(ValueError):
            fn(mask.permute(0, 2, 1))
        with pytest.raises(ValueError):
            fn(mask, exclude=mask[:1])
        with pytest.raises(ValueError, match='connectivity must be 4 or 8'):
            fn(mask, connectivity=5)
    with pytest.raises(ValueError, match='needs a flow'):
        image_ops.find_objects_launch(mask, 4, flow=torch.zeros((2, 40, 50, 3)))
    with pytest.raises(TypeError, match='a flow is float32'):
        image_ops.find_objects_launch(mask, 4, flow=torch.zeros((2, 40, 50, 2), dtype=torch.float64))


def test_moving_objects_step_checks_its_arguments_before_any_device_work():
    from tf_raft_amd import model
    assert model.MovingObjects._fields == model.CameraMotion._fields + ('labels', 'count', 'area', 'boxes', 'centroid', 'mean_flow')
    assert model.SmallRAFT.moving_objects_step is model.RAFT.moving_objects_step
    step = model.RAFT.moving_objects_step
    frames = (np.zeros((1, 64, 64, 3), np.uint8),) * 2
    for kw, match in ((dict(max_objects=0), 'max_objects must'), (dict(max_objects=2000), 'max_objects must'),
                      (dict(min_area=0), 'min_area must'), (dict(connectivity=6), 'connectivity must')):
        with pytest.raises(ValueError, match=match):
            step(None, frames, **kw)                        # (raised before `self` is touched)
    import inspect
    sig = inspect.signature(step)
    assert [sig.parameters[k].default for k in ('model', 'threshold', 'max_objects', 'min_area', 'connectivity', 'occlusion_test')] == \
        ['affine', 1.0, 64, 64, 8, 'consistency']

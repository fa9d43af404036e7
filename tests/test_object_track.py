"""Object identity through a video, the part that needs no GPU: the NumPy restatement of the three entries
(``np_object_overlap``, ``np_match_objects`` as the sorted greedy walk, ``np_chain_ids`` as plain loops) with answers known by hand,
the mutual-best rounds the kernel runs against the walk on random tables, the header and the library, and every argument error of
the C entries and of the Python layer, none of which may reach a device.  tests/test_gpu_object_track.py compares the kernels with
these restatements on the cases built here, integer for integer.
"""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

from tf_raft_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SLOTS = 128


# ------------------------------------------------------------------ the restatement
def np_object_overlap(labels_prev, flow, labels_next, K):
    """``raft_object_overlap``: (overlap (M, K, K), landed (M, K)) int32."""
    labels_prev, labels_next = np.asarray(labels_prev), np.asarray(labels_next)
    flow = np.asarray(flow, np.float32)
    M, H, W = labels_prev.shape
    overlap, landed = np.zeros((M, K, K), np.int32), np.zeros((M, K), np.int32)
    u, v = flow[..., 0], flow[..., 1]
    with np.errstate(over='ignore', invalid='ignore'):
        fx = np.arange(W, dtype=np.float32)[None, None, :] + u               # ONE float32 addition
        fy = np.arange(H, dtype=np.float32)[None, :, None] + v
        assert fx.dtype == np.float32 and fy.dtype == np.float32
        qx, qy = np.rint(fx), np.rint(fy)                                    # ties to even
        a = labels_prev.astype(np.int64) - 1
        inside = (qx >= 0) & (qx.astype(np.float64) <= W - 1) & (qy >= 0) & (qy.astype(np.float64) <= H - 1)
        ok = (a >= 0) & (a < K) & np.isfinite(u) & np.isfinite(v) & inside
    for m in range(M):
        ys, xs = np.nonzero(ok[m])
        am = a[m, ys, xs]
        np.add.at(landed[m], am, 1)
        b = labels_next[m, qy[m, ys, xs].astype(np.int64), qx[m, ys, xs].astype(np.int64)].astype(np.int64) - 1
        hit = (b >= 0) & (b < K)
        np.add.at(overlap[m], (am[hit], b[hit]), 1)
    return overlap, landed


def key_of(c, a, b):
    return (int(c) << 32) | ((0xFFFF - a) << 16) | (0xFFFF - b)


def admissible(c, landed_a, area_b, min_overlap):
    """One float64 product, one comparison; ``min_overlap`` goes through float32 first, as the C entry receives it."""
    return c >= 1 and float(c) >= float(np.float32(min_overlap)) * float(min(int(landed_a), int(area_b)))


def _origin(table):
    K = table.shape[0]
    origin = np.full((K,), -1, np.int32)
    for b in range(K):
        keys = [key_of(table[a, b], a, b) for a in range(K) if table[a, b] >= 1]
        if keys:
            origin[b] = 0xFFFF - ((max(keys) >> 16) & 0xFFFF)
    return origin


def np_match_objects(overlap, landed, area_next, min_overlap):
    """``raft_match_objects`` as THE WALK: the admissible pairs sorted by key, largest first, a pair taken iff both slots are free.
    Any leading axes; returns (match, match_overlap, origin)."""
    overlap, landed, area_next = np.asarray(overlap), np.asarray(landed), np.asarray(area_next)
    if overlap.ndim > 2:
        parts = [np_match_objects(o, l, r, min_overlap) for o, l, r in zip(overlap, landed, area_next)]
        return tuple(np.stack(p) for p in zip(*parts))
    K = overlap.shape[0]
    match, count = np.full((K,), -1, np.int32), np.zeros((K,), np.int32)
    pairs = [(key_of(overlap[a, b], a, b), a, b) for a in range(K) for b in range(K)
             if admissible(overlap[a, b], landed[a], area_next[b], min_overlap)]
    taken = set()
    for _, a, b in sorted(pairs, reverse=True):
        if a not in taken and match[b] < 0:
            match[b], count[b] = a, overlap[a, b]
            taken.add(a)
    return match, count, _origin(overlap)


def np_match_mutual(overlap, landed, area_next, min_overlap):
    """The rounds the kernel runs: every free a picks its best free admissible b, every free b its best free a, pairs that picked
    each other are matched, until a round matches nothing.  Returns (match, rounds that matched something)."""
    K = overlap.shape[0]
    match = np.full((K,), -1, np.int32)
    free_a, rounds = [True] * K, 0
    for _ in range(K + 1):
        best_row, best_col = [0] * K, [0] * K
        for a in range(K):
            for b in range(K):
                if free_a[a] and match[b] < 0 and admissible(overlap[a, b], landed[a], area_next[b], min_overlap):
                    key = key_of(overlap[a, b], a, b)
                    best_row[a], best_col[b] = max(best_row[a], key), max(best_col[b], key)
        any_matched = False
        for b in range(K):
            key = best_col[b]
            if key:
                a = 0xFFFF - ((key >> 16) & 0xFFFF)
                if best_row[a] == key:
                    match[b], free_a[a], any_matched = a, False, True
        if not any_matched:
            return match, rounds
        rounds += 1
    raise AssertionError('more than K rounds')


def np_chain_ids(match, count, t0, ids_in, born_in, next_id):
    """``raft_chain_object_ids`` as plain loops: (ids (S, N, K), born (S, N, K), next_id (N,) afterwards)."""
    match, count = np.asarray(match), np.asarray(count)
    S, N, K = match.shape
    ids, born = np.full((S, N, K), -1, np.int32), np.full((S, N, K), -1, np.int32)
    nxt = np.array(next_id, np.int32).copy()
    for n in range(N):
        prev_ids, prev_born = np.array(ids_in[n]), np.array(born_in[n])
        for s in range(S):
            filled = min(max(int(count[s, n]), 0), K)
            for b in range(filled):
                a = int(match[s, n, b])
                if 0 <= a < K:
                    ids[s, n, b], born[s, n, b] = prev_ids[a], prev_born[a]
                else:
                    ids[s, n, b], born[s, n, b] = nxt[n], t0 + s
                    nxt[n] += 1
            prev_ids, prev_born = ids[s, n], born[s, n]
    return ids, born, nxt


def slot_areas(labels, K):
    """The pixels of every slot of a label map, (M, K) int32: what ``raft_find_objects`` reports as ``area`` for a map it wrote."""
    return np.stack([np.bincount(l[(l >= 1) & (l <= K)].astype(np.int64) - 1, minlength=K)[:K] for l in labels]).astype(np.int32)


# ------------------------------------------------------------------ the cases (shared with the GPU tests; built once, read-only)
SPECIAL_VECTORS = np.array([0.0, 0.5, -0.5, 1.5, -1.5, 2.5, 0.49999997, -0.4, 0.4, -0.6, 0.6, -3.0, 7.25, 40.0, -80.0, np.nan, np.inf,
                            -np.inf, 3e38, -3e38, 1e10], np.float32)


def _case_specials():
    """(3, 37, 70), neither a multiple of the 32 x 16 tile: labels that touch every border, among them values above K and negative
    ones; every vector component drawn from SPECIAL_VECTORS -- halves (ties to even both ways, since x runs over even and odd
    columns), vectors that leave the frame by less than half a pixel and by more, NaN, both infinities, values near the largest
    float32."""
    rng = np.random.default_rng(310)
    M, H, W = 3, 37, 70
    prev = np.zeros((M, H, W), np.int32)
    prev[0, :, :35], prev[0, :, 35:] = 1, 2
    prev[0, 10:20, 20:50] = 3
    prev[0, 30:, 60:] = 0
    prev[1] = rng.integers(-3, 9, (H, W)).astype(np.int32)                    # a map no labelling would write: harmless all the same
    prev[2, :18], prev[2, 18:] = 130, -2147483648                             # nothing but values outside 0 .. K
    prev[2, 5:9, 5:9] = 2
    nxt = np.zeros((M, H, W), np.int32)
    nxt[0, :, :20], nxt[0, :, 25:45], nxt[0, 5:30, 50:] = 2, 1, 3
    nxt[1] = np.repeat(np.repeat(rng.integers(-1, 6, (10, 18)), 4, 0), 4, 1)[:H, :W].astype(np.int32)
    nxt[2] = rng.integers(0, 2147483647, (H, W), dtype=np.int64).astype(np.int32)
    nxt[2, :12, :12] = 1
    flow = SPECIAL_VECTORS[rng.integers(0, len(SPECIAL_VECTORS), (M, H, W, 2))]
    # the frame's edges, planted: out by less than half a pixel (in frame), by exactly half (ties to even: -0.5 -> -0 is in, 69.5 ->
    # 70 is out, 36.5 -> 36 is in) and by more
    flow[0, 0:6, 0] = [(-0.4, 0), (-0.5, 0), (-0.6, 0), (-1.5, 0), (0.4, 0), (0, 0)]
    flow[0, 0:6, W - 1] = [(0.4, 0), (0.5, 0), (0.6, 0), (1.5, 0), (-0.5, 0), (40, 0)]
    flow[0, 0, 10:14] = [(0, -0.4), (0, -0.5), (0, -0.6), (0, -2)]
    flow[0, H - 1, 10:14] = [(0, 0.4), (0, 0.5), (0, 0.6), (0, 2)]
    return dict(prev=prev, flow=flow, next=nxt)


def _rect(labels, m, label, rows, cols):
    labels[m, rows[0]:rows[1], cols[0]:cols[1]] = label


def _case_objects():
    """(2, 16, 32), one tile per image, rectangles under exact integer flows, every count known by hand (KNOWN below)."""
    M, H, W = 2, 16, 32
    prev, nxt, flow = np.zeros((M, H, W), np.int32), np.zeros((M, H, W), np.int32), np.zeros((M, H, W, 2), np.float32)
    # image 0 -- a split: previous 1 (48 px) lies still, the next pair sees it as 2 and 3 (24 px each): equal overlaps
    _rect(prev, 0, 1, (1, 7), (1, 9)), _rect(nxt, 0, 2, (1, 7), (1, 5)), _rect(nxt, 0, 3, (1, 7), (5, 9))
    # a merge: previous 2 (24 px) and 3 (36 px) become next 1 (60 px)
    _rect(prev, 0, 2, (9, 15), (1, 5)), _rect(prev, 0, 3, (9, 15), (5, 11)), _rect(nxt, 0, 1, (9, 15), (1, 11))
    # half out of frame: previous 4 (64 px) moves 4 px right, 32 px land; next 4 has 48 px of which 32 are hit
    _rect(prev, 0, 4, (2, 10), (24, 32)), _rect(nxt, 0, 4, (2, 10), (26, 32))
    flow[0, 2:10, 24:32] = (4.0, 0.0)
    # image 1 -- two objects swap places (and slots)
    _rect(prev, 1, 1, (2, 8), (2, 10)), _rect(prev, 1, 2, (2, 7), (18, 26))
    flow[1, 2:8, 2:10], flow[1, 2:7, 18:26] = (16.0, 0.0), (-16.0, 0.0)
    _rect(nxt, 1, 2, (2, 8), (18, 26)), _rect(nxt, 1, 1, (2, 7), (2, 10))
    # the boundary: previous 3 (32 px) shares 8 px = 0.25 * 32 with next 3 (32 px); previous 4 shares 16 = 0.5 * 32 with next 4
    _rect(prev, 1, 3, (10, 14), (2, 10)), _rect(nxt, 1, 3, (10, 14), (8, 16))
    _rect(prev, 1, 4, (10, 14), (18, 26)), _rect(nxt, 1, 4, (10, 14), (22, 30))
    # equal overlaps from two previous objects: 5 and 6 (8 px each) both end in next 5 (16 px): the smaller previous slot wins
    _rect(prev, 1, 5, (14, 16), (2, 6)), _rect(prev, 1, 6, (14, 16), (6, 10)), _rect(nxt, 1, 5, (14, 16), (2, 10))
    return dict(prev=prev, flow=flow, next=nxt)


def _case_empty():
    """An empty previous side, an empty next side, and neither."""
    M, H, W = 3, 16, 32
    prev, nxt = np.zeros((M, H, W), np.int32), np.zeros((M, H, W), np.int32)
    prev[1, 2:9, 3:20] = 1
    nxt[0, 2:9, 3:20] = 1
    prev[2, 4:8, 4:8], nxt[2, 4:8, 4:8] = 2, 1
    return dict(prev=prev, flow=np.zeros((M, H, W, 2), np.float32), next=nxt)


def _case_blobs():
    """Label maps as ``raft_find_objects`` writes them: tests/test_components.py's blobs and the same blobs moved by (3, 2), under
    a flow of (3, 2) plus noise of up to 0.7 px."""
    from test_components import case_args, np_find_objects
    mask = case_args('blobs')['mask']
    moved = np.roll(mask, (2, 3), axis=(1, 2))
    prev = np_find_objects(mask, 8, 10, 8)[0]
    nxt = np_find_objects(moved, 8, 10, 8)[0]
    rng = np.random.default_rng(311)
    flow = (np.array([3.0, 2.0]) + rng.uniform(-0.7, 0.7, mask.shape + (2,))).astype(np.float32)
    return dict(prev=prev.astype(np.int32), flow=flow, next=nxt.astype(np.int32))


CASES = collections.OrderedDict([('specials', _case_specials), ('objects', _case_objects), ('empty', _case_empty), ('blobs', _case_blobs)])
SLOTS = (3, 64, 128)
_BUILT, _WANT = {}, {}


def case_args(name):
    if name not in _BUILT:
        case = CASES[name]()
        for a in case.values():
            a.setflags(write=False)
        _BUILT[name] = case
    return _BUILT[name]


def want_overlap(name, K):
    """(overlap, landed, area_next) of a case by the restatement, computed once."""
    if (name, K) not in _WANT:
        c = case_args(name)
        res = np_object_overlap(c['prev'], c['flow'], c['next'], K) + (slot_areas(c['next'], K),)
        for a in res:
            a.setflags(write=False)
        _WANT[(name, K)] = res
    return _WANT[(name, K)]


def random_chain(seed, S, N, K):
    """Inputs of ``raft_chain_object_ids``: matches with values outside -1 .. K - 1 among them, counts below 0 and above K."""
    rng = np.random.default_rng(seed)
    match = rng.integers(-1, K, (S, N, K)).astype(np.int32)
    match[rng.random((S, N, K)) < 0.1] = K
    match[rng.random((S, N, K)) < 0.05] = -7
    match[rng.random((S, N, K)) < 0.05] = 1 << 20
    count = rng.integers(-2, K + 3, (S, N)).astype(np.int32)
    count[0, 0] = 0
    ids_in = rng.integers(-1, 50, (N, K)).astype(np.int32)
    born_in = rng.integers(-1, 9, (N, K)).astype(np.int32)
    next_id = rng.integers(50, 90, (N,)).astype(np.int32)
    return match, count, ids_in, born_in, next_id


# ------------------------------------------------------------------ the restatement against answers known by hand
def test_the_objects_case_by_hand():
    for K in (64, 128):
        overlap, landed, area = want_overlap('objects', K)
        assert overlap.shape == (2, K, K) and overlap.dtype == np.int32 and landed.dtype == np.int32
        assert landed[0, :4].tolist() == [48, 24, 36, 32] and area[0, :4].tolist() == [60, 24, 24, 48]       # 32 of 64 px landed
        want0 = np.zeros((K, K), np.int32)
        want0[0, 1] = want0[0, 2] = 24
        want0[1, 0], want0[2, 0], want0[3, 3] = 24, 36, 32
        np.testing.assert_array_equal(overlap[0], want0)
        want1 = np.zeros((K, K), np.int32)
        want1[0, 1], want1[1, 0], want1[2, 2], want1[3, 3], want1[4, 4], want1[5, 4] = 48, 40, 8, 16, 8, 8
        np.testing.assert_array_equal(overlap[1], want1)
        match, count, origin = np_match_objects(overlap, landed, area, 0.25)
        # the split: previous 0 goes to the smaller of the two next slots, the other half is new but names where it came from;
        # the merge: next 0 takes the larger part; half out of frame: matched
        assert match[0, :4].tolist() == [2, 0, -1, 3] and origin[0, :4].tolist() == [2, 0, 0, 3]
        assert count[0, :4].tolist() == [36, 24, 0, 32]
        # the swap; both boundary pairs admissible at 0.25; of the two equal overlaps the smaller previous slot
        assert match[1, :5].tolist() == [1, 0, 2, 3, 4] and origin[1, :5].tolist() == [1, 0, 2, 3, 4]
        assert (match[:, 5:] == -1).all() and (origin[:, 5:] == -1).all() and (count[:, 5:] == 0).all()
        half = np_match_objects(overlap, landed, area, 0.5)[0]
        assert half[1, :5].tolist() == [1, 0, -1, 3, 4]                       # 8 < 0.5 * 32, 16 == 0.5 * 32
        above = np_match_objects(overlap, landed, area, np.nextafter(np.float32(0.25), np.float32(1)))[0]
        assert above[1, 2] == -1 and above[1, 3] == 3
        whole = np_match_objects(overlap, landed, area, 1.0)[0]
        # landed is the denominator, not the area: 32 >= 1.0 * min(32 landed, 48) holds, against the 64 px of the object it would not
        assert whole[0, :4].tolist() == [2, 0, -1, 3] and whole[1, :5].tolist() == [1, 0, -1, -1, 4]
        assert not admissible(32, 64, 48, 1.0) and admissible(32, 32, 48, 1.0)
    overlap, landed, area = want_overlap('objects', 3)                        # more objects than slots: labels 4 .. 6 are background
    assert landed.tolist() == [[48, 24, 36], [48, 40, 32]] and overlap[1].tolist() == [[0, 48, 0], [40, 0, 0], [0, 0, 8]]


def test_the_specials_case_holds_what_it_is_there_for():
    c = case_args('specials')
    prev, flow = c['prev'], c['flow']
    H, W = prev.shape[1:]
    lab = (prev >= 1) & (prev <= 3)
    x = np.arange(W, dtype=np.float32)[None, None, :]
    u = flow[..., 0]
    with np.errstate(over='ignore', invalid='ignore'):
        fx = x + u
        halves = lab & np.isfinite(fx) & (fx - np.floor(fx) == 0.5)
        assert (halves & (np.rint(fx) > fx)).any() and (halves & (np.rint(fx) < fx)).any()        # ties to even, both ways
        assert (lab & (fx < 0) & (fx >= -0.5)).any() and (lab & (fx < -0.5) & (fx > -1)).any()    # out by less than half: in frame
        assert (lab & (fx > W - 1) & (np.rint(fx) == W - 1)).any() and (lab & (np.rint(fx) == W)).any()
        assert (lab & np.isnan(u)).any() and (lab & np.isposinf(u)).any() and (lab & np.isneginf(u)).any()
        assert (lab & np.isfinite(u) & (np.abs(u) > 1e38)).any()
    assert (prev > 3).any() and (prev < 0).any() and (c['next'] > 128).any() and (c['next'] < 0).any()
    for K in SLOTS:
        overlap, landed, _ = want_overlap('specials', K)
        assert (landed >= overlap.sum(-1)).all() and (landed > overlap.sum(-1)).any()             # pixels landing on background
        assert landed.sum() > 0 and overlap.sum() > 0
    overlap, landed, _ = want_overlap('specials', 3)
    assert (overlap[0] > 0).sum() >= 6 and landed[2].tolist() == [0, int(landed[2, 1]), 0] and landed[2, 1] > 0
    overlap, landed, _ = want_overlap('empty', 64)
    assert overlap[:2].sum() == 0 and landed[0].sum() == 0 and landed[1, 0] == 7 * 17 and overlap[2, 1, 0] == 16


def test_the_blobs_move_with_their_flow():
    overlap, landed, area = want_overlap('blobs', 64)
    match, count, origin = np_match_objects(overlap, landed, area, 0.25)
    filled = (area > 0).sum(-1)
    assert filled.tolist() == [4, 1]
    for m in range(2):
        assert sorted(match[m, :filled[m]].tolist()) == list(range(filled[m]))       # everybody is found again
        assert (match[m, filled[m]:] == -1).all()
    np.testing.assert_array_equal(match, origin)


def test_the_rounds_of_mutual_best_picks_are_the_walk():
    rng = np.random.default_rng(312)
    most = 0
    for trial in range(300):
        K = int(rng.integers(1, 9))
        table = rng.integers(0, 6, (K, K)).astype(np.int32) * (rng.random((K, K)) < 0.6)      # small counts: many ties
        landed = np.maximum(table.sum(1) + rng.integers(0, 4, K), 0).astype(np.int32)
        area = (table.sum(0) + rng.integers(0, 4, K)).astype(np.int32)
        share = float(rng.choice([0.05, 0.25, 0.5, 1.0]))
        walk = np_match_objects(table, landed, area, share)[0]
        mutual, rounds = np_match_mutual(table, landed, area, share)
        np.testing.assert_array_equal(mutual, walk)
        assert rounds <= K
        most = max(most, rounds)
    assert most >= 3                                                         # the rounds were needed
    # a chain that needs K rounds: every pair but the largest waits for the one above it
    K = 6
    table = np.zeros((K, K), np.int32)
    for i in range(K):
        table[i, i] = 2 * (K - i)
        if i + 1 < K:
            table[i + 1, i] = 2 * (K - i) - 1
    ones = np.ones((K,), np.int32)
    mutual, rounds = np_match_mutual(table, ones, ones, 1.0)
    assert rounds == K and mutual.tolist() == list(range(K))
    np.testing.assert_array_equal(mutual, np_match_objects(table, ones, ones, 1.0)[0])


def test_chained_ids_by_hand():
    K = 4
    match = np.array([[[-1, -1, -1, -1]], [[1, -1, 0, 7]], [[2, 2, -1, 0]]], np.int32)       # (S = 3, N = 1, K)
    count = np.array([[2], [3], [9]], np.int32)
    start = np.full((1, K), -1, np.int32)
    ids, born, nxt = np_chain_ids(match, count, 5, start, start, np.zeros((1,), np.int32))
    assert ids[:, 0].tolist() == [[0, 1, -1, -1], [1, 2, 0, -1], [0, 0, 3, 1]]               # (two slots may name one ancestor:
    assert born[:, 0].tolist() == [[5, 5, -1, -1], [5, 6, 5, -1], [5, 5, 7, 5]]              # only raft_match_objects is one-to-one)
    assert nxt.tolist() == [4]
    # S steps are S single steps
    match, count, ids_in, born_in, next_id = random_chain(313, 5, 3, 7)
    ids, born, nxt = np_chain_ids(match, count, 2, ids_in, born_in, next_id)
    state = (ids_in, born_in, next_id)
    for s in range(5):
        i1, b1, n1 = np_chain_ids(match[s:s + 1], count[s:s + 1], 2 + s, *state)
        np.testing.assert_array_equal(i1[0], ids[s]), np.testing.assert_array_equal(b1[0], born[s])
        state = (i1[0], b1[0], n1)
    np.testing.assert_array_equal(state[2], nxt)


# ------------------------------------------------------------------ the C entries
ENTRIES = ('raft_object_overlap', 'raft_match_objects', 'raft_chain_object_ids')


def test_the_header_declares_and_the_library_exports_the_entries():
    from tf_raft_amd import build, image_ops
    assert 'object_track.hip' in build.SOURCES
    with open(os.path.join(ROOT, 'include', 'raft_hip.h')) as f:
        text = f.read()
    header = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    sigs = _ffi.header_signatures(text)
    P, I, F = C.c_void_p, C.c_int, C.c_float
    assert sigs['raft_object_overlap'] == (I, [P, P, P, P, P, I, I, I, I, P])
    assert sigs['raft_match_objects'] == (I, [P, P, P, F, P, P, P, I, I, P])
    assert sigs['raft_chain_object_ids'] == (I, [P, P, I, P, P, P, P, P, I, I, I, P])
    assert set(ENTRIES) <= set(_ffi.EXPORTED_SYMBOLS)
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, header)
    assert _ffi.ABI_VERSION == 222                                   # entries were added, no signature changed
    lib = _ffi.load_library()
    assert lib.raft_version() == 222
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == sigs[name][1] and getattr(lib, name).restype is sigs[name][0]
    consts = _ffi.header_constants(text)
    assert consts['RAFT_TRACK_OBJECTS_MAX'] == image_ops.OBJECT_TRACK_MAX == MAX_SLOTS
    assert image_ops.OBJECT_MIN_OVERLAP == 0.25
    src = open(os.path.join(ROOT, 'tf_raft_amd', 'csrc', 'object_track.hip')).read()
    assert '#pragma clang fp contract(off)' in src
    assert not re.search(r'atomic\w*\s*\(\s*\(?\s*float', src)        # no float atomic


def test_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the memset or the launch (a positive hipError_t) or crash."""
    lib = _ffi.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off1, off2 = C.c_void_p(p.value + 1), C.c_void_p(p.value + 2)
    # ---- overlap
    #       prev flow next overlap landed M  H   W   K  stream
    good = [p, p, p, p, p, 2, 37, 70, 64, None]
    fn = lib.raft_object_overlap
    for k in range(5):
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    for bad in ((0, 5, 3), (1, -5, 3), (1, 5, 0), (1, 1 << 16, 1 << 15), (2, 1 << 15, 1 << 15), (1 << 20, 1 << 6, 1 << 5)):
        args = list(good)
        args[5:8] = bad
        assert fn(*args) == -2, bad
    for K in (0, -1, 129, 1 << 20):
        args = list(good)
        args[8] = K
        assert fn(*args) == -2, K
    for k in range(5):
        for off in (off1, off2):
            args = list(good)
            args[k] = off
            assert fn(*args) == -4, k
    args = list(good)
    args[0], args[8], args[1] = None, 0, off1                                # precedence: NULL before shape before alignment
    assert fn(*args) == -1
    args[0] = p
    assert fn(*args) == -2
    args[8] = 128
    assert fn(*args) == -4
    # ---- matching
    #       overlap landed area share match count origin M  K  stream
    good = [p, p, p, 0.25, p, p, p, 2, 64, None]
    fn = lib.raft_match_objects
    for k in (0, 1, 2, 4):
        for opt in (p, None):                                                # (match_overlap and origin may be NULL)
            args = list(good)
            args[k], args[5], args[6] = None, opt, opt
            assert fn(*args) == -1, k
    for k, values in {3: (0.0, -0.25, 1.0000001, 2.0, float('nan'), float('inf'), -float('inf')), 7: (0, -1), 8: (0, -1, 129)}.items():
        for v in values:
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for k in (0, 1, 2, 4, 5, 6):
        args = list(good)
        args[k] = off1
        assert fn(*args) == -4, k
    args = list(good)
    args[4], args[3], args[6] = None, 1.5, off2
    assert fn(*args) == -1
    args[4] = p
    assert fn(*args) == -2
    args[3] = 1.0
    assert fn(*args) == -4
    # ---- chaining
    #       match count t0 ids_in born_in next_id ids born S  N  K  stream
    good = [p, p, 0, p, p, p, p, p, 3, 2, 64, None]
    fn = lib.raft_chain_object_ids
    for k in (0, 1, 3, 4, 5, 6, 7):
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    for k, values in {2: (-1, -(1 << 31)), 8: (0, -1), 9: (0, -3), 10: (0, -1, 129)}.items():
        for v in values:
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    args = list(good)
    args[8:11] = (1 << 15, 1 << 10, 64)                                      # S * N * K = 2^31
    assert fn(*args) == -2
    for k in (0, 1, 3, 4, 5, 6, 7):
        args = list(good)
        args[k] = off2
        assert fn(*args) == -4, k
    args = list(good)
    args[7], args[2], args[0] = None, -1, off1
    assert fn(*args) == -1
    args[7] = p
    assert fn(*args) == -2
    args[2] = 7
    assert fn(*args) == -4


# ------------------------------------------------------------------ the Python layer, nothing reaches the device
class _Side:
    def __init__(self, labels, area):
        self.labels, self.area = labels, area


def test_the_public_functions_check_their_arguments_without_a_gpu():
    import torch
    from tf_raft_amd import image_ops
    assert image_ops.check_object_track_args(128, 1.0) == (128, 1.0)
    assert image_ops.check_object_track_args(np.int64(3), np.float32(0.25)) == (3, 0.25)
    assert image_ops.check_object_track_args(1, 1e-30)[1] > 0
    for bad in (0, -1, 129, 64.0, True, None, '4'):
        with pytest.raises(ValueError, match='max_objects must be an integer in 1 .. 128'):
            image_ops.check_object_track_args(bad)
    for bad in (0, 0.0, -0.25, 1.0000001, 2, float('nan'), float('inf'), 1e-60):
        with pytest.raises(ValueError, match='min_overlap must lie in'):
            image_ops.check_object_track_args(4, bad)
    for bad in (None, '0.25', True):
        with pytest.raises(ValueError, match='min_overlap must be a number'):
            image_ops.check_object_track_args(4, bad)
    assert image_ops.ObjectMatch._fields == ('match', 'overlap', 'origin')
    labels, area, flow = np.zeros((2, 40, 50), np.int32), np.zeros((2, 8), np.int32), np.zeros((2, 40, 50, 2), np.float32)
    good = _Side(labels, area)
    call = image_ops.match_objects
    with pytest.raises(ValueError, match='min_overlap must lie in'):
        call(good, flow, good, min_overlap=0.0)
    with pytest.raises(ValueError, match='needs prev.labels'):
        call(_Side(None, area), flow, good)
    with pytest.raises(ValueError, match='needs prev.labels'):
        call(good, flow, _Side(labels, None))
    with pytest.raises(TypeError, match='is int32'):
        call(_Side(labels.astype(np.int64), area), flow, good)
    with pytest.raises(TypeError, match='is int32'):
        call(good, flow, _Side(labels, area.astype(np.uint8)))
    with pytest.raises(ValueError, match=r'expects next.labels'):
        call(good, flow, _Side(labels[:, :39], area))
    with pytest.raises(ValueError, match=r'expects labels'):
        call(_Side(labels[0, 0], area), flow, good)
    with pytest.raises(ValueError, match=r'expects next.area'):
        call(good, flow, _Side(labels, area[0]))
    with pytest.raises(ValueError, match='max_objects must be an integer in 1 .. 128'):
        call(good, flow, _Side(labels, np.zeros((2, 129), np.int32)))
    with pytest.raises(ValueError, match='expects a flow'):
        call(good, flow[..., :1], good)
    with pytest.raises(TypeError, match='a flow is float32'):
        call(good, flow.astype(np.uint8), good)
    big = torch.empty((1 << 11, 1 << 10, 1 << 10), dtype=torch.int32, device='meta')
    with pytest.raises(ValueError, match='too large'):
        call(_Side(big, None), torch.empty((1 << 11, 1 << 10, 1 << 10, 2), device='meta'),
             _Side(big, torch.empty((1 << 11, 4), dtype=torch.int32, device='meta')))


def test_the_launch_functions_check_their_tensors_without_a_gpu():
    import torch
    from tf_raft_amd import image_ops
    labels, flow = torch.zeros((2, 40, 50), dtype=torch.int32), torch.zeros((2, 40, 50, 2))
    fn = image_ops.object_overlap_launch
    with pytest.raises(ValueError, match='expected int32 labels'):
        fn(labels.numpy(), flow, labels, 4)
    with pytest.raises(ValueError, match='expected int32 labels'):
        fn(labels[0], flow, labels, 4)
    with pytest.raises(ValueError, match='labels_prev must be'):
        fn(labels.to(torch.int64), flow, labels, 4)
    with pytest.raises(ValueError, match='labels_next must be'):
        fn(labels, flow, labels[:1], 4)
    with pytest.raises(ValueError, match='labels_next must be'):
        fn(labels, flow, labels.permute(0, 2, 1), 4)
    with pytest.raises(ValueError, match='need a flow'):
        fn(labels, flow[:, :, :, :1], labels, 4)
    with pytest.raises(TypeError, match='a flow is float32'):
        fn(labels, flow.to(torch.float64), labels, 4)
    for bad in (0, 129, 4.0):
        with pytest.raises(ValueError, match='max_objects must'):
            fn(labels, flow, labels, bad)
    table, row = torch.zeros((2, 8, 8), dtype=torch.int32), torch.zeros((2, 8), dtype=torch.int32)
    fn = image_ops.match_objects_launch
    with pytest.raises(ValueError, match='expected an int32 overlap table'):
        fn(table[:, :, :7], row, row)
    with pytest.raises(ValueError, match='expected an int32 overlap table'):
        fn(table[0], row, row)
    with pytest.raises(ValueError, match='overlap must be'):
        fn(table.to(torch.float32), row, row)
    with pytest.raises(ValueError, match='landed must be'):
        fn(table, row[:1], row)
    with pytest.raises(ValueError, match='area_next must be'):
        fn(table, row, row.to(torch.int64))
    with pytest.raises(ValueError, match='min_overlap must lie in'):
        fn(table, row, row, 1.5)
    with pytest.raises(ValueError, match='max_objects must'):
        fn(torch.zeros((1, 129, 129), dtype=torch.int32), row, row)
    match, count, one = torch.zeros((3, 2, 8), dtype=torch.int32), torch.zeros((3, 2), dtype=torch.int32), torch.zeros((2,), dtype=torch.int32)
    fn = image_ops.chain_object_ids_launch
    with pytest.raises(ValueError, match='expected int32 matches'):
        fn(match[0], count, 0, row, row, one)
    with pytest.raises(ValueError, match='count must be'):
        fn(match, count[:2], 0, row, row, one)
    with pytest.raises(ValueError, match='ids must be'):
        fn(match, count, 0, row[:1], row, one)
    with pytest.raises(ValueError, match='born must be'):
        fn(match, count, 0, row, row.to(torch.int16), one)
    with pytest.raises(ValueError, match='next_id must be'):
        fn(match, count, 0, row, row, one[:1])
    with pytest.raises(ValueError, match='out must be a pair'):
        fn(match, count, 0, row, row, one, out=match)
    with pytest.raises(ValueError, match='out must be a contiguous'):
        fn(match, count, 0, row, row, one, out=(match, match[:1]))
    for bad in (-1, 1.0, True):
        with pytest.raises(ValueError):
            fn(match, count, bad, row, row, one)


def test_the_tracker_and_the_video_call_check_their_arguments_before_any_device_work():
    import inspect
    from tf_raft_amd import model, video
    assert video.TrackedObjects._fields == model.MovingObjects._fields + ('ids', 'born', 'match', 'origin')
    assert video.ObjectTracks._fields == ('count', 'ids', 'born', 'area', 'boxes', 'centroid', 'mean_flow', 'labels')
    for name in ('object_tracker', 'track_objects_video'):
        assert getattr(model.SmallRAFT, name) is getattr(model.RAFT, name)
        sig = inspect.signature(getattr(model.RAFT, name))
        assert sig.parameters['max_objects'].default == 64 and sig.parameters['min_overlap'].default == 0.25
    assert inspect.signature(model.RAFT.track_objects_video).parameters['batch_size'].default == 4
    make = model.RAFT.object_tracker
    for kw, error, match in ((dict(max_objects=129), ValueError, 'max_objects must'), (dict(max_objects=0), ValueError, 'max_objects must'),
                             (dict(min_overlap=0), ValueError, 'min_overlap must'), (dict(min_overlap=1.5), ValueError, 'min_overlap must'),
                             (dict(min_area=0), ValueError, 'min_area must'), (dict(connectivity=6), ValueError, 'connectivity must'),
                             (dict(model='rigid'), ValueError, 'model must'), (dict(threshold=-1.0), ValueError, 'threshold must'),
                             (dict(occlusion_test='none'), ValueError, 'occlusion_test'), (dict(speed=3), TypeError, 'unexpected keyword')):
        with pytest.raises(error, match=match):
            make(None, **kw)                                                 # (raised before `self` is touched)
        with pytest.raises(error, match=match):
            model.RAFT.track_objects_video(None, np.zeros((3, 64, 64, 3), np.uint8), **kw)
    tracker = make(None, max_objects=128, min_overlap=1.0, min_area=12, alpha=1.9)
    assert tracker.max_objects == 128 and tracker.min_overlap == 1.0 and tracker.ids is None
    for bad in (np.zeros((64, 64, 3), np.uint8), np.zeros((1, 64, 64, 1), np.uint8), np.zeros((0, 64, 64, 3), np.uint8)):
        with pytest.raises(ValueError, match='frames must be'):
            tracker.push(bad)
    run = model.RAFT.track_objects_video
    with pytest.raises(ValueError, match='frames must be one video'):
        run(None, np.zeros((64, 64, 3), np.uint8))
    with pytest.raises(ValueError, match='frames must be one video'):
        run(None, np.zeros((3, 64, 64, 1), np.uint8))
    with pytest.raises(ValueError, match='at least two frames'):
        run(None, np.zeros((1, 64, 64, 3), np.uint8))
    with pytest.raises(TypeError, match='unsupported type int32'):
        run(None, np.zeros((3, 64, 64, 3), np.int32))
    with pytest.raises(TypeError, match='uint8 or float32'):
        run(None, np.zeros((3, 64, 64, 3), np.bool_))
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='batch_size must be'):
            run(None, np.zeros((3, 64, 64, 3), np.uint8), batch_size=bad)

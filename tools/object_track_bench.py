"""Measurements behind docs/NOTEBOOK.md section 44 (object identity through a video), all in one job.

  python tools/object_track_bench.py [kernels] [model]      (no argument: both)
      kernels  label maps (4, 1080, 1920) of two kinds, made by raft_find_objects (K = 64, min_area 64) from a mask and from the
               same mask moved by (3, 2) pixels, under a flow of (3, 2) plus noise of half a pixel -- (a) `blobs`: a few dozen
               filled ellipses per image, what a `moving` mask looks like; (b) `busy`: an 8 x 8 grid of rectangles a pixel apart,
               64 objects over 98 % of the frame, so nearly every pixel lands, counts and gathers -- through raft_object_overlap,
               raft_match_objects and raft_chain_object_ids (N = 4 videos, one step; one video, four steps); next to them, in the
               same job, raft_find_objects on the same masks and raft_stream_copy_f32 at the overlap kernel's compulsory 16 bytes
               per pixel (a label and a vector read, a label gathered).  HIP-event times of back-to-back calls, alternating in one
               process, three rounds.
      model    an ObjectTracker push against moving_objects_step alone at 4 videos of 448 x 512 uint8, SmallRAFT and RAFT at
               iters_pred 12, on a texture that shifts by two pixels, with alpha = 1.9 and threshold = 5 pixels as in
               tools/objects_bench.py (random weights fail UnFlow's forward-backward test nearly everywhere).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402
from objects_bench import _fmt, _masks, _measure, _timed      # noqa: E402

SHAPE = (4, 1080, 1920)
K, MIN_AREA, CONN = 64, 64, 8
MODEL, ITERS = (4, 448, 512), 12


def _grid_mask(N, H, W):
    m = torch.ones((N, H, W), device='cuda', dtype=torch.uint8)
    for i in range(1, 8):
        m[:, i * H // 8, :] = 0
        m[:, :, i * W // 8] = 0
    return m


class _Entries:
    def __init__(self):
        from tf_raft_amd import _dev, image_ops
        from tf_raft_amd._ffi import check
        self.dev, self.check, self.lib = _dev, check, _dev.lib()
        N, H, W = SHAPE
        g = torch.Generator(device='cuda').manual_seed(0)
        self.masks = {'blobs': _masks(N, H, W, g)['blobs'], 'busy': _grid_mask(N, H, W)}
        self.flow = (torch.tensor([3.0, 2.0], device='cuda') + torch.rand((N, H, W, 2), device='cuda', generator=g) - 0.5).contiguous()
        self.sides = {}
        for kind, m in self.masks.items():
            prev = image_ops.find_objects_launch(m, K, MIN_AREA, CONN)
            nxt = image_ops.find_objects_launch(torch.roll(m, (2, 3), (1, 2)).contiguous(), K, MIN_AREA, CONN)
            self.sides[kind] = (prev.labels, nxt.labels, nxt.area, nxt.count)
        self.overlap = torch.empty((N, K, K), device='cuda', dtype=torch.int32)
        self.landed = torch.empty((N, K), device='cuda', dtype=torch.int32)
        self.match = torch.empty((N, K), device='cuda', dtype=torch.int32)
        self.match_overlap, self.origin = torch.empty_like(self.match), torch.empty_like(self.match)
        self.ids, self.born = torch.full((N, K), -1, device='cuda', dtype=torch.int32), torch.full((N, K), -1, device='cuda', dtype=torch.int32)
        self.next_id = torch.zeros((N,), device='cuda', dtype=torch.int32)
        self.ids_out, self.born_out = torch.empty((N, K), device='cuda', dtype=torch.int32), torch.empty((N, K), device='cuda', dtype=torch.int32)
        self.ws = torch.empty((image_ops.components_workspace_bytes(N, H, W, CONN, 1),), device='cuda', dtype=torch.uint8)
        self.find_out = (torch.empty((N, H, W), device='cuda', dtype=torch.int32), torch.empty((N,), device='cuda', dtype=torch.int32),
                         torch.empty((N, K), device='cuda', dtype=torch.int32), torch.empty((N, K, 4), device='cuda', dtype=torch.int32),
                         torch.empty((N, K, 2), device='cuda'))

    def overlap_(self, kind):
        N, H, W = SHAPE
        p = self.dev.ptr
        prev, nxt, _, _ = self.sides[kind]
        self.check(self.lib.raft_object_overlap(p(prev), p(self.flow), p(nxt), p(self.overlap), p(self.landed), N, H, W, K,
                                                self.dev.stream_ptr()), 'object_overlap')

    def match_(self, kind):
        p = self.dev.ptr
        self.check(self.lib.raft_match_objects(p(self.overlap), p(self.landed), p(self.sides[kind][2]), 0.25, p(self.match),
                                               p(self.match_overlap), p(self.origin), SHAPE[0], K, self.dev.stream_ptr()), 'match_objects')

    def chain_(self, kind, S):
        p = self.dev.ptr
        N = SHAPE[0] // S
        self.check(self.lib.raft_chain_object_ids(p(self.match), p(self.sides[kind][3]), 1, p(self.ids), p(self.born), p(self.next_id),
                                                  p(self.ids_out), p(self.born_out), S, N, K, self.dev.stream_ptr()), 'chain_object_ids')

    def find_(self, kind):
        N, H, W = SHAPE
        p = self.dev.ptr
        labels, count, area, boxes, centroid = self.find_out
        self.check(self.lib.raft_find_objects(p(self.masks[kind]), None, None, p(labels), p(count), p(area), p(boxes), p(centroid), None,
                                              N, H, W, CONN, MIN_AREA, K, p(self.ws), self.dev.stream_ptr()), 'find_objects')

    def runs(self, kind):
        return [(f'{kind}: object_overlap, K = {K}', lambda: self.overlap_(kind)),
                (f'{kind}: match_objects, K = {K}', lambda: self.match_(kind)),
                (f'{kind}: chain_object_ids, 4 videos x 1 step', lambda: self.chain_(kind, 1)),
                (f'{kind}: chain_object_ids, 1 video x 4 steps', lambda: self.chain_(kind, 4)),
                (f'{kind}: find_objects, K = {K}, no flow', lambda: self.find_(kind))]


def kernels(rounds=3):
    e = _Entries()
    N, H, W = SHAPE
    px = N * H * W
    p, st = e.dev.ptr, e.dev.stream_ptr
    n = px * 2                                       # floats of a copy that moves 16 bytes per pixel (4 read + 4 written per float)
    a, b = torch.randn((n,), device='cuda'), torch.empty((n,), device='cuda')

    def copy():
        e.check(e.lib.raft_stream_copy_f32(p(a), p(b), n, st()), 'stream_copy')
    k_copy = 'stream copy of 16 bytes per pixel'
    runs = [r for kind in e.masks for r in e.runs(kind)] + [(k_copy, copy)]
    for kind in e.masks:                             # (the matching reads what the overlap wrote for ITS kind: fill it first)
        e.overlap_(kind)
    t = _measure(runs, rounds)
    for k, _ in runs:
        print(f'{k} at {SHAPE}, us per call: {_fmt(t[k])}  min {min(t[k]):.1f}  spread {max(t[k]) - min(t[k]):.1f}', flush=True)
    best = {k: min(v) for k, v in t.items()}
    for kind in e.masks:
        k_over, k_find = e.runs(kind)[0][0], e.runs(kind)[4][0]
        total = sum(best[e.runs(kind)[i][0]] for i in range(3))
        print(f'{kind}: object_overlap {best[k_over] / best[k_copy]:.2f} x the stream copy of its compulsory bytes, {best[k_over] / best[k_find]:.2f} x '
              f'find_objects; overlap + match + chain {total:.1f} us = {total / best[k_find]:.2f} x find_objects', flush=True)
    for kind in e.masks:
        e.overlap_(kind), e.match_(kind)
        torch.cuda.synchronize()
        first = [x.clone() for x in (e.overlap, e.landed, e.match, e.match_overlap, e.origin)]
        e.overlap_(kind), e.match_(kind)
        torch.cuda.synchronize()
        same = all(x.equal(y) for x, y in zip(first, (e.overlap, e.landed, e.match, e.match_overlap, e.origin)))
        prev, _, area, count = e.sides[kind]
        print(f'({kind}: labelled share {float((prev > 0).float().mean()):.3f}, count {count.tolist()}, pairs with a count '
              f'{(e.overlap > 0).sum((1, 2)).tolist()}, matched {(e.match >= 0).sum(1).tolist()}, landed share '
              f'{float(e.landed.sum()) / max(float((prev > 0).sum()), 1.0):.3f}; repeat bit-identical: {same})', flush=True)


def model(repeats=5, steps=4):
    from tf_raft_amd import weights as wm
    N, H, W = MODEL
    g = torch.Generator(device='cuda').manual_seed(1)
    base = (torch.rand((N, H + 8, W + 8, 3), device='cuda', generator=g) * 255).to(torch.uint8)
    frames = [base[:, 4 + t:4 + t + H, 4 - 2 * (t % 2):4 - 2 * (t % 2) + W].contiguous() for t in range(2)]
    kw = dict(alpha=1.9, threshold=5.0)
    for name, cls in (('small', tf_raft_amd.SmallRAFT), ('raft', tf_raft_amd.RAFT)):
        net = cls(weights=wm.init_weights(name, seed=0), iters_pred=ITERS)
        tracker = net.object_tracker(max_objects=64, **kw)
        state = {'t': 0}

        def push():
            state['t'] += 1
            return tracker.push(frames[state['t'] % 2])

        def step():
            state['t'] += 1
            return net.moving_objects_step((frames[(state['t'] + 1) % 2], frames[state['t'] % 2]), max_objects=64, **kw)
        calls = {'moving_objects_step': step, 'ObjectTracker.push': push}
        for fn in calls.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for _ in range(repeats):
            for k, fn in calls.items():
                t[k].append(_timed(fn, steps))
        for k in calls:
            print(f"{name}: {k}, {N} x {H} x {W} uint8, iters_pred={ITERS}, ms per call: {' '.join(f'{x:.3f}' for x in t[k])}  "
                  f'mean {np.mean(t[k]):.3f} spread {max(t[k]) - min(t[k]):.3f}', flush=True)
        extra = np.mean(t['ObjectTracker.push']) - np.mean(t['moving_objects_step'])
        res = push()
        print(f"{name}: identity costs {1e3 * extra:.1f} us per push (ratio {np.mean(t['ObjectTracker.push']) / np.mean(t['moving_objects_step']):.4f}); "
              f'objects {res.count.tolist()}, matched {(res.match >= 0).sum(1).tolist()}, ids handed out {tracker._next_id.tolist()} '
              f'(random weights, a shifted texture)', flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('object_track_bench.py measures on a GPU; none is visible')
    for mode in sys.argv[1:] or ['kernels', 'model']:
        {'kernels': kernels, 'model': model}[mode]()

"""Measurements behind docs/NOTEBOOK.md section 43 (connected components and moving objects), all in one job.

  python tools/objects_bench.py [kernels] [model] [profile]      (no argument: kernels and model)
      kernels  uint8 masks (4, 1080, 1920) of three kinds -- (a) `blobs`: a few dozen filled ellipses per image, what a `moving` mask
               looks like; (b) `noise`: uniform noise at 50 % density, the worst case for merges; (c) `full`: all foreground, one
               component, the deepest chains -- through raft_label_components, raft_find_objects (K = 64, min_area 64) with and
               without a flow, and raft_remove_small_components, 8-connectivity; next to them raft_flow_residual_f32 on the same
               slices and raft_stream_copy_f32 at labelling's compulsory 5 bytes per pixel (1 read, 4 written).  HIP-event times of
               back-to-back calls, alternating in one process, three rounds.
      model    moving_objects_step against camera_motion_step at 4 pairs of 448 x 512 uint8, SmallRAFT and RAFT at iters_pred 12, on a
               texture that shifts by two pixels.  Random weights fail UnFlow's forward-backward test nearly everywhere, which would
               leave no foreground at all, so both steps run with alpha = 1.9 (about half the pixels pass) and threshold = 5 pixels.
      profile  a few calls of every entry on every mask and nothing else: the program of a `rocprofv3 --kernel-trace --stats` run,
               which says which launch takes the time.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402

SHAPE = (4, 1080, 1920)
K, MIN_AREA, CONN = 64, 64, 8
MODEL, ITERS = (4, 448, 512), 12


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _fmt(v):
    return ' '.join(f'{x:.1f}' for x in v)


def _measure(runs, rounds, budget_ms=150.0):
    """runs: (name, call) -> {name: [us per call, one per round]}, the calls alternating inside every round; a call is repeated
    until about `budget_ms` have gone (2 .. 20 times), judged by one timed call after the warm-up."""
    reps = {}
    for k, run in runs:
        run()
        run()
        reps[k] = int(min(20, max(2, budget_ms / max(_timed(run, 1), 1e-3))))
    torch.cuda.synchronize()
    t = {k: [] for k, _ in runs}
    for _ in range(rounds):
        for k, run in runs:
            t[k].append(_timed(run, reps[k]) * 1e3)
    return t


def _masks(N, H, W, g):
    yy = torch.arange(H, device='cuda', dtype=torch.float32)[None, :, None]
    xx = torch.arange(W, device='cuda', dtype=torch.float32)[None, None, :]
    blobs = torch.zeros((N, H, W), device='cuda', dtype=torch.bool)
    for _ in range(36):                                   # filled ellipses of 10 .. 120 pixels half-axes, some overlapping
        cy, cx = (torch.rand((N, 1, 1), device='cuda', generator=g) * s for s in (H, W))
        ry, rx = (10 + torch.rand((N, 1, 1), device='cuda', generator=g) * 110 for _ in range(2))
        blobs |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    blobs |= torch.rand((N, H, W), device='cuda', generator=g) < 0.002          # and specks
    noise = torch.rand((N, H, W), device='cuda', generator=g) < 0.5
    full = torch.ones((N, H, W), device='cuda', dtype=torch.bool)
    return {'blobs': blobs.to(torch.uint8).contiguous(), 'noise': noise.to(torch.uint8).contiguous(), 'full': full.to(torch.uint8)}


class _Entries:
    def __init__(self):
        from tf_raft_amd import _dev, image_ops
        from tf_raft_amd._ffi import check
        self.dev, self.check, self.lib = _dev, check, _dev.lib()
        N, H, W = SHAPE
        g = torch.Generator(device='cuda').manual_seed(0)
        self.masks = _masks(N, H, W, g)
        self.flow = (torch.randn((N, H, W, 2), device='cuda', generator=g) * 3).contiguous()
        self.labels = torch.empty((N, H, W), device='cuda', dtype=torch.int32)
        self.small = torch.empty((N, H, W), device='cuda', dtype=torch.uint8)
        self.count = torch.empty((N,), device='cuda', dtype=torch.int32)
        self.area = torch.empty((N, K), device='cuda', dtype=torch.int32)
        self.boxes = torch.empty((N, K, 4), device='cuda', dtype=torch.int32)
        self.centroid = torch.empty((N, K, 2), device='cuda')
        self.mean_flow = torch.empty((N, K, 2), device='cuda')
        self.ws = torch.empty((image_ops.components_workspace_bytes(N, H, W, CONN, 1),), device='cuda', dtype=torch.uint8)

    def label(self, m):
        N, H, W = SHAPE
        p = self.dev.ptr
        self.check(self.lib.raft_label_components(p(m), None, p(self.labels), N, H, W, CONN, p(self.ws), self.dev.stream_ptr()), 'label')

    def find(self, m, flow):
        N, H, W = SHAPE
        p = self.dev.ptr
        self.check(self.lib.raft_find_objects(p(m), None, p(self.flow) if flow else None, p(self.labels), p(self.count), p(self.area),
                                              p(self.boxes), p(self.centroid), p(self.mean_flow) if flow else None, N, H, W, CONN, MIN_AREA,
                                              K, p(self.ws), self.dev.stream_ptr()), 'find_objects')

    def remove(self, m):
        N, H, W = SHAPE
        p = self.dev.ptr
        self.check(self.lib.raft_remove_small_components(p(m), None, p(self.small), N, H, W, CONN, MIN_AREA, p(self.ws),
                                                         self.dev.stream_ptr()), 'remove_small')

    def runs(self, kind):
        m = self.masks[kind]
        return [(f'{kind}: label_components', lambda: self.label(m)),
                (f'{kind}: find_objects, K = {K}, no flow', lambda: self.find(m, False)),
                (f'{kind}: find_objects, K = {K}, with flow', lambda: self.find(m, True)),
                (f'{kind}: remove_small_components, min_area = {MIN_AREA}', lambda: self.remove(m))]


def kernels(rounds=3):
    e = _Entries()
    N, H, W = SHAPE
    px = N * H * W
    p, st = e.dev.ptr, e.dev.stream_ptr
    motion = torch.tensor([[1.0, 0.0, 0.5], [0.0, 1.0, -0.5]], device='cuda').repeat(N, 1, 1).contiguous()
    residual, moving = torch.empty((N, H, W, 2), device='cuda'), torch.empty((N, H, W), device='cuda', dtype=torch.uint8)

    def flow_residual():
        e.check(e.lib.raft_flow_residual_f32(p(e.flow), p(motion), p(residual), p(moving), N, H, W, 1.0, st()), 'flow_residual')
    n = (px * 5 // 8) // 4 * 4                       # floats of a copy that moves 5 bytes per pixel (4 read + 4 written per float)
    a, b = torch.randn((n,), device='cuda'), torch.empty((n,), device='cuda')

    def copy():
        e.check(e.lib.raft_stream_copy_f32(p(a), p(b), n, st()), 'stream_copy')
    refs = [('flow_residual_f32 (residual + moving) on the same slices', flow_residual), ('stream copy of 5 bytes per pixel', copy)]
    runs = [r for kind in e.masks for r in e.runs(kind)] + refs
    t = _measure(runs, rounds)
    for k, _ in runs:
        print(f'{k} at {SHAPE}, us per call: {_fmt(t[k])}  min {min(t[k]):.1f}  spread {max(t[k]) - min(t[k]):.1f}', flush=True)
    best = {k: min(v) for k, v in t.items()}
    k_res, k_copy = refs[0][0], refs[1][0]
    for k, _ in runs[:-2]:
        print(f'{k}: {best[k] / best[k_res]:.2f} x flow_residual, {best[k] / best[k_copy]:.2f} x the stream copy of the compulsory bytes',
              flush=True)
    for kind in e.masks:
        print(f'{kind} / blobs: ' + ', '.join(f'{name.split(": ")[1].split(",")[0]} {best[name] / best[name.replace(kind, "blobs", 1)]:.2f}'
                                              for name, _ in e.runs(kind)), flush=True)
    for kind, m in e.masks.items():
        e.find(m, True)
        torch.cuda.synchronize()
        first = [t_.clone() for t_ in (e.labels, e.count, e.area, e.boxes, e.centroid, e.mean_flow)]
        off = 2 * ((px * 4 + 7) // 8 * 8) + px * 4
        cands = e.ws[off:off + N * 4].view(torch.int32).tolist()
        e.find(m, True)
        torch.cuda.synchronize()
        same = all(x.view(torch.int32).equal(y.view(torch.int32)) for x, y in
                   zip(first, (e.labels, e.count, e.area, e.boxes, e.centroid, e.mean_flow)))
        e.label(m)
        comps = [int(torch.unique(e.labels[i]).numel()) - int((e.labels[i] == 0).any()) for i in range(N)]
        print(f'({kind}: foreground {float(m.float().mean()):.3f}, components per image {comps}, of at least {MIN_AREA} pixels {cands}, '
              f'count {e.count.tolist()}, largest area {e.area[:, 0].tolist()}; repeat bit-identical: {same})', flush=True)


def profile():
    e = _Entries()
    for kind in e.masks:
        for _, run in e.runs(kind):
            for _ in range(3):
                run()
    torch.cuda.synchronize()


def model(repeats=5, steps=4):
    from tf_raft_amd import weights as wm
    N, H, W = MODEL
    g = torch.Generator(device='cuda').manual_seed(1)
    base = (torch.rand((N, H + 8, W + 8, 3), device='cuda', generator=g) * 255).to(torch.uint8)
    pair = (base[:, 4:4 + H, 4:4 + W].contiguous(), base[:, 5:5 + H, 2:2 + W].contiguous())
    kw = dict(alpha=1.9, threshold=5.0)
    for name, cls in (('small', tf_raft_amd.SmallRAFT), ('raft', tf_raft_amd.RAFT)):
        net = cls(weights=wm.init_weights(name, seed=0), iters_pred=ITERS)
        calls = {'camera_motion_step': lambda: net.camera_motion_step(pair, **kw),
                 'moving_objects_step': lambda: net.moving_objects_step(pair, **kw)}
        for fn in calls.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for _ in range(repeats):
            for k, fn in calls.items():
                t[k].append(_timed(fn, steps))
        for k in calls:
            print(f"{name}: {k}, {N} x {H} x {W} uint8, iters_pred={ITERS}, ms per call: {' '.join(f'{x:.3f}' for x in t[k])}  "
                  f'mean {np.mean(t[k]):.3f} spread {max(t[k]) - min(t[k]):.3f}', flush=True)
        extra = np.mean(t['moving_objects_step']) - np.mean(t['camera_motion_step'])
        res = net.moving_objects_step(pair, **kw)
        print(f"{name}: the objects cost {1e3 * extra:.1f} us per call (ratio {np.mean(t['moving_objects_step']) / np.mean(t['camera_motion_step']):.4f}); "
              f'moving share {float(res.moving.float().mean()):.3f}, occluded share {float(res.occluded_forward.float().mean()):.3f}, objects '
              f'{res.count.tolist()} largest {res.area[:, 0].tolist()} (random weights, a shifted texture)', flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('objects_bench.py measures on a GPU; none is visible')
    modes = sys.argv[1:] or ['kernels', 'model']
    for mode in modes:
        {'kernels': kernels, 'model': model, 'profile': profile}[mode]()

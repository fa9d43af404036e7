"""Measurements behind docs/NOTEBOOK.md section 18 (flow colour coding on the device).

  python tools/flow_viz_bench.py [--reps 100] [--warmup 20] [--no-predict]
      Per shape -- (4, 448, 512) and (1, 436, 1024) flows, device-resident, N(0, 5 px) -- the two kernels of
      `image_ops.flow_to_image` (events around `reps` back-to-back calls after a warm-up, the median of five such windows),
      the same with a fixed radius (one launch), their algorithmic bytes (8 read twice + 3 written per pixel; 8 + 3 with a
      fixed radius) over that time, and `io.flow_to_image` on the host for the same arrays (per image, best of 3).
      Then `RAFT.predict` pairs/s on host uint8 frames of 448 x 512 (RAFT(pipeline=True), 24 iterations) with output='flow' and output='image', alternating, three
      windows each.
  python tools/flow_viz_bench.py trace <0|1>
      60 calls on one of the two shapes and nothing else, meant to run under `rocprofv3 --kernel-trace --stats -- python ...`:
      the device time of each of the two kernels (the event windows above contain the host's enqueue of two launches per call).
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_raft_amd import image_ops, io       # noqa: E402

SHAPES = ((4, 448, 512), (1, 436, 1024))


def windows(fn, reps, n=5):
    """Median over n windows of the device time of `reps` back-to-back calls, in microseconds per call."""
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return float(np.median(out)), min(out), max(out)


def kernels(reps, warmup):
    for N, H, W in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(0)
        flow = torch.randn((N, H, W, 2), device='cuda', generator=g) * 5
        out = torch.empty((N, H, W, 3), device='cuda', dtype=torch.uint8)
        calls = {'own maximum (2 launches)': (lambda: image_ops.flow_to_image_launch(flow, H, W, out=out), 8 + 8 + 3),
                 'fixed radius (1 launch)': (lambda: image_ops.flow_to_image_launch(flow, H, W, fixed_rad_max=10.0, out=out), 8 + 3)}
        for name, (fn, bytes_per_pixel) in calls.items():
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            med, lo, hi = windows(fn, reps)
            mb = N * H * W * bytes_per_pixel / 1e6
            print(f'({N}, {H}, {W}) {name}: {med:.1f} us per call (windows {lo:.1f} .. {hi:.1f}); {mb:.2f} MB algorithmic = '
                  f'{mb / med:.3f} TB/s', flush=True)
        host = flow.cpu().numpy()
        best = []
        for _ in range(3):
            t0 = time.perf_counter()
            for f in host:
                io.flow_to_image(f)
            best.append((time.perf_counter() - t0) / N * 1e3)
        t0 = time.perf_counter()
        for _ in range(5):
            flow.cpu()
            torch.cuda.synchronize()
        down = (time.perf_counter() - t0) / 5 / N * 1e3
        print(f'({N}, {H}, {W}) host io.flow_to_image: {min(best):.1f} ms per image (best of 3); pageable download of the flow it '
              f'needs {down:.2f} ms per image', flush=True)


def trace(k):
    N, H, W = SHAPES[k]
    flow = torch.randn((N, H, W, 2), device='cuda', generator=torch.Generator(device='cuda').manual_seed(0)) * 5
    out = torch.empty((N, H, W, 3), device='cuda', dtype=torch.uint8)
    torch.cuda.synchronize()
    for _ in range(60):
        image_ops.flow_to_image_launch(flow, H, W, out=out)
    torch.cuda.synchronize()
    print(f'({N}, {H}, {W}): 60 calls', flush=True)


def predict(reps):
    import tf_raft_amd
    from tf_raft_amd import weights as wm
    rng = np.random.default_rng(0)
    n = 64
    a, b = (rng.integers(0, 256, size=(n, 448, 512, 3), dtype=np.uint8) for _ in range(2))
    model = tf_raft_amd.RAFT(weights=wm.init_weights('raft', seed=0), iters_pred=24, pipeline=True)
    for output in ('flow', 'image'):
        model.predict([a[:8], b[:8]], batch_size=4, output=output)
    rates = {'flow': [], 'image': []}
    for _ in range(3):
        for output in rates:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                model.predict([a, b], batch_size=4, output=output)
            torch.cuda.synchronize()
            rates[output].append(n * reps / (time.perf_counter() - t0))
    for output, r in rates.items():
        print(f"predict(batch_size=4, output='{output}') on {n} host uint8 pairs of 448 x 512: {np.median(r):.1f} pairs/s "
              f'(windows {min(r):.1f} .. {max(r):.1f})', flush=True)


if __name__ == '__main__':
    args = sys.argv[1:]
    if args[:1] == ['trace']:
        trace(int(args[1]))
        sys.exit(0)
    kernels(int(args[args.index('--reps') + 1]) if '--reps' in args else 100, int(args[args.index('--warmup') + 1]) if '--warmup' in args else 20)
    if '--no-predict' not in args:
        predict(6)

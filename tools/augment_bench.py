"""Measurements behind docs/NOTEBOOK.md sections 15 (device-side FlowAugmentor) and 16 (SparseFlowAugmentor).

  python tools/augment_bench.py [--reps 200] [--warmup 20]
      augmented pairs/s of `FlowAugmentor.batch` at batch 4 and the reference's training crop 368 x 496, from device-resident
      uint8 frames of MPI-Sintel (436 x 1024) and FlyingChairs (384 x 512) size.  Per shape: the whole call (host draws + record
      upload + two launches) timed with device events around `reps` back-to-back calls, as the median of five such windows after a
      warm-up; the two kernels alone (fixed records, no host draw), the same way; and the host time of the draws alone.
  python tools/augment_bench.py trace
      a few calls per shape and nothing else, meant to run under `rocprofv3 --kernel-trace --memory-copy-trace --stats -- python ...`:
      the structural claim is two launches and one small upload per batch.
  python tools/augment_bench.py sparse [--reps 200] [--warmup 20] [--dense-only]
      the dense and the sparse call on the same frames and crop: batch 4, KITTI-sized frames (375 x 1242) to the reference's KITTI
      crop 288 x 960, device-resident inputs, validity at 60 % density.  Windows of the two calls alternate, five each; per call the
      median window, and the same for `apply` with fixed records (no host draw).  `--dense-only` times the dense call alone and
      imports nothing else, so the file also runs in a checkout that has no sparse class (the parent commit of section 16).
  python tools/augment_bench.py sparse-trace [--dense-only]
      40 calls of each on those frames and nothing else, for `rocprofv3 --kernel-trace --stats`: the kernels' device time.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tf_raft_amd.augment import FlowAugmentor       # noqa: E402

SHAPES = (('sintel', 436, 1024), ('chairs', 384, 512))
CROP, BATCH = (368, 496), 4
KITTI, KITTI_CROP = (375, 1242), (288, 960)


def inputs(H, W):
    g = torch.Generator(device='cuda').manual_seed(0)
    i1 = torch.randint(0, 256, (BATCH, H, W, 3), dtype=torch.uint8, device='cuda', generator=g)
    i2 = torch.randint(0, 256, (BATCH, H, W, 3), dtype=torch.uint8, device='cuda', generator=g)
    fl = torch.randn((BATCH, H, W, 2), device='cuda', generator=g) * 20
    return i1, i2, fl


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


def bench(reps, warmup):
    for name, H, W in SHAPES:
        aug = FlowAugmentor(CROP, rng=np.random.RandomState(0), photo_rng=np.random.RandomState(1))
        i1, i2, fl = inputs(H, W)
        for _ in range(warmup):
            aug.batch(i1, i2, fl)
        torch.cuda.synchronize()
        call = windows(lambda: aug.batch(i1, i2, fl), reps)
        # the kernels alone: every fixed batch of records has its own mix of resize / colour / eraser work, so take several
        kernel = []
        for _ in range(8):
            recs = aug.draw(H, W, BATCH)
            aug.apply(recs, i1, i2, fl)
            kernel.append(windows(lambda: aug.apply(recs, i1, i2, fl), reps, n=3)[0])
        t0 = time.perf_counter()
        for _ in range(reps):
            aug.draw(H, W, BATCH)
        host = (time.perf_counter() - t0) / reps * 1e6
        print(f'{name} {H}x{W} -> {CROP[0]}x{CROP[1]} batch {BATCH}: call {call[0]:.1f} us per batch (windows {call[1]:.1f} .. {call[2]:.1f}) = '
              f'{BATCH / call[0] * 1e6:.0f} augmented pairs/s; apply with fixed records {np.median(kernel):.1f} us '
              f'({min(kernel):.1f} .. {max(kernel):.1f} over 8 record sets); host draws alone {host:.1f} us per batch', flush=True)


def trace():
    for name, H, W in SHAPES:
        aug = FlowAugmentor(CROP, rng=np.random.RandomState(0), photo_rng=np.random.RandomState(1))
        i1, i2, fl = inputs(H, W)
        torch.cuda.synchronize()
        for _ in range(10):
            aug.batch(i1, i2, fl)
        torch.cuda.synchronize()
        print(f'{name}: 10 batches of {BATCH}', flush=True)


def sparse_calls(dense_only):
    """name -> (augmentor, the inputs of its call): the dense and the sparse augmentor on the same frames, flow and crop."""
    H, W = KITTI
    i1, i2, fl = inputs(H, W)
    calls = {'dense': (FlowAugmentor(KITTI_CROP, rng=np.random.RandomState(0), photo_rng=np.random.RandomState(1)), (i1, i2, fl))}
    if not dense_only:
        from tf_raft_amd.augment import SparseFlowAugmentor
        g = torch.Generator(device='cuda').manual_seed(1)
        valid = (torch.rand((BATCH, H, W), device='cuda', generator=g) < 0.6).float()
        calls['sparse'] = (SparseFlowAugmentor(KITTI_CROP, do_flip=True, rng=np.random.RandomState(0), photo_rng=np.random.RandomState(1)),
                           (i1, i2, fl, valid))
    return calls


def sparse(reps, warmup, dense_only):
    H, W = KITTI
    calls = sparse_calls(dense_only)
    for aug, args in calls.values():
        for _ in range(warmup):
            aug.batch(*args)
    torch.cuda.synchronize()
    whole = {name: [] for name in calls}
    for _ in range(5):                                  # alternate, so that a drift of the machine meets both calls
        for name, (aug, args) in calls.items():
            whole[name].append(windows(lambda: aug.batch(*args), reps, n=1)[0])
    fixed = {name: [] for name in calls}
    for _ in range(8):                                  # every fixed batch of records has its own mix of work: take several
        for name, (aug, args) in calls.items():
            recs = aug.draw(H, W, BATCH)
            aug.apply(recs, *args)
            fixed[name].append(windows(lambda: aug.apply(recs, *args), reps, n=3)[0])
    for name in calls:
        w, k = whole[name], fixed[name]
        print(f'{name} kitti {H}x{W} -> {KITTI_CROP[0]}x{KITTI_CROP[1]} batch {BATCH}: call {np.median(w):.1f} us per batch (windows {min(w):.1f} .. '
              f'{max(w):.1f}); apply with fixed records {np.median(k):.1f} us ({min(k):.1f} .. {max(k):.1f} over 8 record sets)', flush=True)
    if 'sparse' in calls:
        print(f"sparse / dense: call {np.median(whole['sparse']) / np.median(whole['dense']):.3f}, apply with fixed records "
              f"{np.median(fixed['sparse']) / np.median(fixed['dense']):.3f}", flush=True)


def sparse_trace(dense_only):
    for name, (aug, args) in sparse_calls(dense_only).items():
        torch.cuda.synchronize()
        for _ in range(40):
            aug.batch(*args)
        torch.cuda.synchronize()
        print(f'{name}: 40 batches of {BATCH}', flush=True)


if __name__ == '__main__':
    args = sys.argv[1:]
    if args[:1] == ['trace']:
        trace()
    elif args[:1] == ['sparse-trace']:
        sparse_trace('--dense-only' in args)
    elif args[:1] == ['sparse']:
        sparse(int(args[args.index('--reps') + 1]) if '--reps' in args else 200, int(args[args.index('--warmup') + 1]) if '--warmup' in args else 20,
               '--dense-only' in args)
    else:
        bench(int(args[args.index('--reps') + 1]) if '--reps' in args else 200, int(args[args.index('--warmup') + 1]) if '--warmup' in args else 20)

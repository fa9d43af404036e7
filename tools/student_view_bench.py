"""Measurements behind docs/NOTEBOOK.md section 33 (the student's view: the two affine gathers and the step that uses them).

  python tools/student_view_bench.py kernel
      raft_view_frames_f32 (C = 3) and raft_view_flow_f32 (with the trust mask) for 8 slices of 304 x 432 out of 368 x 496, under
      the identity view at (32, 32) and under one generic view (rotation 7 degrees, zoom 1.13, centred), each alternating with
      raft_stream_copy_f32 at the SAME byte count; and image_ops.warp (raft_warp_f32) on 8 student-sized frames under a smooth
      flow, the same way, in the same job.  The compulsory bytes count what must move whatever the kernel does: the output
      written, and the footprint of the view in the teacher read once -- frames: npix * 12 written + footprint * 12 read; flow:
      npix * (8 + 1) written + footprint * (8 + 1) read, the footprint being npix * |det M| teacher pixels; warp: npix * (12 + 8)
      read + npix * 12 written.  HIP-event times of 200 back-to-back calls of the C entries, two measurements each, reported as a
      fraction of the stream-copy rate.
  python tools/student_view_bench.py step [repeats]
      RAFT, trainable='all', iters = 12, bidirectional, selfsup_crop=(32, 32): ms per train_step at (4, 368, 496) with
      selfsup_transform set (a seeded generic draw per step: flips, zoom (0.9, 1.3), rotation 10 degrees, gain, bias) against
      unset (the centre crop of section 22), alternating in one process with warmed shapes and device events; the round is
      repeated (default 5 times) for the run-to-run spread.  Peak allocated device memory per kind of step.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402

N_PRED, SHAPE, CROP = 12, (4, 368, 496), (32, 32)
GENERIC = dict(rotate=7.0, zoom=1.13)


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _against_copy(what, nbytes, run, reps):
    from tf_raft_amd import _dev
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    n = (nbytes // 8) // 4 * 4
    a = torch.randn((n,), device='cuda')
    b = torch.empty_like(a)
    copy = lambda: check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, _dev.stream_ptr()), 'stream_copy')
    for _ in range(5):
        copy()
        run()
    torch.cuda.synchronize()
    t = {k: [] for k in ('copy', 'run')}
    for _ in range(2):
        for k, fn in (('copy', copy), ('run', run)):
            t[k].append(_timed(fn, reps) * 1e3)
    r_copy, r_run = 8 * n / min(t['copy']) / 1e6, nbytes / min(t['run']) / 1e6
    print(f'{what}: {nbytes} compulsory bytes; back-to-back events: stream copy {t["copy"][0]:.1f} / {t["copy"][1]:.1f} us = '
          f'{r_copy:.2f} TB/s, entry {t["run"][0]:.1f} / {t["run"][1]:.1f} us = {r_run:.3f} TB/s = {r_run / r_copy:.3f} of the '
          f'stream-copy rate', flush=True)


def kernel(reps=200):
    from tf_raft_amd import _dev, image_ops
    from tf_raft_amd._ffi import check
    from tf_raft_amd.augment import StudentView
    B, Ht, Wt = 2 * SHAPE[0], SHAPE[1], SHAPE[2]
    H, W = Ht - 2 * CROP[0], Wt - 2 * CROP[1]
    npix = B * H * W
    g = torch.Generator(device='cuda').manual_seed(0)
    frames = torch.rand((B, Ht, Wt, 3), device='cuda', generator=g) * 255
    flow = torch.randn((B, Ht, Wt, 2), device='cuda', generator=g) * 3
    tv = torch.ones((B, Ht, Wt), dtype=torch.uint8, device='cuda')
    t = np.deg2rad(GENERIC['rotate'])
    M = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]) / GENERIC['zoom']
    o = np.array([(Wt - 1) / 2, (Ht - 1) / 2]) - M @ np.array([(W - 1) / 2, (H - 1) / 2])
    views = {'identity': StudentView.identity(B, CROP), 'generic': StudentView(np.tile(np.concatenate([M, o[:, None]], 1), (B, 1, 1)))}
    # the C entries are called directly on outputs made once: the Python launch forms allocate and check per call, which at
    # these sizes (6 to 9 us per launch) would time the host
    lib, ptr, stream = _dev.lib(), _dev.ptr, _dev.stream_ptr
    out = torch.empty((B, H, W, 3), device='cuda')
    target, vis = torch.empty((B, H, W, 2), device='cuda'), torch.empty((B, H, W), dtype=torch.uint8, device='cuda')
    for name, view in views.items():
        recs = image_ops.view_records(view, B, frames.device)
        foot = int(npix * abs(np.linalg.det(view.matrix()[0])))
        _against_copy(f'view_frames, {name} view, {(B, H, W)} out of {(B, Ht, Wt)}', 12 * (npix + foot),
                      lambda: check(lib.raft_view_frames_f32(ptr(frames), ptr(recs), ptr(out), B, Ht, Wt, H, W, 3, stream()), 'view_frames'), reps)
        _against_copy(f'view_flow with the mask, {name} view, {(B, H, W)} out of {(B, Ht, Wt)}', 9 * (npix + foot),
                      lambda: check(lib.raft_view_flow_f32(ptr(flow), ptr(tv), ptr(recs), ptr(target), ptr(vis), B, Ht, Wt, H, W, stream()),
                                    'view_flow'), reps)
        print(f'({name}: {float(vis.float().mean()):.3f} of the student in frame and trusted)', flush=True)
    ys, xs = torch.meshgrid(torch.arange(H, device='cuda'), torch.arange(W, device='cuda'), indexing='ij')
    smooth = torch.stack([2.0 + 1.5 * torch.sin(ys / 13.0), -1.0 + 1.2 * torch.cos(xs / 15.0)], -1).expand(B, H, W, 2).contiguous()
    small = frames[:, :H, :W].contiguous()
    _against_copy(f'warp (raft_warp_f32), {(B, H, W, 3)} under a smooth flow', npix * (12 + 8 + 12),
                  lambda: check(lib.raft_warp_f32(ptr(small), ptr(smooth), ptr(out), None, B, H, W, 3, stream()), 'warp'), reps)


def step(repeats=5, reps=3):
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    from tf_raft_amd.augment import StudentTransform
    rng = np.random.default_rng(0)
    i1, i2 = (torch.as_tensor(rng.uniform(0, 255, SHAPE + (3,)).astype(np.float32)).cuda() for _ in range(2))
    wts = wm.init_weights('raft', seed=0)
    transform = StudentTransform(flip_x=0.5, flip_y=0.5, zoom=(0.9, 1.3), rotate=10.0, gain=(0.8, 1.2), bias=(-10.0, 10.0), asymmetric=0.5,
                                 rng=np.random.RandomState(0))

    def model(**kw):
        m = tf_raft_amd.RAFT(weights={k: v.copy() for k, v in wts.items()}, iters=N_PRED)
        m.compile(optimizer=training.AdamW(1e-4, 1e-4), clip_norm=1.0, loss=losses.PhotometricSequenceLoss(), bidirectional=True,
                  selfsup_crop=CROP, **kw)
        return m
    viewed, cropped = model(selfsup_transform=transform), model()
    runs = {'selfsup_transform set (generic draw)': lambda: viewed.train_step((i1, i2)),
            'selfsup_transform unset (the centre crop)': lambda: cropped.train_step((i1, i2))}
    for _ in range(2):
        for run in runs.values():
            run()
    torch.cuda.synchronize()
    t, peak = {k: [] for k in runs}, {}
    for _ in range(repeats):
        for k, run in runs.items():
            torch.cuda.reset_peak_memory_stats()
            t[k].append(_timed(run, reps))
            peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated())
    fmt = lambda v: ' '.join(f'{x:.2f}' for x in v)
    for k, v in t.items():
        print(f'train_step, {k}, iters={N_PRED} at {SHAPE} crop {CROP}, ms per step: {fmt(v)}  mean {np.mean(v):.2f} spread {max(v) - min(v):.2f}; '
              f'peak allocated {peak[k] / 2 ** 20:.0f} MiB', flush=True)
    means = [float(np.mean(v)) for v in t.values()]
    print(f'with the view {means[0]:.2f} ms against {means[1]:.2f} ms without ({means[0] - means[1]:+.2f} ms)', flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('student_view_bench.py measures on a GPU; none is visible')
    if sys.argv[1] == 'kernel':
        kernel()
    else:
        step(*(int(v) for v in sys.argv[2:3]))

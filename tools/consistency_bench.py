"""Measurements behind docs/NOTEBOOK.md section 21 (bidirectional flow with occlusion masks).

  python tools/consistency_bench.py kernels
      at (4, 1080, 1920): the warp of uint8 3-channel frames (with the in-frame map), the consistency check of both directions in
      ONE launch, and the same as TWO one-direction launches, each alternating with raft_stream_copy_f32 at the SAME byte count
      (every distinct byte read or written counted once: the gathered taps are re-reads of bytes already counted).  HIP-event
      times of back-to-back launches, reported as a fraction of the stream-copy rate; run it under
      `rocprofv3 --kernel-trace --stats -- python ...` for the kernels' own times.
  python tools/consistency_bench.py step [repeats]
      at (4, 448, 512), iters_pred=24, serial RAFT: ms per call of predict_step_bidirectional (the mirrored pass: fnet once per
      frame) against predict_step(([i1 | i2], [i2 | i1])) (the doubled batch through the unchanged forward path) plus the same
      consistency launch, alternating in one process with warmed shapes and device events; the pair of measurements is repeated
      (default 7 times) for the run-to-run spread.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402

FRAMES = (4, 1080, 1920)
STEP = (4, 448, 512)


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(reps=30):
    from tf_raft_amd import _dev, image_ops
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    N, H, W = FRAMES
    g = torch.Generator(device='cuda').manual_seed(0)
    frames = torch.randint(0, 256, FRAMES + (3,), dtype=torch.uint8, device='cuda', generator=g)
    # a few pixels of smooth motion, the backward flow roughly its negative: neighbouring lanes gather neighbouring taps
    coarse = torch.randn((N, 2, H // 64 + 2, W // 64 + 2), device='cuda', generator=g) * 4
    smooth = torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    fwd = (smooth + 0.3 * torch.randn((N, H, W, 2), device='cuda', generator=g)).contiguous()
    bwd = (-smooth + 0.3 * torch.randn((N, H, W, 2), device='cuda', generator=g)).contiguous()
    px = N * H * W
    warped, inside = torch.empty(FRAMES + (3,), device='cuda'), torch.empty(FRAMES, dtype=torch.uint8, device='cuda')
    cases = [
        ('warp uint8 frames, 3 channels, with the in-frame map', px * (3 + 8 + 12 + 1),
         lambda: image_ops.warp_launch(frames, fwd, out=warped, inside=inside)),
        ('consistency check, both directions in one launch', px * (8 + 8 + 1 + 1),
         lambda: image_ops.flow_consistency_launch(fwd, bwd)),
        ('consistency check, two one-direction launches', px * (8 + 8 + 1 + 1),
         lambda: (image_ops.flow_consistency_launch(fwd, bwd, both=False), image_ops.flow_consistency_launch(bwd, fwd, both=False))),
    ]
    for what, nbytes, run in cases:
        n = (nbytes // 8) // 4 * 4
        a = torch.randn((n,), device='cuda')
        b = torch.empty_like(a)
        copy = lambda: check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, _dev.stream_ptr()), 'stream_copy')
        torch.cuda.synchronize()
        for _ in range(reps):
            copy()
            run()
        torch.cuda.synchronize()
        t_copy, t_run = _timed(copy, reps) * 1e3, _timed(run, reps) * 1e3
        t_copy2, t_run2 = _timed(copy, reps) * 1e3, _timed(run, reps) * 1e3
        r_copy, r_run = 8 * n / min(t_copy, t_copy2) / 1e6, nbytes / min(t_run, t_run2) / 1e6
        print(f'{what} at {FRAMES}: {nbytes} bytes read + written; back-to-back events: stream copy {t_copy:.1f} / {t_copy2:.1f} us = '
              f'{r_copy:.2f} TB/s, kernel {t_run:.1f} / {t_run2:.1f} us = {r_run:.2f} TB/s = {r_run / r_copy:.2f} of the stream-copy rate',
              flush=True)
        del a, b
    occ = image_ops.flow_consistency_launch(fwd, bwd)
    print(f'(flows of the measurement: {100 * float(occ[0].float().mean()):.1f} % / {100 * float(occ[1].float().mean()):.1f} % of the '
          f'pixels occluded, {100 * float(1 - inside.float().mean()):.1f} % of the warp out of frame)', flush=True)


def step(repeats=7, reps=10):
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(0)
    model = tf_raft_amd.RAFT(iters_pred=24)
    i1, i2 = (torch.as_tensor(rng.uniform(0, 255, STEP + (3,)).astype(np.float32)).cuda() for _ in range(2))
    d1, d2 = torch.cat([i1, i2]), torch.cat([i2, i1])
    B = STEP[0]

    def mirrored():
        return model.predict_step_bidirectional((i1, i2))

    def doubled():
        flows = model.predict_step((d1, d2)).as_subclass(torch.Tensor)
        return (flows[:B], flows[B:]) + image_ops.flow_consistency_launch(flows[:B], flows[B:])

    m, d = mirrored(), doubled()
    torch.cuda.synchronize()
    diff = max(float((m.forward.as_subclass(torch.Tensor) - d[0]).norm(dim=-1).max()), float((m.backward.as_subclass(torch.Tensor) - d[1]).norm(dim=-1).max()))
    print(f'mirrored against doubled batch at {STEP}: max EPE {diff:.2e}, masks differ in '
          f'{int((m.occluded_forward.as_subclass(torch.Tensor) != d[2]).sum()) + int((m.occluded_backward.as_subclass(torch.Tensor) != d[3]).sum())} pixels',
          flush=True)
    for _ in range(3):
        mirrored(), doubled()
    torch.cuda.synchronize()
    tm, td = [], []
    for _ in range(repeats):
        tm.append(_timed(mirrored, reps))
        td.append(_timed(doubled, reps))
    fmt = lambda v: ' '.join(f'{x:.3f}' for x in v)
    print(f'predict_step_bidirectional (mirrored pass) ms per call: {fmt(tm)}  mean {np.mean(tm):.3f} spread {max(tm) - min(tm):.3f}', flush=True)
    print(f'doubled batch + consistency launch ms per call:       {fmt(td)}  mean {np.mean(td):.3f} spread {max(td) - min(td):.3f}', flush=True)
    print(f'difference of the means {np.mean(td) - np.mean(tm):.3f} ms; larger spread {max(max(tm) - min(tm), max(td) - min(td)):.3f} ms', flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('consistency_bench.py measures on a GPU; none is visible')
    if sys.argv[1] == 'kernels':
        kernels()
    else:
        step(*(int(v) for v in sys.argv[2:3]))

"""Measurements behind docs/NOTEBOOK.md section 37 (frame interpolation: the forward splat of frames).

  python tools/frame_splat_bench.py kernels
      at (4, 1080, 1920) uint8: raft_interpolate_frames_u8 (both frames, 2N slices of sums) and raft_splat_frames_u8_f32 (N slices)
      on preallocated outputs, alternating in one process with raft_flow_range_occlusion_f32 (both directions) and raft_warp_u8_f32
      on the SAME flows and frames and with raft_stream_copy_f32 at each entry's compulsory byte count (the inputs read once, the
      outputs written once: the uint64 sums are a workspace -- zeroed, added to and read back -- and are NOT counted, so the share
      says what the splat costs over a gather of the same inputs).  Also the interpolation under flows ten times as long (most
      adds miss the LDS window).  HIP-event times of back-to-back calls; every figure with the rounds it came from.
  python tools/frame_splat_bench.py step [repeats]
      at 4 pairs of 448 x 512, RAFT, iters_pred=12: ms per interpolate_step against predict_step_bidirectional, one model,
      alternating in one process with warmed shapes and device events; the pair is repeated (default 5 times) for the spread.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402

SHAPE = (4, 1080, 1920)
ITERS, STEP = 12, (4, 448, 512)


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


def kernels(reps=20, rounds=3):
    from tf_raft_amd import _dev
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    N, H, W = SHAPE
    g = torch.Generator(device='cuda').manual_seed(0)
    # a few pixels of smooth motion, the backward flow roughly its negative: a wave's adds to one row are neighbours
    coarse = torch.randn((N, 2, H // 64 + 2, W // 64 + 2), device='cuda', generator=g) * 4
    smooth = torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    fwd = (smooth + 0.3 * torch.randn((N, H, W, 2), device='cuda', generator=g)).contiguous()
    bwd = (-smooth + 0.3 * torch.randn((N, H, W, 2), device='cuda', generator=g)).contiguous()
    fwd10, bwd10 = (fwd * 10).contiguous(), (bwd * 10).contiguous()
    i1, i2 = (torch.randint(0, 256, (N, H, W, 3), device='cuda', dtype=torch.uint8, generator=g) for _ in range(2))
    px = N * H * W
    out_u8 = torch.empty((N, H, W, 3), device='cuda', dtype=torch.uint8)
    out_f32 = torch.empty((N, H, W, 3), device='cuda')
    weight = torch.empty((N, H, W), device='cuda')
    holes = torch.empty((N, H, W), device='cuda', dtype=torch.uint8)
    masks = torch.empty((2 * N, H, W), device='cuda', dtype=torch.uint8)
    sums = torch.empty((int(lib.raft_frame_splat_workspace_bytes(2 * N, H, W, 3)) // 8,), device='cuda', dtype=torch.int64)
    st = _dev.stream_ptr

    def interpolate(f=fwd, b=bwd):
        check(lib.raft_interpolate_frames_u8(_dev.ptr(i1), _dev.ptr(i2), _dev.ptr(f), _dev.ptr(b), None, None, 0.5, _dev.ptr(out_u8),
                                             _dev.ptr(holes), N, H, W, 3, _dev.ptr(sums), st()), 'interpolate_frames')

    def splat():
        check(lib.raft_splat_frames_u8_f32(_dev.ptr(i1), _dev.ptr(fwd), None, 0.5, _dev.ptr(out_f32), _dev.ptr(weight), N, H, W, 3,
                                           _dev.ptr(sums), st()), 'splat_frames')

    def range_occlusion():
        check(lib.raft_flow_range_occlusion_f32(_dev.ptr(fwd), _dev.ptr(bwd), _dev.ptr(masks[:N]), _dev.ptr(masks[N:]), N, H, W, 0.5,
                                                _dev.ptr(sums), st()), 'range_occlusion')

    def warp():
        check(lib.raft_warp_u8_f32(_dev.ptr(i2), _dev.ptr(fwd), _dev.ptr(out_f32), None, N, H, W, 3, st()), 'warp')
    copies = {}

    def copy_of(nbytes):
        n = (nbytes // 8) // 4 * 4
        if n not in copies:
            copies[n] = (torch.randn((n,), device='cuda'), torch.empty((n,), device='cuda'))
        a, b = copies[n]
        return lambda: check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, st()), 'stream_copy')
    # (name, compulsory bytes or None, call)
    runs = [('interpolate_frames_u8, holes written (2N slices of sums)', px * (3 + 3 + 8 + 8 + 3 + 1), interpolate),
            ('splat_frames_u8_f32 with the weight (N slices of sums)', px * (3 + 8 + 12 + 4), splat),
            ('range_occlusion, both directions (2N slices of sums)', px * (8 + 8 + 1 + 1), range_occlusion),
            ('warp_u8_f32', px * (3 + 8 + 12), warp),
            ('interpolate_frames_u8 under flows ten times as long', None, lambda: interpolate(fwd10, bwd10))]
    runs = [(k, nb, run, copy_of(nb) if nb else None) for k, nb, run in runs]
    for _ in range(3):
        for _, _, run, copy in runs:
            run()
            if copy:
                copy()
    torch.cuda.synchronize()
    t, tc = {k: [] for k, *_ in runs}, {k: [] for k, *_ in runs}
    for _ in range(rounds):
        for k, _, run, copy in runs:
            if copy:
                tc[k].append(_timed(copy, reps) * 1e3)
            t[k].append(_timed(run, reps) * 1e3)
    for k, nb, _, copy in runs:
        line = f'{k} at {SHAPE}, us per call: {_fmt(t[k])}  min {min(t[k]):.1f}'
        if copy:
            r_run, r_copy = nb / min(t[k]) / 1e6, (nb // 32 * 32) / min(tc[k]) / 1e6
            line += (f'; {nb} compulsory bytes = {r_run:.2f} TB/s; stream copy of as many bytes {_fmt(tc[k])} us = {r_copy:.2f} TB/s: '
                     f'{r_run / r_copy:.2f} of the stream-copy rate')
        print(line, flush=True)
    ratio = lambda a, b: min(t[a]) / min(t[b])      # noqa: E731
    print(f'interpolate_frames / range_occlusion = {ratio(runs[0][0], runs[2][0]):.2f} (4 times the adds per vector), '
          f'splat_frames / warp = {ratio(runs[1][0], runs[3][0]):.2f} at {SHAPE}', flush=True)
    # what the measurement's flows are, and that the entry repeats
    interpolate()
    first, first_holes = out_u8.clone(), holes.clone()
    interpolate()
    print(f'(holes: {float(holes.float().mean()):.5f} of the pixels; repeat bit-identical: {bool(first.equal(out_u8) and first_holes.equal(holes))}; '
          f'mean |flow| {float(fwd.norm(dim=-1).mean()):.2f} px)', flush=True)


def step(repeats=5, reps=3):
    from tf_raft_amd import weights as wm
    rng = np.random.default_rng(0)
    i1, i2 = (torch.as_tensor(rng.integers(0, 256, STEP + (3,), dtype=np.uint8)).cuda() for _ in range(2))
    model = tf_raft_amd.RAFT(weights=wm.init_weights('raft', seed=0), iters_pred=ITERS)
    runs = {'predict_step_bidirectional': lambda: model.predict_step_bidirectional((i1, i2)),
            'interpolate_step, t=0.5': lambda: model.interpolate_step((i1, i2), 0.5),
            'interpolate_step, t=(0.25, 0.5, 0.75)': lambda: model.interpolate_step((i1, i2), (0.25, 0.5, 0.75))}
    for run in runs.values():
        for _ in range(2):
            run()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(repeats):
        for k, run in runs.items():
            t[k].append(_timed(run, reps))
    for k, v in t.items():
        print(f"{k}, iters_pred={ITERS} at {STEP} uint8, ms per call: {' '.join(f'{x:.2f}' for x in v)}  mean {np.mean(v):.2f} "
              f'spread {max(v) - min(v):.2f}', flush=True)
    base = np.mean(t['predict_step_bidirectional'])
    print('interpolate_step / predict_step_bidirectional = ' + ', '.join(f'{np.mean(v) / base:.4f}' for k, v in t.items() if k[0] == 'i'),
          flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('frame_splat_bench.py measures on a GPU; none is visible')
    if sys.argv[1] == 'kernels':
        kernels()
    else:
        step(*(int(v) for v in sys.argv[2:3]))

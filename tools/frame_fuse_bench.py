"""Measurements behind docs/NOTEBOOK.md section 40 (temporal fusion), all in one job.

  python tools/frame_fuse_bench.py
      At (4, 1080, 1920) uint8 frames of 3 channels, K = 4 neighbours under a few pixels of smooth motion, with a skip mask (10 %
      set): raft_fuse_frames_u8 at patch_radius 0, 1 and 2; K raft_warp_f32 launches (float32 frames) and K raft_warp_u8_f32
      launches on the SAME flows; and raft_stream_copy_f32 at the bytes the fusion cannot avoid.  HIP-event times of back-to-back
      calls, the calls alternating inside each of three rounds.  Then RAFT.denoise_video on a 6-frame clip at 448 x 512 (radius 2)
      against its five bidirectional passes alone, wall clock with a synchronise, three times each, alternating.

The compulsory bytes of a fusion, per pixel and slice, for uint8 frames of C channels: the centre (C), per neighbour its frame once
(C), its vector (8) and its skip byte (1), and the result (C): C + K (C + 9) + C = 54 at C = 3, K = 4.  The four warps move
K (C' + 8 + 4 * 3) bytes, C' = 12 for float32 frames and 3 for uint8 ones.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402, F401

SHAPE = (4, 1080, 1920)
K, C = 4, 3


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
    px = N * H * W
    g = torch.Generator(device='cuda').manual_seed(0)
    video = torch.randint(0, 256, (K + 1, N, H, W, C), device='cuda', generator=g, dtype=torch.uint8)
    video_f = video.to(torch.float32)
    ys, xs = torch.meshgrid(torch.arange(H, device='cuda', dtype=torch.float32), torch.arange(W, device='cuda', dtype=torch.float32),
                            indexing='ij')
    shifts = [(-2.5, 1.25), (-1.0, 0.5), (1.5, -0.75), (3.25, 2.0)]
    flows = torch.stack([torch.stack([dx + 1.5 * torch.sin(ys / 90.0 + k), dy + 1.5 * torch.cos(xs / 120.0 - k)], dim=-1)[None].expand(N, H, W, 2)
                         for k, (dx, dy) in enumerate(shifts)]).contiguous()
    skip = (torch.rand((K, N, H, W), device='cuda', generator=g) < 0.1).to(torch.uint8)
    out = torch.empty((N, H, W, C), device='cuda', dtype=torch.uint8)
    warped = torch.empty((N, H, W, C), device='cuda', dtype=torch.float32)
    index = (__import__('ctypes').c_int64 * K)(*range(1, K + 1))
    st = _dev.stream_ptr

    def fuse(r):
        check(lib.raft_fuse_frames_u8(_dev.ptr(video[0]), _dev.ptr(video), index, _dev.ptr(flows), _dev.ptr(skip), 0, 10.0, 1.0, r,
                                      _dev.ptr(out), None, K, N, H, W, C, st()), 'fuse_frames')

    def warps_f32():
        for k in range(K):
            check(lib.raft_warp_f32(_dev.ptr(video_f[k + 1]), _dev.ptr(flows[k]), _dev.ptr(warped), None, N, H, W, C, st()), 'warp')

    def warps_u8():
        for k in range(K):
            check(lib.raft_warp_u8_f32(_dev.ptr(video[k + 1]), _dev.ptr(flows[k]), _dev.ptr(warped), None, N, H, W, C, st()), 'warp')

    nbytes = px * (C + K * (C + 9) + C)
    n = (nbytes // 8) // 4 * 4                      # floats read (and as many written): nbytes moved in all
    a, b = torch.randn((n,), device='cuda'), torch.empty((n,), device='cuda')

    def copy():
        check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, st()), 'stream_copy')

    runs = [('fuse, r = 0', lambda: fuse(0)), ('fuse, r = 1', lambda: fuse(1)), ('fuse, r = 2', lambda: fuse(2)),
            (f'{K} warps, float32 frames', warps_f32), (f'{K} warps, uint8 frames', warps_u8), ('stream copy of the fusion\'s bytes', copy)]
    for _ in range(3):
        for _, run in runs:
            run()
    torch.cuda.synchronize()
    t = {k: [] for k, _ in runs}
    for _ in range(rounds):
        for k, run in runs:
            t[k].append(_timed(run, reps) * 1e3)
    for k, _ in runs:
        print(f'{k} at {SHAPE} x {C}, K = {K}, us per call: {_fmt(t[k])}  min {min(t[k]):.1f}', flush=True)
    t_copy = min(t['stream copy of the fusion\'s bytes'])
    r_copy = n * 8 / t_copy / 1e6
    for r in (0, 1, 2):
        r_run = nbytes / min(t[f'fuse, r = {r}']) / 1e6
        print(f'fuse, r = {r}: {nbytes} compulsory bytes = {r_run:.2f} TB/s; stream copy {r_copy:.2f} TB/s: {r_run / r_copy:.2f} of the '
              f'stream-copy rate', flush=True)
    for name in (f'{K} warps, float32 frames', f'{K} warps, uint8 frames'):
        print(f'fuse, r = 1 against {name} plus one stream copy of its bytes: {min(t["fuse, r = 1"]):.1f} us against '
              f'{min(t[name]) + t_copy:.1f} us', flush=True)
    fuse(1)
    first = out.clone()
    fuse(1)
    torch.cuda.synchronize()
    print(f'(repeat bit-identical: {bool(first.equal(out))}; mean |fused - centre| {float((out.float() - video[0].float()).abs().mean()):.2f})',
          flush=True)


def whole_video(rounds=3):
    from tf_raft_amd import weights as wm
    model = tf_raft_amd.RAFT(weights=wm.init_weights('raft', seed=0), iters_pred=24)
    rng = np.random.default_rng(0)
    T, H, W = 6, 448, 512
    base = rng.uniform(0, 255, (H + 16, W + 16, 3))
    clip = np.stack([base[8 + t:8 + t + H, 8 - t:8 - t + W] for t in range(T)])
    clip = np.round((clip + rng.normal(0, 4, clip.shape)).clip(0, 255)).astype(np.uint8)
    dclip = torch.from_numpy(clip).cuda()

    def passes():
        model.predict_step_bidirectional((dclip[0:4], dclip[1:5]))
        model.predict_step_bidirectional((dclip[4:5], dclip[5:6]))
        torch.cuda.synchronize()

    def denoise():
        model.denoise_video(dclip, radius=2, batch_size=4)

    for fn in (passes, denoise):
        fn()
    t = {'bidirectional passes alone': [], 'denoise_video': []}
    for _ in range(rounds):
        for name, fn in (('bidirectional passes alone', passes), ('denoise_video', denoise)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[name].append((time.perf_counter() - t0) * 1e3)
    for name, v in t.items():
        print(f'{name}, {T} frames at {H} x {W}, ms: {_fmt(v)}  min {min(v):.1f}', flush=True)
    print(f'tracking, fusing and the download cost {min(t["denoise_video"]) - min(t["bidirectional passes alone"]):.1f} ms of '
          f'{min(t["denoise_video"]):.1f} ms', flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('frame_fuse_bench.py measures on a GPU; none is visible')
    kernels()
    whole_video()

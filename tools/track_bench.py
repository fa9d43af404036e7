"""Measurements behind docs/NOTEBOOK.md section 38 (points followed through a video), all in one job.

  python tools/track_bench.py [dense] [sparse] [video]      (no argument: all three)
      dense   a dense grid at (4, 1080, 1920), S = 1, raft_track_points_f32 on preallocated outputs with the backward flow and
              without it, alternating in one process with raft_flow_consistency_f32 (direction a alone: ONE of this kernel's two
              dependent gathers) on the SAME flows and with raft_stream_copy_f32 at the compulsory 34 bytes per point (position and
              code read and written, one vector of each flow).  HIP-event times of back-to-back calls, three rounds.
      sparse  1024 points in each of 4 videos of 1080 x 1920 over S = 8 steps as ONE launch against eight S = 1 launches in place.
      video   track_video on 9 frames of 448 x 512 (a grid of every 4th pixel, batch_size 4), SmallRAFT and RAFT at iters_pred 12,
              against predict_bidirectional on the same 8 pairs: host clock around calls that end in a download, alternating,
              five repeats.  The difference is what tracking costs.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402

SHAPE = (4, 1080, 1920)
SPARSE_POINTS, SPARSE_STEPS = 1024, 8
VIDEO, ITERS = (9, 448, 512), 12


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


def _flows(S, N, H, W, g):
    """A few pixels of smooth motion, the backward flow roughly its negative: a wave's gathers are neighbours."""
    coarse = torch.randn((S * N, 2, H // 64 + 2, W // 64 + 2), device='cuda', generator=g) * 4
    smooth = torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    fwd = (smooth + 0.3 * torch.randn((S * N, H, W, 2), device='cuda', generator=g)).reshape(S, N, H, W, 2).contiguous()
    bwd = (-smooth + 0.3 * torch.randn((S * N, H, W, 2), device='cuda', generator=g)).reshape(S, N, H, W, 2).contiguous()
    return fwd, bwd


def _measure(runs, reps, rounds):
    """runs: (name, call) -> {name: [us per call, one per round]}, the calls alternating inside every round."""
    for _ in range(3):
        for _, run in runs:
            run()
    torch.cuda.synchronize()
    t = {k: [] for k, _ in runs}
    for _ in range(rounds):
        for k, run in runs:
            t[k].append(_timed(run, reps) * 1e3)
    return t


def dense(reps=20, rounds=3):
    from tf_raft_amd import _dev, image_ops
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    N, H, W = SHAPE
    g = torch.Generator(device='cuda').manual_seed(0)
    fwd, bwd = _flows(1, N, H, W, g)
    pts = torch.from_numpy(image_ops.point_grid(H, W, N=N)).cuda()
    P = pts.shape[1]
    px = N * P
    lost_in = torch.zeros((N, P), device='cuda', dtype=torch.uint8)
    pos_out, lost_out = torch.empty((1, N, P, 2), device='cuda'), torch.empty((1, N, P), device='cuda', dtype=torch.uint8)
    occ = torch.empty((N, H, W), device='cuda', dtype=torch.uint8)
    st = _dev.stream_ptr

    def track(b=bwd):
        check(lib.raft_track_points_f32(_dev.ptr(pts), _dev.ptr(lost_in), None, 0, _dev.ptr(fwd), _dev.ptr(b) if b is not None else None,
                                        _dev.ptr(pos_out), _dev.ptr(lost_out), 1, N, P, H, W, 0.01, 0.5, st()), 'track_points')

    def consistency():
        check(lib.raft_flow_consistency_f32(_dev.ptr(fwd), _dev.ptr(bwd), _dev.ptr(occ), None, N, H, W, 0.01, 0.5, st()), 'flow_consistency')
    nbytes = px * 34
    n = (nbytes // 8) // 4 * 4
    a, b = torch.randn((n,), device='cuda'), torch.empty((n,), device='cuda')

    def copy():
        check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, st()), 'stream_copy')
    runs = [('track_points, dense grid, S = 1, with the backward flow', track),
            ('track_points, dense grid, S = 1, no backward flow', lambda: track(None)),
            ('flow_consistency, direction a alone', consistency),
            ('stream copy of 34 bytes per point', copy)]
    t = _measure(runs, reps, rounds)
    for k, _ in runs:
        print(f'{k} at {SHAPE}, us per call: {_fmt(t[k])}  min {min(t[k]):.1f}', flush=True)
    best = {k: min(v) for k, v in t.items()}
    k_track, k_half, k_cons, k_copy = (k for k, _ in runs)
    r_run, r_copy = nbytes / best[k_track] / 1e6, (n * 8) / best[k_copy] / 1e6
    print(f'track_points: {nbytes} compulsory bytes = {r_run:.2f} TB/s; stream copy {r_copy:.2f} TB/s: {r_run / r_copy:.2f} of the '
          f'stream-copy rate; track_points / flow_consistency = {best[k_track] / best[k_cons]:.2f} '
          f'(no backward flow: {best[k_half] / best[k_cons]:.2f})', flush=True)
    track()
    first = (pos_out.clone(), lost_out.clone())
    track()
    codes = torch.bincount(lost_out.reshape(-1).long(), minlength=3).tolist()
    print(f'(codes after the step: tracked {codes[0]}, left the frame {codes[1]}, failed the test {codes[2]}; repeat bit-identical: '
          f'{bool(first[0].view(torch.int32).equal(pos_out.view(torch.int32)) and first[1].equal(lost_out))}; mean |flow| '
          f'{float(fwd.norm(dim=-1).mean()):.2f} px)', flush=True)


def sparse(reps=50, rounds=3):
    from tf_raft_amd import _dev
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    N, H, W = SHAPE
    S, P = SPARSE_STEPS, SPARSE_POINTS
    g = torch.Generator(device='cuda').manual_seed(1)
    fwd, bwd = _flows(S, N, H, W, g)
    pts = torch.stack([torch.rand((N, P), device='cuda', generator=g) * (W - 1), torch.rand((N, P), device='cuda', generator=g) * (H - 1)],
                      dim=-1).contiguous()
    pos_out, lost_out = torch.empty((S, N, P, 2), device='cuda'), torch.empty((S, N, P), device='cuda', dtype=torch.uint8)
    state_p, state_l = pts.clone(), torch.zeros((N, P), device='cuda', dtype=torch.uint8)
    st = _dev.stream_ptr

    def chained():
        check(lib.raft_track_points_f32(_dev.ptr(pts), None, None, 0, _dev.ptr(fwd), _dev.ptr(bwd), _dev.ptr(pos_out), _dev.ptr(lost_out),
                                        S, N, P, H, W, 0.01, 0.5, st()), 'track_points')

    def put_back():
        state_p.copy_(pts)
        state_l.zero_()

    def stepwise():
        put_back()                                   # (measured alone below and subtracted)
        for s in range(S):
            check(lib.raft_track_points_f32(_dev.ptr(state_p), _dev.ptr(state_l), None, s, _dev.ptr(fwd[s]), _dev.ptr(bwd[s]),
                                            _dev.ptr(state_p), _dev.ptr(state_l), 1, N, P, H, W, 0.01, 0.5, st()), 'track_points')
    runs = [(f'track_points, {P} points x {N} videos, S = {S}, ONE launch', chained),
            (f'the same as {S} in-place launches of S = 1, the state put back by two copies first', stepwise),
            ('the two copies alone', put_back)]
    t = _measure(runs, reps, rounds)
    for k, _ in runs:
        print(f'{k} at {SHAPE}, us per call: {_fmt(t[k])}  min {min(t[k]):.1f}', flush=True)
    k1, k8, kc = (k for k, _ in runs)
    stepwise()
    chained()
    torch.cuda.synchronize()
    same = bool(state_p.view(torch.int32).equal(pos_out[-1].view(torch.int32)) and state_l.equal(lost_out[-1]))
    codes = torch.bincount(lost_out[-1].reshape(-1).long(), minlength=3).tolist()
    eight = min(t[k8]) - min(t[kc])
    print(f'{S} launches without the copies {eight:.1f} us; one launch / {S} launches = {min(t[k1]) / eight:.2f}; the two agree bit for '
          f'bit: {same}; codes after {S} steps: tracked {codes[0]}, left {codes[1]}, failed {codes[2]}', flush=True)


def whole_video(repeats=5):
    from tf_raft_amd import image_ops
    from tf_raft_amd import weights as wm
    T, H, W = VIDEO
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    pts = image_ops.point_grid(H, W, stride=4)[0]
    for name, cls in (('small', tf_raft_amd.SmallRAFT), ('raft', tf_raft_amd.RAFT)):
        model = cls(weights=wm.init_weights(name, seed=0), iters_pred=ITERS)
        runs = {'predict_bidirectional': lambda: model.predict_bidirectional([frames[:-1], frames[1:]], batch_size=4),
                'track_video': lambda: model.track_video(frames, pts, batch_size=4),
                'track_video, consistency=False': lambda: model.track_video(frames, pts, consistency=False, batch_size=4)}
        for run in runs.values():
            for _ in range(2):
                run()
        t = {k: [] for k in runs}
        for _ in range(repeats):
            for k, run in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                t[k].append((time.perf_counter() - t0) * 1e3)
        for k, v in t.items():
            print(f"{name}: {k}, {T} frames of {H} x {W} uint8, {len(pts)} points, iters_pred={ITERS}, ms per call: "
                  f"{' '.join(f'{x:.2f}' for x in v)}  mean {np.mean(v):.2f} spread {max(v) - min(v):.2f}", flush=True)
        print(f"{name}: track_video - predict_bidirectional = {np.mean(t['track_video']) - np.mean(t['predict_bidirectional']):.2f} ms "
              f"(ratio {np.mean(t['track_video']) / np.mean(t['predict_bidirectional']):.4f})", flush=True)
        # the same work on device frames with nothing downloaded (predict_bidirectional brings 18 bytes per pixel and pair back,
        # track_video 9 bytes per point and frame): the bidirectional passes alone against the passes with their track launches
        dev_frames, dev_pts = torch.from_numpy(frames).cuda(), torch.from_numpy(pts).cuda()[None]

        def passes(track):
            pos, lost = dev_pts, None
            for a in range(0, T - 1, 4):
                res = model.predict_step_bidirectional((dev_frames[a:a + 4], dev_frames[a + 1:a + 5]))
                if track:
                    p, c = image_ops.track_launch(pos, res.forward.as_subclass(torch.Tensor)[:, None],
                                                  res.backward.as_subclass(torch.Tensor)[:, None], lost, None, a)
                    pos, lost = p[-1], c[-1]
        for track in (False, True):
            passes(track)
        torch.cuda.synchronize()
        td = {False: [], True: []}
        for _ in range(repeats):
            for track in (False, True):
                td[track].append(_timed(lambda: passes(track), 3))
        print(f"{name}: two bidirectional passes of 4 pairs on device frames, ms: {' '.join(f'{x:.3f}' for x in td[False])}  mean "
              f"{np.mean(td[False]):.3f}; with one track launch each: {' '.join(f'{x:.3f}' for x in td[True])}  mean {np.mean(td[True]):.3f}; "
              f"difference {1e3 * (np.mean(td[True]) - np.mean(td[False])):.1f} us (spread {max(td[False]) - min(td[False]):.3f} / "
              f"{max(td[True]) - min(td[True]):.3f} ms)", flush=True)
        lost = model.track_video(frames, pts, batch_size=4)[1]
        print(f'{name}: codes in the last frame: {np.bincount(lost[-1], minlength=3).tolist()} (random weights, random frames)', flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('track_bench.py measures on a GPU; none is visible')
    modes = sys.argv[1:] or ['dense', 'sparse', 'video']
    for mode in modes:
        {'dense': dense, 'sparse': sparse, 'video': whole_video}[mode]()

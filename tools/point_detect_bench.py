"""Measurements behind docs/NOTEBOOK.md section 42 (corner detection and re-seeding), all in one job.

  python tools/point_detect_bench.py [kernels] [tracker]      (no argument: both)
      kernels  uint8 frames (4, 1080, 1920, 3), defaults (min_distance 7, block_radius 1, min_eig, border 8), K = 1024: the score
               launch alone (raft_corner_score_u8_f32 with its maximum), the full detection (raft_detect_points), the detection at
               min_distance = 1 (where the candidate list is longest and ONE workgroup per image selects from it), the detection
               with 1024 live points per image as `avoid`, the refill at P = 1024 (raft_refill_points, in place), one
               raft_warp_u8_f32 launch on the same frames, and raft_stream_copy_f32 at the score map's compulsory 7 bytes per pixel
               (3 read, 4 written).  HIP-event times of back-to-back calls, alternating in one process, three rounds.
      tracker  a FlowTracker push at 4 x 448 x 512 uint8, SmallRAFT and RAFT at iters_pred 12, points=None with max_points = 1024,
               with replenish and without it: HIP-event time per push over pushes that alternate between two frames, five repeats.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402

SHAPE = (4, 1080, 1920)
K = 1024
TRACKER, ITERS = (4, 448, 512), 12


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


def _frames(N, H, W, g):
    """Textured frames: smooth structure of a few dozen pixels plus fine noise, so corners are neither everywhere nor nowhere."""
    coarse = torch.rand((N, 3, H // 24 + 2, W // 24 + 2), device='cuda', generator=g) * 255
    smooth = torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    noise = torch.randn((N, H, W, 3), device='cuda', generator=g) * 12
    return (smooth + noise).clamp(0, 255).round().to(torch.uint8).contiguous()


def kernels(reps=20, rounds=3):
    from tf_raft_amd import _dev, image_ops
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    N, H, W = SHAPE
    g = torch.Generator(device='cuda').manual_seed(0)
    frames = _frames(N, H, W, g)
    st = _dev.stream_ptr
    score, smax = torch.empty((N, H, W), device='cuda'), torch.empty((N,), device='cuda')
    points, scores = torch.empty((N, K, 2), device='cuda'), torch.empty((N, K), device='cuda')
    count, lost = torch.empty((N,), device='cuda', dtype=torch.int32), torch.empty((N, K), device='cuda', dtype=torch.uint8)
    ws = torch.empty((image_ops.detect_workspace_bytes(N, H, W, 1),), device='cuda', dtype=torch.uint8)      # (the larger of the two)
    live = torch.stack([torch.rand((N, K), device='cuda', generator=g) * (W - 1), torch.rand((N, K), device='cuda', generator=g) * (H - 1)],
                       dim=-1).contiguous()
    live_codes = torch.zeros((N, K), device='cuda', dtype=torch.uint8)

    def score_alone():
        check(lib.raft_corner_score_u8_f32(_dev.ptr(frames), _dev.ptr(score), _dev.ptr(smax), N, H, W, 3, 1, 0, 0.04, 8, st()), 'corner_score')

    def detect(m=image_ops.DETECT_MIN_DISTANCE, avoid=False):
        check(lib.raft_detect_points(_dev.ptr(frames), 1, None, _dev.ptr(live) if avoid else None, _dev.ptr(live_codes) if avoid else None,
                                     K if avoid else 0, _dev.ptr(points), _dev.ptr(scores), _dev.ptr(count), _dev.ptr(lost), N, H, W, 3, K, m,
                                     0.01, 1, 0, 0.04, 8, _dev.ptr(ws), st()), 'detect_points')

    # the refill: a state with half its slots lost, refilled in place (the codes are put back by a copy, measured alone)
    pos = live.clone()
    codes0 = (torch.rand((N, K), device='cuda', generator=g) < 0.5).to(torch.uint8) * 2
    codes = codes0.clone()
    born, ids = torch.zeros((N, K), device='cuda', dtype=torch.int32), torch.arange(K, device='cuda', dtype=torch.int32).repeat(N, 1)
    next_id = torch.full((N,), K, device='cuda', dtype=torch.int32)
    detect()
    torch.cuda.synchronize()

    def put_back():
        codes.copy_(codes0)

    def refill():
        put_back()
        check(lib.raft_refill_points(_dev.ptr(pos), _dev.ptr(codes), _dev.ptr(points), _dev.ptr(count), 1, _dev.ptr(pos), _dev.ptr(codes),
                                     _dev.ptr(born), _dev.ptr(ids), _dev.ptr(next_id), N, K, K, st()), 'refill_points')

    flow = torch.randn((N, H, W, 2), device='cuda', generator=g) * 3
    warped = torch.empty((N, H, W, 3), device='cuda')

    def warp():
        check(lib.raft_warp_u8_f32(_dev.ptr(frames), _dev.ptr(flow), _dev.ptr(warped), None, N, H, W, 3, st()), 'warp')
    px = N * H * W
    n = (px * 7 // 8) // 4 * 4                       # floats of a copy that moves 7 bytes per pixel (4 read + 4 written per float)
    a, b = torch.randn((n,), device='cuda'), torch.empty((n,), device='cuda')

    def copy():
        check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, st()), 'stream_copy')
    runs = [('corner_score_u8_f32 (score + maximum)', score_alone),
            (f'detect_points, defaults, K = {K}', detect),
            (f'detect_points, min_distance = 1, K = {K}', lambda: detect(1)),
            (f'detect_points, defaults, avoid = {K} live points per image', lambda: detect(avoid=True)),
            (f'refill_points in place, P = K = {K}, after one copy of the codes', refill),
            ('the copy of the codes alone', put_back),
            ('warp_u8_f32, one launch on the same frames', warp),
            ('stream copy of 7 bytes per pixel', copy)]
    t = _measure(runs, reps, rounds)
    for k, _ in runs:
        print(f'{k} at {SHAPE}, us per call: {_fmt(t[k])}  min {min(t[k]):.1f}  spread {max(t[k]) - min(t[k]):.1f}', flush=True)
    best = {k: min(v) for k, v in t.items()}
    k_score, k_det, k_det1, k_avoid, k_refill, k_back, k_warp, k_copy = (k for k, _ in runs)
    r_copy = (n * 8) / best[k_copy] / 1e6
    for k in (k_score, k_det, k_det1, k_avoid):
        r = px * 7 / best[k] / 1e6
        print(f'{k}: {px * 7} compulsory bytes = {r:.2f} TB/s; stream copy {r_copy:.2f} TB/s: {r / r_copy:.2f} of the stream-copy rate',
              flush=True)
    print(f'detection - score: defaults {best[k_det] - best[k_score]:.1f} us, min_distance = 1 {best[k_det1] - best[k_score]:.1f} us; '
          f'refill without the copy {best[k_refill] - best[k_back]:.1f} us; detection / warp = {best[k_det] / best[k_warp]:.2f}', flush=True)
    for m in (image_ops.DETECT_MIN_DISTANCE, 1):
        detect(m)
        torch.cuda.synchronize()
        first = (points.clone(), scores.clone(), count.clone())
        bound = -(-H // (m + 1)) * -(-W // (m + 1))
        off = N * bound * 8 + (px * 4 + 7) // 8 * 8 + N * 4
        cands = ws[off:off + N * 4].view(torch.int32).tolist()
        detect(m)
        torch.cuda.synchronize()
        same = bool(first[0].view(torch.int32).equal(points.view(torch.int32)) and first[1].view(torch.int32).equal(scores.view(torch.int32))
                    and first[2].equal(count))
        print(f'(min_distance = {m}: candidates per image {cands} of at most {bound}, count {count.tolist()}; repeat bit-identical: {same})',
              flush=True)


def tracker(repeats=5, pushes=6):
    from tf_raft_amd import weights as wm
    N, H, W = TRACKER
    g = torch.Generator(device='cuda').manual_seed(1)
    two = [_frames(N, H, W, g), _frames(N, H, W, g)]
    for name, cls in (('small', tf_raft_amd.SmallRAFT), ('raft', tf_raft_amd.RAFT)):
        model = cls(weights=wm.init_weights(name, seed=0), iters_pred=ITERS)
        t = {}
        trackers = {r: model.tracker(None, max_points=K, replenish=r) for r in (False, True)}
        for tr in trackers.values():
            for i in range(3):
                tr.push(two[i % 2])
        torch.cuda.synchronize()
        for _ in range(repeats):
            for r, tr in trackers.items():
                i = [0]

                def push():
                    tr.push(two[i[0] % 2])
                    i[0] += 1
                t.setdefault(r, []).append(_timed(push, pushes))
        for r in (False, True):
            print(f"{name}: FlowTracker.push, {N} x {H} x {W} uint8, max_points={K}, iters_pred={ITERS}, replenish={r}, ms per push: "
                  f"{' '.join(f'{x:.3f}' for x in t[r])}  mean {np.mean(t[r]):.3f} spread {max(t[r]) - min(t[r]):.3f}", flush=True)
        print(f"{name}: replenish costs {1e3 * (np.mean(t[True]) - np.mean(t[False])):.1f} us per push "
              f"(ratio {np.mean(t[True]) / np.mean(t[False]):.4f}); live points at the end: without {int((trackers[False]._lost == 0).sum())}, "
              f"with {int((trackers[True]._lost == 0).sum())} of {N * K} (random weights, synthetic frames)", flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('point_detect_bench.py measures on a GPU; none is visible')
    modes = sys.argv[1:] or ['kernels', 'tracker']
    for mode in modes:
        {'kernels': kernels, 'tracker': tracker}[mode]()

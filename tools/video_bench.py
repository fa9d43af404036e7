"""Measurements behind docs/NOTEBOOK.md section 23 (flow over frame sequences).

  python tools/video_bench.py push [repeats]
      at N = 4 videos of 448 x 512, iters_pred=24, serial RAFT: ms per FlowVideo.push with warm_start False and True against ms per
      predict_step on the same pairs (the yardstick: the unchanged forward path, fnet on 2N frames), alternating in one process
      with warmed shapes and device events; the triple is repeated (default 7 times) for the run-to-run spread.
  python tools/video_bench.py step [repeats]
      the predict_step measurement alone: what runs on a tree without the video path (the parent commit).
  python tools/video_bench.py kernel
      raft_forward_interpolate_f32 alone at (4, 56, 64) and (6, 56, 128), in us: HIP-event times of back-to-back launches on a
      flow of a few cells of smooth motion; run it under `rocprofv3 --kernel-trace --stats -- python ...` for the kernel's own time.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402

STEP = (4, 448, 512)
CLIP = 6                   # frames of the clip the pushes walk through, again and again
LOW = [(4, 56, 64), (6, 56, 128)]


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _fmt(v):
    return ' '.join(f'{x:.3f}' for x in v)


def _clip():
    rng = np.random.default_rng(0)
    return [torch.as_tensor(rng.uniform(0, 255, STEP + (3,)).astype(np.float32)).cuda() for _ in range(CLIP)]


def push(repeats=7, reps=10, with_push=True):
    model = tf_raft_amd.RAFT(iters_pred=24)
    clip = _clip()
    at = [0]

    def step():
        at[0] += 1
        return model.predict_step((clip[(at[0] - 1) % CLIP], clip[at[0] % CLIP]))

    runs = [('predict_step (fnet on 2N frames)', step)]
    if with_push:
        for warm in (False, True):
            video = model.video(warm_start=warm)
            video.push(clip[0])

            def pushed(video=video):
                at[0] += 1
                return video.push(clip[at[0] % CLIP])
            runs.append((f'push warm_start={warm} (fnet on N frames)', pushed))
    for _ in range(3):
        for _, fn in runs:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in runs]
    for _ in range(repeats):
        for acc, (_, fn) in zip(times, runs):
            acc.append(_timed(fn, reps))
    for (what, _), t in zip(runs, times):
        print(f'{what} at {STEP} ms per call: {_fmt(t)}  mean {np.mean(t):.3f} spread {max(t) - min(t):.3f}', flush=True)
    base = np.mean(times[0])
    for (what, _), t in list(zip(runs, times))[1:]:
        print(f'{what}: {base - np.mean(t):+.3f} ms saved per call against predict_step; larger spread '
              f'{max(max(t) - min(t), max(times[0]) - min(times[0])):.3f} ms', flush=True)


def kernel(reps=50):
    from tf_raft_amd import image_ops
    g = torch.Generator(device='cuda').manual_seed(0)
    for B, h, w in LOW:
        coarse = torch.randn((B, 2, h // 8 + 2, w // 8 + 2), device='cuda', generator=g) * 3
        flow = torch.nn.functional.interpolate(coarse, size=(h, w), mode='bilinear', align_corners=False).permute(0, 2, 3, 1).contiguous()
        out = torch.empty_like(flow)
        run = lambda: image_ops.forward_interpolate_launch(flow, out=out)
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        t = [_timed(run, reps) * 1e3 for _ in range(5)]
        print(f'forward_interpolate at {(B, h, w)}: {B * (h * w) ** 2 / 1e6:.1f} M candidates; back-to-back events us per launch: '
              f'{" ".join(f"{x:.1f}" for x in t)}  mean {np.mean(t):.1f} spread {max(t) - min(t):.1f}', flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('video_bench.py measures on a GPU; none is visible')
    mode = sys.argv[1] if len(sys.argv) > 1 else 'push'
    if mode == 'kernel':
        kernel()
    else:
        push(*(int(v) for v in sys.argv[2:3]), with_push=mode == 'push')

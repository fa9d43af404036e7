"""Writes tests/golden/conditioning_video.json: the fp32-against-fp64 self-agreement of the CPU oracle (see make_conditioning.py)
when its recurrence starts from a given low-resolution flow instead of from zero -- the warm start of a video stream (DESIGN.md
section 16).  The oracle is a subclass, defined here, whose ``initialize_flow`` returns ``(coords0, coords0 + flow_init)``;
nothing else of it changes.

    epe32v64[i] = max EPE of oracle32(i1, i2; flow_init)[i] against oracle64(...)[i]

The init (``smooth_init``) is a seeded smooth field of about two cells' amplitude: a few low-frequency sinusoids per component.
The discontinuous forward projection is deliberately not part of this comparison (tests/test_gpu_flow_init.py pins it bit for
bit).  tests/test_gpu_video.py asserts the project's 1e-3 bound only on cases this file shows at or below 2e-4.

It also holds, under ``VIDEO_KEY``, the same self-agreement of the plain oracle (zero start) on the consecutive pairs of a short
random video (``video_frames``), final prediction only: the pairs ``predict_video`` is compared on.

Run from the repo root:  python tests/golden/make_conditioning_video.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import oracle                                                      # noqa: E402
from oracle.losses import max_epe                                   # noqa: E402
from make_conditioning import case_inputs                           # noqa: E402

B, ITERS = 2, 12
# (variant, H, W, seed)
CASES = [('raft', 64, 96, 0), ('small', 64, 96, 0), ('raft', 72, 104, 2)]


def case_key(variant, H, W, seed):
    return f'{variant}_{H}x{W}_seed{seed}_it{ITERS}_batch{B}_conditioned_init'


def smooth_init(seed, n, h, w):
    """(n, h, w, 2) float32: per image and component three sinusoids of at most one period across the map, amplitudes summing
    to 2 cells, phases and directions drawn from ``default_rng(7000 + seed)``."""
    rng = np.random.default_rng(7000 + seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((n, h, w, 2))
    for b in range(n):
        for c in range(2):
            for amp in (1.0, 0.6, 0.4):
                fy, fx = rng.uniform(-1, 1, size=2)
                out[b, ..., c] += amp * np.sin(2 * np.pi * (fy * ys / h + fx * xs / w) + rng.uniform(0, 2 * np.pi))
    return out.astype(np.float32)


def oracle_with_init(variant, wts, i1, i2, flow_init, dtype=None):
    """Every prediction of the oracle started from ``flow_init``: a list of (B, H, W, 2)."""
    base = oracle.RAFT if variant == 'raft' else oracle.SmallRAFT

    class Started(base):
        def initialize_flow(self, image):
            coords0, _ = super().initialize_flow(image)
            return coords0, coords0 + torch.as_tensor(flow_init).to(self.dtype)

    kw = {} if dtype is None else {'dtype': dtype}
    return [np.asarray(o) for o in Started(wts, iters_pred=ITERS, **kw)([i1, i2])]


VIDEO = ('raft', 64, 96, 0, 5)             # variant, H, W, seed, T
VIDEO_KEY = 'raft_64x96_seed0_it12_video5_conditioned'


def video_frames(seed, T, H, W):
    """(T, H, W, 3) float32 frames in 0 .. 255 from ``default_rng(8000 + seed)``."""
    return np.random.default_rng(8000 + seed).uniform(0, 255, (T, H, W, 3)).astype(np.float32)


def video_inputs():
    variant, H, W, seed, T = VIDEO
    return variant, video_frames(seed, T, H, W), case_inputs(variant, H, W, seed, 'conditioned')[2]


def oracle_pair(variant, wts, a, b, dtype=None):
    """The oracle's final prediction for one pair of frames (H, W, 3): (H, W, 2)."""
    cls = oracle.RAFT if variant == 'raft' else oracle.SmallRAFT
    kw = {} if dtype is None else {'dtype': dtype}
    return np.asarray(cls(wts, iters_pred=ITERS, **kw)([a[None], b[None]])[-1])[0]


def run_video():
    variant, frames, wts = video_inputs()
    pairs = [(oracle_pair(variant, wts, a, b), oracle_pair(variant, wts, a, b, torch.float64)) for a, b in zip(frames[:-1], frames[1:])]
    return dict(epe32v64=[max_epe(a[None], b[None]) for a, b in pairs], max_abs_flow=[float(np.abs(b).max()) for _, b in pairs])


def run(variant, H, W, seed):
    i1, i2, wts = case_inputs(variant, H, W, seed, 'conditioned', B=B)
    init = smooth_init(seed, B, H // 8, W // 8)
    o32 = oracle_with_init(variant, wts, i1, i2, init)
    o64 = oracle_with_init(variant, wts, i1, i2, init, torch.float64)
    cold = oracle.RAFT(wts, iters_pred=ITERS)([i1, i2]) if variant == 'raft' else oracle.SmallRAFT(wts, iters_pred=ITERS)([i1, i2])
    return dict(epe32v64=[max_epe(a, b) for a, b in zip(o32, o64)], max_abs_flow=[float(np.abs(b).max()) for b in o64],
                max_abs_init=float(np.abs(init).max()), final_epe_from_cold=max_epe(o32[-1], np.asarray(cold[-1])))


if __name__ == '__main__':
    path = os.path.join(HERE, 'conditioning_video.json')
    out = {}
    if os.path.exists(path) and '--all' not in sys.argv:
        with open(path) as f:
            out = json.load(f)                   # keep the cases already computed
    for case in CASES:
        key = case_key(*case)
        if key in out:
            continue
        out[key] = run(*case)
        print(key, ' '.join(f'{e:.1e}' for e in out[key]['epe32v64']), f"init {out[key]['max_abs_init']:.2f} from cold {out[key]['final_epe_from_cold']:.2f}",
              flush=True)
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)
    if VIDEO_KEY not in out:
        out[VIDEO_KEY] = run_video()
        print(VIDEO_KEY, ' '.join(f'{e:.1e}' for e in out[VIDEO_KEY]['epe32v64']), flush=True)
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)
    print('wrote', path)

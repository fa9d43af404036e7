"""Writes tests/golden/conditioning_any_size.json: the fp32-against-fp64 self-agreement of the CPU oracle (see
make_conditioning.py) for the parity cases of frames that are NOT the model's size -- the frames are zero-padded or
centre-cropped to the target by the rule of tf.image.resize_with_crop_or_pad, the oracle runs at the target size, and the
predictions are cropped / padded back before they are compared:

    epe32v64[i] = max EPE of crop(oracle32(pad(frames)))[i] against crop(oracle64(pad(frames)))[i]

tests/test_gpu_any_size.py asserts the project's 1e-3 bound only on cases this file shows below 2e-4.  The first case is the
reference's own validation shape (MPI-Sintel 436 x 1024 frames at target 448 x 1024, train_sintel.py:72-75).

Run from the repo root:  python tests/golden/make_conditioning_any_size.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import oracle                                    # noqa: E402
from oracle.losses import max_epe                 # noqa: E402
from make_conditioning import case_inputs         # noqa: E402

# (variant, frame H, frame W, target H, target W, iterations, seed)
CASES = [('raft', 436, 1024, 448, 1024, 24, 0),
         ('raft', 60, 90, 64, 96, 12, 0), ('small', 60, 90, 64, 96, 12, 0),
         ('raft', 59, 155, 64, 160, 12, 1), ('raft', 70, 100, 64, 96, 12, 0)]


def case_key(variant, H, W, th, tw, iters, seed):
    return f'{variant}_{H}x{W}_to_{th}x{tw}_seed{seed}_it{iters}_conditioned'


def np_crop_or_pad(x, th, tw):
    """tf.image.resize_with_crop_or_pad on (..., H, W, C), restated in NumPy."""
    x = np.asarray(x)
    out = np.zeros(x.shape[:-3] + (th, tw, x.shape[-1]), x.dtype)
    (cy, py, ey), (cx, px, ex) = (((max(-(t - s) // 2, 0), max((t - s) // 2, 0), min(s, t))) for s, t in ((x.shape[-3], th), (x.shape[-2], tw)))
    out[..., py:py + ey, px:px + ex, :] = x[..., cy:cy + ey, cx:cx + ex, :]
    return out


def run(variant, H, W, th, tw, iters, seed):
    i1, i2, wts = case_inputs(variant, H, W, seed, 'conditioned')
    p1, p2 = np_crop_or_pad(i1, th, tw), np_crop_or_pad(i2, th, tw)
    cls = oracle.RAFT if variant == 'raft' else oracle.SmallRAFT
    o32 = [np_crop_or_pad(np.asarray(o), H, W) for o in cls(wts, iters_pred=iters)([p1, p2])]
    o64 = [np_crop_or_pad(np.asarray(o), H, W) for o in cls(wts, iters_pred=iters, dtype=torch.float64)([p1, p2])]
    return dict(epe32v64=[max_epe(a, b) for a, b in zip(o32, o64)], max_abs_flow=[float(np.abs(b).max()) for b in o64])


if __name__ == '__main__':
    path = os.path.join(HERE, 'conditioning_any_size.json')
    out = {}
    if os.path.exists(path) and '--all' not in sys.argv:
        with open(path) as f:
            out = json.load(f)                   # keep the cases already computed
    for case in CASES:
        key = case_key(*case)
        if key in out:
            continue
        out[key] = run(*case)
        print(key, ' '.join(f'{e:.1e}' for e in out[key]['epe32v64']), flush=True)
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)
    print('wrote', path)

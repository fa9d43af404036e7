"""Writes tests/golden/conditioning_tiled.json: the fp32-against-fp64 self-agreement of the CPU oracle (see make_conditioning.py)
for the parity cases of tiled inference -- the frames are cut into overlapping tiles of the model's size
by NumPy slicing, the oracle runs on the tiles as one batch, in float32 and in float64, and both sets of predictions are blended
back to the frame's size in float64 by the restatement of tests/test_tile.py before they are compared:

    epe32v64[i] = max EPE of blend(oracle32(tiles(frames)))[i] against blend(oracle64(tiles(frames)))[i]

tests/test_gpu_tile.py asserts the project's 1e-3 bound only on cases this file shows below 2e-4.

Run from the repo root:  python tests/golden/make_conditioning_tiled.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import oracle                                                      # noqa: E402
from oracle.losses import max_epe                                   # noqa: E402
from make_conditioning import case_inputs                           # noqa: E402
from test_tile import np_origins, np_tile_blend, np_tile_gather     # noqa: E402

TILE = (64, 96)
# (variant, frame H, frame W, overlap, iterations, seed)
CASES = [('raft', 100, 150, 16, 12, 0), ('small', 100, 150, 16, 12, 0), ('raft', 60, 200, 32, 12, 1), ('raft', 170, 96, 8, 12, 2)]


def case_key(variant, H, W, overlap, iters, seed):
    return f'{variant}_{H}x{W}_tiles{TILE[0]}x{TILE[1]}_overlap{overlap}_seed{seed}_it{iters}_conditioned'


def oracle_route(variant, wts, i1, i2, overlap, iters, dtype=None):
    """Every prediction of the oracle on the NumPy-gathered tiles, blended in float64: a list of (N, H, W, 2) float64."""
    H, W = i1.shape[1:3]
    oy, ox = np_origins(H, TILE[0], overlap), np_origins(W, TILE[1], overlap)
    t1, t2 = (np_tile_gather(x, TILE[0], TILE[1], oy, ox) for x in (i1, i2))
    cls = oracle.RAFT if variant == 'raft' else oracle.SmallRAFT
    kw = {} if dtype is None else {'dtype': dtype}
    return [np_tile_blend(np.asarray(o), H, W, oy, ox) for o in cls(wts, iters_pred=iters, **kw)([t1, t2])]


def run(variant, H, W, overlap, iters, seed):
    i1, i2, wts = case_inputs(variant, H, W, seed, 'conditioned')
    o32 = oracle_route(variant, wts, i1, i2, overlap, iters)
    o64 = oracle_route(variant, wts, i1, i2, overlap, iters, torch.float64)
    return dict(epe32v64=[max_epe(a, b) for a, b in zip(o32, o64)], max_abs_flow=[float(np.abs(b).max()) for b in o64])


if __name__ == '__main__':
    path = os.path.join(HERE, 'conditioning_tiled.json')
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

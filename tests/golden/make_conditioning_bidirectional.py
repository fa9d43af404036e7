"""Writes tests/golden/conditioning_bidirectional.json: the fp32-against-fp64 self-agreement of the CPU oracle (see
make_conditioning.py) for the parity cases of the bidirectional step -- the oracle runs on the doubled
batch ``[image1 | image2], [image2 | image1]``, whose first half is the forward and whose second half is the backward direction,
in float32 and in float64:

    epe32v64[i] = max EPE of oracle32([i1 | i2], [i2 | i1])[i] against oracle64(...)[i], over both directions

tests/test_gpu_consistency.py asserts the project's 1e-3 bound only on cases this file shows below 2e-4.

Run from the repo root:  python tests/golden/make_conditioning_bidirectional.py
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
CASES = [('raft', 64, 96, 0), ('small', 64, 96, 0), ('raft', 128, 160, 1), ('raft', 72, 104, 2)]


def case_key(variant, H, W, seed):
    return f'{variant}_{H}x{W}_seed{seed}_it{ITERS}_batch{B}_conditioned_bidirectional'


def oracle_both(variant, wts, i1, i2, dtype=None):
    """Every prediction of the oracle on the doubled batch: a list of (2 B, H, W, 2), forward direction first."""
    cls = oracle.RAFT if variant == 'raft' else oracle.SmallRAFT
    kw = {} if dtype is None else {'dtype': dtype}
    return [np.asarray(o) for o in cls(wts, iters_pred=ITERS, **kw)([np.concatenate([i1, i2]), np.concatenate([i2, i1])])]


def run(variant, H, W, seed):
    i1, i2, wts = case_inputs(variant, H, W, seed, 'conditioned', B=B)
    o32 = oracle_both(variant, wts, i1, i2)
    o64 = oracle_both(variant, wts, i1, i2, torch.float64)
    return dict(epe32v64=[max_epe(a, b) for a, b in zip(o32, o64)], max_abs_flow=[float(np.abs(b).max()) for b in o64])


if __name__ == '__main__':
    path = os.path.join(HERE, 'conditioning_bidirectional.json')
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

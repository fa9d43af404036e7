"""Writes tests/golden/flow_init_golden.npz: the forward projection of a flow on six Gaussian flows, as
SciPy computes it the way the RAFT authors' ``forward_interpolate`` applies it (``griddata(method='nearest')`` over the end
points that fall strictly inside the frame, queried at the integer grid, fill value 0), beside this file's float32 restatement
of the library's rule (``np_forward_interpolate``, which tests/test_flow_init.py and tests/test_gpu_flow_init.py import).

The two are different computations: SciPy builds a k-d tree over float64 end points (``x0 + dx`` with an int64 grid promotes to
float64) and does not promise which of two equidistant points it returns; the library works in float32 and breaks ties towards
the lowest source index.  On the six cases here they agree in EVERY cell and the float32 rule has no distance tie (both are
printed and checked below before the fixture is written), so the tests can ask for exact equality.  The fixture holds the inputs
and SciPy's outputs; SciPy is needed to write it, not to run the tests.

Run from the repo root:  python tests/golden/make_flow_init_golden.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# (seed, h, w, scale): flow = default_rng(seed).standard_normal((h, w, 2)) * scale, as float32
CASES = [(0, 8, 12, 2), (1, 9, 13, 4), (2, 56, 64, 3), (3, 23, 37, 10), (4, 1, 7, 1), (5, 56, 64, 0.25)]


def case_flow(seed, h, w, scale):
    return (np.random.default_rng(seed).standard_normal((h, w, 2)) * scale).astype(np.float32)


def np_forward_interpolate(flow, return_ties=False):
    """The rule of include/raft_hip.h (raft_forward_interpolate_f32) in float32 NumPy, one image ``(h, w, 2)`` or a batch
    ``(..., h, w, 2)``.  ``return_ties``: also the number of targets whose smallest distance is reached by more than one source."""
    flow = np.asarray(flow, np.float32)
    if flow.ndim > 3:
        res = [np_forward_interpolate(f, return_ties) for f in flow.reshape((-1,) + flow.shape[-3:])]
        if return_ties:
            return np.stack([r[0] for r in res]).reshape(flow.shape), sum(r[1] for r in res)
        return np.stack(res).reshape(flow.shape)
    h, w, _ = flow.shape
    ys, xs = np.mgrid[0:h, 0:w]
    gx, gy = xs.reshape(-1).astype(np.float32), ys.reshape(-1).astype(np.float32)
    vec = flow.reshape(-1, 2)
    x1, y1 = gx + vec[:, 0], gy + vec[:, 1]                          # float32 + float32: one rounding each
    with np.errstate(invalid='ignore'):
        valid = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
    out, ties = np.zeros_like(vec), 0
    if valid.any():
        for a in range(0, h * w, 512):                                # targets in blocks: (512, h * w) distances at a time
            ex = gx[a:a + 512, None] - x1[None, :]
            ey = gy[a:a + 512, None] - y1[None, :]
            d = ex * ex + ey * ey                                     # float32: each product and the sum rounded on its own
            d[:, ~valid] = np.inf
            win = np.argmin(d, axis=1)                                # the FIRST minimum: the lowest source index
            out[a:a + 512] = vec[win]
            ties += int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    out = out.reshape(h, w, 2)
    return (out, ties) if return_ties else out


def scipy_forward_interpolate(flow):
    """``forward_interpolate`` of the RAFT authors' evaluation code, restated: the end points in float64, SciPy's nearest
    neighbour interpolation of each component at the integer grid."""
    from scipy import interpolate
    dx, dy = flow[..., 0], flow[..., 1]
    h, w = dx.shape
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    x1, y1 = (x0 + dx).reshape(-1), (y0 + dy).reshape(-1)
    valid = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
    pts = (x1[valid], y1[valid])
    fx = interpolate.griddata(pts, dx.reshape(-1)[valid], (x0, y0), method='nearest', fill_value=0)
    fy = interpolate.griddata(pts, dy.reshape(-1)[valid], (x0, y0), method='nearest', fill_value=0)
    return np.stack([fx, fy], axis=-1).astype(np.float32)


if __name__ == '__main__':
    out = {}
    for seed, h, w, scale in CASES:
        flow = case_flow(seed, h, w, scale)
        want = scipy_forward_interpolate(flow)
        got, ties = np_forward_interpolate(flow, return_ties=True)
        differing = int((got != want).any(axis=-1).sum())
        print(f'seed {seed} {h}x{w} scale {scale}: cells that differ from SciPy {differing}, float32 distance ties {ties}', flush=True)
        assert differing == 0 and ties == 0
        out[f'flow_{seed}'], out[f'scipy_{seed}'] = flow, want
    path = os.path.join(HERE, 'flow_init_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')

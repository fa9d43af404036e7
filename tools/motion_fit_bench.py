"""Measurements behind docs/NOTEBOOK.md section 39 (the camera's motion from a flow), all in one job.

  python tools/motion_fit_bench.py
      At (4, 1080, 1920): raft_flow_fit_motion_f32 (affine) at 1 and 5 iterations, with a mask (70 % used) and without one, on a
      preallocated workspace; raft_flow_residual_f32 with both outputs; raft_flow_consistency_f32 (direction a alone) on the SAME
      flow tensors; and raft_stream_copy_f32 at the byte counts the entries cannot avoid.  HIP-event times of back-to-back calls,
      the calls alternating inside each of three rounds.

The compulsory bytes: a pass of the fit reads 8 bytes of flow and, with a mask, 1 byte of mask per pixel, and a fit of k iterations
is k + 1 passes (k moments passes and the statistics pass): 9 (k + 1) bytes per pixel with a mask, 8 (k + 1) without.  The residual
entry reads 8 and writes 8 + 1.  Each is reported as a fraction of the rate the stream copy reaches on that many bytes.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402, F401

SHAPE = (4, 1080, 1920)


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


def main(reps=20, rounds=3):
    from tf_raft_amd import _dev
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    N, H, W = SHAPE
    px = N * H * W
    g = torch.Generator(device='cuda').manual_seed(0)
    # a camera motion (zoom, a small turn, a shift) with noise, a block that moves on its own, and a rough backward flow
    ys, xs = torch.meshgrid(torch.arange(H, device='cuda') - (H - 1) / 2, torch.arange(W, device='cuda') - (W - 1) / 2, indexing='ij')
    field = torch.stack([0.02 * xs - 0.017 * ys + 3.0, 0.017 * xs + 0.02 * ys - 2.0], dim=-1)
    fwd = (field[None] + 0.05 * torch.randn((N, H, W, 2), device='cuda', generator=g)).contiguous()
    fwd[:, H // 5:H // 5 + H // 3, W // 2:W // 2 + W // 3] = torch.tensor([8.0, 5.0], device='cuda')
    bwd = (-fwd + 0.3 * torch.randn((N, H, W, 2), device='cuda', generator=g)).contiguous()
    mask = (torch.rand((N, H, W), device='cuda', generator=g) < 0.7).to(torch.uint8)
    motion, stats = torch.empty((N, 2, 3), device='cuda'), torch.empty((N, 4), device='cuda')
    ws = torch.empty((int(lib.raft_flow_motion_workspace_doubles(N, H, W)),), device='cuda', dtype=torch.float64)
    residual, moving = torch.empty((N, H, W, 2), device='cuda'), torch.empty((N, H, W), device='cuda', dtype=torch.uint8)
    occ = torch.empty((N, H, W), device='cuda', dtype=torch.uint8)
    st = _dev.stream_ptr

    def fit(iterations, m):
        check(lib.raft_flow_fit_motion_f32(_dev.ptr(fwd), _dev.ptr(m) if m is not None else None, 0, _dev.ptr(motion), _dev.ptr(stats), N, H,
                                           W, 2, iterations, 1.0, _dev.ptr(ws), st()), 'fit_motion')

    def resid():
        check(lib.raft_flow_residual_f32(_dev.ptr(fwd), _dev.ptr(motion), _dev.ptr(residual), _dev.ptr(moving), N, H, W, 1.0, st()), 'residual')

    def consistency():
        check(lib.raft_flow_consistency_f32(_dev.ptr(fwd), _dev.ptr(bwd), _dev.ptr(occ), None, N, H, W, 0.01, 0.5, st()), 'flow_consistency')

    copies = {}

    def copy_of(nbytes):
        n = (nbytes // 8) // 4 * 4                   # floats read (and as many written): nbytes moved in all
        if n not in copies:
            copies[n] = (torch.randn((n,), device='cuda'), torch.empty((n,), device='cuda'))
        a, b = copies[n]
        return n * 8, lambda: check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, st()), 'stream_copy')

    entries = [('fit, 1 iteration, no mask', lambda: fit(1, None), px * 8 * 2),
               ('fit, 1 iteration, mask', lambda: fit(1, mask), px * 9 * 2),
               ('fit, 5 iterations, no mask', lambda: fit(5, None), px * 8 * 6),
               ('fit, 5 iterations, mask', lambda: fit(5, mask), px * 9 * 6),
               ('residual, both outputs', resid, px * 17),
               ('flow_consistency, direction a alone', consistency, None)]
    runs = []
    for name, run, nbytes in entries:
        runs.append((name, run))
        if nbytes is not None:
            runs.append((f'stream copy of the bytes of: {name}', copy_of(nbytes)[1]))
    for _ in range(3):
        for _, run in runs:
            run()
    torch.cuda.synchronize()
    t = {k: [] for k, _ in runs}
    for _ in range(rounds):
        for k, run in runs:
            t[k].append(_timed(run, reps) * 1e3)
    for k, _ in runs:
        print(f'{k} at {SHAPE}, us per call: {_fmt(t[k])}  min {min(t[k]):.1f}', flush=True)
    for name, _, nbytes in entries:
        if nbytes is None:
            continue
        moved = copy_of(nbytes)[0]
        r_run, r_copy = nbytes / min(t[name]) / 1e6, moved / min(t[f'stream copy of the bytes of: {name}']) / 1e6
        print(f'{name}: {nbytes} compulsory bytes = {r_run:.2f} TB/s; stream copy {r_copy:.2f} TB/s: {r_run / r_copy:.2f} of the stream-copy '
              f'rate', flush=True)
    one, five = min(t['fit, 1 iteration, mask']), min(t['fit, 5 iterations, mask'])
    print(f'masked fit: one more iteration (a moments pass and a solve) costs {(five - one) / 4:.1f} us; the one-iteration call (two '
          f'passes, a solve and the final launch) {one:.1f} us; flow_consistency {min(t["flow_consistency, direction a alone"]):.1f} us',
          flush=True)
    fit(5, mask)
    first = (motion.clone(), stats.clone())
    fit(5, mask)
    torch.cuda.synchronize()
    same = bool(first[0].view(torch.int32).equal(motion.view(torch.int32)) and first[1].view(torch.int32).equal(stats.view(torch.int32)))
    print(f'(repeat bit-identical: {same}; motion of slice 0: {[round(v, 5) for v in motion[0].reshape(-1).tolist()]}; stats: '
          f'{[round(v, 4) for v in stats[0].tolist()]})', flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('motion_fit_bench.py measures on a GPU; none is visible')
    main()

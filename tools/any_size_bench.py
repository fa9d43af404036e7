"""Measurements behind docs/NOTEBOOK.md section 13 (frames of any size).

  python tools/any_size_bench.py window a|b|c
      one of the three window copies a step on MPI-Sintel frames launches at 4 pairs, alternating with raft_stream_copy_f32 at the
      SAME byte count (read + written); meant to run under `rocprofv3 --kernel-trace --stats -- python ...` (one run per case);
      prints HIP-event times of back-to-back launches as a second opinion.
        a: uint8 (8, 436, 1024, 3) -> float (8, 448, 1024, 3)      both frames in
        b: float (4, 448, 1024, 2) -> float (4, 436, 1024, 2)      the final flow out
        c: float (96, 448, 1024, 2) -> float (96, 436, 1024, 2)    all 24 predictions out
  python tools/any_size_bench.py predict host|auto|fixed [--tree DIR]
      predict() pairs/s on 128 pairs of raw uint8 436 x 1024 frames, 4 per batch, three timed runs: RAFT(pipeline=True) with
      target_size='auto' / (448, 1024), or ('host') without the option on frames zero-padded to 448 x 1024 on the host outside
      the timed region.  --tree DIR imports the package from another checkout (e.g. the parent commit, built there), so that two
      trees can alternate in one job.
"""
import os
import sys
import time

import numpy as np
import torch

args = sys.argv[1:]
tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if '--tree' in args:
    tree = os.path.abspath(args[args.index('--tree') + 1])
sys.path.insert(0, tree)
import tf_raft_amd                                  # noqa: E402


def window(case, reps=30):
    from tf_raft_amd import _dev, image_ops
    from tf_raft_amd._ffi import check
    if case == 'a':
        src, tgt, dt = torch.randint(0, 256, (8, 436, 1024, 3), dtype=torch.uint8, device='cuda'), (448, 1024), torch.float32
    else:
        src, tgt, dt = torch.randn((4 if case == 'b' else 96, 448, 1024, 2), device='cuda'), (436, 1024), None
    out = image_ops.window_copy(src, *tgt, dt)
    nbytes = src.numel() * src.element_size() + out.numel() * out.element_size()
    n = (nbytes // 8) // 4 * 4
    a = torch.randn((n,), device='cuda')
    b = torch.empty_like(a)
    lib = _dev.lib()
    copy = lambda: check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, _dev.stream_ptr()), 'stream_copy')
    win = lambda: image_ops.window_copy(src, *tgt, dt, out=out)
    torch.cuda.synchronize()
    for _ in range(reps):
        copy()
        win()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    t_copy, t_win = timed(copy), timed(win)
    print(f'case {case}: window {tuple(src.shape)} {src.dtype} -> {tuple(out.shape)} {out.dtype}: {nbytes} bytes read + written; '
          f'stream copy {8 * n} bytes; back-to-back events: stream copy {t_copy:.1f} us = {8 * n / t_copy / 1e6:.2f} TB/s, '
          f'window copy {t_win:.1f} us = {nbytes / t_win / 1e6:.2f} TB/s')


def predict(which, N=128):
    rng = np.random.default_rng(0)
    u1 = rng.integers(0, 256, size=(N, 436, 1024, 3), dtype=np.uint8)
    u2 = rng.integers(0, 256, size=(N, 436, 1024, 3), dtype=np.uint8)
    if which == 'host':
        model = tf_raft_amd.RAFT(pipeline=True)
        u1, u2 = (np.pad(x, ((0, 0), (6, 6), (0, 0), (0, 0))) for x in (u1, u2))
    else:
        model = tf_raft_amd.RAFT(pipeline=True, target_size='auto' if which == 'auto' else (448, 1024))
    model.predict([u1[:16], u2[:16]], batch_size=4)
    rates = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.predict([u1, u2], batch_size=4)
        rates.append(N / (time.perf_counter() - t0))
    print(f'predict {which} ({os.path.relpath(tree)}): out {out.shape}, pairs/s ' + ' '.join(f'{r:.1f}' for r in rates), flush=True)


if __name__ == '__main__':
    {'window': window, 'predict': predict}[args[0]](args[1])

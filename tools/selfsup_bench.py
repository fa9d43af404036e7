"""Measurements behind docs/NOTEBOOK.md section 32 (self-supervision: the student pass and its loss).

  python tools/selfsup_bench.py kernel
      raft_selfsup_loss_f32 at n = 12, 8 slices of 304 x 432 inside a teacher of 368 x 496 at origin (32, 32), both masks given and
      every pixel used (a pixel that is not used reads no prediction): value only, value + gradient stored (the way train_step
      calls it) and value + gradient accumulated, each alternating with raft_stream_copy_f32 at the SAME byte count.  The
      compulsory bytes: n*npix*8 of predictions and npix*(8 + 2) of teacher and masks read; with the gradient n*npix*8 written,
      and n*npix*8 more read when it accumulates.  HIP-event times of back-to-back calls (each call is two launches), two
      measurements each, reported as a fraction of the stream-copy rate.
  python tools/selfsup_bench.py step [repeats]
      RAFT, trainable='all', iters = 12, bidirectional: ms per train_step at (4, 368, 496) with selfsup_crop=(32, 32), of the same
      model with model.selfsup_weight = 0 (the step without the option), and, for orientation, of a bidirectional step on
      (4, 304, 432) frames -- the student pass's size.  They alternate in one process with warmed shapes and device events; the
      round is repeated (default 5 times) for the run-to-run spread.  Peak allocated device memory per kind of step.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402

N_PRED, SHAPE, CROP = 12, (4, 368, 496), (32, 32)


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel(reps=20):
    from tf_raft_amd import _dev, losses
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    B, Ht, Wt = 2 * SHAPE[0], SHAPE[1], SHAPE[2]
    (oy, ox), H, W = CROP, Ht - 2 * CROP[0], Wt - 2 * CROP[1]
    npix = B * H * W
    g = torch.Generator(device='cuda').manual_seed(0)
    teacher = torch.randn((B, Ht, Wt, 2), device='cuda', generator=g) * 3
    window = teacher[:, oy:oy + H, ox:ox + W]
    preds = torch.stack([window + 0.5 * torch.randn((B, H, W, 2), device='cuda', generator=g) for _ in range(N_PRED)]).contiguous()
    tv = torch.ones((B, Ht, Wt), dtype=torch.uint8, device='cuda')
    sv = torch.zeros((B, H, W), dtype=torch.uint8, device='cuda')
    d_preds = torch.zeros_like(preds)
    out3 = torch.empty((3,), device='cuda')
    ws = losses._workspace(out3.device, 8 * int(lib.raft_selfsup_loss_workspace_doubles()))

    def entry(with_grad, accumulate):
        check(lib.raft_selfsup_loss_f32(_dev.ptr(teacher), _dev.ptr(tv), Ht, Wt, oy, ox, _dev.ptr(sv), _dev.ptr(preds), 2 * npix, N_PRED, B,
                                        H, W, 0.8, 0.3, 1e-3, 1.0, None, _dev.ptr(out3), _dev.ptr(d_preds) if with_grad else None,
                                        accumulate, _dev.ptr(ws), _dev.stream_ptr()), 'selfsup_loss')

    read = N_PRED * npix * 8 + npix * 10
    for what, nbytes, with_grad, acc in (('value only', read, False, 0), ('value + gradient stored', read + N_PRED * npix * 8, True, 0),
                                         ('value + gradient accumulated', read + 2 * N_PRED * npix * 8, True, 1)):
        n = (nbytes // 8) // 4 * 4
        a = torch.randn((n,), device='cuda')
        b = torch.empty_like(a)
        copy = lambda: check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, _dev.stream_ptr()), 'stream_copy')
        run = lambda: entry(with_grad, acc)
        d_preds.zero_()
        torch.cuda.synchronize()
        for _ in range(5):
            copy()
            run()
        torch.cuda.synchronize()
        t = {k: [] for k in ('copy', 'selfsup')}
        for _ in range(2):
            for k, fn in (('copy', copy), ('selfsup', run)):
                t[k].append(_timed(fn, reps) * 1e3)
        r_copy, r_run = 8 * n / min(t['copy']) / 1e6, nbytes / min(t['selfsup']) / 1e6
        print(f'selfsup loss, {what}, n={N_PRED}, {(B, H, W)} in {(B, Ht, Wt)} at {CROP}: {nbytes} compulsory bytes; back-to-back '
              f'events: stream copy {t["copy"][0]:.1f} / {t["copy"][1]:.1f} us = {r_copy:.2f} TB/s, selfsup entry '
              f'{t["selfsup"][0]:.1f} / {t["selfsup"][1]:.1f} us = {r_run:.3f} TB/s = {r_run / r_copy:.3f} of the stream-copy rate',
              flush=True)
        del a, b
    print(f'(loss {float(out3[0]):.5f}, selfsup {float(out3[1]):.5f}, used {float(out3[2]):.3f} on the measurement\'s inputs)', flush=True)


def step(repeats=5, reps=3):
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    rng = np.random.default_rng(0)
    N, H, W = SHAPE
    Hs, Ws = H - 2 * CROP[0], W - 2 * CROP[1]
    i1, i2 = (torch.as_tensor(rng.uniform(0, 255, SHAPE + (3,)).astype(np.float32)).cuda() for _ in range(2))
    s1, s2 = (torch.as_tensor(rng.uniform(0, 255, (N, Hs, Ws, 3)).astype(np.float32)).cuda() for _ in range(2))
    wts = wm.init_weights('raft', seed=0)

    def model(**kw):
        m = tf_raft_amd.RAFT(weights={k: v.copy() for k, v in wts.items()}, iters=N_PRED)
        m.compile(optimizer=training.AdamW(1e-4, 1e-4), clip_norm=1.0, loss=losses.PhotometricSequenceLoss(), bidirectional=True, **kw)
        return m
    two, small = model(selfsup_crop=CROP), model()

    def two_pass():
        two.selfsup_weight = 0.3
        two.train_step((i1, i2))

    def one_pass():
        two.selfsup_weight = 0.0
        two.train_step((i1, i2))
    runs = {f'two passes, selfsup_crop={CROP}': two_pass, 'selfsup_weight=0 (the step without the option)': one_pass,
            f'bidirectional step on {(N, Hs, Ws)}': lambda: small.train_step((s1, s2))}
    for _ in range(2):
        for run in runs.values():
            run()
    torch.cuda.synchronize()
    t, peak = {k: [] for k in runs}, {}
    for _ in range(repeats):
        for k, run in runs.items():
            torch.cuda.reset_peak_memory_stats()
            t[k].append(_timed(run, reps))
            peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated())
    fmt = lambda v: ' '.join(f'{x:.2f}' for x in v)
    for k, v in t.items():
        print(f'train_step, {k}, iters={N_PRED} at {SHAPE}, ms per step: {fmt(v)}  mean {np.mean(v):.2f} spread {max(v) - min(v):.2f}; '
              f'peak allocated {peak[k] / 2 ** 20:.0f} MiB', flush=True)
    means = [float(np.mean(v)) for v in t.values()]
    print(f'two passes {means[0]:.2f} ms against the sum of the one-pass steps at the two sizes {means[1] + means[2]:.2f} ms '
          f'({means[0] - means[1] - means[2]:+.2f} ms)', flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('selfsup_bench.py measures on a GPU; none is visible')
    if sys.argv[1] == 'kernel':
        kernel()
    else:
        step(*(int(v) for v in sys.argv[2:3]))

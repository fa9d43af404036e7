"""Measurements behind docs/NOTEBOOK.md section 35 (second-order smoothness of the self-supervised loss).

  python tools/smooth2_loss_bench.py kernel
      raft_smooth2_loss_f32 at (n=12, B=4, 368, 496), value only and value + gradient (accumulate = 1, the way the Python layer
      calls it), each alternating with raft_stream_copy_f32 at the SAME byte count and with raft_photometric_loss_f32 on the same
      inputs.  The compulsory bytes: npix*12 of image1, n*npix*8 of predictions read, and with the gradient n*npix*8 written and
      n*npix*8 read again because it accumulates.  HIP-event times of back-to-back calls (each call is two launches), two
      measurements each, reported as a fraction of the stream-copy rate and of the photometric entry's time.
  python tools/smooth2_loss_bench.py step [repeats]
      at the same shape, iters=12, RAFT, trainable='all': ms per train_step with Smooth2SequenceLoss(smooth2_weight=1) and with
      smooth2_weight=0, two models built from the same weights, alternating in one process with warmed shapes and device events;
      the pair of measurements is repeated (default 5 times) for the run-to-run spread.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402

N_PRED, SHAPE = 12, (4, 368, 496)


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
    B, H, W = SHAPE
    npix = B * H * W
    g = torch.Generator(device='cuda').manual_seed(0)
    image1 = torch.randint(0, 256, SHAPE + (3,), device='cuda', generator=g).float()
    image2 = torch.randint(0, 256, SHAPE + (3,), device='cuda', generator=g).float()
    # a few pixels of smooth motion plus noise, a little different per prediction
    coarse = torch.randn((B, 2, H // 64 + 2, W // 64 + 2), device='cuda', generator=g) * 4
    smooth = torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    preds = torch.stack([smooth + 0.3 * torch.randn((B, H, W, 2), device='cuda', generator=g) for _ in range(N_PRED)]).contiguous()
    d_preds = torch.zeros_like(preds)
    out3, out2 = torch.zeros((3,), device='cuda'), torch.empty((2,), device='cuda')
    ws = losses._workspace(out3.device, 8 * max(int(lib.raft_smooth2_loss_workspace_doubles()),
                                                int(lib.raft_photometric_loss_workspace_doubles())))

    def second(with_grad):
        check(lib.raft_smooth2_loss_f32(_dev.ptr(image1), _dev.ptr(preds), 2 * npix, N_PRED, B, H, W, 0.8, 1.0, 10.0, 0.01, 1.0,
                                        _dev.ptr(out3), _dev.ptr(out2), _dev.ptr(d_preds) if with_grad else None, 1, _dev.ptr(ws),
                                        _dev.stream_ptr()), 'smooth2_loss')

    def first(with_grad):
        check(lib.raft_photometric_loss_f32(_dev.ptr(image1), _dev.ptr(image2), None, _dev.ptr(preds), 2 * npix, N_PRED, B, H, W, 0.8,
                                            0.1, 10.0, 0.01, 1.0, _dev.ptr(out3), _dev.ptr(d_preds) if with_grad else None,
                                            _dev.ptr(ws), _dev.stream_ptr()), 'photometric_loss')

    read = npix * 12 + N_PRED * npix * 8
    for what, nbytes, with_grad in (('value only', read, False), ('value + gradient', read + 2 * N_PRED * npix * 8, True)):
        n = (nbytes // 8) // 4 * 4
        a = torch.randn((n,), device='cuda')
        b = torch.empty_like(a)
        copy = lambda: check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, _dev.stream_ptr()), 'stream_copy')
        run = lambda: second(with_grad)
        ref = lambda: first(with_grad)
        torch.cuda.synchronize()
        for _ in range(5):
            copy()
            ref()
            run()
        torch.cuda.synchronize()
        t = {k: [] for k in ('copy', 'photometric', 'smooth2')}
        for _ in range(2):
            for k, fn in (('copy', copy), ('photometric', ref), ('smooth2', run)):
                t[k].append(_timed(fn, reps) * 1e3)
        r_copy, r_run = 8 * n / min(t['copy']) / 1e6, nbytes / min(t['smooth2']) / 1e6
        print(f'smooth2 loss, {what}, n={N_PRED} at {SHAPE}: {nbytes} compulsory bytes; back-to-back events: stream copy '
              f'{t["copy"][0]:.1f} / {t["copy"][1]:.1f} us = {r_copy:.2f} TB/s, photometric entry {t["photometric"][0]:.1f} / '
              f'{t["photometric"][1]:.1f} us, smooth2 entry {t["smooth2"][0]:.1f} / {t["smooth2"][1]:.1f} us = {r_run:.3f} TB/s = '
              f'{r_run / r_copy:.3f} of the stream-copy rate, {min(t["smooth2"]) / min(t["photometric"]):.2f} x the photometric entry',
              flush=True)
        del a, b
    out3.zero_()
    second(False)
    print(f'(smoothness2 {float(out2[1]):.5f} on the measurement\'s inputs)', flush=True)


def step(repeats=5, reps=3):
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    rng = np.random.default_rng(0)
    i1, i2 = (torch.as_tensor(rng.uniform(0, 255, SHAPE + (3,)).astype(np.float32)).cuda() for _ in range(2))
    mask = (torch.as_tensor(rng.uniform(size=SHAPE) < 0.8).cuda()).to(torch.uint8)
    wts = wm.init_weights('raft', seed=0)
    models = {}
    for name, sw in (('smooth2_weight=1', 1.0), ('smooth2_weight=0', 0.0)):
        m = tf_raft_amd.RAFT(weights={k: v.copy() for k, v in wts.items()}, iters=N_PRED)
        m.compile(optimizer=training.AdamW(1e-4, 1e-4), clip_norm=1.0, loss=losses.Smooth2SequenceLoss(smooth2_weight=sw))
        models[name] = m
    runs = {name: (lambda m=m: m.train_step((i1, i2, mask))) for name, m in models.items()}
    for _ in range(2):
        for run in runs.values():
            run()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(repeats):
        for k, run in runs.items():
            t[k].append(_timed(run, reps))
    fmt = lambda v: ' '.join(f'{x:.2f}' for x in v)
    for k, v in t.items():
        print(f'train_step, {k}, iters={N_PRED} at {SHAPE}, ms per step: {fmt(v)}  mean {np.mean(v):.2f} spread {max(v) - min(v):.2f}', flush=True)
    print(f'difference of the means {np.mean(t["smooth2_weight=1"]) - np.mean(t["smooth2_weight=0"]):.2f} ms', flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('smooth2_loss_bench.py measures on a GPU; none is visible')
    if sys.argv[1] == 'kernel':
        kernel()
    else:
        step(*(int(v) for v in sys.argv[2:3]))

"""Measurements behind docs/NOTEBOOK.md section 24 (self-supervised sequence loss).

  python tools/photometric_loss_bench.py kernel
      raft_photometric_loss_f32 at (n=12, B=4, 368, 496), value only and value + gradient, each alternating with
      raft_stream_copy_f32 at the SAME byte count.  The compulsory bytes: n*npix*8 of predictions read, n*npix*8 of gradient
      written (value + gradient only), 2*npix*12 of frames, npix of mask (the gathered taps and the flow stencil are re-reads of
      bytes already counted).  HIP-event times of back-to-back launches (each includes the one-workgroup reduction launch),
      reported as a fraction of the stream-copy rate.
  python tools/photometric_loss_bench.py step [repeats]
      at the same shape, iters=12, RAFT, trainable='all': ms per train_step with PhotometricSequenceLoss and with sequence_loss,
      two models built from the same weights, alternating in one process with warmed shapes and device events; the pair of
      measurements is repeated (default 5 times) for the run-to-run spread.
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


def kernel(reps=30):
    from tf_raft_amd import _dev, losses
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    B, H, W = SHAPE
    npix = B * H * W
    g = torch.Generator(device='cuda').manual_seed(0)
    image1 = torch.randint(0, 256, SHAPE + (3,), device='cuda', generator=g).float()
    image2 = torch.randint(0, 256, SHAPE + (3,), device='cuda', generator=g).float()
    mask = (torch.rand(SHAPE, device='cuda', generator=g) < 0.8).to(torch.uint8)
    # a few pixels of smooth motion plus noise, a little different per prediction: neighbouring lanes gather neighbouring taps
    coarse = torch.randn((B, 2, H // 64 + 2, W // 64 + 2), device='cuda', generator=g) * 4
    smooth = torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    preds = torch.stack([smooth + 0.3 * torch.randn((B, H, W, 2), device='cuda', generator=g) for _ in range(N_PRED)]).contiguous()
    d_preds = torch.empty_like(preds)
    out = torch.empty((3,), device='cuda')
    ws = losses._photometric_workspace(out.device)

    def launch(with_grad):
        check(lib.raft_photometric_loss_f32(_dev.ptr(image1), _dev.ptr(image2), _dev.ptr(mask), _dev.ptr(preds), 2 * npix, N_PRED, B, H, W,
                                            0.8, 0.1, 10.0, 0.01, 1.0, _dev.ptr(out), _dev.ptr(d_preds) if with_grad else None,
                                            _dev.ptr(ws), _dev.stream_ptr()), 'photometric_loss')

    read = N_PRED * npix * 8 + 2 * npix * 12 + npix
    for what, nbytes, run in (('value only', read, lambda: launch(False)), ('value + gradient', read + N_PRED * npix * 8, lambda: launch(True))):
        n = (nbytes // 8) // 4 * 4
        a = torch.randn((n,), device='cuda')
        b = torch.empty_like(a)
        copy = lambda: check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, _dev.stream_ptr()), 'stream_copy')
        torch.cuda.synchronize()
        for _ in range(reps):
            copy()
            run()
        torch.cuda.synchronize()
        t_copy, t_run = _timed(copy, reps) * 1e3, _timed(run, reps) * 1e3
        t_copy2, t_run2 = _timed(copy, reps) * 1e3, _timed(run, reps) * 1e3
        r_copy, r_run = 8 * n / min(t_copy, t_copy2) / 1e6, nbytes / min(t_run, t_run2) / 1e6
        print(f'photometric loss, {what}, n={N_PRED} at {SHAPE}: {nbytes} compulsory bytes; back-to-back events: stream copy '
              f'{t_copy:.1f} / {t_copy2:.1f} us = {r_copy:.2f} TB/s, entry {t_run:.1f} / {t_run2:.1f} us = {r_run:.2f} TB/s = '
              f'{r_run / r_copy:.2f} of the stream-copy rate', flush=True)
        del a, b
    print(f'(loss {float(out[0]):.5f}, photometric {float(out[1]):.5f}, smoothness {float(out[2]):.5f} on the measurement\'s inputs)', flush=True)


def step(repeats=5, reps=3):
    from tf_raft_amd import losses, training
    rng = np.random.default_rng(0)
    B, H, W = SHAPE
    i1, i2 = (torch.as_tensor(rng.uniform(0, 255, SHAPE + (3,)).astype(np.float32)).cuda() for _ in range(2))
    flow = torch.as_tensor((rng.normal(size=SHAPE + (2,)) * 2).astype(np.float32)).cuda()
    valid = torch.as_tensor(rng.uniform(size=SHAPE) < 0.9).cuda()
    mask = (torch.as_tensor(rng.uniform(size=SHAPE) < 0.8).cuda()).to(torch.uint8)
    models = {}
    for name, loss in (('photometric', losses.PhotometricSequenceLoss()), ('supervised', losses.sequence_loss)):
        m = tf_raft_amd.RAFT(iters=N_PRED)
        m.compile(optimizer=training.AdamW(1e-4, 1e-4), clip_norm=1.0, loss=loss)
        models[name] = m
    runs = {'photometric': lambda: models['photometric'].train_step((i1, i2, mask)),
            'supervised': lambda: models['supervised'].train_step((i1, i2, flow, valid))}
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
        print(f'train_step, {k} loss, iters={N_PRED} at {SHAPE}, ms per step: {fmt(v)}  mean {np.mean(v):.2f} spread {max(v) - min(v):.2f}', flush=True)
    print(f'difference of the means {np.mean(t["photometric"]) - np.mean(t["supervised"]):.2f} ms', flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('photometric_loss_bench.py measures on a GPU; none is visible')
    if sys.argv[1] == 'kernel':
        kernel()
    else:
        step(*(int(v) for v in sys.argv[2:3]))

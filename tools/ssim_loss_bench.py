"""Measurements behind docs/NOTEBOOK.md section 29 (SSIM term of the self-supervised loss).

  python tools/ssim_loss_bench.py kernel
      raft_ssim_loss_f32 at (n=12, B=4, 368, 496), value only and value + gradient (accumulate = 1, the way the Python layer calls
      it), each alternating with raft_stream_copy_f32 at the SAME byte count and, for orientation, with raft_census_loss_f32 on the
      same inputs.  The compulsory bytes are tools/census_loss_bench.py's: n*npix*8 of predictions read, 2*npix*12 of frames,
      npix of mask, and with the gradient n*npix*8 read and n*npix*8 written (the workspace planes are the design's own traffic
      and not counted).  HIP-event times of back-to-back calls (each call is three launches), two measurements each, reported
      as a fraction of the stream-copy rate.
  python tools/ssim_loss_bench.py step [repeats]
      at the same shape, iters=12, RAFT, trainable='all': ms per train_step with SSIMSequenceLoss(ssim_weight=1) and with
      ssim_weight=0, two models built from the same weights, alternating in one process with warmed shapes and device events;
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
    mask = (torch.rand(SHAPE, device='cuda', generator=g) < 0.8).to(torch.uint8)
    # a few pixels of smooth motion plus noise, a little different per prediction: neighbouring lanes gather neighbouring taps
    coarse = torch.randn((B, 2, H // 64 + 2, W // 64 + 2), device='cuda', generator=g) * 4
    smooth = torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    preds = torch.stack([smooth + 0.3 * torch.randn((B, H, W, 2), device='cuda', generator=g) for _ in range(N_PRED)]).contiguous()
    d_preds = torch.zeros_like(preds)
    out3, out2 = torch.empty((3,), device='cuda'), torch.empty((2,), device='cuda')
    need = int(lib.raft_ssim_loss_workspace_bytes(N_PRED, B, H, W))
    need_census = int(lib.raft_census_loss_workspace_bytes(N_PRED, B, H, W))
    ws = losses._workspace(out3.device, max(need, need_census))
    print(f'workspace {need} bytes = {need / 2 ** 20:.1f} MiB at n={N_PRED}, {SHAPE} (census entry: {need_census} bytes)', flush=True)

    def entry(fn, name, with_grad):
        check(fn(_dev.ptr(image1), _dev.ptr(image2), _dev.ptr(mask), _dev.ptr(preds), 2 * npix, N_PRED, B, H, W, 0.8, 1.0, 1.0,
                 _dev.ptr(out3), _dev.ptr(out2), _dev.ptr(d_preds) if with_grad else None, 1, _dev.ptr(ws), _dev.stream_ptr()), name)

    out3.zero_()
    read = N_PRED * npix * 8 + 2 * npix * 12 + npix
    for what, nbytes, with_grad in (('value only', read, False), ('value + gradient', read + 2 * N_PRED * npix * 8, True)):
        n = (nbytes // 8) // 4 * 4
        a = torch.randn((n,), device='cuda')
        b = torch.empty_like(a)
        copy = lambda: check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, _dev.stream_ptr()), 'stream_copy')
        run = lambda: entry(lib.raft_ssim_loss_f32, 'ssim_loss', with_grad)
        ref = lambda: entry(lib.raft_census_loss_f32, 'census_loss', with_grad)
        torch.cuda.synchronize()
        for _ in range(5):
            copy()
            ref()
            run()
        torch.cuda.synchronize()
        t = {k: [] for k in ('copy', 'census', 'ssim')}
        for _ in range(2):
            for k, fn in (('copy', copy), ('census', ref), ('ssim', run)):
                t[k].append(_timed(fn, reps) * 1e3)
        r_copy, r_run = 8 * n / min(t['copy']) / 1e6, nbytes / min(t['ssim']) / 1e6
        print(f'ssim loss, {what}, n={N_PRED} at {SHAPE}: {nbytes} compulsory bytes; back-to-back events: stream copy '
              f'{t["copy"][0]:.1f} / {t["copy"][1]:.1f} us = {r_copy:.2f} TB/s, census entry {t["census"][0]:.1f} / '
              f'{t["census"][1]:.1f} us, ssim entry {t["ssim"][0]:.1f} / {t["ssim"][1]:.1f} us = {r_run:.3f} TB/s = '
              f'{r_run / r_copy:.3f} of the stream-copy rate, {min(t["ssim"]) / min(t["census"]):.2f} x the census entry',
              flush=True)
        del a, b
    print(f'(loss {float(out2[0]):.5f}, ssim {float(out2[1]):.5f} on the measurement\'s inputs)', flush=True)


def step(repeats=5, reps=3):
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    rng = np.random.default_rng(0)
    i1, i2 = (torch.as_tensor(rng.uniform(0, 255, SHAPE + (3,)).astype(np.float32)).cuda() for _ in range(2))
    mask = (torch.as_tensor(rng.uniform(size=SHAPE) < 0.8).cuda()).to(torch.uint8)
    wts = wm.init_weights('raft', seed=0)
    models = {}
    for name, sw in (('ssim_weight=1', 1.0), ('ssim_weight=0', 0.0)):
        m = tf_raft_amd.RAFT(weights={k: v.copy() for k, v in wts.items()}, iters=N_PRED)
        m.compile(optimizer=training.AdamW(1e-4, 1e-4), clip_norm=1.0, loss=losses.SSIMSequenceLoss(ssim_weight=sw))
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
    print(f'difference of the means {np.mean(t["ssim_weight=1"]) - np.mean(t["ssim_weight=0"]):.2f} ms', flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('ssim_loss_bench.py measures on a GPU; none is visible')
    if sys.argv[1] == 'kernel':
        kernel()
    else:
        step(*(int(v) for v in sys.argv[2:3]))

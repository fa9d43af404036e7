"""Measurements behind docs/NOTEBOOK.md section 19 (tiled inference): 1080 x 1920 uint8 frames under 448 x 1024 tiles at the default
overlap of 64, which is 3 x 2 = 6 tiles per frame.

  python tools/tile_bench.py kernels
      the three launches of one call, each alternating with raft_stream_copy_f32 at the SAME byte count (read + written, every
      byte counted once): the gather of one frame tensor in front of the model, the blend of the final prediction (predict_step)
      and the blend of all 24 predictions (__call__), at 1 pair per call.  HIP-event times of back-to-back launches; run it under
      `rocprofv3 --kernel-trace --stats -- python ...` for the kernels' own times.
  python tools/tile_bench.py predict tile|plain|resize
      predict() pairs/s of RAFT(pipeline=True, target_size=(448, 1024)), three timed runs:
        tile    64 pairs of 1080p frames, fit='tile', batch_size=1 (6 tiles per model call)
        plain   the same model WITHOUT the option on 384 = 64 x 6 pairs of 448 x 1024 frames, batch_size=6: what the tiles alone
                cost; reported in 1080p pairs (model pairs / 6) so that the difference from 'tile' is the feature's whole overhead
        resize  64 pairs of 1080p frames, fit='resize', batch_size=1, for context (one model pair per frame pair)
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402

FRAME, TILE, OVERLAP = (1080, 1920), (448, 1024), 64


def kernels(reps=30):
    from tf_raft_amd import _dev, image_ops
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    plan = image_ops.TilePlan(torch.device('cuda', torch.cuda.current_device()), *FRAME, *TILE, OVERLAP)
    assert plan.K == 6, plan.K

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    frames = torch.randint(0, 256, (1,) + FRAME + (3,), dtype=torch.uint8, device='cuda')
    cases = [('gather uint8 frame -> 6 float tiles', frames, lambda s, o: image_ops.tile_gather_launch(s, plan, out=o))]
    for M, what in ((1, 'blend the final prediction'), (24, 'blend 24 predictions')):
        cases.append((what, torch.randn((M, plan.K) + TILE + (2,), device='cuda'), lambda s, o: image_ops.tile_blend_launch(s, plan, out=o)))
    for what, src, launch in cases:
        out = launch(src, None)
        nbytes = src.numel() * src.element_size() + out.numel() * out.element_size()
        n = (nbytes // 8) // 4 * 4
        a = torch.randn((n,), device='cuda')
        b = torch.empty_like(a)
        copy = lambda: check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, _dev.stream_ptr()), 'stream_copy')
        run = lambda: launch(src, out)
        torch.cuda.synchronize()
        for _ in range(reps):
            copy()
            run()
        torch.cuda.synchronize()
        t_copy, t_run = timed(copy), timed(run)
        t_copy2, t_run2 = timed(copy), timed(run)
        print(f'{what}: {tuple(src.shape)} {src.dtype} -> {tuple(out.shape)}: {nbytes} bytes read + written; back-to-back events: '
              f'stream copy {t_copy:.1f} / {t_copy2:.1f} us = {8 * n / min(t_copy, t_copy2) / 1e6:.2f} TB/s, '
              f'kernel {t_run:.1f} / {t_run2:.1f} us = {nbytes / min(t_run, t_run2) / 1e6:.2f} TB/s', flush=True)
        del a, b, out


def predict(which, N=64):
    rng = np.random.default_rng(0)
    K = 6
    if which == 'plain':
        model, shape, bs, per = tf_raft_amd.RAFT(pipeline=True), (N * K,) + TILE + (3,), K, K
    else:
        kw = {'fit': 'tile', 'tile_overlap': OVERLAP} if which == 'tile' else {'fit': 'resize'}
        model, shape, bs, per = tf_raft_amd.RAFT(pipeline=True, target_size=TILE, **kw), (N,) + FRAME + (3,), 1, 1
    u1 = rng.integers(0, 256, size=shape, dtype=np.uint8)
    u2 = rng.integers(0, 256, size=shape, dtype=np.uint8)
    model.predict([u1[:4 * bs], u2[:4 * bs]], batch_size=bs)
    rates = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.predict([u1, u2], batch_size=bs)
        rates.append(shape[0] / per / (time.perf_counter() - t0))
    print(f'predict {which}: in {shape}, batch_size {bs}, out {out.shape}, 1080p pairs/s ' + ' '.join(f'{r:.2f}' for r in rates), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('tile_bench.py measures on a GPU; none is visible')
    if sys.argv[1] == 'kernels':
        kernels()
    else:
        predict(sys.argv[2])

"""Measurements behind docs/NOTEBOOK.md section 30 (bidirectional training step with in-step occlusion masks).

  python tools/bidirectional_train_bench.py kernel
      raft_flow_visibility_f32 (two launches: the test with its count, the one-workgroup sum) on (2*4, 368, 496) flows, with and
      without a mask and count only, against raft_flow_consistency_f32 (one launch, no count) on the same flows, alternating, all on
      preallocated outputs; and the Python launcher, which allocates its two outputs.  HIP-event times of back-to-back calls.
  python tools/bidirectional_train_bench.py step [repeats]
      at (4, 368, 496), iters=12, RAFT, trainable='all', PhotometricSequenceLoss: ms per step of
        bidirectional      train_step((image1, image2)) of a model compiled with bidirectional=True (occlusion on)
        (a) unidirectional train_step((image1, image2)) on the same 4 pairs
        (b) doubled batch  the unidirectional train_step on the 8 pairs [image1 | image2], [image2 | image1]
        (c) two passes     predict_step_bidirectional((image1, image2)), then the unidirectional train_step with
                           occluded_forward == 0 as its mask: the recipe without this step
      four models built from the same weights, alternating in one process with warmed shapes and device events; the round of
      measurements is repeated (default 5 times) for the run-to-run spread.  Peak device memory of each route is printed too (the
      bidirectional step keeps the loop's tape for 2N pairs).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402

ITERS, SHAPE = 12, (4, 368, 496)


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _fmt(v):
    return ' '.join(f'{x:.2f}' for x in v)


def kernel(reps=50, rounds=3):
    from tf_raft_amd import _dev, image_ops, losses
    from tf_raft_amd._ffi import check
    N, H, W = SHAPE
    g = torch.Generator(device='cuda').manual_seed(0)
    # a few pixels of smooth motion, the backward flow roughly its negative: neighbouring lanes gather neighbouring taps
    coarse = torch.randn((N, 2, H // 64 + 2, W // 64 + 2), device='cuda', generator=g) * 4
    smooth = torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    fwd = (smooth + 0.3 * torch.randn((N, H, W, 2), device='cuda', generator=g)).contiguous()
    bwd = (-smooth + 0.3 * torch.randn((N, H, W, 2), device='cuda', generator=g)).contiguous()
    flows = torch.cat([fwd, bwd]).contiguous()
    mask = (torch.rand((2 * N, H, W), device='cuda', generator=g) < 0.8).to(torch.uint8)
    # the C entries themselves on preallocated outputs (the Python launchers add two allocations per call)
    lib = _dev.lib()
    out = torch.empty((2 * N, H, W), device='cuda', dtype=torch.uint8)
    share = torch.empty((), device='cuda')
    ws = losses._workspace(out.device, 8 * int(lib.raft_flow_visibility_workspace_doubles()))

    def consistency():
        check(lib.raft_flow_consistency_f32(_dev.ptr(fwd), _dev.ptr(bwd), _dev.ptr(out[:N]), _dev.ptr(out[N:]), N, H, W, 0.01, 0.5,
                                            _dev.stream_ptr()), 'flow_consistency')

    def visibility(m, vis=out):
        check(lib.raft_flow_visibility_f32(_dev.ptr(flows), _dev.ptr(m) if m is not None else None, _dev.ptr(vis) if vis is not None else None,
                                           _dev.ptr(share), N, H, W, 0.01, 0.5, 1, _dev.ptr(ws), _dev.stream_ptr()), 'flow_visibility')
    runs = {'flow_consistency (one launch, no count)': consistency,
            'flow_visibility, no mask (two launches)': lambda: visibility(None),
            'flow_visibility, mask': lambda: visibility(mask),
            'flow_visibility, count only (visible = NULL)': lambda: visibility(None, None),
            'flow_visibility_launch, no mask (Python launcher: + two allocations)': lambda: image_ops.flow_visibility_launch(flows, N)}
    for _ in range(5):
        for run in runs.values():
            run()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(rounds):
        for k, run in runs.items():
            t[k].append(_timed(run, reps) * 1e3)
    for k, v in t.items():
        print(f'{k}, {2 * N} slices of {H}x{W}, us per call: {_fmt(v)}  min {min(v):.1f}', flush=True)
    occ = image_ops.flow_consistency_launch(fwd, bwd)
    vis, frac = image_ops.flow_visibility_launch(flows, N)
    same = bool((torch.cat(occ) == 0).to(torch.uint8).equal(vis))
    print(f'(occluded share {float(frac):.4f} on the measurement\'s flows; visible == !occluded of the consistency kernel: {same})', flush=True)


def step(repeats=5, reps=2):
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    rng = np.random.default_rng(0)
    i1, i2 = (torch.as_tensor(rng.uniform(0, 255, SHAPE + (3,)).astype(np.float32)).cuda() for _ in range(2))
    d1, d2 = torch.cat([i1, i2]), torch.cat([i2, i1])
    wts = wm.init_weights('raft', seed=0)

    def model(**kw):
        m = tf_raft_amd.RAFT(weights={k: v.copy() for k, v in wts.items()}, iters=ITERS, iters_pred=ITERS)
        m.compile(optimizer=training.AdamW(1e-4, 1e-4), clip_norm=1.0, loss=losses.PhotometricSequenceLoss(), **kw)
        return m
    bi, uni, dbl, two = model(bidirectional=True), model(), model(), model()

    def two_passes():
        res = two.predict_step_bidirectional((i1, i2))
        return two.train_step((i1, i2, res.occluded_forward == 0))
    runs = {'bidirectional step, 4 pairs both ways': lambda: bi.train_step((i1, i2)),
            '(a) unidirectional step, 4 pairs': lambda: uni.train_step((i1, i2)),
            '(b) unidirectional step, doubled batch of 8': lambda: dbl.train_step((d1, d2)),
            '(c) predict_step_bidirectional + masked unidirectional step': two_passes}
    peak = {}
    for k, run in runs.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() / 2 ** 30
    t = {k: [] for k in runs}
    for _ in range(repeats):
        for k, run in runs.items():
            t[k].append(_timed(run, reps))
    for k, v in t.items():
        print(f'{k}, iters={ITERS} at {SHAPE}, ms per step: {_fmt(v)}  mean {np.mean(v):.2f} spread {max(v) - min(v):.2f}; '
              f'peak allocated while warming {peak[k]:.2f} GiB (the models before it included)', flush=True)
    m = {k: float(np.mean(v)) for k, v in t.items()}
    b, a, d, c = (m[k] for k in runs)
    print(f'bidirectional / (a) = {b / a:.3f}, / (b) = {b / d:.3f}, / (c) = {b / c:.3f}; the occluded share the step reported: '
          f'{float(bi.flow_metrics["occluded"].result()):.4f} (random weights: a number about the inputs, not about accuracy)', flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('bidirectional_train_bench.py measures on a GPU; none is visible')
    if sys.argv[1] == 'kernel':
        kernel()
    else:
        step(*(int(v) for v in sys.argv[2:3]))

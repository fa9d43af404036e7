"""Measurements behind docs/NOTEBOOK.md section 31 (the range map as a second occlusion test).

  python tools/range_occlusion_bench.py kernels
      at (4, 1080, 1920) and at 2 x 4 slices of 368 x 496: raft_flow_range_map_f32, raft_flow_range_occlusion_f32 (both directions)
      and raft_flow_range_visibility_f32 on preallocated outputs, alternating in one process with raft_flow_consistency_f32 /
      raft_flow_visibility_f32 on the SAME flows and with raft_stream_copy_f32 at each entry's compulsory byte count (the flows
      read once, the outputs written once: the uint64 sums are a workspace -- zeroed, added to and read back -- and are NOT
      counted, so the share says what the splat costs over a gather of the same inputs).  Also the zeroing alone (a torch fill of
      the same bytes, for scale) and the scatter under a flow that sends every vector of a frame to one pixel.  HIP-event times of
      back-to-back calls; run it under `rocprofv3 --kernel-trace --stats -- python ...` for the kernels' own times.
  python tools/range_occlusion_bench.py step [repeats]
      at (4, 368, 496), iters=12, RAFT, trainable='all', PhotometricSequenceLoss, bidirectional=True: ms per train_step with
      occlusion_test='range' against 'consistency', two models built from the same weights, alternating in one process with warmed
      shapes and device events; the pair is repeated (default 5 times) for the run-to-run spread.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_raft_amd                                  # noqa: E402

SHAPES = ((4, 1080, 1920), (4, 368, 496))
ITERS, STEP = 12, (4, 368, 496)


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


def _kernels_at(shape, reps, rounds):
    from tf_raft_amd import _dev, image_ops
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    N, H, W = shape
    g = torch.Generator(device='cuda').manual_seed(0)
    # a few pixels of smooth motion, the backward flow roughly its negative: a wave's adds to one row are neighbours
    coarse = torch.randn((N, 2, H // 64 + 2, W // 64 + 2), device='cuda', generator=g) * 4
    smooth = torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    fwd = (smooth + 0.3 * torch.randn((N, H, W, 2), device='cuda', generator=g)).contiguous()
    bwd = (-smooth + 0.3 * torch.randn((N, H, W, 2), device='cuda', generator=g)).contiguous()
    flows = torch.cat([fwd, bwd]).contiguous()
    ys, xs = torch.arange(H, device='cuda', dtype=torch.float32), torch.arange(W, device='cuda', dtype=torch.float32)
    one = torch.stack([(W // 3 - xs)[None, :].expand(H, W), (H // 2 - ys)[:, None].expand(H, W)], dim=-1)[None].expand(N, H, W, 2).contiguous()
    px = N * H * W
    rng_out = torch.empty((N, H, W), device='cuda')
    masks = torch.empty((2 * N, H, W), device='cuda', dtype=torch.uint8)
    share = torch.empty((), device='cuda')
    sums = torch.empty((int(lib.raft_flow_range_workspace_bytes(2 * N, H, W)) // 8,), device='cuda', dtype=torch.int64)
    records = torch.empty((int(lib.raft_flow_visibility_workspace_doubles()),), device='cuda', dtype=torch.float64)
    st = _dev.stream_ptr

    def range_map(f=fwd):
        check(lib.raft_flow_range_map_f32(_dev.ptr(f), _dev.ptr(rng_out), N, H, W, _dev.ptr(sums), st()), 'range_map')

    def range_occlusion():
        check(lib.raft_flow_range_occlusion_f32(_dev.ptr(fwd), _dev.ptr(bwd), _dev.ptr(masks[:N]), _dev.ptr(masks[N:]), N, H, W, 0.5,
                                                _dev.ptr(sums), st()), 'range_occlusion')

    def range_visibility():
        check(lib.raft_flow_range_visibility_f32(_dev.ptr(flows), None, _dev.ptr(masks), _dev.ptr(share), N, H, W, 0.5, 1, _dev.ptr(sums),
                                                 _dev.ptr(records), st()), 'range_visibility')

    def consistency():
        check(lib.raft_flow_consistency_f32(_dev.ptr(fwd), _dev.ptr(bwd), _dev.ptr(masks[:N]), _dev.ptr(masks[N:]), N, H, W, 0.01, 0.5, st()),
              'flow_consistency')

    def visibility():
        check(lib.raft_flow_visibility_f32(_dev.ptr(flows), None, _dev.ptr(masks), _dev.ptr(share), N, H, W, 0.01, 0.5, 1, _dev.ptr(records),
                                           st()), 'flow_visibility')
    copies = {}

    def copy_of(nbytes):
        n = (nbytes // 8) // 4 * 4
        if n not in copies:
            copies[n] = (torch.randn((n,), device='cuda'), torch.empty((n,), device='cuda'))
        a, b = copies[n]
        return lambda: check(lib.raft_stream_copy_f32(_dev.ptr(a), _dev.ptr(b), n, st()), 'stream_copy')
    # (name, compulsory bytes or None, call)
    runs = [('range_map, N slices', px * (8 + 4), range_map),
            ('range_occlusion, both directions (2N slices of sums)', px * (8 + 8 + 1 + 1), range_occlusion),
            ('flow_consistency, both directions', px * (8 + 8 + 1 + 1), consistency),
            ('range_visibility, no mask (2N slices of sums)', 2 * px * (8 + 1), range_visibility),
            ('flow_visibility, no mask', 2 * px * (8 + 1), visibility),
            ('torch fill of the 2N slices of sums (the zeroing alone, for scale)', None, lambda: sums.zero_()),
            ('range_map, every vector of a frame on one pixel', None, lambda: range_map(one))]
    runs = [(k, nb, run, copy_of(nb) if nb else None) for k, nb, run in runs]
    for _ in range(3):
        for _, _, run, copy in runs:
            run()
            if copy:
                copy()
    torch.cuda.synchronize()
    t, tc = {k: [] for k, *_ in runs}, {k: [] for k, *_ in runs}
    for _ in range(rounds):
        for k, _, run, copy in runs:
            if copy:
                tc[k].append(_timed(copy, reps) * 1e3)
            t[k].append(_timed(run, reps) * 1e3)
    for k, nb, _, copy in runs:
        line = f'{k} at {shape}, us per call: {_fmt(t[k])}  min {min(t[k]):.1f}'
        if copy:
            r_run, r_copy = nb / min(t[k]) / 1e6, (nb // 32 * 32) / min(tc[k]) / 1e6
            line += (f'; {nb} compulsory bytes = {r_run:.2f} TB/s; stream copy of as many bytes {_fmt(tc[k])} us = {r_copy:.2f} TB/s: '
                     f'{r_run / r_copy:.2f} of the stream-copy rate')
        print(line, flush=True)
    ratio = lambda a, b: min(t[a]) / min(t[b])
    print(f'range_occlusion / flow_consistency = {ratio(runs[1][0], runs[2][0]):.2f}, range_visibility / flow_visibility = '
          f'{ratio(runs[3][0], runs[4][0]):.2f} at {shape}', flush=True)
    # what the measurement's flows are, and that the entries repeat
    range_visibility()
    first, s1 = masks.clone(), float(share)
    range_visibility()
    occ = image_ops.flow_consistency_launch(fwd, bwd)
    print(f'(range test: occluded share {s1:.4f}, repeat bit-identical: {bool(first.equal(masks)) and s1 == float(share)}; consistency test on the '
          f'same flows: {float(torch.cat(occ).float().mean()):.4f})', flush=True)


def kernels(reps=30, rounds=3):
    for shape in SHAPES:
        _kernels_at(shape, reps, rounds)


def step(repeats=5, reps=2):
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    rng = np.random.default_rng(0)
    i1, i2 = (torch.as_tensor(rng.uniform(0, 255, STEP + (3,)).astype(np.float32)).cuda() for _ in range(2))
    wts = wm.init_weights('raft', seed=0)

    def model(test):
        m = tf_raft_amd.RAFT(weights={k: v.copy() for k, v in wts.items()}, iters=ITERS, iters_pred=ITERS)
        m.compile(optimizer=training.AdamW(1e-4, 1e-4), clip_norm=1.0, loss=losses.PhotometricSequenceLoss(), bidirectional=True,
                  occlusion_test=test)
        return m
    models = {test: model(test) for test in ('range', 'consistency')}
    for m in models.values():
        for _ in range(2):
            m.train_step((i1, i2))
    torch.cuda.synchronize()
    t = {k: [] for k in models}
    for _ in range(repeats):
        for k, m in models.items():
            t[k].append(_timed(lambda: m.train_step((i1, i2)), reps))
    for k, v in t.items():
        print(f"train_step, occlusion_test='{k}', iters={ITERS} at {STEP}, ms per step: {' '.join(f'{x:.2f}' for x in v)}  mean {np.mean(v):.2f} "
              f'spread {max(v) - min(v):.2f}; occluded share reported: {float(models[k].flow_metrics["occluded"].result()):.4f} '
              f'(random weights: a number about the inputs, not about accuracy)', flush=True)
    print(f"range / consistency = {np.mean(t['range']) / np.mean(t['consistency']):.4f}", flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        sys.exit('range_occlusion_bench.py measures on a GPU; none is visible')
    if sys.argv[1] == 'kernels':
        kernels()
    else:
        step(*(int(v) for v in sys.argv[2:3]))

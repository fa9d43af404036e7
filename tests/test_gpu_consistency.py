"""Backward warp, forward-backward consistency check and the bidirectional step on the GPU: ``raft_warp_*`` and
``raft_flow_consistency_f32`` against the float64 restatements of tests/test_consistency.py, the public ops, and
``predict_step_bidirectional`` / ``predict_bidirectional`` on RAFT / SmallRAFT.

Bounds (u = 2^-24).  The warp: the sample position is the restatement's own float32 value, ``a`` and ``b`` are exact differences,
``1 - a`` and ``1 - b`` one rounding each, every term then passes at most three products and three additions and the weights sum
to at most ``1 + u`` -- fewer than 8 roundings of at most ``max|src|``:

    |got - want| <= 8 * 2^-24 * max|src|

The consistency check compares ``lhs = |f + s|^2`` with ``rhs = alpha * (|f|^2 + |s|^2) + beta``.  With M the largest flow component
of either input the sample carries at most ``8 u M`` per component, so ``lhs`` moves by at most ``2 * 4M * 8uM + 4u * 8M^2 = 96 u M^2``
and the right side by a few ``u M^2``: where the restatement's ``|lhs - rhs| <= 128 * 2^-24 * (1 + M)^2`` either answer passes, every
other pixel must agree, and the pixels so excluded are at most 0.5 % (the restatement alone excludes 0.05 %:
tests/test_consistency.py).  Zero and integer flows, the in-frame map and the analytic case are compared bit for bit.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, report
from test_consistency import (analytic_case, consistency_band, np_flow_consistency, np_warp, parity_flows, push_past_borders)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TOL = 1e-3            # tests/test_gpu_model.py TOL: max EPE against the oracle
# (H, W)        what it exercises
# (37, 53)      no dimension a multiple of a wave or a workgroup
# (64, 96)      the model's smallest size
# (3, 2051)     a row longer than one workgroup's 256 pixels, and few rows
# (100, 150)    several workgroups per image, rows that straddle them
SHAPES = [(37, 53), (64, 96), (3, 2051), (100, 150)]
IDS = [f'{h}x{w}' for h, w in SHAPES]


def _np(t):
    return t.detach().cpu().numpy()


def _src(rng, shape, kind):
    if kind == 'u8':
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    return (rng.normal(size=shape) * 60).astype(np.float32)


def _guarded(numel, dtype=torch.float32):
    """A destination of ``numel`` elements between two guard bands, and the check that only it was written."""
    fill = float('nan') if dtype == torch.float32 else 0xAB
    slab = torch.full((numel + 64,), fill, dtype=dtype, device='cuda')

    def untouched():
        edge = torch.cat([slab[:32], slab[32 + numel:]])
        return bool(torch.isnan(edge).all()) if dtype == torch.float32 else bool((edge == 0xAB).all())
    return slab[32:32 + numel], untouched


# ------------------------------------------------------------------ the warp
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_warp_by_zero_and_integer_flow_is_bitwise_a_shift(shape):
    """Zero flow returns the source; an integer flow returns the shifted source, with zeros and inside = 0 exactly where the shift
    leaves the frame.  C = 1 .. 4, N = 1 .. 3, both source types."""
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(21)
    H, W = shape
    for C_ in (1, 2, 3, 4):
        N = 1 + C_ % 3
        for kind in ('u8', 'f32'):
            x = _src(rng, (N, H, W, C_), kind)
            got, inside = image_ops.warp(x, np.zeros((N, H, W, 2), np.float32), return_inside=True)
            assert got.dtype == torch.float32 and inside.dtype == torch.uint8 and tuple(inside.shape) == (N, H, W)
            np.testing.assert_array_equal(_np(got), x.astype(np.float32))
            assert _np(inside).all()
            for dx, dy in ((3, -2), (-5, 1), (W, 0), (0, -H)):
                flow = np.empty((N, H, W, 2), np.float32)
                flow[..., 0], flow[..., 1] = dx, dy
                want, keep = np.zeros((N, H, W, C_), np.float32), np.zeros((N, H, W), np.uint8)
                ya, yb, xa, xb = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
                if ya < yb and xa < xb:
                    want[:, ya:yb, xa:xb] = x[:, ya + dy:yb + dy, xa + dx:xb + dx]
                    keep[:, ya:yb, xa:xb] = 1
                got, inside = image_ops.warp(x, flow, return_inside=True)
                np.testing.assert_array_equal(_np(got), want, err_msg=str((kind, C_, dx, dy)))
                np.testing.assert_array_equal(_np(inside), keep)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_warp_is_the_float64_rule(shape):
    """The bound of the module's docstring on smooth noise plus the moving square plus border-crossing vectors; the in-frame map
    bit for bit; zeros exactly out of frame; nothing written outside ``out``; (H, W, C) inputs; C = 5 (the kernel for any C)."""
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(22)
    H, W = shape
    worst = 0.0
    for C_ in (1, 2, 3, 4, 5):
        N = 1 + (C_ + 1) % 3
        fwd, _ = parity_flows(H, W, N, seed=100 + C_)
        for kind in ('u8', 'f32'):
            x = _src(rng, (N, H, W, C_), kind)
            want, keep = np_warp(x, fwd)
            bound = 8 * U * float(np.abs(x.astype(np.float64)).max())
            out, untouched = _guarded(N * H * W * C_)
            mask, mask_untouched = _guarded(N * H * W, torch.uint8)
            got = image_ops.warp_launch(torch.as_tensor(x).cuda(), torch.as_tensor(fwd).cuda(), out=out.view(N, H, W, C_), inside=mask.view(N, H, W))
            assert got.data_ptr() == out.data_ptr() and untouched() and mask_untouched()
            res = _np(got)
            assert not np.isnan(res).any(), 'an element of the destination was left unwritten'
            err = np.abs(res - want).max()
            worst = max(worst, err / bound)
            assert err <= bound, (kind, C_, N, err, bound)
            np.testing.assert_array_equal(_np(mask).reshape(N, H, W), keep.astype(np.uint8))
            assert not res[~keep].any()
            if H >= 12:
                assert (~keep).any() and keep.any()
            single, inside = image_ops.warp(x[0], fwd[0], return_inside=True)        # the public op from the host, (H, W, C)
            assert tuple(single.shape) == (H, W, C_) and tuple(inside.shape) == (H, W)
            np.testing.assert_array_equal(_np(single), res[0])
            np.testing.assert_array_equal(_np(inside), keep[0].astype(np.uint8))
    print(f'[consistency] warp {shape}: worst error / bound = {worst:.3f}')


# ------------------------------------------------------------------ the consistency check
def _compare_masks(got, flow_a, flow_b, alpha=0.01, beta=0.5):
    """One direction against the restatement: out of frame is 1, every pixel outside the band agrees; returns the excluded share."""
    occ, inside, margin = np_flow_consistency(flow_a, flow_b, alpha, beta)
    band = consistency_band(flow_a, flow_b)
    assert set(np.unique(got)) <= {0, 1}
    assert (got[~inside] == 1).all()
    with np.errstate(invalid='ignore'):
        free = inside & (np.abs(margin) <= band)
    np.testing.assert_array_equal(got[~free], occ[~free].astype(np.uint8))
    return float(free.mean())


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_flow_consistency_is_the_float64_rule(shape):
    from tf_raft_amd import image_ops
    H, W = shape
    worst = 0.0
    for N in (1, 2, 3):
        fwd, bwd = parity_flows(H, W, N, seed=200 + N)
        occ_f, occ_b = image_ops.flow_consistency(fwd, bwd)
        assert occ_f.dtype == occ_b.dtype == torch.uint8 and tuple(occ_f.shape) == tuple(occ_b.shape) == (N, H, W)
        for got, a, b in ((occ_f, fwd, bwd), (occ_b, bwd, fwd)):
            share = _compare_masks(_np(got), a, b)
            worst = max(worst, share)
            assert share <= 0.005, (N, share)
            if H >= 12:
                assert _np(got).any() and not _np(got).all()
        # other thresholds, (H, W, 2) inputs
        a_f, a_b = image_ops.flow_consistency(fwd[0], bwd[0], alpha=0.05, beta=0.125)
        assert tuple(a_f.shape) == (H, W)
        assert _compare_masks(_np(a_f)[None], fwd[:1], bwd[:1], 0.05, 0.125) <= 0.005
        assert _compare_masks(_np(a_b)[None], bwd[:1], fwd[:1], 0.05, 0.125) <= 0.005
    print(f'[consistency] check {shape}: largest share of pixels inside the band {100 * worst:.3f} %')


@pytest.mark.parametrize('H,W', [(9, 1), (9, 2), (1, 7)])
def test_frames_one_or_two_pixels_wide(H, W):
    """A row of one pixel has no neighbour to pair a tap with (the check then reads its taps one by one), in a row of two every
    paired read starts at pixel 0, and one row has no second row: vectors along the axis that has room, plus some that leave."""
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(25)
    fwd, bwd = ((rng.uniform(-1.5, 1.5, size=(2, H, W, 2)) * (H > 1, W > 1)[::-1]).astype(np.float32) for _ in range(2))
    occ_f, occ_b = image_ops.flow_consistency(fwd, bwd)
    for got, a, b in ((occ_f, fwd, bwd), (occ_b, bwd, fwd)):
        _compare_masks(_np(got), a, b)
        inside = np_flow_consistency(a, b)[1]
        assert inside.any() and (H * W == 1 or not inside.all())
    x = _src(rng, (2, H, W, 3), 'f32')
    want, keep = np_warp(x, fwd)
    got, inside = image_ops.warp(x, fwd, return_inside=True)
    assert np.abs(_np(got) - want).max() <= 8 * U * float(np.abs(x).max())
    np.testing.assert_array_equal(_np(inside), keep.astype(np.uint8))


@pytest.mark.parametrize('H,W', [(37, 53), (64, 96)])
def test_the_moving_square_bit_for_bit(H, W):
    """Integer vectors: no band.  Forward-occluded is the background the moved square covers, backward-occluded the background it
    uncovered, the warp of frame 2 by the forward flow is frame 1 off the occluded set; vectors pushed past each border are out
    of frame, zero and occluded, those that end ON a border are not; non-finite vectors mark their pixel."""
    from tf_raft_amd import image_ops
    f1, f2, fwd, bwd, sq1, sq2 = analytic_case(H, W, N=2)
    occ_f, occ_b = (_np(m) for m in image_ops.flow_consistency(fwd, bwd))
    for n in range(2):
        np.testing.assert_array_equal(occ_f[n], (sq2 & ~sq1).astype(np.uint8))
        np.testing.assert_array_equal(occ_b[n], (sq1 & ~sq2).astype(np.uint8))
    got, inside = image_ops.warp(f2, fwd, return_inside=True)
    assert _np(inside).all()
    keep = occ_f == 0
    np.testing.assert_array_equal(_np(got)[keep], f1[keep].astype(np.float32))
    np.testing.assert_array_equal(_np(got), np_warp(f2, fwd)[0].astype(np.float32))
    pushed, out = push_past_borders(fwd)
    got, inside = image_ops.warp(f2, pushed, return_inside=True)
    np.testing.assert_array_equal(_np(inside), (~out).astype(np.uint8))
    np.testing.assert_array_equal(_np(got), np_warp(f2, pushed)[0].astype(np.float32))
    assert not _np(got)[out].any()
    p_f, p_b = (_np(m) for m in image_ops.flow_consistency(pushed, bwd))
    np.testing.assert_array_equal(p_f, np_flow_consistency(pushed, bwd)[0].astype(np.uint8))
    np.testing.assert_array_equal(p_b, np_flow_consistency(bwd, pushed)[0].astype(np.uint8))
    assert p_f[out].all()
    bad = fwd.copy()
    bad[0, 5, 7], bad[0, 6, 7], bad[1, 7, 7] = (np.nan, 0), (0, np.inf), (-np.inf, np.nan)
    got, inside = image_ops.warp(f2, bad, return_inside=True)
    n_f, n_b = (_np(m) for m in image_ops.flow_consistency(bad, bwd))
    for n, y in ((0, 5), (0, 6), (1, 7)):
        assert _np(inside)[n, y, 7] == 0 and not _np(got)[n, y, 7].any() and n_f[n, y, 7] == 1
    np.testing.assert_array_equal(n_f, np_flow_consistency(bad, bwd)[0].astype(np.uint8))
    np.testing.assert_array_equal(n_b, np_flow_consistency(bwd, bad)[0].astype(np.uint8))
    assert n_b[0, 5, 7] == 1                                       # a finite vector whose sample touches a NaN


def test_one_launch_is_two_launches_a_sample_is_the_sample_alone_and_calls_repeat():
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(23)
    for (H, W) in ((37, 53), (100, 150)):
        fwd, bwd = (torch.as_tensor(f).cuda() for f in parity_flows(H, W, 3, seed=300))
        both_f, both_b = image_ops.flow_consistency_launch(fwd, bwd)
        only_f, none = image_ops.flow_consistency_launch(fwd, bwd, both=False)
        only_b, _ = image_ops.flow_consistency_launch(bwd, fwd, both=False)
        assert none is None and torch.equal(both_f, only_f) and torch.equal(both_b, only_b)
        again = image_ops.flow_consistency_launch(fwd, bwd)
        assert torch.equal(again[0], both_f) and torch.equal(again[1], both_b)
        x = torch.as_tensor(_src(rng, (3, H, W, 3), 'u8')).cuda()
        whole, inside = image_ops.warp(x, fwd, return_inside=True)
        assert torch.equal(image_ops.warp(x, fwd).as_subclass(torch.Tensor), whole.as_subclass(torch.Tensor))
        for n in range(3):
            one_f, one_b = image_ops.flow_consistency(fwd[n], bwd[n])
            assert torch.equal(one_f.as_subclass(torch.Tensor), both_f[n]) and torch.equal(one_b.as_subclass(torch.Tensor), both_b[n])
            w1, i1 = image_ops.warp(x[n:n + 1], fwd[n:n + 1], return_inside=True)
            assert torch.equal(w1.as_subclass(torch.Tensor)[0], whole.as_subclass(torch.Tensor)[n])
            assert torch.equal(i1.as_subclass(torch.Tensor)[0], inside.as_subclass(torch.Tensor)[n])


def test_the_ops_follow_the_current_stream_and_take_or_reject_views_as_the_tile_ops_do():
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(24)
    H, W = 40, 70
    fwd_h, bwd_h = parity_flows(H, W, 2, seed=400)
    x_h = _src(rng, (2, H, W, 3), 'f32')
    fwd, bwd, x = (torch.as_tensor(a).cuda() for a in (fwd_h, bwd_h, x_h))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        f2, b2, x2 = fwd * 2, bwd * 2, x * 2                              # produced on `side`: only stream order makes the ops see them
        warped = image_ops.warp(x2, f2)
        occ_f, occ_b = image_ops.flow_consistency(f2, b2)
    side.synchronize()
    want, _ = np_warp(x_h * 2, fwd_h * 2)
    assert np.abs(_np(warped) - want).max() <= 8 * U * float(np.abs(x_h * 2).max())
    assert _compare_masks(_np(occ_f), fwd_h * 2, bwd_h * 2) <= 0.005 and _compare_masks(_np(occ_b), bwd_h * 2, fwd_h * 2) <= 0.005
    # views: a non-contiguous or offset input is made contiguous (as by every op here), with the same result
    wide = torch.zeros((2, H, W, 5), device='cuda')
    wide[..., 1:4] = x
    base = _np(image_ops.warp(x, fwd))
    np.testing.assert_array_equal(_np(image_ops.warp(wide[..., 1:4], fwd)), base)
    fl = torch.zeros((2, H, W, 3), device='cuda')
    fl[..., 1:] = fwd
    np.testing.assert_array_equal(_np(image_ops.warp(x, fl[..., 1:])), base)
    np.testing.assert_array_equal(_np(image_ops.flow_consistency(fl[..., 1:], bwd)[0]), _np(image_ops.flow_consistency(fwd, bwd)[0]))
    np.testing.assert_array_equal(_np(image_ops.warp(x[1], fwd[1])), base[1])                   # an offset view, 8-byte aligned
    # a flow is read as whole vectors: 4 bytes off is refused by the launch forms, before anything is written
    slab = torch.zeros((2 * H * W * 2 + 2,), device='cuda')
    off = slab[1:1 + 2 * H * W * 2].view(2, H, W, 2)
    out = torch.full((2, H, W, 3), float('nan'), device='cuda')
    with pytest.raises(ValueError, match='aligned'):
        image_ops.warp_launch(x, off, out=out)
    assert torch.isnan(out).all()
    with pytest.raises(ValueError, match='aligned'):
        image_ops.flow_consistency_launch(off, bwd)
    with pytest.raises(ValueError, match='aligned'):
        image_ops.flow_consistency_launch(fwd, off)
    # ... and so is a strided tensor (the public ops make it contiguous first)
    with pytest.raises(ValueError, match='contiguous'):
        image_ops.warp_launch(wide[..., 1:4], fwd, out=out)
    with pytest.raises(ValueError, match='contiguous'):
        image_ops.warp_launch(x, fl[..., 1:], out=out)
    with pytest.raises(ValueError, match='contiguous'):
        image_ops.flow_consistency_launch(fl[..., 1:], bwd)
    assert torch.isnan(out).all()
    # a refused destination stays untouched
    for make in (lambda: torch.full((2, H, W, 2), float('nan'), device='cuda'),
                 lambda: torch.full((2, H, W, 4), float('nan'), device='cuda')[..., :3],      # not contiguous
                 lambda: torch.full((2, H, W, 3), float('nan'), device='cuda', dtype=torch.float64),
                 lambda: torch.full((1, H, W, 3), float('nan'), device='cuda')):
        out = make()
        with pytest.raises(ValueError, match='out'):
            image_ops.warp(x, fwd, out=out)
        assert torch.isnan(out).all()
    out = torch.full((2, H, W, 3), float('nan'), device='cuda')
    assert image_ops.warp(x, fwd, out=out).data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(_np(out), base)
    # shapes and types
    with pytest.raises(ValueError):
        image_ops.warp(x, fwd[:1])
    with pytest.raises(ValueError):
        image_ops.warp(x, fwd[..., :1])
    with pytest.raises(ValueError):
        image_ops.warp(x[0, 0], fwd[0, 0])
    with pytest.raises(ValueError):
        image_ops.warp(torch.zeros((0, H, W, 3)), torch.zeros((0, H, W, 2)))
    with pytest.raises(TypeError):
        image_ops.warp(x.to(torch.float16), fwd)
    with pytest.raises(TypeError):
        image_ops.warp(x, fwd.to(torch.float16))
    with pytest.raises(ValueError):
        image_ops.flow_consistency(fwd, bwd[:1])
    with pytest.raises(ValueError):
        image_ops.flow_consistency(x, x)                                   # a flow has two channels
    with pytest.raises(TypeError):
        image_ops.flow_consistency(fwd.to(torch.float16), bwd.to(torch.float16))
    with pytest.raises(ValueError):
        image_ops.flow_consistency(torch.zeros((0, H, W, 2)), torch.zeros((0, H, W, 2)))
    with pytest.raises(ValueError, match='beta'):
        image_ops.flow_consistency(fwd, bwd, beta=-1.0)
    assert image_ops.warp(np.zeros((4, 5, 1), np.float64), np.zeros((4, 5, 2))).dtype == torch.float32      # float64 narrows


# ------------------------------------------------------------------ the model
def _cls(variant):
    import tf_raft_amd
    return tf_raft_amd.RAFT if variant == 'raft' else tf_raft_amd.SmallRAFT


def _frames(seed, B, H, W, dtype):
    rng = np.random.default_rng(seed)
    return tuple(_src(rng, (B, H, W, 3), 'u8') if dtype == np.uint8 else rng.uniform(0, 255, size=(B, H, W, 3)).astype(np.float32)
                 for _ in range(2))


def _plain(t):
    return t.as_subclass(torch.Tensor)


def _check_result(res, N, H, W):
    from tf_raft_amd.model import BidirectionalFlow
    assert isinstance(res, BidirectionalFlow)
    for f in (res.forward, res.backward):
        assert tuple(f.shape) == (N, H, W, 2) and f.dtype == torch.float32 and f.is_cuda
    for m in (res.occluded_forward, res.occluded_backward):
        assert tuple(m.shape) == (N, H, W) and m.dtype == torch.uint8 and m.is_cuda


@pytest.mark.parametrize('variant,H,W,seed', [('raft', 64, 96, 0), ('small', 64, 96, 0), ('raft', 128, 160, 1), ('raft', 72, 104, 2)])
def test_bidirectional_step_against_the_oracle(variant, H, W, seed):
    """Both returned flows within the project's bound of the oracle's final prediction of the matching direction (the oracle runs
    on the doubled batch [i1 | i2], [i2 | i1]), only where tests/golden/conditioning_bidirectional.json shows the oracle itself
    well conditioned; the difference from the doubled-batch ``predict_step`` is printed."""
    from oracle.losses import max_epe
    sys.path.insert(0, GOLDEN)
    from make_conditioning import case_inputs
    from make_conditioning_bidirectional import B, ITERS, case_key, oracle_both
    with open(os.path.join(GOLDEN, 'conditioning_bidirectional.json')) as f:
        cond = json.load(f)[case_key(variant, H, W, seed)]
    assert max(cond['epe32v64']) <= 2e-4, 'fixture: the oracle itself is ill conditioned on this case'
    i1, i2, wts = case_inputs(variant, H, W, seed, 'conditioned', B=B)
    want = oracle_both(variant, wts, i1, i2)[-1]
    model = _cls(variant)(weights=wts, iters_pred=ITERS)
    res = model.predict_step_bidirectional((i1, i2))
    _check_result(res, B, H, W)
    err_f, err_b = max_epe(_np(res.forward), want[:B]), max_epe(_np(res.backward), want[B:])
    doubled = _np(model.predict_step((np.concatenate([i1, i2]), np.concatenate([i2, i1]))))
    report(f'bidirectional {variant} {H}x{W}', forward_epe=err_f, backward_epe=err_b, oracle32_vs_64_worst=max(cond['epe32v64']),
           vs_doubled_batch=max(max_epe(_np(res.forward), doubled[:B]), max_epe(_np(res.backward), doubled[B:])),
           final_max_abs_flow=cond['max_abs_flow'][-1])
    assert err_f <= TOL and err_b <= TOL, (err_f, err_b)
    assert max_epe(_np(res.forward), _np(res.backward)) > 0                # two directions, not one twice


@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_masks_are_the_public_op_on_the_returned_flows_and_predict_is_the_steps(variant):
    from tf_raft_amd import image_ops
    from tf_raft_amd import weights as wm
    from tf_raft_amd.model import BidirectionalFlow
    wts = wm.init_weights(variant, seed=6, perturb=True)
    model = _cls(variant)(weights=wts, iters_pred=3)
    B, H, W = 3, 64, 96
    i1, i2 = _frames(60, B, H, W, np.float32)
    res = model.predict_step_bidirectional((i1, i2))
    _check_result(res, B, H, W)
    for alpha, beta, r in ((0.01, 0.5, res), (0.05, 0.125, model.predict_step_bidirectional((i1, i2), alpha=0.05, beta=0.125))):
        occ_f, occ_b = image_ops.flow_consistency(r.forward, r.backward, alpha, beta)
        assert torch.equal(_plain(r.occluded_forward), _plain(occ_f)) and torch.equal(_plain(r.occluded_backward), _plain(occ_b))
        assert torch.equal(_plain(r.forward), _plain(res.forward)) and torch.equal(_plain(r.backward), _plain(res.backward))
    with pytest.raises(ValueError, match='alpha'):
        model.predict_step_bidirectional((i1, i2), alpha=-1.0)
    # predict_bidirectional(batch_size=1): the concatenated single steps, as host arrays
    singles = [model.predict_step_bidirectional((i1[k:k + 1], i2[k:k + 1])) for k in range(B)]
    got = model.predict_bidirectional([i1, i2], batch_size=1)
    assert isinstance(got, BidirectionalFlow)
    for name in BidirectionalFlow._fields:
        arr = getattr(got, name)
        assert isinstance(arr, np.ndarray) and arr.shape == ((B, H, W, 2) if 'occluded' not in name else (B, H, W))
        assert arr.dtype == (np.uint8 if 'occluded' in name else np.float32)
        np.testing.assert_array_equal(arr, np.concatenate([_np(getattr(s, name)) for s in singles]))
    assert model.predict_bidirectional([i1, i2], batch_size=2, steps=1).forward.shape == (2, H, W, 2)
    with pytest.raises(ValueError):
        model.predict_bidirectional(iter(()))


OVERLAP = (16, 32)


def _by_hand(plain, i1, i2, fit):
    """The public op in, a model without the option, the public op back, then the public consistency check."""
    from tf_raft_amd import image_ops
    H, W = i1.shape[1:3]
    if fit == 'crop_or_pad':
        a, b = (image_ops.resize_with_crop_or_pad(x, 64, 96, dtype=torch.float32) for x in (i1, i2))
        back = lambda f: image_ops.resize_with_crop_or_pad(f, H, W)
    elif fit == 'resize':
        a, b = (image_ops.resize(x, 64, 96, antialias=True) for x in (i1, i2))
        back = lambda f: image_ops.resize_flow(f, H, W, antialias=True)
    else:
        a, b = (image_ops.tile_gather(x, 64, 96, overlap=OVERLAP) for x in (i1, i2))
        back = lambda f: image_ops.tile_blend(f, H, W, overlap=OVERLAP)
    res = plain.predict_step_bidirectional((a, b))
    fwd, bwd = back(res.forward), back(res.backward)
    return (fwd, bwd) + tuple(image_ops.flow_consistency(fwd, bwd))


@pytest.mark.parametrize('fit', ['crop_or_pad', 'resize', 'tile'])
@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_a_frame_size_route_is_bitwise_the_route_done_by_hand(variant, fit):
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=7, perturb=True)
    kw = {'tile_overlap': OVERLAP} if fit == 'tile' else {}
    model = _cls(variant)(weights=wts, iters_pred=3, target_size=(64, 96), fit=fit, **kw)
    plain = _cls(variant)(weights=wts, iters_pred=3)
    B, H, W = 2, 100, 150
    i1, i2 = _frames(70, B, H, W, np.uint8)
    res = model.predict_step_bidirectional((i1, i2))
    _check_result(res, B, H, W)
    for got, want in zip(res, _by_hand(plain, i1, i2, fit)):
        assert torch.equal(_plain(got), _plain(want))
    assert _np(res.forward).any() and _np(res.occluded_forward).any()


@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_the_step_joins_a_pipelined_model(variant):
    """After three pipelined ``predict_step`` calls (loops in flight on the lanes) the step equals a fresh serial model's."""
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=8, perturb=True)
    piped = _cls(variant)(weights=wts, iters_pred=3, pipeline=True)
    serial = _cls(variant)(weights=wts, iters_pred=3)
    i1, i2 = _frames(80, 2, 64, 96, np.float32)
    pending = [piped.predict_step((i1, i2)) for _ in range(3)]
    got = piped.predict_step_bidirectional((i1, i2))
    want = serial.predict_step_bidirectional((i1, i2))
    for g, w_ in zip(got, want):
        assert torch.equal(_plain(g), _plain(w_))
    np.testing.assert_array_equal(_np(piped.predict_step((i1, i2))), _np(pending[0]))      # and pipelined calls go on as before

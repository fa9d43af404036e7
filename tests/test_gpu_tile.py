"""Tiled inference on the GPU: the tile gather and the weighted blend against the NumPy / float64 restatements of
tests/test_tile.py, the public ops, and ``fit='tile'`` on RAFT / SmallRAFT through every inference entry point.  Tiles are
(64, 96) throughout.

The gather is a copy: it is compared bit for bit.  The blend's bound is the one tests/test_gpu_resize.py derives for the same
arithmetic.  An output is ``sum_kx b[kx] * sum_ky a[ky] * x[ky, kx]`` in float32 with ``ty x tx`` tiles at most; the weights are
non-negative, sum to 1 per axis in float64 and are each rounded ONCE to float32 (relative error <= u = 2^-24), the tile values are
exact.  To first order in u every term carries its two weight roundings, its two products and the additions it passes through --
at most ``ty + tx + 2`` roundings, fewer than ``ty * tx + 2`` whenever there is more than one tile -- and the weights summing to 1
turn the sum of |terms| into at most ``max|x|``; with the resize's allowance of two more roundings kept (the channel factor is 1
here), as the issue states the bound:

    |got - want| <= (ty * tx + 4) * 2^-24 * max|x|

with ``ty``, ``tx`` the largest number of tiles over one coordinate of the axis (1 .. 3 here).  Where a single tile covers the frame
the weight is exactly 1.0 and the blend is compared bit for bit, as is the model's route: it runs the same kernels on the same bytes.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, report
from test_tile import np_max_cover, np_origins, np_tile_blend, np_tile_gather

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TOL = 1e-3            # tests/test_gpu_model.py TOL: max EPE against the oracle
TILE = (64, 96)
# (H, W)        what it exercises
# (100, 150)    2 x 2 tiles
# (60, 200)     a padded axis and three tiles
# (170, 96)     one axis of the tile's own length; three tiles over one row at overlap 32 (tests/test_tile.py)
# (65, 97)      two tiles one pixel apart per axis
# (40, 70)      a single padded tile
# (64, 96)      no launch
FRAMES = [(100, 150), (60, 200), (170, 96), (65, 97), (40, 70), (64, 96)]
OVERLAPS = (0, 16, 32)


def _np(t):
    return t.detach().cpu().numpy()


def _grid(H, W, overlap):
    return np_origins(H, TILE[0], overlap), np_origins(W, TILE[1], overlap)


def _bound(H, W, overlap, maxabs):
    oy, ox = _grid(H, W, overlap)
    return (np_max_cover(H, TILE[0], oy) * np_max_cover(W, TILE[1], ox) + 4) * U * maxabs


def _data(rng, shape, kind):
    if kind == 'u8':
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    return rng.uniform(0, 255, size=shape).astype(np.float32)


def _skewed(x, skew):
    """``x`` on the device, ``skew`` elements past a 16-byte boundary, with NaN (0xAB for bytes) around it."""
    t = torch.as_tensor(x)
    slab = torch.full((t.numel() + 64,), float('nan') if t.dtype == torch.float32 else 0xAB, dtype=t.dtype, device='cuda')
    slab[32 + skew:32 + skew + t.numel()] = t.reshape(-1).cuda()
    return slab[32 + skew:32 + skew + t.numel()].view(t.shape)


def _run(op, x, shape, src_skew=0, dst_skew=0, **kw):
    """One launch into a NaN slab: the result, after checking that the guard bands on both sides are still NaN."""
    n = int(np.prod(shape))
    slab = torch.full((n + 64,), float('nan'), device='cuda')
    out = slab[32 + dst_skew:32 + dst_skew + n].view(shape)
    src = _skewed(x, src_skew)
    assert src.data_ptr() % 16 == (src_skew * src.element_size()) % 16 and out.data_ptr() % 16 == (4 * dst_skew) % 16
    got = op(src, out=out, **kw)
    assert got.data_ptr() == out.data_ptr() and got.dtype == torch.float32 and tuple(got.shape) == tuple(shape)
    assert torch.isnan(slab[:32 + dst_skew]).all() and torch.isnan(slab[32 + dst_skew + n:]).all(), 'written outside the destination'
    res = _np(out)
    assert not np.isnan(res).any(), 'an element of the destination was left unwritten'
    return res


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('frame', FRAMES, ids=[f'{h}x{w}' for h, w in FRAMES])
def test_tile_gather_is_numpy_slicing_with_zero_fill(frame):
    """Bit for bit, at every overlap, 1 / 2 / 3 channels, one and three frames, both source types, with source and destination
    1 and 3 elements off 16 bytes; and the rule's own origins are the restated ones."""
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(11)
    H, W = frame
    for overlap in OVERLAPS:
        oy, ox = _grid(H, W, overlap)
        assert (image_ops.tile_origins(H, TILE[0], overlap), image_ops.tile_origins(W, TILE[1], overlap)) == (oy, ox)
        K = len(oy) * len(ox)
        for C_ in (1, 2, 3):
            for N in (1, 3):
                for kind in ('u8', 'f32'):
                    x = _data(rng, (N, H, W, C_), kind)
                    want = np_tile_gather(x, *TILE, oy, ox)
                    assert want.shape == (N * K,) + TILE + (C_,)
                    runs = [(0, 0)] + ([(1, 1), (3, 3), (0, 1), (3, 0)] if N == 1 else [])
                    for src_skew, dst_skew in runs:
                        got = _run(image_ops.tile_gather, x, want.shape, src_skew, dst_skew, height=TILE[0], width=TILE[1], overlap=overlap)
                        np.testing.assert_array_equal(got, want, err_msg=str((kind, x.shape, overlap, src_skew, dst_skew)))
                    # the public op from the host, (N, H, W, C) and (H, W, C)
                    np.testing.assert_array_equal(_np(image_ops.tile_gather(x, *TILE, overlap=overlap)), want)
                    np.testing.assert_array_equal(_np(image_ops.tile_gather(x[0], *TILE, overlap=overlap)), want[:K])


@pytest.mark.parametrize('frame', FRAMES, ids=[f'{h}x{w}' for h, w in FRAMES])
def test_tile_blend_is_the_float64_rule(frame):
    """The bound of the module's docstring against the non-separable float64 restatement, at every overlap, over leading axes
    (), (3,) and (2, 3), tiles and destination 16-byte aligned and 8 bytes off; constant tiles blend to the constant and tiles cut
    from an affine field of the frame's coordinates blend back to it (a wrong origin or weight cannot pass either)."""
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(12)
    H, W = frame
    worst = 0.0
    for overlap in OVERLAPS:
        oy, ox = _grid(H, W, overlap)
        K = len(oy) * len(ox)
        for lead, N in (((), 2), ((3,), 1), ((2, 3), 2)):
            t = (rng.normal(size=lead + (N * K,) + TILE + (2,)) * 40).astype(np.float32)
            want = np_tile_blend(t, H, W, oy, ox)
            bound = _bound(H, W, overlap, float(np.abs(t).max()))
            for skew in (0, 2):
                got = _run(image_ops.tile_blend, t, want.shape, skew, skew, H=H, W=W, overlap=overlap)
                err = np.abs(got - want).max()
                worst = max(worst, err / bound)
                assert err <= bound, ((H, W), overlap, lead, skew, err, bound)
            assert np.abs(_np(image_ops.tile_blend(t, H, W, overlap=overlap)) - want).max() <= bound        # from the host
        # partition of unity
        const = np.empty((K,) + TILE + (2,), np.float32)
        const[..., 0], const[..., 1] = 37.25, -113.5
        got = _run(image_ops.tile_blend, const, (1, H, W, 2), H=H, W=W, overlap=overlap)
        err = max(np.abs(got[..., 0] - 37.25).max(), np.abs(got[..., 1] + 113.5).max())
        worst = max(worst, err / _bound(H, W, overlap, 113.5))
        assert err <= _bound(H, W, overlap, 113.5), ('constant', (H, W), overlap, err)
        # an affine field of the frame's coordinates (exact in float32), cut into tiles by the origins
        def field(y, x):
            return np.stack([0.5 * y - 0.25 * x + 3.0, -0.125 * y + 0.75 * x - 7.0], axis=-1)
        ty, tx = np.meshgrid(np.arange(TILE[0], dtype=np.float64), np.arange(TILE[1], dtype=np.float64), indexing='ij')
        cut = np.stack([field(y0 + ty, x0 + tx) for y0 in oy for x0 in ox]).astype(np.float32)
        fy, fx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
        got = _run(image_ops.tile_blend, cut, (1, H, W, 2), H=H, W=W, overlap=overlap)
        err = np.abs(got[0] - field(fy, fx)).max()
        bound = _bound(H, W, overlap, float(np.abs(cut).max()))
        worst = max(worst, err / bound)
        assert err <= bound, ('affine', (H, W), overlap, err, bound)
    print(f'[tile] blend {frame}: worst error / bound = {worst:.3f}')


def test_a_single_padded_tile_is_crop_or_pad_both_ways_bit_for_bit():
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(13)
    for (H, W) in ((40, 70), (63, 96), (64, 95), (1, 1)):
        for kind in ('u8', 'f32'):
            x = torch.as_tensor(_data(rng, (3, H, W, 3), kind)).cuda()
            for overlap in OVERLAPS:
                got = image_ops.tile_gather(x, *TILE, overlap=overlap)
                assert torch.equal(got.as_subclass(torch.Tensor), image_ops.resize_with_crop_or_pad(x, *TILE, dtype=torch.float32).as_subclass(torch.Tensor))
        t = torch.as_tensor((rng.normal(size=(3,) + TILE + (2,)) * 40).astype(np.float32)).cuda()
        back = image_ops.tile_blend(t, H, W, overlap=16)
        assert tuple(back.shape) == (3, H, W, 2)
        assert torch.equal(back.as_subclass(torch.Tensor), image_ops.resize_with_crop_or_pad(t, H, W).as_subclass(torch.Tensor))


def test_a_sample_of_a_batch_is_bitwise_the_sample_alone_and_calls_repeat():
    from tf_raft_amd import image_ops
    rng = np.random.default_rng(14)
    for (H, W), overlap, kind in (((100, 150), 16, 'u8'), ((60, 200), 32, 'f32'), ((170, 96), 32, 'f32')):
        oy, ox = _grid(H, W, overlap)
        K = len(oy) * len(ox)
        x = torch.as_tensor(_data(rng, (4, H, W, 3), kind)).cuda()
        whole = _np(image_ops.tile_gather(x, *TILE, overlap=overlap))
        np.testing.assert_array_equal(_np(image_ops.tile_gather(x, *TILE, overlap=overlap)), whole)
        t = torch.as_tensor((rng.normal(size=(2, 4 * K) + TILE + (2,)) * 40).astype(np.float32)).cuda()
        blended = _np(image_ops.tile_blend(t, H, W, overlap=overlap))
        np.testing.assert_array_equal(_np(image_ops.tile_blend(t, H, W, overlap=overlap)), blended)
        for n in range(4):
            np.testing.assert_array_equal(_np(image_ops.tile_gather(x[n:n + 1], *TILE, overlap=overlap)), whole[n * K:(n + 1) * K])
            np.testing.assert_array_equal(_np(image_ops.tile_gather(x[n], *TILE, overlap=overlap)), whole[n * K:(n + 1) * K])
            for m in range(2):
                np.testing.assert_array_equal(_np(image_ops.tile_blend(t[m, n * K:(n + 1) * K], H, W, overlap=overlap))[0], blended[m, n])


def test_element_offsets_beyond_two_to_the_31():
    """111900 predictions of 64 x 150 frames (two tiles each) are 2^31 + 996352 destination elements: the last one, whose offsets
    do not fit 32 bits, is bitwise the same prediction blended alone, and nothing is written behind it."""
    from tf_raft_amd import image_ops
    M, H, W, overlap = 111900, 64, 150, 16
    per = H * W * 2
    assert M * per > 2 ** 31 and _grid(H, W, overlap) == ([0], [0, 54])
    tiles = torch.empty((M, 2) + TILE + (2,), device='cuda').normal_()
    slab = torch.empty((M * per + 64,), device='cuda')
    slab[-64:] = float('nan')
    slab[(M - 1) * per:M * per] = float('nan')
    out = slab[:M * per].view(M, 1, H, W, 2)
    image_ops.tile_blend(tiles, H, W, overlap=overlap, out=out)
    for k in (0, 55555, M - 1):
        assert torch.equal(out[k], image_ops.tile_blend(tiles[k], H, W, overlap=overlap).as_subclass(torch.Tensor)), k
    assert not torch.isnan(out[M - 1]).any() and torch.isnan(slab[-64:]).all()


def test_equal_sizes_launch_nothing():
    from tf_raft_amd import image_ops
    x = torch.rand((2,) + TILE + (3,), device='cuda')
    assert image_ops.tile_gather(x, *TILE, overlap=16).data_ptr() == x.data_ptr()
    assert image_ops.tile_gather(x[0], *TILE, overlap=0).data_ptr() == x[0].data_ptr()
    f = torch.rand((3, 2) + TILE + (2,), device='cuda')
    assert image_ops.tile_blend(f, *TILE, overlap=32).data_ptr() == f.data_ptr()
    u = torch.randint(0, 256, (2,) + TILE + (3,), dtype=torch.uint8, device='cuda')
    same = image_ops.tile_gather(u, *TILE, overlap=16)
    assert same.dtype == torch.float32 and torch.equal(same.as_subclass(torch.Tensor), u.to(torch.float32))


def test_tile_ops_follow_the_current_stream_and_reject_what_they_cannot_take():
    from tf_raft_amd import image_ops
    H, W, overlap = 101, 151, 24                                          # (tables of sizes no other test uses: uploaded on `side`)
    oy, ox = _grid(H, W, overlap)
    side = torch.cuda.Stream()
    x = torch.arange(2 * H * W * 2, dtype=torch.float32, device='cuda').view(2, H, W, 2) % 251 + 1
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        y = x * 2                                                       # produced on `side`: only stream order makes the ops see it
        tiles = image_ops.tile_gather(y, *TILE, overlap=overlap)
        back = image_ops.tile_blend(tiles, H, W, overlap=overlap)
    side.synchronize()
    want = np_tile_gather(_np(x) * 2, *TILE, oy, ox)
    np.testing.assert_array_equal(_np(tiles), want)
    assert np.abs(_np(back) - _np(x) * 2.0).max() <= _bound(H, W, overlap, 502.0)     # tiles cut from a field blend back to it
    back2 = image_ops.tile_blend(tiles, H, W, overlap=overlap)          # the cached tables, now from another stream than their own
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(back2), _np(back))

    K = len(oy) * len(ox)
    t = tiles.as_subclass(torch.Tensor)
    with pytest.raises(TypeError):
        image_ops.tile_gather(torch.zeros((1, 100, 150, 1), dtype=torch.int32), *TILE, overlap=16)
    with pytest.raises(TypeError):
        image_ops.tile_gather(torch.zeros((1, 100, 150, 1), dtype=torch.float16, device='cuda'), *TILE, overlap=16)
    with pytest.raises(TypeError):
        image_ops.tile_blend(torch.zeros((4,) + TILE + (2,), dtype=torch.uint8), 100, 150, overlap=16)
    with pytest.raises(ValueError):
        image_ops.tile_gather(x[0, 0], *TILE, overlap=16)                 # rank
    with pytest.raises(ValueError):
        image_ops.tile_gather(x[None], *TILE, overlap=16)
    with pytest.raises(ValueError):
        image_ops.tile_blend(t[0, 0], H, W, overlap=overlap)
    with pytest.raises(ValueError):
        image_ops.tile_gather(torch.zeros((0, 100, 150, 3)), *TILE, overlap=16)
    with pytest.raises(ValueError):
        image_ops.tile_blend(torch.zeros((0,) + TILE + (2,)), 100, 150, overlap=16)
    with pytest.raises(ValueError):
        image_ops.tile_blend(torch.zeros((4,) + TILE + (3,)), 100, 150, overlap=16)       # a flow has two channels
    with pytest.raises(ValueError):
        image_ops.tile_blend(t[:K + 1], H, W, overlap=overlap)            # no whole number of frames
    for bad in (33, (16, 49), -1):
        with pytest.raises(ValueError, match='overlap'):
            image_ops.tile_gather(x, *TILE, overlap=bad)
        with pytest.raises(ValueError, match='overlap'):
            image_ops.tile_blend(t, H, W, overlap=bad)
    # a refused destination stays untouched
    for make in (lambda: torch.full((2 * K,) + TILE + (1,), float('nan'), device='cuda'),
                 lambda: torch.full((2 * K,) + TILE + (4,), float('nan'), device='cuda')[..., :2],      # not contiguous
                 lambda: torch.full((2 * K,) + TILE + (2,), float('nan'), device='cuda', dtype=torch.float64),
                 lambda: torch.full((K,) + TILE + (2,), float('nan'), device='cuda')):
        out = make()
        with pytest.raises(ValueError, match='out'):
            image_ops.tile_gather(x, *TILE, overlap=overlap, out=out)
        assert torch.isnan(out).all()
    for make in (lambda: torch.full((2, H, W, 1), float('nan'), device='cuda'),
                 lambda: torch.full((2, H, W, 4), float('nan'), device='cuda')[..., :2],
                 lambda: torch.full((2, H, W, 2), float('nan'), device='cuda', dtype=torch.float64),
                 lambda: torch.full((1, H, W, 2), float('nan'), device='cuda'),
                 lambda: torch.full((2, H, W + 1, 2), float('nan'), device='cuda')):
        out = make()
        with pytest.raises(ValueError, match='out'):
            image_ops.tile_blend(t, H, W, overlap=overlap, out=out)
        assert torch.isnan(out).all()
    # a flow is read and written as whole vectors: 4 bytes off is refused, on either side
    slab = torch.full((2 * H * W * 2 + 4,), float('nan'), device='cuda')
    with pytest.raises(ValueError, match='aligned'):
        image_ops.tile_blend(t, H, W, overlap=overlap, out=slab[1:1 + 2 * H * W * 2].view(2, H, W, 2))
    with pytest.raises(ValueError, match='aligned'):
        image_ops.tile_blend(_skewed(_np(t), 1), H, W, overlap=overlap, out=slab[:2 * H * W * 2].view(2, H, W, 2))
    assert torch.isnan(slab).all()
    with pytest.raises(ValueError, match='per axis'):
        image_ops.tile_gather(torch.zeros((1, 64, 64 * 40, 1), device='cuda'), 64, 64, overlap=0)


# ------------------------------------------------------------------ the model option
def _cls(variant):
    import tf_raft_amd
    return tf_raft_amd.RAFT if variant == 'raft' else tf_raft_amd.SmallRAFT


def _frames(seed, B, H, W, dtype):
    rng = np.random.default_rng(seed)
    return tuple(_data(rng, (B, H, W, 3), 'u8' if dtype == np.uint8 else 'f32') for _ in range(2))


def _route(plain, i1, i2, overlap, entry='call'):
    """image_ops.tile_gather -> a model WITHOUT the option on the N * K tiles -> image_ops.tile_blend: every prediction (or the last)."""
    from tf_raft_amd import image_ops
    H, W = i1.shape[1:3]
    t1, t2 = (image_ops.tile_gather(x, *TILE, overlap=overlap) for x in (i1, i2))
    if entry == 'call':
        preds = torch.stack([p.as_subclass(torch.Tensor) for p in plain([t1, t2])])
        return [_np(p) for p in image_ops.tile_blend(preds, H, W, overlap=overlap)]
    return _np(image_ops.tile_blend(plain.predict_step((t1, t2)), H, W, overlap=overlap))


OVERLAP = (16, 32)
CASES = [(np.uint8, (2, 100, 150)), (np.float32, (2, 60, 200))]


@pytest.mark.parametrize('pipeline', [False, True], ids=['serial', 'pipelined'])
@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_fit_tile_is_bitwise_gather_model_blend(variant, pipeline):
    """__call__, predict_step, predict(batch_size=1) and predict(output='image') with ``target_size=(64, 96), fit='tile'`` on uint8
    and float frames."""
    from tf_raft_amd import image_ops
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=4, perturb=True)
    model = _cls(variant)(weights=wts, iters_pred=3, target_size=TILE, fit='tile', tile_overlap=OVERLAP, pipeline=pipeline)
    assert model.fit == 'tile' and model.tile_overlap == OVERLAP
    plain = _cls(variant)(weights=wts, iters_pred=3, pipeline=False, loop_concurrency=model.lanes if pipeline else None)
    for seed, (dtype, (B, H, W)) in enumerate(CASES):
        i1, i2 = _frames(20 + seed, B, H, W, dtype)
        want = _route(plain, i1, i2, OVERLAP)
        got = model([i1, i2])
        assert len(got) == 3
        if pipeline:
            assert all(g.__dict__.get('_pending') is not None for g in got)      # the caller's stream did not wait for the loop
        base = got[0].data_ptr()
        for k, (g, w_) in enumerate(zip(got, want)):
            assert tuple(g.shape) == (B, H, W, 2) and g.is_contiguous() and g.data_ptr() == base + 4 * k * B * H * W * 2
            np.testing.assert_array_equal(_np(g), w_)
        assert np.abs(want[-1]).max() > 0
        np.testing.assert_array_equal(_np(model.predict_step((i1, i2))), want[-1])
        np.testing.assert_array_equal(_np(model.predict_step((torch.as_tensor(i1).cuda(), torch.as_tensor(i2).cuda()))), want[-1])
        single = np.concatenate([_route(plain, i1[k:k + 1], i2[k:k + 1], OVERLAP, entry='predict_step') for k in range(B)])
        pred = model.predict([i1, i2], batch_size=1)
        assert isinstance(pred, np.ndarray) and pred.shape == (B, H, W, 2)
        np.testing.assert_array_equal(pred, single)
        pics = model.predict([i1, i2], batch_size=1, output='image')
        assert pics.dtype == np.uint8 and pics.shape == (B, H, W, 3)
        np.testing.assert_array_equal(pics, _np(image_ops.flow_to_image(single)))
        with pytest.raises(ValueError):
            model([i1[:, :, :149], i2[:, :, :149]], training=True)        # training-mode calls keep their check


@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_frames_no_larger_than_the_tile_are_the_crop_or_pad_route(variant):
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=5, perturb=True)
    tiled = _cls(variant)(weights=wts, iters_pred=3, target_size=TILE, fit='tile', tile_overlap=16)
    padded = _cls(variant)(weights=wts, iters_pred=3, target_size=TILE)
    plain = _cls(variant)(weights=wts, iters_pred=3)
    for seed, (dtype, (B, H, W)) in enumerate([(np.uint8, (2, 40, 70)), (np.float32, (1, 64, 90))]):
        i1, i2 = _frames(30 + seed, B, H, W, dtype)
        for g, w_ in zip(tiled([i1, i2]), padded([i1, i2])):
            assert tuple(g.shape) == (B, H, W, 2)
            np.testing.assert_array_equal(_np(g), _np(w_))
        np.testing.assert_array_equal(_np(tiled.predict_step((i1, i2))), _np(padded.predict_step((i1, i2))))
    # frames that already have the tile's size: the model without the option, on the buffers that came in
    a, b = (torch.as_tensor(x).cuda() for x in _frames(7, 2, *TILE, np.float32))
    for g, w_ in zip(tiled([a, b]), plain([a, b])):
        np.testing.assert_array_equal(_np(g), _np(w_))
    fa, fb, window = tiled._fit_frames(a, b)
    assert window is None and fa.data_ptr() == a.data_ptr() and fb.data_ptr() == b.data_ptr()


@pytest.mark.parametrize('pipeline', [False, True], ids=['serial', 'pipelined'])
@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_test_step_with_fit_tile_scores_at_the_frames_own_size(variant, pipeline):
    """Ground truth of the frames' own size against the blended last prediction.  Both sides reduce the same float values with the
    same kernel; the mean comes back as float32, so one float32 ulp (1.2e-7 relative) is allowed, as in
    tests/test_gpu_resize.py::test_test_step_with_fit_resize_scores_at_the_frames_own_size."""
    from tf_raft_amd import losses
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=9, perturb=True)
    model = _cls(variant)(weights=wts, iters_pred=3, target_size=TILE, fit='tile', tile_overlap=OVERLAP, pipeline=pipeline)
    model.compile(optimizer=None)
    plain = _cls(variant)(weights=wts, iters_pred=3, pipeline=False, loop_concurrency=model.lanes if pipeline else None)
    rng = np.random.default_rng(31)
    for seed, (dtype, (B, H, W)) in enumerate(CASES):
        model.reset_metrics()
        i1, i2 = _frames(50 + seed, B, H, W, dtype)
        flow = (rng.normal(size=(B, H, W, 2)) * 2).astype(np.float32)
        valid = rng.uniform(size=(B, H, W)) < 0.9
        got = {k: float(v) for k, v in model.test_step((i1, i2, flow, valid)).items()}
        last = torch.as_tensor(_route(plain, i1, i2, OVERLAP, entry='predict_step')).cuda()
        want = {k: float(v) for k, v in losses.end_point_error([flow, valid], last).items()}
        for k in ('u1', 'u3', 'u5'):
            assert abs(got[k] - want[k]) <= 1.2e-7 * abs(want[k]), (k, got[k], want[k])
        assert want['epe'] > 0 and abs(got['epe'] - want['epe']) <= 1.2e-7 * abs(want['epe']), (got['epe'], want['epe'])


# ------------------------------------------------------------------ against the CPU oracle
@pytest.mark.parametrize('variant,frame,overlap,iters,seed', [('raft', (100, 150), 16, 12, 0), ('small', (100, 150), 16, 12, 0),
                                                              ('raft', (60, 200), 32, 12, 1), ('raft', (170, 96), 8, 12, 2)])
def test_fit_tile_against_the_oracle(variant, frame, overlap, iters, seed):
    """Free-running, every prediction within the project's bound of blend64(oracle32(numpy tiles)): the blend is a convex
    combination, so it cannot enlarge the per-tile error the project already bounds.  Only where
    tests/golden/conditioning_tiled.json shows the oracle itself well conditioned on the case."""
    from oracle.losses import max_epe
    sys.path.insert(0, GOLDEN)
    from make_conditioning import case_inputs
    from make_conditioning_tiled import case_key, oracle_route
    H, W = frame
    with open(os.path.join(GOLDEN, 'conditioning_tiled.json')) as f:
        cond = json.load(f)[case_key(variant, H, W, overlap, iters, seed)]
    assert max(cond['epe32v64']) <= 2e-4, 'fixture: the oracle itself is ill conditioned on this case'
    i1, i2, wts = case_inputs(variant, H, W, seed, 'conditioned')
    want = oracle_route(variant, wts, i1, i2, overlap, iters)
    model = _cls(variant)(weights=wts, iters_pred=iters, target_size=TILE, fit='tile', tile_overlap=overlap)
    got = model([i1, i2])
    errs = [max_epe(_np(g), w_) for g, w_ in zip(got, want)]
    report(f'tiled {variant} {H}x{W} overlap {overlap}', final_epe=errs[-1], worst_epe=max(errs), oracle32_vs_64_worst=max(cond['epe32v64']),
           final_max_abs_flow=cond['max_abs_flow'][-1])
    print('[parity] per-iteration max EPE hip-vs-oracle32 :', ' '.join(f'{e:.2e}' for e in errs))
    assert len(got) == iters and all(tuple(g.shape) == (1, H, W, 2) for g in got)
    assert max(errs) <= TOL, errs
    assert max_epe(_np(model.predict_step((i1, i2))), want[-1]) <= TOL

"""Flow over frame sequences on the GPU (``RAFT.video`` / ``FlowVideo.push`` / ``RAFT.predict_video``): the
feature encoder runs once per frame, nothing but the previous frame reaches a pair, the warm start is the composition of the
public pieces bit for bit, and the flows are within the project's bound of the CPU oracle, cold and from a given init, only where
the fixtures (tests/golden/conditioning_bidirectional.json, conditioning_video.json) show the oracle itself well conditioned.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, report

pytestmark = pytest.mark.gpu

TOL = 1e-3            # tests/test_gpu_model.py TOL: max EPE against the oracle
OVERLAP = (16, 32)


def _np(t):
    return t.detach().cpu().numpy()


def _plain(t):
    return t.as_subclass(torch.Tensor)


def _cls(variant):
    import tf_raft_amd
    return tf_raft_amd.RAFT if variant == 'raft' else tf_raft_amd.SmallRAFT


def _clip(seed, T, N, H, W, dtype=np.float32):
    """T time steps of N frames each."""
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return [rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8) for _ in range(T)]
    return [rng.uniform(0, 255, size=(N, H, W, 3)).astype(np.float32) for _ in range(T)]


def _model(variant, seed, **kw):
    from tf_raft_amd import weights as wm
    return _cls(variant)(weights=wm.init_weights(variant, seed=seed, perturb=True), **kw)


def _pushes(video, clip):
    return [video.push(f) for f in clip]


@pytest.mark.parametrize('variant,H,W', [('raft', 64, 96), ('small', 64, 96), ('raft', 72, 104)])
def test_history_does_not_leak_into_a_pair(variant, H, W):
    """Cold stream: the flow of pair (t, t + 1) from a stream that has seen frames 0 .. t + 1 is bitwise the flow of a fresh
    stream pushed t and t + 1 only."""
    model = _model(variant, 11, iters_pred=3)
    clip = _clip(110, 4, 2, H, W)
    flows = _pushes(model.video(), clip)
    assert flows[0] is None
    for t in range(3):
        got = flows[t + 1]
        assert tuple(got.shape) == (2, H, W, 2) and got.dtype == torch.float32 and got.is_cuda
        fresh = model.video()
        assert fresh.push(clip[t]) is None
        assert torch.equal(_plain(fresh.push(clip[t + 1])), _plain(got)), t
    assert not torch.equal(_plain(flows[1]), _plain(flows[2]))


@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_each_frame_is_encoded_once(variant):
    model = _model(variant, 12, iters_pred=3)
    seen = []
    encode = model.fnet.forward_device

    def counted(images, input_affine=False, images_b=None):
        seen.append((images.shape[0], images_b is not None))
        return encode(images, input_affine=input_affine, images_b=images_b)

    model.fnet.forward_device = counted
    T, N = 4, 2
    video = model.video(warm_start=True)
    flows = _pushes(video, _clip(120, T, N, 64, 96))
    assert sum(n for n, _ in seen) == T * N and len(seen) == T
    assert not any(pair for _, pair in seen), 'the feature encoder was handed a second batch'
    assert tuple(video.flow_low.shape) == (N, 8, 12, 2) and all(f is not None for f in flows[1:])
    # ... and predict_video encodes each of its T frames once, in chunks
    del seen[:]
    model.predict_video(np.concatenate(_clip(121, 5, 1, 64, 96)), batch_size=2)
    assert [n for n, _ in seen] == [1, 2, 2] and not any(pair for _, pair in seen)


@pytest.mark.parametrize('variant,H,W,seed', [('raft', 64, 96, 0), ('small', 64, 96, 0), ('raft', 128, 160, 1), ('raft', 72, 104, 2)])
def test_a_cold_push_against_the_oracle(variant, H, W, seed):
    """The pushed flow within the project's bound of the oracle's final prediction, on the cases of the bidirectional step
    (forward direction), whose fixture shows the oracle well conditioned.  The difference from ``predict_step`` is printed, not
    asserted: the launch plan may pick other encoder variants for N frames than for 2N."""
    import oracle
    from oracle.losses import max_epe
    sys.path.insert(0, GOLDEN)
    from make_conditioning import case_inputs
    from make_conditioning_bidirectional import B, ITERS, case_key
    with open(os.path.join(GOLDEN, 'conditioning_bidirectional.json')) as f:
        cond = json.load(f)[case_key(variant, H, W, seed)]
    assert max(cond['epe32v64']) <= 2e-4, 'fixture: the oracle itself is ill conditioned on this case'
    i1, i2, wts = case_inputs(variant, H, W, seed, 'conditioned', B=B)
    want = np.asarray((oracle.RAFT if variant == 'raft' else oracle.SmallRAFT)(wts, iters_pred=ITERS)([i1, i2])[-1])
    model = _cls(variant)(weights=wts, iters_pred=ITERS)
    video = model.video()
    assert video.push(i1) is None
    got = _np(video.push(i2))
    err = max_epe(got, want)
    report(f'video cold {variant} {H}x{W}', epe=err, oracle32_vs_64_worst=max(cond['epe32v64']),
           vs_predict_step=max_epe(got, _np(model.predict_step((i1, i2)))))
    assert err <= TOL, err


def _init_cases():
    sys.path.insert(0, GOLDEN)
    from make_conditioning_video import CASES
    return CASES


@pytest.mark.parametrize('variant,H,W,seed', _init_cases())
def test_a_push_from_an_init_against_the_oracle(variant, H, W, seed):
    """``push(frames, flow_init=...)`` against the oracle whose ``initialize_flow`` returns ``(coords0, coords0 + flow_init)``: a
    smooth init of about two cells, asserted only where tests/golden/conditioning_video.json shows the oracle at or below 2e-4."""
    from oracle.losses import max_epe
    from make_conditioning import case_inputs
    from make_conditioning_video import B, ITERS, case_key, oracle_with_init, smooth_init
    with open(os.path.join(GOLDEN, 'conditioning_video.json')) as f:
        cond = json.load(f)[case_key(variant, H, W, seed)]
    assert max(cond['epe32v64']) <= 2e-4, 'fixture: the oracle itself is ill conditioned on this case'
    i1, i2, wts = case_inputs(variant, H, W, seed, 'conditioned', B=B)
    init = smooth_init(seed, B, H // 8, W // 8)
    want = oracle_with_init(variant, wts, i1, i2, init)[-1]
    model = _cls(variant)(weights=wts, iters_pred=ITERS)
    video = model.video()
    video.push(i1)
    got = _np(video.push(i2, flow_init=init))
    cold = model.video()
    cold.push(i1)
    from_cold = max_epe(got, _np(cold.push(i2)))
    err = max_epe(got, want)
    report(f'video init {variant} {H}x{W}', epe=err, oracle32_vs_64_worst=max(cond['epe32v64']), from_cold=from_cold,
           max_abs_init=float(np.abs(init).max()))
    assert err <= TOL, err
    assert from_cold > 1.0, 'the init did not reach the loop'


@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_the_warm_chain_is_the_composition_of_the_public_pieces(variant):
    """A ``warm_start=True`` stream returns, bit for bit, what a cold stream returns when every push is handed
    ``forward_interpolate(video.flow_low)`` by hand -- and not what the cold stream returns on its own."""
    from tf_raft_amd import image_ops
    model = _model(variant, 13, iters_pred=4)
    clip = _clip(130, 4, 2, 64, 96)
    warm = _pushes(model.video(warm_start=True), clip)
    hand = model.video()
    by_hand = [hand.push(clip[0]), hand.push(clip[1])]
    for t in (2, 3):
        init = image_ops.forward_interpolate(hand.flow_low)
        assert tuple(init.shape) == (2, 8, 12, 2) and _np(init).any()
        by_hand.append(hand.push(clip[t], flow_init=init))
    cold = _pushes(model.video(), clip)
    assert warm[0] is None and by_hand[0] is None
    for t in (1, 2, 3):
        assert torch.equal(_plain(warm[t]), _plain(by_hand[t])), t
    assert torch.equal(_plain(warm[1]), _plain(cold[1]))                   # the first pair has nothing to start from
    for t in (2, 3):
        assert not torch.equal(_plain(warm[t]), _plain(cold[t])), t


def _by_hand_route(fit, H, W):
    """The public op in and the public op back of a frame-size route around a model of 64 x 96."""
    from tf_raft_amd import image_ops
    if fit == 'crop_or_pad':
        return (lambda x: image_ops.resize_with_crop_or_pad(x, 64, 96, dtype=torch.float32)), (lambda f: image_ops.resize_with_crop_or_pad(f, H, W))
    if fit == 'resize':
        return (lambda x: image_ops.resize(x, 64, 96, antialias=True)), (lambda f: image_ops.resize_flow(f, H, W, antialias=True))
    return (lambda x: image_ops.tile_gather(x, 64, 96, overlap=OVERLAP)), (lambda f: image_ops.tile_blend(f, H, W, overlap=OVERLAP))


@pytest.mark.parametrize('fit', ['crop_or_pad', 'resize', 'tile'])
@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_a_frame_size_route_is_bitwise_the_route_done_by_hand(variant, fit):
    """Warm streams (the first pair cold, the second started from the first): the carried map and the carried flow live in model
    space, per tile under ``fit='tile'``."""
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=14, perturb=True)
    kw = {'tile_overlap': OVERLAP} if fit == 'tile' else {}
    model = _cls(variant)(weights=wts, iters_pred=3, target_size=(64, 96), fit=fit, **kw)
    plain = _cls(variant)(weights=wts, iters_pred=3)
    N, H, W = 2, 100, 150
    clip = _clip(140, 3, N, H, W, np.uint8)
    video, by_hand = model.video(warm_start=True), plain.video(warm_start=True)
    way_in, way_back = _by_hand_route(fit, H, W)
    for t, frames in enumerate(clip):
        got, want = video.push(frames), by_hand.push(way_in(frames))
        if t == 0:
            assert got is None and want is None
            continue
        assert tuple(got.shape) == (N, H, W, 2)
        assert torch.equal(_plain(got), _plain(way_back(want))), t
        assert torch.equal(video.flow_low, by_hand.flow_low)
        assert _np(got).any()
    assert tuple(video.flow_low.shape) == (N * (4 if fit == 'tile' else 1), 8, 12, 2)          # 2 x 2 tiles cover 100 x 150


def test_predict_video_is_the_pushes_and_its_chunks_meet_the_oracle():
    from oracle.losses import max_epe
    sys.path.insert(0, GOLDEN)
    from make_conditioning_video import ITERS, VIDEO_KEY, oracle_pair, video_inputs
    with open(os.path.join(GOLDEN, 'conditioning_video.json')) as f:
        cond = json.load(f)[VIDEO_KEY]
    assert max(cond['epe32v64']) <= 2e-4, 'fixture: the oracle itself is ill conditioned on this video'
    variant, frames, wts = video_inputs()
    T = frames.shape[0]
    assert T == 5
    model = _cls(variant)(weights=wts, iters_pred=ITERS)
    # warm: the concatenated pushes of one video
    video = model.video(warm_start=True)
    pushed = [video.push(frames[t:t + 1]) for t in range(T)]
    got = model.predict_video(frames, warm_start=True)
    assert isinstance(got, np.ndarray) and got.shape == (T - 1,) + frames.shape[1:3] + (2,) and got.dtype == np.float32
    np.testing.assert_array_equal(got, np.concatenate([_np(f) for f in pushed[1:]]))
    np.testing.assert_array_equal(model.predict_video(torch.as_tensor(frames).cuda(), warm_start=True), got)      # device frames
    # cold: two pairs per call, the last call one pair; every pair against the oracle
    cold = model.predict_video(frames, batch_size=2)
    assert cold.shape == got.shape
    singles = model.video()
    singles.push(frames[:1])
    for t in range(T - 1):
        want = oracle_pair(variant, wts, frames[t], frames[t + 1])
        err = max_epe(cold[t:t + 1], want[None])
        report(f'predict_video pair {t}', epe=err, oracle32_vs_64=cond['epe32v64'][t],
               vs_single_push=max_epe(cold[t:t + 1], _np(singles.push(frames[t + 1:t + 2]))))
        assert err <= TOL, (t, err)
    assert model.predict_video(frames, batch_size=2, steps=1).shape[0] == 2
    assert model.predict_video(frames[:2]).shape[0] == 1
    for bad in (frames[:1], frames[:0]):
        with pytest.raises(ValueError):
            model.predict_video(bad)


@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_a_push_joins_a_pipelined_model(variant):
    """After three pipelined ``predict_step`` calls (loops in flight on the lanes) the pushes equal a fresh serial model's."""
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=15, perturb=True)
    piped = _cls(variant)(weights=wts, iters_pred=3, pipeline=True)
    serial = _cls(variant)(weights=wts, iters_pred=3)
    clip = _clip(150, 3, 2, 64, 96)
    pending = [piped.predict_step((clip[0], clip[1])) for _ in range(3)]
    got = _pushes(piped.video(warm_start=True), clip)
    want = _pushes(serial.video(warm_start=True), clip)
    for g, w_ in zip(got[1:], want[1:]):
        assert torch.equal(_plain(g), _plain(w_))
    np.testing.assert_array_equal(_np(piped.predict_step((clip[0], clip[1]))), _np(pending[0]))      # and pipelined calls go on as before


def test_a_stream_holds_one_frame_shape_until_it_is_reset():
    model = _model('small', 16, iters_pred=3)
    video = model.video()
    clip = _clip(160, 2, 2, 64, 96)
    with pytest.raises(ValueError, match='flow_init'):
        video.push(clip[0], flow_init=np.zeros((2, 8, 12, 2), np.float32))
    assert video.push(clip[0]) is None
    for bad in (clip[1][:1],                                       # another N
                clip[1][:, :56],                                   # another size
                clip[1].astype(np.uint8),                          # another type
                clip[1][0], clip[1][..., :2]):                     # not (N, H, W, 3)
        with pytest.raises(ValueError):
            video.push(bad)
    for bad_init in (np.zeros((2, 8, 12, 3), np.float32), np.zeros((1, 8, 12, 2), np.float32), np.zeros((2, 64, 96, 2), np.float32)):
        with pytest.raises(ValueError, match='flow_init'):
            video.push(clip[1], flow_init=bad_init)
    want = video.push(clip[1])                                     # the refused pushes left the stream as it was
    fresh = model.video()
    fresh.push(clip[0])
    assert torch.equal(_plain(want), _plain(fresh.push(clip[1])))
    video.reset()
    assert video.flow_low is None
    small = _clip(161, 2, 1, 72, 104, np.uint8)
    assert video.push(small[0]) is None
    assert tuple(video.push(small[1]).shape) == (1, 72, 104, 2)
    with pytest.raises(ValueError, match='multiples of 8'):
        model.video().push(np.zeros((1, 70, 96, 3), np.float32))

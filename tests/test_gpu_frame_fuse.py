"""Motion-compensated temporal filtering on the GPU: the three ``raft_fuse_frames_*`` entries against the
float32 NumPy restatement of tests/test_frame_fuse.py, bit for bit, at every shared shape, with and without ``skip``, in both
vector forms, twice into buffers pre-filled with two different sentinels (an element that is not written differs between the
runs); the indirection through a stack, other alignments, the public functions, and the model's ``fuse_step`` and
``denoise_video`` against their compositions."""
import numpy as np
import pytest
import torch

from conftest import report
from test_frame_fuse import IDS, SHAPES, assert_same, bits, expected, fuse_case, np_fuse_frames

pytestmark = pytest.mark.gpu

GUARD = 64
ENTRIES = {'f32': ('raft_fuse_frames_f32', torch.float32), 'u8_f32': ('raft_fuse_frames_u8_f32', torch.float32),
           'u8': ('raft_fuse_frames_u8', torch.uint8)}


def _np(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy()


def _dev():
    from tf_raft_amd import _dev as d
    return d.require_gpu()


def _on(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(n, dtype, device, fill):
    """A buffer of ``n`` elements between two guard bands, every byte ``fill``: (whole buffer, the view a launch writes)."""
    size = torch.empty((), dtype=dtype).element_size()
    buf = torch.full(((2 * GUARD + n) * size,), fill, dtype=torch.uint8, device=device)
    return buf, buf[GUARD * size:(GUARD + n) * size].view(dtype)


def _intact(buf, n_bytes, fill):
    b = buf.cpu().numpy()
    band = (len(b) - n_bytes) // 2
    return bool((b[:band] == fill).all() and (b[-band:] == fill).all())


def _fuse(kind, center, stack, index, vectors, skip, absolute, sigma, cw, r, fill=0xAB, want_weight=True):
    """``raft_fuse_frames_*`` through the library itself on device tensors, into guarded outputs every byte of which is ``fill``
    beforehand: (dst (N, H, W, C), weight (N, H, W)) as host arrays."""
    import ctypes
    from tf_raft_amd import _dev as d
    from tf_raft_amd._ffi import check
    name, out_dtype = ENTRIES[kind]
    N, H, W, Cn = center.shape
    K = vectors.shape[0]
    buf_o, out = _guarded(N * H * W * Cn, out_dtype, center.device, fill)
    buf_w, weight = _guarded(N * H * W, torch.float32, center.device, fill)
    idx = None if index is None else (ctypes.c_int64 * len(index))(*index)
    check(getattr(d.lib(), name)(d.ptr(center), d.ptr(stack), idx, d.ptr(vectors), d.ptr(skip) if skip is not None else None,
                                 int(absolute), sigma, cw, r, d.ptr(out), d.ptr(weight) if want_weight else None, K, N, H, W, Cn,
                                 d.stream_ptr()), name)
    torch.cuda.synchronize()
    assert _intact(buf_o, out.numel() * out.element_size(), fill) and _intact(buf_w, N * H * W * 4, fill)
    return out.cpu().numpy().reshape(N, H, W, Cn), weight.cpu().numpy().reshape(N, H, W)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_the_entries_are_the_restatement_bit_for_bit(shape):
    dev = _dev()
    K, N, H, W, Cn, r = shape
    c = fuse_case(shape)
    on = {k: _on(c[k], dev) for k in ('center', 'neighbours', 'center_f', 'neighbours_f', 'flows', 'positions', 'skip')}
    for kind in ENTRIES:
        f = '_f' if kind == 'f32' else ''
        for with_skip in (True, False):
            for absolute in (False, True):
                want, want_w = expected(shape, 'f32' if kind == 'f32' else 'u8', kind == 'u8', with_skip, absolute)
                runs = [_fuse(kind, on['center' + f], on['neighbours' + f], None, on['positions' if absolute else 'flows'],
                              on['skip'] if with_skip else None, absolute, c['sigma'], c['center_weight'], r, fill)
                        for fill in (0xAB, 0x54)]
                what = (kind, with_skip, absolute)
                assert runs[0][0].dtype == want.dtype, what
                np.testing.assert_array_equal(bits(runs[0][0]), bits(want), err_msg=str(what))
                np.testing.assert_array_equal(bits(runs[0][1]), bits(want_w), err_msg=str(what))
                np.testing.assert_array_equal(bits(runs[1][0]), bits(runs[0][0]), err_msg=str(what))
                np.testing.assert_array_equal(bits(runs[1][1]), bits(runs[0][1]), err_msg=str(what))
    # without a weight output the frame is the same
    got, untouched = _fuse('u8', on['center'], on['neighbours'], None, on['flows'], on['skip'], False, c['sigma'], c['center_weight'], r,
                           want_weight=False)
    assert_same(got, expected(shape, 'u8', True, True, False)[0])
    assert (untouched.view(np.uint8) == 0xAB).all()


def test_neighbours_through_a_stack_and_its_index():
    dev = _dev()
    shape = SHAPES[6]                                                    # (3, 2, 17, 64, 2, 1)
    K, N, H, W, Cn, r = shape
    c = fuse_case(shape)
    want, want_w = expected(shape, 'u8', True, True, False)
    flows, skip = _on(c['flows'], dev), _on(c['skip'], dev)
    # a window of a video: the centre in the middle, the index skips it
    video = np.concatenate([c['neighbours'][:2], c['center'][None], c['neighbours'][2:], c['center'][None]])
    dvideo = _on(video, dev)
    got, got_w = _fuse('u8', dvideo[2], dvideo, [0, 1, 3], flows, skip, False, c['sigma'], c['center_weight'], r)
    assert_same(got, want)
    assert_same(got_w, want_w)
    # any order, and a block may repeat
    order = [3, 0, 0]
    want2 = np_fuse_frames(c['center'], video[order], c['flows'], c['skip'], False, c['sigma'], c['center_weight'], r, out_uint8=True)
    got2 = _fuse('u8', dvideo[4], dvideo, order, flows, skip, False, c['sigma'], c['center_weight'], r)
    assert_same(got2[0], want2[0])
    assert_same(got2[1], want2[1])
    assert not np.array_equal(got2[0], got)
    # slices and neighbours are kept apart: neighbour 1 of slice 1 changes slice 1 only, and only where it is seen
    changed = video.copy()
    changed[1, 1] = 255 - changed[1, 1]
    got3, _ = _fuse('u8', dvideo[2], _on(changed, dev), [0, 1, 3], flows, skip, False, c['sigma'], c['center_weight'], r)
    assert_same(got3[0], got[0])
    assert not np.array_equal(got3[1], got[1])
    want3 = np_fuse_frames(c['center'], changed[[0, 1, 3]], c['flows'], c['skip'], False, c['sigma'], c['center_weight'], r, out_uint8=True)
    assert_same(got3, want3[0])
    # the public launch form takes the same stack
    from tf_raft_amd import image_ops
    out, weight = image_ops.fuse_frames_launch(dvideo[2], dvideo, flows, [0, 1, 3], skip, False, c['sigma'], r, c['center_weight'], True)
    assert_same(_np(out), want)
    assert_same(_np(weight), want_w)


def test_other_alignments():
    dev = _dev()
    shape = SHAPES[3]                                                    # (3, 1, 9, 33, 3, 2)
    K, N, H, W, Cn, r = shape
    c = fuse_case(shape)
    want, want_w = expected(shape, 'u8', True, True, False)
    n_frame = N * H * W * Cn
    # frames at odd byte addresses
    raw = torch.zeros((1 + (K + 1) * n_frame + 16,), dtype=torch.uint8, device=dev)
    frames = raw[1:1 + (K + 1) * n_frame].view(K + 1, N, H, W, Cn)
    frames.copy_(_on(np.concatenate([c['center'][None], c['neighbours']]), dev))
    assert frames.data_ptr() % 2 == 1
    # vectors at 8 mod 16
    rawv = torch.zeros((K * N * H * W * 2 + 8,), dtype=torch.float32, device=dev)
    off = 2 if rawv.data_ptr() % 16 == 0 else 0
    vec = rawv[off:off + K * N * H * W * 2].view(K, N, H, W, 2)
    vec.copy_(_on(c['flows'], dev))
    assert vec.data_ptr() % 16 == 8
    got, got_w = _fuse('u8', frames[0], frames, [1, 2, 3], vec, _on(c['skip'], dev), False, c['sigma'], c['center_weight'], r)
    assert_same(got, want)
    assert_same(got_w, want_w)
    got, got_w = _fuse('u8_f32', frames[0], frames[1:], None, vec, _on(c['skip'], dev), False, c['sigma'], c['center_weight'], r)
    assert_same(got, expected(shape, 'u8', False, True, False)[0])


@pytest.mark.parametrize('shape', [SHAPES[2], SHAPES[4]], ids=[IDS[2], IDS[4]])
def test_the_public_functions(shape):
    from tf_raft_amd import image_ops
    K, N, H, W, Cn, r = shape
    c = fuse_case(shape)
    kw = dict(sigma=c['sigma'], patch_radius=r, center_weight=c['center_weight'])
    # uint8 frames give uint8; host inputs; the weight on request
    got = image_ops.fuse_frames(c['center'], c['neighbours'], c['flows'], skip=c['skip'], **kw)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (N, H, W, Cn)
    assert_same(_np(got), expected(shape, 'u8', True, True, False)[0])
    got, weight = image_ops.fuse_frames(c['center'], c['neighbours'], positions=c['positions'], skip=c['skip'].astype(bool),
                                        return_weight=True, dtype=torch.float32, **kw)
    assert got.dtype == torch.float32 and weight.dtype == torch.float32 and tuple(weight.shape) == (N, H, W)
    want, want_w = expected(shape, 'u8', False, True, True)
    assert_same(_np(got), want)
    assert_same(_np(weight), want_w)
    # float32 frames on the device, a list of neighbours, no skip
    dev = _dev()
    got = image_ops.fuse_frames(_on(c['center_f'], dev), [_on(a, dev) for a in c['neighbours_f']], _on(c['flows'], dev), **kw)
    assert got.dtype == torch.float32
    assert_same(_np(got), expected(shape, 'f32', False, False, False)[0])
    # one frame without a batch axis; float64 narrows
    got, weight = image_ops.fuse_frames(c['center_f'][0].astype(np.float64), c['neighbours_f'][:, 0], c['flows'][:, 0], skip=c['skip'][:, 0],
                                        return_weight=True, **kw)
    assert tuple(got.shape) == (H, W, Cn) and tuple(weight.shape) == (H, W)
    want1 = np_fuse_frames(c['center_f'][:1], c['neighbours_f'][:, :1], c['flows'][:, :1], c['skip'][:, :1], False, c['sigma'],
                           c['center_weight'], r)
    assert_same(_np(got), want1[0][0])
    assert_same(_np(weight), want1[1][0])
    # out= of the launch form
    out = torch.full((N, H, W, Cn), 7, dtype=torch.uint8, device=dev)
    res, none = image_ops.fuse_frames_launch(_on(c['center'], dev), _on(c['neighbours'], dev), _on(c['flows'], dev), None,
                                             _on(c['skip'], dev), False, c['sigma'], r, c['center_weight'], out=out)
    assert res is out and none is None
    assert_same(_np(out), expected(shape, 'u8', True, True, False)[0])


# ------------------------------------------------------------------ the model
def _plain(t):
    return t.detach().as_subclass(torch.Tensor)


def _model(route, conditioned=False):
    """``conditioned``: a flow head scaled down as by weights.condition_weights, with a drift of (0.005, -0.004) feature pixels
    per iteration: after 3 iterations both directions predict about (0.12, -0.1) pixels, |f + b|^2 is about 0.1 and passes the
    consistency test (beta = 0.5), so chained points survive and the fusion has neighbours to use.  With the plain random weights
    (flows of about 6 pixels) 99.98 % of the chained points fail the test and every frame comes back nearly unchanged."""
    import tf_raft_amd
    from tf_raft_amd import weights as wm
    wts = wm.init_weights('small', seed=6, perturb=True)
    if conditioned:
        wts = wm.condition_weights('small', wts, 'conditioned')
        wts['update_block/flow_head/conv2/bias'] = np.array([0.005, -0.004], np.float32)
    if route == 'plain':
        return tf_raft_amd.SmallRAFT(weights=wts, iters_pred=3), (64, 96)
    return tf_raft_amd.SmallRAFT(weights=wts, iters_pred=3, target_size=(64, 96), fit='resize'), (100, 150)


def _footage(H, W, T=5, seed=80, dtype=np.uint8):
    """One video of T frames: a texture that shifts by a pixel or two per frame, plus noise."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0, 255, (H + 16, W + 16, 3))
    video = np.stack([base[8 + t:8 + t + H, 8 - t:8 - t + W] for t in range(T)])
    video = (video + rng.normal(0, 4, video.shape)).clip(0, 255)
    return np.round(video).astype(np.uint8) if dtype == np.uint8 else video.astype(np.float32)


@pytest.mark.parametrize('route', ['plain', 'resize'])
def test_fuse_step_is_its_composition(route):
    from tf_raft_amd import image_ops
    model, (H, W) = _model(route)
    dev = _dev()
    for dtype in (np.uint8, np.float32):
        video = _footage(H, W, dtype=dtype)
        center, neighbours = video[2:4], np.stack([video[0:2], video[1:3], video[3:5]])          # N = 2, K = 3
        for kw in ({}, {'sigma': 4.0, 'patch_radius': 2, 'center_weight': 0.5, 'occlusion_test': 'range'}):
            got = model.fuse_step((center, neighbours), **kw)
            assert got.is_cuda and tuple(got.shape) == center.shape and got.dtype == (torch.uint8 if dtype == np.uint8 else torch.float32)
            first = np.concatenate([center] * 3)
            res = model.predict_step_bidirectional((first, neighbours.reshape((6,) + center.shape[1:])),
                                                   occlusion_test=kw.get('occlusion_test', 'consistency'))
            want, _ = image_ops.fuse_frames_launch(_on(center, dev), _on(neighbours, dev), _plain(res.forward).reshape(3, 2, H, W, 2),
                                                   None, _plain(res.occluded_forward).reshape(3, 2, H, W), False,
                                                   kw.get('sigma', 10.0), kw.get('patch_radius', 1), kw.get('center_weight', 1.0))
            np.testing.assert_array_equal(bits(_np(got)), bits(_np(want)))
            assert not np.array_equal(_np(got), center)
    report(f'fuse_step ({route})', occluded=float(_np(res.occluded_forward).mean()),
           change=float(np.abs(_np(got).astype(np.float64) - center).mean()))


@pytest.mark.parametrize('route', ['plain', 'resize'])
def test_denoise_video_is_its_composition_and_one_frame_is_returned(route):
    from tf_raft_amd import image_ops
    model, (H, W) = _model(route, conditioned=True)
    dev = _dev()
    for dtype in (np.uint8, np.float32):
        video = _footage(H, W, dtype=dtype)
        T = video.shape[0]
        one = model.denoise_video(video[:1])
        assert one.dtype == dtype and np.array_equal(one, video[:1])
        got = model.denoise_video(torch.from_numpy(video) if dtype == np.uint8 else video, radius=2, batch_size=3)
        assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == video.shape
        # the composition: the passes, the grid chained both ways (back in time by one-step launches, which give the bits of the
        # one S-step launch), one fuse launch on separate tensors, fewer neighbours at the ends
        res = model.predict_bidirectional([video[:-1], video[1:]], batch_size=3)
        fwd, bwd = _on(res.forward, dev)[:, None], _on(res.backward, dev)[:, None]
        grid = _on(image_ops.point_grid(H, W), dev)
        dvideo = _on(video, dev)
        lost_share = []
        for t in range(T):
            back, ahead = min(2, t), min(2, T - 1 - t)
            pos, lost, nbs = [], [], []
            p, l = grid, None
            for s in range(back):
                P, L = image_ops.track_launch(p, bwd[t - 1 - s:t - s], fwd[t - 1 - s:t - s], lost=l)
                p, l = P[0], L[0]
                pos.append(p), lost.append(l), nbs.append(t - 1 - s)
            if ahead:
                P, L = image_ops.track_launch(grid, fwd[t:t + ahead], bwd[t:t + ahead])
                pos += list(P)
                lost += list(L)
                nbs += list(range(t + 1, t + 1 + ahead))
            K = len(nbs)
            assert K == back + ahead and 2 <= K <= 4
            want, _ = image_ops.fuse_frames_launch(dvideo[t:t + 1], torch.stack([dvideo[s:s + 1] for s in nbs]),
                                                   torch.stack(pos).reshape(K, 1, H, W, 2), None, torch.stack(lost).reshape(K, 1, H, W), True)
            np.testing.assert_array_equal(bits(got[t]), bits(_np(want)[0]), err_msg=f't = {t}')
            lost_share.append(float((_np(torch.stack(lost)) != 0).mean()))
        assert not np.array_equal(got, video)
        assert np.mean(lost_share) < 0.5                     # (the weights are made so: the fusion has neighbours to use)
    report(f'denoise_video ({route})', lost=float(np.mean(lost_share)), change=float(np.abs(got.astype(np.float64) - video).mean()))

"""The range map and its occlusion test on the GPU: the three entries against the NumPy restatement of
tests/test_range_occlusion.py BIT FOR BIT (integer sums: no tolerance), guard bands, the NULL forms and repeats; the predictor's
``occlusion_test='range'``; one update-block training step with it against section 20's float64 oracle procedure within the
bounds of tests/test_gpu_bidirectional_step.py; and the unchanged defaults.
"""
import numpy as np
import pytest
import torch

from conftest import report
from test_bidirectional_step import (ORACLE_CLIP, ORACLE_ITERS, ORACLE_LR0, ORACLE_WD, oracle_case, oracle_schedule,
                                     reference_bidirectional_train_steps)
from test_photometric_loss import DEFAULTS
from test_range_occlusion import np_range_acc, np_range_map, np_range_occlusion, np_range_visibility, range_flows

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xAB
SHAPES = [(1, 1, 1), (1, 3, 1), (1, 5, 7), (2, 37, 53), (2, 368, 496)]
IDS = ['1x1x1', '1x3x1', '1x5x7', '2x37x53', '2x368x496']


def _np(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy()


def _guarded(n, dtype, device):
    """A buffer of ``n`` elements between two guard bands, every byte FILL: (whole buffer, the view a launch writes)."""
    size = torch.empty((), dtype=dtype).element_size()
    buf = torch.full(((2 * GUARD + n) * size,), FILL, dtype=torch.uint8, device=device)
    return buf, buf[GUARD * size:(GUARD + n) * size]


def _intact(buf, n_bytes):
    b = buf.cpu().numpy()
    band = (len(b) - n_bytes) // 2
    return bool((b[:band] == FILL).all() and (b[-band:] == FILL).all())


def _sums(lib, slices, H, W, device):
    """The workspace of the sums, full of garbage: the entry has to zero it itself."""
    nbytes = int(lib.raft_flow_range_workspace_bytes(slices, H, W))
    assert nbytes == slices * H * W * 8
    return torch.full((nbytes // 8,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=device)


def _range_map(flow):
    from tf_raft_amd import _dev
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    N, H, W, _ = flow.shape
    buf, out = _guarded(N * H * W, torch.float32, flow.device)
    ws = _sums(lib, N, H, W, flow.device)
    check(lib.raft_flow_range_map_f32(_dev.ptr(flow), _dev.ptr(out), N, H, W, _dev.ptr(ws), _dev.stream_ptr()), 'range_map')
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.float32).reshape(N, H, W), _intact(buf, N * H * W * 4)


def _range_occlusion(fa, fb, threshold, both=True):
    from tf_raft_amd import _dev
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    N, H, W, _ = fa.shape
    buf_a, occ_a = _guarded(N * H * W, torch.uint8, fa.device)
    buf_b, occ_b = _guarded(N * H * W, torch.uint8, fa.device)
    ws = _sums(lib, 2 * N if both else N, H, W, fa.device)
    check(lib.raft_flow_range_occlusion_f32(_dev.ptr(fa), _dev.ptr(fb), _dev.ptr(occ_a), _dev.ptr(occ_b) if both else None, N, H, W,
                                            threshold, _dev.ptr(ws), _dev.stream_ptr()), 'range_occlusion')
    torch.cuda.synchronize()
    intact = _intact(buf_a, N * H * W) and _intact(buf_b, N * H * W)
    return occ_a.cpu().numpy().reshape(N, H, W), occ_b.cpu().numpy().reshape(N, H, W), intact


def _range_visibility(flows, N, mask, threshold, apply, want_visible=True):
    """raft_flow_range_visibility_f32 through the library itself: (visible, guard bytes intact, the share's float32)."""
    from tf_raft_amd import _dev
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    B, H, W, _ = flows.shape
    buf, vis = _guarded(B * H * W, torch.uint8, flows.device)
    frac = torch.full((3,), -7.0, dtype=torch.float32, device=flows.device)
    ws = _sums(lib, B, H, W, flows.device)
    records = torch.full((int(lib.raft_flow_visibility_workspace_doubles()),), float('nan'), dtype=torch.float64, device=flows.device)
    check(lib.raft_flow_range_visibility_f32(_dev.ptr(flows), _dev.ptr(mask) if mask is not None else None,
                                             _dev.ptr(vis) if want_visible else None, _dev.ptr(frac[1:]), N, H, W, threshold, int(apply),
                                             _dev.ptr(ws), _dev.ptr(records), _dev.stream_ptr()), 'range_visibility')
    torch.cuda.synchronize()
    frac = frac.cpu().numpy()
    assert frac[0] == -7.0 and frac[2] == -7.0                               # one float is written
    return vis.cpu().numpy().reshape(B, H, W), _intact(buf, B * H * W), frac[1]


_CASES = {}


def _case(shape):
    """The flows of one shape and everything the restatement says about them, computed once and left unchanged."""
    if shape not in _CASES:
        N, H, W = shape
        host = range_flows(N, H, W, seed=H + W)
        mask = (np.random.default_rng(7).uniform(size=(2 * N, H, W)) < 0.7).astype(np.uint8) * 5       # (nonzero = use)
        acc = np_range_acc(host)                                             # the sums once; everything below is derived from them
        want = {'range': (acc.astype(np.float64) * 2.0 ** -24).astype(np.float32)}
        if H * W <= 64:
            np.testing.assert_array_equal(want['range'], np_range_map(host))
        for t in (0.5, 1.0):
            want['occ', t] = (np_range_occlusion(host[:N], host[N:], t, acc[N:]).astype(np.uint8),
                              np_range_occlusion(host[N:], host[:N], t, acc[:N]).astype(np.uint8))
        for key, m, apply in (('plain', None, 1), ('mask', mask, 1), ('count', mask, 0)):
            want['vis', key] = np_range_visibility(host, N, m, 0.5, apply, acc)[:2]
        for v in want.values():
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        host.setflags(write=False)
        mask.setflags(write=False)
        _CASES[shape] = (host, mask, want)
    return _CASES[shape]


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_the_range_map_is_the_restatement_bit_for_bit(shape):
    from tf_raft_amd import _dev, image_ops
    host, _, want = _case(shape)
    flow = torch.from_numpy(host.copy()).to(_dev.require_gpu())
    got, intact = _range_map(flow)
    np.testing.assert_array_equal(_bits(got), _bits(want['range']))
    assert intact
    for _ in range(5):                                                       # integer sums: any arrival order, the same bits
        again, _ = _range_map(flow)
        np.testing.assert_array_equal(_bits(again), _bits(got))
    pub = image_ops.range_map(flow)
    assert tuple(pub.shape) == host.shape[:-1] and pub.dtype == torch.float32
    np.testing.assert_array_equal(_bits(_np(pub)), _bits(got))
    np.testing.assert_array_equal(_bits(_np(image_ops.range_map(host[0].copy()))), _bits(got[0]))     # (H, W, 2) from the host
    report(f'range map {shape}', largest=float(got.max()), share_below_half=float((got < 0.5).mean()))


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_the_occlusion_masks_are_the_restatement_bit_for_bit(shape):
    from tf_raft_amd import _dev, image_ops
    N = shape[0]
    host, _, want = _case(shape)
    flows = torch.from_numpy(host.copy()).to(_dev.require_gpu())
    fa, fb = flows[:N], flows[N:]
    for t in (0.5, 1.0):
        occ_a, occ_b, intact = _range_occlusion(fa, fb, t)
        np.testing.assert_array_equal(occ_a, want['occ', t][0])
        np.testing.assert_array_equal(occ_b, want['occ', t][1])
        assert intact
        only_a, untouched, intact = _range_occlusion(fa, fb, t, both=False)   # occluded_b = NULL: only flow_b is splatted
        np.testing.assert_array_equal(only_a, occ_a)
        assert intact and (untouched == FILL).all()
    for _ in range(5):
        again = _range_occlusion(fa, fb, 1.0)
        np.testing.assert_array_equal(again[0], occ_a)
        np.testing.assert_array_equal(again[1], occ_b)
    pub_a, pub_b = image_ops.range_occlusion(fa, fb)
    np.testing.assert_array_equal(_np(pub_a), want['occ', 0.5][0])
    np.testing.assert_array_equal(_np(pub_b), want['occ', 0.5][1])
    one_a, none_b = image_ops.range_occlusion_launch(fa, fb, 0.5, both=False)
    assert none_b is None
    np.testing.assert_array_equal(_np(one_a), want['occ', 0.5][0])


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_the_visibility_entry_is_the_restatement_bit_for_bit(shape):
    from tf_raft_amd import _dev, image_ops
    N, H, W = shape
    host, mask_h, want = _case(shape)
    dev = _dev.require_gpu()
    flows = torch.from_numpy(host.copy()).to(dev)
    mask = torch.from_numpy(mask_h.copy()).to(dev)
    if shape == SHAPES[-1]:                                                  # more 256-pixel runs than records: workgroups stride
        assert (2 * N * H * W + 255) // 256 > int(_dev.lib().raft_flow_visibility_workspace_doubles())
    for key, m, apply in (('plain', None, 1), ('mask', mask, 1), ('count', mask, 0)):
        want_vis, want_frac = want['vis', key]
        vis, intact, frac = _range_visibility(flows, N, m, 0.5, apply)
        np.testing.assert_array_equal(vis, want_vis)
        assert intact
        assert _bits(frac) == _bits(want_frac), (frac, want_frac)
        vis0, intact0, frac0 = _range_visibility(flows, N, m, 0.5, apply, want_visible=False)      # visible = NULL: the same share
        assert intact0 and (vis0 == FILL).all() and _bits(frac0) == _bits(frac)
    for _ in range(5):
        vis2, _, frac2 = _range_visibility(flows, N, mask, 0.5, 0)
        np.testing.assert_array_equal(vis2, vis)
        assert _bits(frac2) == _bits(frac)
    v3, f3 = image_ops.range_visibility_launch(flows, N, mask, 0.5, apply=True)
    np.testing.assert_array_equal(_np(v3), want['vis', 'mask'][0])
    assert _bits(_np(f3)) == _bits(want['vis', 'mask'][1])
    v4, f4 = image_ops.range_visibility_launch(flows, N, want_visible=False)
    assert v4 is None and _bits(_np(f4)) == _bits(want['vis', 'plain'][1])
    report(f'range visibility {shape}', occluded_fraction=float(frac))


# ------------------------------------------------------------------ the predictor
def _frames(seed, B, H, W):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32), rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32)


def _plain(t):
    return t.detach().as_subclass(torch.Tensor)


@pytest.mark.parametrize('route', ['plain', 'resize'])
def test_the_predictor_takes_its_masks_from_the_range_map_on_the_returned_flows(route):
    import tf_raft_amd
    from tf_raft_amd import image_ops
    from tf_raft_amd import weights as wm
    wts = wm.init_weights('small', seed=6, perturb=True)
    if route == 'plain':
        model, (B, H, W) = tf_raft_amd.SmallRAFT(weights=wts, iters_pred=3), (2, 64, 96)
    else:
        model, (B, H, W) = tf_raft_amd.SmallRAFT(weights=wts, iters_pred=3, target_size=(64, 96), fit='resize'), (2, 100, 150)
    i1, i2 = _frames(60, B, H, W)
    default = model.predict_step_bidirectional((i1, i2))
    for t, res in ((0.5, model.predict_step_bidirectional((i1, i2), occlusion_test='range')),
                   (0.9, model.predict_step_bidirectional((i1, i2), occlusion_test='range', range_threshold=0.9))):
        assert tuple(res.forward.shape) == (B, H, W, 2) and tuple(res.occluded_forward.shape) == (B, H, W)
        assert res.occluded_forward.dtype == torch.uint8
        occ_f, occ_b = image_ops.range_occlusion(res.forward, res.backward, t)
        assert torch.equal(_plain(res.occluded_forward), _plain(occ_f)) and torch.equal(_plain(res.occluded_backward), _plain(occ_b))
        assert torch.equal(_plain(res.forward), _plain(default.forward)) and torch.equal(_plain(res.backward), _plain(default.backward))
        np.testing.assert_array_equal(_np(occ_f), np_range_occlusion(_np(res.forward), _np(res.backward), t))
    # the default call and the spelled-out one: today's consistency masks
    occ_f, occ_b = image_ops.flow_consistency(default.forward, default.backward)
    spelled = model.predict_step_bidirectional((i1, i2), occlusion_test='consistency')
    for r in (default, spelled):
        assert torch.equal(_plain(r.occluded_forward), _plain(occ_f)) and torch.equal(_plain(r.occluded_backward), _plain(occ_b))
    if route == 'plain':
        got = model.predict_bidirectional([i1, i2], batch_size=1, occlusion_test='range', range_threshold=0.9)
        np.testing.assert_array_equal(got.occluded_forward, _np(res.occluded_forward))
        np.testing.assert_array_equal(got.occluded_backward, _np(res.occluded_backward))
    report(f'predictor range masks ({route})', occluded_forward=float(_np(res.occluded_forward).mean()),
           consistency_forward=float(_np(occ_f).mean()))


# ------------------------------------------------------------------ the training step
def _update_errors(want_w, new_w, wts, lr):
    total, bad, num, den = 0, 0, 0.0, 0.0
    for k, ref in want_w.items():
        upd_ref = ref - wts[k].astype(np.float64)
        upd_got = new_w[k].astype(np.float64) - wts[k].astype(np.float64)
        total += upd_ref.size
        bad += int((np.abs(upd_got - upd_ref) > 0.25 * lr).sum())
        num += float(((upd_got - upd_ref) ** 2).sum())
        den += float((upd_ref ** 2).sum())
    return bad / total, float(np.sqrt(num / den))


def test_the_update_block_step_with_the_range_mask_matches_the_oracle(monkeypatch):
    """One step at (1, 64, 96) -- the loop runs at batch 2 --, iters = 3, conditioned weights, trainable='update_block', cyclical
    learning rate + AdamW + clip 1.0, a user mask pair, ``occlusion_test='range'``.  The mask is the restatement on the flows the
    step handed to its launch, bit for bit; section 20's oracle takes the device's mask as the constant of its loss.  Bounds:
    tests/test_gpu_bidirectional_step.py::test_the_update_block_step_matches_the_oracle_on_the_doubled_batch."""
    import tf_raft_amd
    from tf_raft_amd import image_ops, losses, training
    wts, batches = oracle_case()
    batches = batches[:1]
    N, H, W = batches[0][0].shape[:3]
    sched = oracle_schedule()
    model = tf_raft_amd.RAFT(weights=wts, iters=ORACLE_ITERS, iters_pred=4)
    model.compile(optimizer=training.AdamW(ORACLE_WD, sched), clip_norm=ORACLE_CLIP, loss=losses.PhotometricSequenceLoss(**DEFAULTS),
                  trainable='update_block', bidirectional=True, occlusion=True, occlusion_test='range')
    seen = []
    launch = image_ops.range_visibility_launch
    monkeypatch.setattr(image_ops, 'range_visibility_launch', lambda flows, *a, **k: (seen.append(flows.clone()), launch(flows, *a, **k))[1])
    monkeypatch.setattr(image_ops, 'flow_visibility_launch', None)           # (the consistency launch is not what runs)
    res = model.train_step(batches[0])
    assert list(res) == ['loss', 'photometric', 'smoothness', 'occluded']
    got_loss, occluded = float(res['loss']), np.float32(float(res['occluded']))
    assert tuple(model.last_visibility.shape) == (2 * N, H, W) and model.last_visibility.dtype == torch.uint8
    mask = _np(model.last_visibility).copy()
    assert len(seen) == 1 and tuple(seen[0].shape) == (2 * N, H, W, 2)       # one launch, on preds[-1]
    user = np.concatenate(batches[0][2])
    want_vis, want_share, occ = np_range_visibility(_np(seen[0]), N, user, image_ops.RANGE_THRESHOLD, True)
    np.testing.assert_array_equal(mask, want_vis)                            # bit for bit
    assert _bits(occluded) == _bits(want_share), (occluded, want_share)
    assert occ.any() and not occ.all()
    want_losses, want_w, _, _ = reference_bidirectional_train_steps(wts, batches, ORACLE_ITERS, sched, ORACLE_WD, ORACLE_CLIP, 1, DEFAULTS,
                                                                    0.0, 1.4, loss_masks=[mask])
    report('range update-block step', occluded=float(occluded), visible_share=float(mask.mean()), got_loss=got_loss, want_loss=want_losses[0])
    np.testing.assert_allclose([got_loss], want_losses, rtol=1e-4)
    new_w = model.get_weights_dict()
    assert all(np.abs(ref - wts[k].astype(np.float64)).max() > 0 for k, ref in want_w.items())
    for k, v in wts.items():
        if not k.startswith('update_block'):
            np.testing.assert_array_equal(new_w[k], v)                        # frozen encoders, bit for bit
    frac, rel = _update_errors(want_w, new_w, wts, ORACLE_LR0)
    report('range update-block updated weights', frac_elements_off_by_quarter_lr=frac, rel_l2_of_update=rel)
    assert frac <= 0.02
    assert rel <= 0.1


def test_the_default_step_is_bit_for_bit_the_consistency_step_spelled_out(rng):
    import tf_raft_amd
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    N, H, W = 1, 64, 96
    wts = wm.condition_weights('raft', wm.init_weights('raft', seed=5))
    i1 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
    i2 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
    results = []
    for kw in ({}, {'occlusion_test': 'consistency'}, {'occlusion_test': 'range'}):
        model = tf_raft_amd.RAFT(weights=wts, iters=2, iters_pred=2)
        model.compile(optimizer=training.AdamW(1e-4, 4e-4), clip_norm=1.0, loss=losses.PhotometricSequenceLoss(), trainable='update_block',
                      bidirectional=True, alpha=0.0, beta=0.55, **kw)
        res = model.train_step((i1, i2))
        assert list(res) == ['loss', 'photometric', 'smoothness', 'occluded']
        results.append((losses.to_floats(res), _np(model.last_visibility).copy(), model.get_weights_dict()))
    assert results[0][0] == results[1][0]
    np.testing.assert_array_equal(results[0][1], results[1][1])
    for k in results[0][2]:
        np.testing.assert_array_equal(results[0][2][k], results[1][2][k])
    assert (results[2][1] != results[0][1]).any()                             # ... and 'range' is another mask

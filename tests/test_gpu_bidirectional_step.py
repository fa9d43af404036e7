"""Bidirectional training step with in-step occlusion masks on the GPU: the visibility launch against the
existing consistency kernel bit for bit, the mirror functions, the update-block and the full-model step against the float64
oracle on the doubled batch within the bounds of the unidirectional tests, the other configurations, and the unchanged default.
The restatements, the oracle and the derivation of its ``beta`` are in tests/test_bidirectional_step.py.
"""
import numpy as np
import pytest
import torch

from conftest import report
from test_bidirectional_step import (ORACLE_ALPHA, ORACLE_BETA, ORACLE_CLIP, ORACLE_ITERS, ORACLE_LR0, ORACLE_STEPS, ORACLE_WD,
                                     np_flow_visibility, oracle_case, oracle_schedule,
                                     reference_bidirectional_train_steps, visibility_flows)
from test_photometric_loss import DEFAULTS, torch_photometric_loss

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy()


# ------------------------------------------------------------------ the visibility entry
GUARD, FILL = 64, 0xAB


def _visibility(flows, N, mask, alpha, beta, apply, want_visible=True):
    """raft_flow_visibility_f32 through the library itself, ``visible`` inside a buffer with guard bands: (visible, guard bytes
    intact, the fraction's float32)."""
    from tf_raft_amd import _dev, losses
    from tf_raft_amd._ffi import check
    lib = _dev.lib()
    B, H, W, _ = flows.shape
    buf = torch.full((GUARD + B * H * W + GUARD,), FILL, dtype=torch.uint8, device=flows.device)
    vis = buf[GUARD:GUARD + B * H * W]
    frac = torch.full((3,), -7.0, dtype=torch.float32, device=flows.device)
    ws = losses._workspace(flows.device, 8 * int(lib.raft_flow_visibility_workspace_doubles()))
    check(lib.raft_flow_visibility_f32(_dev.ptr(flows), _dev.ptr(mask) if mask is not None else None,
                                       _dev.ptr(vis) if want_visible else None, _dev.ptr(frac[1:]), N, H, W, alpha, beta, int(apply),
                                       _dev.ptr(ws), _dev.stream_ptr()), 'flow_visibility')
    torch.cuda.synchronize()
    buf, frac = buf.cpu().numpy(), frac.cpu().numpy()
    assert frac[0] == -7.0 and frac[2] == -7.0                               # one float is written
    intact = bool((buf[:GUARD] == FILL).all() and (buf[-GUARD:] == FILL).all())
    return buf[GUARD:-GUARD].reshape(B, H, W), intact, frac[1]


@pytest.mark.parametrize('apply', [0, 1], ids=['count', 'apply'])
@pytest.mark.parametrize('with_mask', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('shape', [(1, 3, 1), (1, 5, 7), (2, 37, 53)], ids=['1x3x1', '1x5x7', '2x37x53'])
def test_visibility_is_the_consistency_kernel_inverted_masked_and_counted(shape, with_mask, apply):
    from tf_raft_amd import _dev, image_ops
    N, H, W = shape
    alpha, beta = 0.01, 0.5
    dev = _dev.require_gpu()
    host = visibility_flows(N, H, W, seed=H + W)
    flows = torch.from_numpy(host).to(dev)
    mask_h = (np.random.default_rng(7).uniform(size=(2 * N, H, W)) < 0.7).astype(np.uint8) * 5 if with_mask else None    # (nonzero = use)
    mask = torch.from_numpy(mask_h).to(dev) if with_mask else None
    occ_f, occ_b = image_ops.flow_consistency(flows[:N].contiguous(), flows[N:].contiguous(), alpha, beta)
    occ = np.concatenate([_np(occ_f), _np(occ_b)])
    assert occ.any() and not occ.all()
    use = mask_h != 0 if with_mask else np.ones(occ.shape, bool)
    want = (use & ((occ == 0) | (apply == 0))).astype(np.uint8)
    want_frac = np.float32(np.float64(int(occ.sum())) / np.float64(occ.size))
    vis, intact, frac = _visibility(flows, N, mask, alpha, beta, apply)
    np.testing.assert_array_equal(vis, want)                                  # bit for bit
    assert intact
    assert frac.view(np.uint32) == want_frac.view(np.uint32), (frac, want_frac)
    # visible = NULL: the same fraction, nothing written; a repeat: the same bits
    vis0, intact0, frac0 = _visibility(flows, N, mask, alpha, beta, apply, want_visible=False)
    assert intact0 and (vis0 == FILL).all() and frac0.view(np.uint32) == frac.view(np.uint32)
    vis2, _, frac2 = _visibility(flows, N, mask, alpha, beta, apply)
    np.testing.assert_array_equal(vis2, vis)
    assert frac2.view(np.uint32) == frac.view(np.uint32)
    # the public launch gives the same, and the restatement agrees off the rounding band (these flows leave nothing in it)
    v3, f3 = image_ops.flow_visibility_launch(flows, N, mask, alpha, beta, apply=bool(apply))
    np.testing.assert_array_equal(_np(v3), vis)
    assert _np(f3).view(np.uint32) == frac.view(np.uint32)
    np_vis, np_frac, _ = np_flow_visibility(host, N, mask_h, alpha, beta, apply)
    report(f'visibility {shape} mask={with_mask} apply={apply}', occluded_fraction=float(frac),
           pixels_differing_from_restatement=int((np_vis != vis).sum()))
    if vis.size >= 1000:
        assert (np_vis != vis).mean() <= 0.005                                # tests/test_gpu_consistency.py's share for the band


def test_visibility_strides_over_a_frame_larger_than_its_record_grid():
    """(2, 368, 496): more 256-pixel runs than records, so every workgroup walks several; still the consistency kernel's bits."""
    from tf_raft_amd import _dev, image_ops
    from test_consistency import parity_flows
    N, H, W = 2, 368, 496
    fwd, bwd = parity_flows(H, W, N, seed=3)
    flows = torch.from_numpy(np.concatenate([fwd, bwd])).to(_dev.require_gpu())
    occ_f, occ_b = image_ops.flow_consistency(flows[:N].contiguous(), flows[N:].contiguous())
    occ = np.concatenate([_np(occ_f), _np(occ_b)])
    assert (2 * N * H * W + 255) // 256 > int(_dev.lib().raft_flow_visibility_workspace_doubles())
    vis, frac = image_ops.flow_visibility_launch(flows, N)
    np.testing.assert_array_equal(_np(vis), (occ == 0).astype(np.uint8))
    assert _np(frac).view(np.uint32) == np.float32(np.float64(int(occ.sum())) / occ.size).view(np.uint32)


# ------------------------------------------------------------------ the mirror functions
def test_mirror_feature_maps_and_their_adjoint(rng):
    from tf_raft_amd import _dev, grad
    N, h, w, Cn = 2, 3, 5, 4
    dev = _dev.require_gpu()
    fout = torch.from_numpy(rng.normal(size=(2 * N, h, w, Cn)).astype(np.float32)).to(dev)
    f1, f2 = grad.mirror_feature_maps(fout, N)
    assert f1.is_contiguous() and f2.is_contiguous()
    np.testing.assert_array_equal(_np(f1), _np(fout))
    np.testing.assert_array_equal(_np(f2[:N]), _np(fout[N:]))
    np.testing.assert_array_equal(_np(f2[N:]), _np(fout[:N]))
    d1 = torch.from_numpy(rng.normal(size=(2 * N, h, w, Cn)).astype(np.float32)).to(dev)
    d2 = torch.from_numpy((rng.normal(size=(2 * N, h, w, Cn)) * 1e3).astype(np.float32)).to(dev)
    got = grad.mirror_feature_maps_backward(d1, d2, N)
    assert tuple(got.shape) == (2 * N, h, w, Cn) and got.dtype == torch.float32
    np.testing.assert_array_equal(_np(got[:N]), _np(d1[:N] + d2[N:]))         # one float32 addition: exact to compare
    np.testing.assert_array_equal(_np(got[N:]), _np(d1[N:] + d2[:N]))
    # <mirror(x), (d1, d2)> == <x, adjoint(d1, d2)>
    lhs = float((f1.double() * d1.double()).sum() + (f2.double() * d2.double()).sum())
    rhs = float((fout.double() * got.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(lhs))
    for bad in (fout[:3], fout[0]):
        with pytest.raises(ValueError, match='2N'):
            grad.mirror_feature_maps(bad, N)
    with pytest.raises(ValueError, match='2N'):
        grad.mirror_feature_maps_backward(d1, d2[:2], N)


# ------------------------------------------------------------------ the steps against the float64 oracle
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


def test_the_update_block_step_matches_the_oracle_on_the_doubled_batch():
    """Two steps at (1, 64, 96) -- the loop runs at batch 2 --, iters = 3, conditioned weights, trainable='update_block', cyclical
    learning rate + AdamW + clip 1.0: step 0 with a mask pair, step 1 with none, occlusion on.  The oracle's own float64 mask
    may differ from the device's on at most 1e-3 of the pixels; its loss then takes the device's mask as the constant.  Bounds:
    tests/test_gpu_photometric_loss.py::test_train_step_with_the_photometric_loss_matches_reference_semantics."""
    import tf_raft_amd
    from tf_raft_amd import losses, training
    wts, batches = oracle_case()
    N, H, W = batches[0][0].shape[:3]
    sched = oracle_schedule()
    model = tf_raft_amd.RAFT(weights=wts, iters=ORACLE_ITERS, iters_pred=4)
    model.compile(optimizer=training.AdamW(ORACLE_WD, sched), clip_norm=ORACLE_CLIP, loss=losses.PhotometricSequenceLoss(**DEFAULTS),
                  trainable='update_block', bidirectional=True, occlusion=True, alpha=ORACLE_ALPHA, beta=ORACLE_BETA)
    with pytest.raises(ValueError, match=r'\(image1, image2, \(mask1, mask2\)\)'):
        model.train_step((batches[0][0], batches[0][1], batches[0][2][0]))
    got_losses, masks, occluded = [], [], []
    for step in range(ORACLE_STEPS):
        model.reset_metrics()                                                 # (the means are then this step's values)
        res = model.train_step(batches[step])
        assert list(res) == ['loss', 'photometric', 'smoothness', 'occluded']
        got_losses.append(float(res['loss']))
        occluded.append(np.float32(float(res['occluded'])))
        assert tuple(model.last_visibility.shape) == (2 * N, H, W) and model.last_visibility.dtype == torch.uint8
        masks.append(_np(model.last_visibility).copy())
    want_losses, want_w, occ64, _ = reference_bidirectional_train_steps(wts, batches, ORACLE_ITERS, sched, ORACLE_WD, ORACLE_CLIP,
                                                                         ORACLE_STEPS, DEFAULTS, ORACLE_ALPHA, ORACLE_BETA, loss_masks=masks)
    for step in range(ORACLE_STEPS):
        user = np.concatenate(batches[step][2]) != 0 if len(batches[step]) == 3 else np.ones(masks[step].shape, bool)
        own = user & ~occ64[step]
        differ = float((own != (masks[step] != 0)).mean())
        report(f'bidirectional update-block step {step}', mask_disagreement=differ, oracle_occluded=float(occ64[step].mean()),
               got_loss=got_losses[step], want_loss=want_losses[step])
        assert differ <= 1e-3
    assert 0.2 <= float(occ64[0].mean()) <= 0.8
    # no user mask at step 1: the reported share is the complement of the kept mask, exactly
    want_share = np.float32(np.float64(int((masks[1] == 0).sum())) / np.float64(masks[1].size))
    assert occluded[1].view(np.uint32) == want_share.view(np.uint32), (occluded[1], want_share)
    np.testing.assert_allclose(got_losses, want_losses, rtol=1e-4)
    new_w = model.get_weights_dict()
    # (the unidirectional test also asks that the reference moved every tensor by 0.1 lr; here convf2's two Adam steps nearly
    # cancel in the oracle itself -- 3e-5 of movement -- which says nothing about the device, so that is not asked)
    assert all(np.abs(ref - wts[k].astype(np.float64)).max() > 0 for k, ref in want_w.items())
    for k, v in wts.items():
        if not k.startswith('update_block'):
            np.testing.assert_array_equal(new_w[k], v)                        # frozen encoders, bit for bit
    frac, rel = _update_errors(want_w, new_w, wts, ORACLE_LR0)
    report('bidirectional update-block updated weights', frac_elements_off_by_quarter_lr=frac, rel_l2_of_update=rel)
    assert frac <= 0.02
    assert rel <= 0.1


def test_the_full_step_matches_the_oracle_on_the_doubled_batch(rng):
    """One step at (2, 64, 96), iters = 2, ALL weights trainable, occlusion off, no masks, against ``oracle.RAFT(...)([i1 | i2,
    i2 | i1], training=True)`` in float64 under autograd with the yardstick loss (the procedure and the bounds of
    tests/test_gpu_backward.py::test_full_train_step_matches_reference_semantics).  The oracle's fnet sees every frame in both
    roles, so a wrong or missing half of the fnet gradient shows here."""
    import oracle
    import tf_raft_amd
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    N, H, W, iters = 2, 64, 96, 2
    wts = wm.condition_weights('raft', wm.init_weights('raft', seed=6, perturb=True))
    i1 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
    i2 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
    lr, wd, clip = 4e-4, 1e-4, 1.0
    a, b = np.concatenate([i1, i2]), np.concatenate([i2, i1])
    om = oracle.RAFT(wts, iters=iters, dtype=torch.float64)
    names = sorted(k for k in wts if 'moving' not in k)
    for k in names:
        om.w.t[k].requires_grad_(True)
    preds = om([a, b], training=True, return_numpy=False)
    assert len(preds) == iters and preds[-1].shape[0] == 2 * N
    loss = torch_photometric_loss(a, b, None, preds, **DEFAULTS)[0]
    loss.backward()
    g = {k: om.w.t[k].grad for k in names}
    gnorm = float(torch.sqrt(sum((v ** 2).sum() for v in g.values())))
    scale = clip / max(gnorm, clip)
    lr_t = lr * np.sqrt(1 - 0.999) / (1 - 0.9)
    want = {}
    for k in names:
        gk = g[k] * scale
        v0 = torch.tensor(wts[k], dtype=torch.float64)
        want[k] = ((v0 - wd * v0) - lr_t * (0.1 * gk) / (torch.sqrt(0.001 * gk * gk) + 1e-7)).numpy()
    model = tf_raft_amd.RAFT(weights=wts, iters=iters, iters_pred=3)
    model.compile(optimizer=training.AdamW(wd, lr), clip_norm=clip, loss=losses.PhotometricSequenceLoss(**DEFAULTS), bidirectional=True,
                  occlusion=False)
    res = model.train_step((i1, i2))
    assert list(res) == ['loss', 'photometric', 'smoothness', 'occluded']
    want_loss = float(loss.detach())
    report('bidirectional full train_step', loss=float(res['loss']), want_loss=want_loss, global_norm=gnorm, occluded=float(res['occluded']))
    np.testing.assert_allclose(float(res['loss']), want_loss, rtol=1e-4)
    assert _np(model.last_visibility).all()                                   # occlusion off, no masks: all ones
    new_w = model.get_weights_dict()
    frac, rel = _update_errors(want, new_w, wts, lr)
    fnet = {k: v for k, v in want.items() if k.startswith('fnet')}
    frac_f, rel_f = _update_errors(fnet, new_w, wts, lr)
    report('bidirectional full train_step updated weights', frac_elements_off_by_quarter_lr=frac, rel_l2_of_update=rel,
           fnet_frac=frac_f, fnet_rel_l2=rel_f)
    assert frac <= 2e-3
    assert rel <= 0.1
    moved = [k for k in wts if k.endswith('moving_mean') and not np.array_equal(new_w[k], wts[k])]
    assert len(moved) == 15                                                   # every batch-norm layer of cnet
    out = model([i1, i2])
    assert len(out) == 3 and np.isfinite(out[-1].numpy()).all()


# ------------------------------------------------------------------ other configurations and the unchanged default
@pytest.mark.parametrize('variant', ['small', 'raft_all_bf16_dropout', 'census_ssim'])
def test_one_bidirectional_step_of_the_other_configurations(rng, variant):
    """SmallRAFT; RAFT with all weights, the bf16 tape and dropout; a loss with the census and SSIM terms: finite positive terms,
    exactly the documented keys, moved weights, the kept mask.  With these weights the two directions disagree by pixels, so
    ``beta`` is the median of the float64 oracle's ``|f + s|^2`` on these inputs (58 for SmallRAFT, 12 for RAFT)."""
    import tf_raft_amd
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    N, H, W = 2, 64, 96
    keys = ['loss', 'photometric', 'smoothness', 'occluded']
    kind = 'small' if variant == 'small' else 'raft'
    wts = wm.condition_weights(kind, wm.init_weights(kind, seed=2, perturb=True), 'mid')
    opt = training.AdamW(1e-4, 1e-3)
    if variant == 'small':
        model = tf_raft_amd.SmallRAFT(weights=wts, iters=2, iters_pred=2)
        model.compile(optimizer=opt, clip_norm=1.0, loss=losses.PhotometricSequenceLoss(), bidirectional=True, alpha=0.0, beta=58.0)
    elif variant == 'raft_all_bf16_dropout':
        model = tf_raft_amd.RAFT(drop_rate=0.1, weights=wts, iters=2, iters_pred=2)
        model.compile(optimizer=opt, clip_norm=1.0, loss=losses.PhotometricSequenceLoss(), trainable='all', tape_dtype='bf16',
                      bidirectional=True, alpha=0.0, beta=12.0)
    else:
        model = tf_raft_amd.RAFT(weights=wts, iters=2, iters_pred=2)
        model.compile(optimizer=opt, clip_norm=1.0, loss=losses.SSIMSequenceLoss(census_weight=0.5, ssim_weight=0.5),
                      bidirectional=True, alpha=0.0, beta=12.0)
        keys = ['loss', 'photometric', 'census', 'ssim', 'smoothness', 'occluded']
    i1 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
    i2 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
    masks = (rng.uniform(size=(N, H, W)) < 0.8, rng.uniform(size=(N, H, W)) < 0.8)
    res = model.train_step((i1, i2, masks))
    assert list(res) == keys
    vals = losses.to_floats(res)
    assert all(np.isfinite(v) for v in vals.values()) and all(vals[k] > 0 for k in keys[:-1]) and 0.0 <= vals['occluded'] <= 1.0, vals
    vis = _np(model.last_visibility)
    assert vis.shape == (2 * N, H, W) and vis.dtype == np.uint8 and set(np.unique(vis)) <= {0, 1}
    assert not vis[~np.concatenate(masks)].any()                              # the user's masks are kept out
    new = model.get_weights_dict()
    assert all(not np.array_equal(new[k], wts[k]) for k in new if k.endswith('kernel'))
    assert 0.02 < vals['occluded'] < 0.98                                     # (beta: the float64 oracle's median of |f + s|^2 here)
    out = model([i1, i2])
    assert np.isfinite(_np(out[-1])).all()
    report(f'bidirectional train_step {variant}', visible_share=float(vis.mean()), **vals)


def test_occlusion_may_be_flipped_between_steps(rng, monkeypatch):
    """Off: ``last_visibility`` is all ones; on: it is the existing consistency kernel's verdict on the flows the step handed to
    its visibility launch (captured here); ``occluded`` is reported in both.  alpha = 0, beta = 0.55: between the two modes of
    the float64 oracle's ``|f + s|^2`` on these inputs (quartiles 0.35 / 0.75 / 0.80)."""
    import tf_raft_amd
    from tf_raft_amd import image_ops, losses, training
    from tf_raft_amd import weights as wm
    N, H, W = 1, 64, 96
    wts = wm.condition_weights('raft', wm.init_weights('raft', seed=5))
    i1 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
    i2 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)

    def fresh(occlusion):
        m = tf_raft_amd.RAFT(weights=wts, iters=2, iters_pred=2)
        m.compile(optimizer=training.AdamW(0.0, 0.0), clip_norm=1.0, loss=losses.PhotometricSequenceLoss(), trainable='update_block',
                  bidirectional=True, occlusion=occlusion, alpha=0.0, beta=0.55)
        return m
    seen = []
    launch = image_ops.flow_visibility_launch
    monkeypatch.setattr(image_ops, 'flow_visibility_launch', lambda flows, *a, **k: (seen.append(flows.clone()), launch(flows, *a, **k))[1])
    model = fresh(False)                                                      # (no decay, learning rate 0: both steps see the same weights)
    res0 = losses.to_floats(model.train_step((i1, i2)))
    assert _np(model.last_visibility).all() and 0.0 < res0['occluded'] < 1.0
    model.occlusion = True
    model.reset_metrics()
    res1 = losses.to_floats(model.train_step((i1, i2)))
    vis = _np(model.last_visibility)
    assert res1['occluded'] == res0['occluded']
    assert np.float32(res1['occluded']) == np.float32(np.float64(int((vis == 0).sum())) / vis.size)
    assert res1['photometric'] < res0['photometric']                          # fewer pixels in the same divisor
    assert len(seen) == 2 and tuple(seen[1].shape) == (2 * N, H, W, 2)        # one visibility launch per step, on preds[-1]
    occ_f, occ_b = image_ops.flow_consistency(seen[1][:N].contiguous(), seen[1][N:].contiguous(), 0.0, 0.55)
    np.testing.assert_array_equal(vis, (np.concatenate([_np(occ_f), _np(occ_b)]) == 0).astype(np.uint8))
    assert 0.2 < res1['occluded'] < 0.8


def test_the_default_step_is_bit_for_bit_what_bidirectional_false_gives(rng):
    import tf_raft_amd
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    N, H, W = 1, 64, 96
    wts = wm.condition_weights('raft', wm.init_weights('raft', seed=5))
    i1 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
    i2 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
    mask = rng.uniform(size=(N, H, W)) < 0.8
    results = []
    for kw in ({}, {'bidirectional': False}):
        model = tf_raft_amd.RAFT(weights=wts, iters=2, iters_pred=2)
        model.compile(optimizer=training.AdamW(1e-4, 4e-4), clip_norm=1.0, loss=losses.PhotometricSequenceLoss(), **kw)
        res = model.train_step((i1, i2, mask))
        assert list(res) == ['loss', 'photometric', 'smoothness'] and model.last_visibility is None
        results.append((losses.to_floats(res), model.get_weights_dict()))
    assert results[0][0] == results[1][0]
    for k in results[0][1]:
        np.testing.assert_array_equal(results[0][1][k], results[1][1][k])

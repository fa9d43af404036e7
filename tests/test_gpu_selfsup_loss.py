"""Self-supervision on the GPU: raft_selfsup_loss_f32 and the layers above it against the float64 yardstick
of tests/test_selfsup_loss.py, the entry's bit-for-bit properties, and the two-pass ``train_step`` against the float64 oracle.

Tolerances of the parity test, per case: four times the float32 restatement's own measured distance to the yardstick (the table in
tests/test_selfsup_loss.py), for the loss, the last distance and the gradient; the share of used pixels is exact.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import report
from test_gpu_bidirectional_step import _update_errors
from test_photometric_loss import DEFAULTS
from test_selfsup_loss import (CASE_IDS, CASES, ORACLE_ALPHA, ORACLE_BETA, ORACLE_CLIP, ORACLE_CROP, ORACLE_ITERS, ORACLE_LR0,
                               ORACLE_OCCLUSION, ORACLE_SELFSUP, ORACLE_STEPS, ORACLE_WD, PARAMS, SMALL, equal_case, np_selfsup_loss,
                               full_step_oracle, oracle_case, oracle_schedule, ramp_case, reference_selfsup_train_steps,
                               restatement_distance, selfsup_case, selfsup_yardstick, used_pixels)

pytestmark = pytest.mark.gpu

GUARD = 64
MID = (SMALL[2], 3, 'both')


def _np(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _yardstick(case):
    return selfsup_yardstick(case)


def _entry(data, upstream=1.0, add_to=None, alias=False, prefill=None, want_grad=True, gap=0, **params):
    """raft_selfsup_loss_f32 called directly on ``data = (teacher, tv, origin, sv, preds)``: ``(out3 float32 NumPy, d_preds
    (n, B, H, W, 2) or None, intact)``.  d_preds lies in a slab of NaN with ``GUARD`` floats around it and ``gap`` floats behind
    every prediction, out3 between two guard floats; ``intact`` says that all of those still hold what they were filled with.
    ``prefill`` (with accumulate = 1) fills d_preds before the call; ``alias``: add_to is out3 itself."""
    from tf_raft_amd import _dev, losses
    from tf_raft_amd._ffi import check
    teacher, tv, (oy, ox), sv, preds = data
    params = dict(PARAMS, **params)
    B, H, W, _ = preds[0].shape
    _, Ht, Wt, _ = teacher.shape
    n, npix = len(preds), B * H * W
    stride = 2 * npix + gap
    dev = _dev.require_gpu()
    up = lambda a: None if a is None else torch.tensor(np.array(a)).to(dev)
    te, tvd, svd = up(teacher), up(tv), up(sv)
    src = torch.zeros((n * stride,), dtype=torch.float32, device=dev)
    for i, p in enumerate(preds):
        src[i * stride:i * stride + 2 * npix] = up(p).reshape(-1)
    slab = torch.full((n * stride + 2 * GUARD,), float('nan'), dtype=torch.float32, device=dev)
    dst = slab[GUARD:GUARD + n * stride]
    if prefill is not None:
        dst.reshape(n, stride)[:, :2 * npix] = torch.tensor(prefill).to(dev).reshape(n, -1)
    outbuf = torch.full((5,), -7.0, dtype=torch.float32, device=dev)
    out = outbuf[1:4]
    add = None
    if alias:
        out[0] = float(add_to)
        add = out
    elif add_to is not None:
        add = torch.tensor([add_to], dtype=torch.float32, device=dev)
    lib = _dev.lib()
    ws = losses._workspace(dev, 8 * int(lib.raft_selfsup_loss_workspace_doubles()))
    ptr = lambda t: None if t is None else _dev.ptr(t)
    check(lib.raft_selfsup_loss_f32(ptr(te), ptr(tvd), Ht, Wt, oy, ox, ptr(svd), ptr(src), stride, n, B, H, W, params['gamma'],
                                    params['weight'], params['eps'], upstream, ptr(add), ptr(out), ptr(dst) if want_grad else None,
                                    0 if prefill is None else 1, ptr(ws), _dev.stream_ptr()), 'selfsup_loss')
    torch.cuda.synchronize()
    slab_h, out_h = _np(slab), _np(outbuf)
    body = slab_h[GUARD:-GUARD].reshape(n, stride)
    intact = bool(np.isnan(slab_h[:GUARD]).all() and np.isnan(slab_h[-GUARD:]).all() and np.isnan(body[:, 2 * npix:]).all()
                  and out_h[0] == -7.0 and out_h[4] == -7.0)
    if not want_grad:
        intact = intact and bool(np.isnan(body).all())
    d = body[:, :2 * npix].reshape(n, B, H, W, 2).copy() if want_grad else None
    return out_h[1:4].copy(), d, intact


def _rel(got, want):
    return abs(float(got) - want) / abs(want) if want else abs(float(got))


# ------------------------------------------------------------------ the entry against the yardstick
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_value_and_gradient_match_the_float64_yardstick(case):
    data = selfsup_case(case)
    want_loss, want_last, want_share, want_g = _yardstick(case)
    base_loss, base_last, base_g, max_g = restatement_distance(case)
    out3, d, intact = _entry(data)
    assert intact
    rel, rel_last = _rel(out3[0], want_loss), _rel(out3[1], want_last)
    diff = max(float(np.abs(d[i].astype(np.float64) - g).max()) for i, g in enumerate(want_g))
    own3, own_d = np_selfsup_loss(*data, **PARAMS)
    report(f'selfsup {CASE_IDS[CASES.index(case)]}', base_loss_rel=base_loss, loss_rel=rel, base_last_rel=base_last, last_rel=rel_last,
           base_grad=base_g, grad=diff, grad_over_max=diff / max_g, used=float(out3[2]),
           gradient_elements_differing_from_restatement=int((own_d.view(np.uint32) != d.view(np.uint32)).sum()))
    assert rel <= 4 * base_loss
    assert rel_last <= 4 * base_last
    assert diff <= 4 * base_g
    assert out3[2].view(np.uint32) == np.float32(want_share).view(np.uint32)            # exact
    assert not d[:, ~used_pixels(*data[:4], d.shape[1:4])].any()                          # exactly 0 where a pixel is not used
    # the Python layers launch the same: the same bits
    from tf_raft_amd import grad, losses
    teacher, tv, origin, sv, preds = data
    terms, grads = grad.selfsup_loss_value_and_grad(teacher, preds, origin, tv, sv, **PARAMS)
    assert list(terms) == ['loss', 'selfsup', 'selfsup_used']
    assert [_np(terms[k]).view(np.uint32) for k in terms] == [v.view(np.uint32) for v in out3]
    for i, g in enumerate(grads):
        np.testing.assert_array_equal(_np(g), d[i])
    only = losses.SelfSupervisionLoss(**PARAMS).terms(teacher, preds, origin, tv, sv)
    assert [_np(only[k]).view(np.uint32) for k in only] == [v.view(np.uint32) for v in out3]


def test_upstream_and_weight_scale_the_gradient_and_add_to_joins_the_loss():
    data = selfsup_case(MID)
    want = selfsup_yardstick(MID, upstream=-2.5, add_to=1.75, weight=0.7)
    base = restatement_distance(MID)
    out3, d, intact = _entry(data, upstream=-2.5, add_to=1.75, weight=0.7)
    own3, own_d = np_selfsup_loss(*data, **dict(PARAMS, weight=0.7), upstream=-2.5, add_to=1.75)
    assert intact
    own_rel = _rel(own3[0], want[0])
    diff = max(float(np.abs(d[i].astype(np.float64) - g).max()) for i, g in enumerate(want[3]))
    own_diff = max(float(np.abs(own_d[i].astype(np.float64) - g).max()) for i, g in enumerate(want[3]))
    report('selfsup upstream -2.5 weight 0.7 add_to 1.75', base_loss_rel=own_rel, loss_rel=_rel(out3[0], want[0]), base_grad=own_diff, grad=diff)
    assert _rel(out3[0], want[0]) <= 4 * own_rel
    assert diff <= 4 * own_diff
    assert _rel(out3[1], want[1]) <= 4 * base[1]


# ------------------------------------------------------------------ the entry bit for bit
def test_guard_bands_gaps_accumulate_value_only_aliasing_and_repeats():
    data = selfsup_case(MID)
    n, (B, H, W) = MID[1], MID[0][0]
    out3, d, intact = _entry(data)
    assert intact
    # a gapped pred_stride (even): the gaps, prefilled with NaN, stay; the values do not change
    out_g, d_g, intact_g = _entry(data, gap=6)
    assert intact_g and out_g.tobytes() == out3.tobytes()
    np.testing.assert_array_equal(d_g, d)
    # accumulate = 1 on a prefilled buffer (negative zeros and a huge value included) = store, then ONE float32 addition
    rng = np.random.default_rng(9)
    prefill = rng.normal(0, 1e-4, d.shape).astype(np.float32)
    prefill[:, 0, :3] = -0.0
    prefill[:, -1, -1, -1] = 3e38
    out_a, d_a, intact_a = _entry(data, prefill=prefill, gap=2)
    assert intact_a and out_a.tobytes() == out3.tobytes()
    np.testing.assert_array_equal(d_a.view(np.uint32), (prefill + d).view(np.uint32))
    # value only: nothing of d_preds is written, the same value bits
    out_v, d_v, intact_v = _entry(data, want_grad=False)
    assert intact_v and d_v is None and out_v.tobytes() == out3.tobytes()
    # add_to in its own scalar and aliasing out3: the same bits, the other two values unchanged
    out_s, _, _ = _entry(data, add_to=0.625)
    out_i, d_i, intact_i = _entry(data, add_to=0.625, alias=True)
    assert intact_i and out_i.tobytes() == out_s.tobytes() and out_i[1:].tobytes() == out3[1:].tobytes()
    np.testing.assert_array_equal(d_i, d)
    # repeats
    for _ in range(2):
        out_r, d_r, _ = _entry(data)
        assert out_r.tobytes() == out3.tobytes()
        np.testing.assert_array_equal(d_r.view(np.uint32), d.view(np.uint32))


def test_known_answers_on_the_device():
    root = np.sqrt(np.float32(PARAMS['eps']) * np.float32(PARAMS['eps']))
    teacher, tv, origin, preds, share = equal_case()
    out3, d, intact = _entry((teacher, tv, origin, None, preds))
    assert intact and not d.any()                                              # the gradient is exactly 0
    assert out3[2] == np.float32(share)
    np.testing.assert_allclose(out3[1], float(root) * share, rtol=2e-7)
    np.testing.assert_allclose(out3[0], float(np.float32(0.3)) * 1.8 * float(root) * share, rtol=3e-7)
    moved = [p + np.float32(0.5) for p in preds]
    for tv0, sv0 in ((np.zeros(teacher.shape[:3], np.uint8), None), (None, np.full(preds[0].shape[:3], 3, np.uint8))):
        out3, d, intact = _entry((teacher, tv0, origin, sv0, moved), add_to=None)
        assert intact and out3.tolist() == [0.0, 0.0, 0.0] and not d.any()
    teacher, origin, preds, want = ramp_case()
    out3, d, intact = _entry((teacher, None, origin, None, preds), weight=1.0)
    assert intact and out3[2] == 1.0
    np.testing.assert_allclose(out3[1], want, rtol=2e-7)
    np.testing.assert_allclose(out3[0], want, rtol=2e-7)
    assert (np.sign(d[0, 0, 0, :, 0]) == np.sign(7.25 - 5 - np.arange(6))).all()


# ------------------------------------------------------------------ the update-block steps against the float64 oracle
@pytest.mark.parametrize('mode', ['teacher', 'occluded'])
def test_the_update_block_steps_match_the_two_pass_oracle(mode):
    """Two steps at N = 1, frames 80 x 112, selfsup_crop = (8, 8) (student 64 x 96), iters = 3, conditioned weights,
    trainable='update_block', cyclical learning rate + AdamW + clip 1.0; step 0 with a mask pair, step 1 with none.  The oracle
    (tests/test_selfsup_loss.py) differentiates loss1 + weight * selfsup(student, teacher.detach()) in float64; its own masks may
    differ from the device's on at most 1e-3 of the pixels, and its losses take the device's as constants.  Bounds: those of
    tests/test_gpu_photometric_loss.py::test_train_step_with_the_photometric_loss_matches_reference_semantics, with no element
    of the update off by 0.25 lr.

    Measured (MI355X): see DESIGN.md section 22."""
    import tf_raft_amd
    from tf_raft_amd import losses, training
    wts, batches = oracle_case()
    N, H, W = batches[0][0].shape[:3]
    cy, cx = ORACLE_CROP
    sched = oracle_schedule()
    model = tf_raft_amd.RAFT(weights=wts, iters=ORACLE_ITERS, iters_pred=4)
    model.compile(optimizer=training.AdamW(ORACLE_WD, sched), clip_norm=ORACLE_CLIP, loss=losses.PhotometricSequenceLoss(**DEFAULTS),
                  trainable='update_block', bidirectional=True, occlusion=ORACLE_OCCLUSION[0], alpha=ORACLE_ALPHA, beta=ORACLE_BETA,
                  selfsup_crop=ORACLE_CROP, selfsup_mask=mode, **{'selfsup_' + k: v for k, v in ORACLE_SELFSUP.items()})
    got, masks1, masks2 = [], [], []
    for step in range(ORACLE_STEPS):
        model.occlusion = ORACLE_OCCLUSION[step]
        model.reset_metrics()                                                 # (the means are then this step's values)
        res = model.train_step(batches[step])
        assert list(res) == ['loss', 'photometric', 'smoothness', 'occluded', 'selfsup', 'selfsup_used']
        got.append(losses.to_floats(res))
        assert tuple(model.last_visibility.shape) == (2 * N, H, W)
        masks1.append(_np(model.last_visibility).copy())
        if mode == 'occluded':
            sv = model.last_student_visibility
            assert tuple(sv.shape) == (2 * N, H - 2 * cy, W - 2 * cx) and sv.dtype == torch.uint8
            masks2.append(_np(sv).copy())
        else:
            assert model.last_student_visibility is None
    want_losses, parts, want_w, occ1, occ2, _, _ = reference_selfsup_train_steps(
        wts, batches, ORACLE_ITERS, sched, ORACLE_WD, ORACLE_CLIP, ORACLE_STEPS, DEFAULTS, ORACLE_ALPHA, ORACLE_BETA, ORACLE_CROP,
        ORACLE_SELFSUP, mode, teacher_masks=masks1, student_masks=masks2 if mode == 'occluded' else None, occlusion=ORACLE_OCCLUSION)
    for step in range(ORACLE_STEPS):
        user = np.concatenate(batches[step][2]) != 0 if len(batches[step]) == 3 else np.ones(masks1[step].shape, bool)
        own1 = user & ~(occ1[step] & ORACLE_OCCLUSION[step])
        differ1 = float((own1 != (masks1[step] != 0)).mean())
        differ2 = float(((~occ2[step]) != (masks2[step] != 0)).mean()) if mode == 'occluded' else 0.0
        # the reported share of occluded pixels is the device's count of the teacher pass, whatever model.occlusion is
        differ_occ = abs(got[step]['occluded'] - float(occ1[step].mean()))
        report(f'selfsup update-block step {step} mask={mode}', teacher_mask_disagreement=differ1, student_mask_disagreement=differ2,
               oracle_occluded_teacher=float(occ1[step].mean()), oracle_occluded_student=float(occ2[step].mean()),
               got_loss=got[step]['loss'], want_loss=want_losses[step], got_selfsup=got[step]['selfsup'], want_selfsup=parts[step][1],
               got_used=got[step]['selfsup_used'], want_used=parts[step][2])
        assert differ1 <= 1e-3 and differ2 <= 1e-3 and differ_occ <= 1e-3
        assert np.float32(got[step]['selfsup_used']) == np.float32(parts[step][2])      # (the oracle's count is over the device's masks)
    assert 0.2 <= float(occ1[0].mean()) <= 0.8 and 0.2 <= float(occ2[0].mean()) <= 0.8
    np.testing.assert_allclose([g['loss'] for g in got], want_losses, rtol=1e-4)
    np.testing.assert_allclose([g['selfsup'] for g in got], [p[1] for p in parts], rtol=1e-4)
    new_w = model.get_weights_dict()
    assert all(np.abs(ref - wts[k].astype(np.float64)).max() > 0 for k, ref in want_w.items())
    for k, v in wts.items():
        if not k.startswith('update_block'):
            np.testing.assert_array_equal(new_w[k], v)                        # frozen encoders, bit for bit
    frac, rel = _update_errors(want_w, new_w, wts, ORACLE_LR0)
    report(f'selfsup update-block updated weights mask={mode}', frac_elements_off_by_quarter_lr=frac, rel_l2_of_update=rel)
    assert frac == 0.0
    assert rel <= 0.1


# ------------------------------------------------------------------ the full step against oracle.RAFT
def test_the_full_step_matches_the_oracle_with_two_updates_of_the_moving_statistics():
    """One step at (2, 80, 112), crop (8, 8), iters = 2, ALL weights trainable, occlusion off, no masks, against ``oracle.RAFT`` run
    twice in float64 under autograd -- on the doubled batch of the frames and on the doubled batch of their centre crops -- with
    the yardstick losses (the procedure and the bounds of tests/test_gpu_bidirectional_step.py's full step).  The batch-norm
    layers' moving statistics must hold TWO updates, with the first pass's batch statistics and then the second's.  Their bound:
    a moving value is 0.9801 of the old one plus 0.0099 / 0.01 of two batch statistics; those are means over float32 activations
    whose relative error through the 15 layers of cnet stays below 1e-3 here, so the sum is within 2e-5 of the statistics'
    magnitude -- rtol 1e-4 on the moving value plus atol 2e-5.  ONE update, or the second pass's statistics taken twice, would
    be off by 1e-2 of the difference between the statistics (tests/test_selfsup_loss.py checks that this is at least ten times
    the bound in every tensor)."""
    import tf_raft_amd
    from tf_raft_amd import losses, training
    wts, (i1, i2), (cy, cx), iters, (lr, wd, clip), want, moving, once, scalars = full_step_oracle()
    want_loss, loss1, dist, share, gnorm = scalars
    model = tf_raft_amd.RAFT(weights=wts, iters=iters, iters_pred=3)
    model.compile(optimizer=training.AdamW(wd, lr), clip_norm=clip, loss=losses.PhotometricSequenceLoss(**DEFAULTS), bidirectional=True,
                  occlusion=False, selfsup_crop=(cy, cx), **{'selfsup_' + k: v for k, v in ORACLE_SELFSUP.items()})
    res = losses.to_floats(model.train_step((i1, i2)))
    assert list(res) == ['loss', 'photometric', 'smoothness', 'occluded', 'selfsup', 'selfsup_used']
    report('selfsup full train_step', loss=res['loss'], want_loss=want_loss, loss1=loss1, selfsup=res['selfsup'], want_selfsup=dist,
           global_norm=gnorm)
    np.testing.assert_allclose(res['loss'], want_loss, rtol=1e-4)
    np.testing.assert_allclose(res['selfsup'], dist, rtol=1e-4)
    assert res['selfsup_used'] == 1.0 and share == 1.0
    new_w = model.get_weights_dict()
    frac, rel = _update_errors(want, new_w, wts, lr)
    frac_f, rel_f = _update_errors({k: v for k, v in want.items() if k.startswith('fnet')}, new_w, wts, lr)
    report('selfsup full train_step updated weights', frac_elements_off_by_quarter_lr=frac, rel_l2_of_update=rel, fnet_frac=frac_f,
           fnet_rel_l2=rel_f)
    assert frac <= 2e-3
    assert rel <= 0.1
    worst = 0.0
    for k, ref in moving.items():
        worst = max(worst, float(np.abs(new_w[k] - ref).max()))
    report('selfsup full train_step moving statistics', largest_difference=worst)
    for k, ref in moving.items():
        np.testing.assert_allclose(new_w[k], ref, rtol=1e-4, atol=2e-5, err_msg=k)
    out = model([i1, i2])
    assert len(out) == 3 and np.isfinite(out[-1].numpy()).all()


# ------------------------------------------------------------------ other configurations
@pytest.mark.parametrize('variant', ['small', 'raft_all_dropout', 'raft_all_bf16'])
def test_one_two_pass_step_of_the_other_configurations(rng, variant):
    """SmallRAFT; RAFT with all weights and dropout; RAFT with all weights and the bf16 tape: exactly the documented keys, finite
    positive terms, moved weights, both kept masks.  ``beta`` as in tests/test_gpu_bidirectional_step.py's counterpart."""
    import tf_raft_amd
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    N, H, W, crop = 2, 80, 112, (8, 8)
    kind = 'small' if variant == 'small' else 'raft'
    wts = wm.condition_weights(kind, wm.init_weights(kind, seed=2, perturb=True), 'mid')
    common = dict(optimizer=training.AdamW(1e-4, 1e-3), clip_norm=1.0, loss=losses.PhotometricSequenceLoss(), bidirectional=True,
                  occlusion=False, alpha=0.0, selfsup_crop=crop, selfsup_mask='occluded')
    if variant == 'small':
        model = tf_raft_amd.SmallRAFT(weights=wts, iters=2, iters_pred=2)
        model.compile(beta=58.0, **common)
    elif variant == 'raft_all_dropout':
        model = tf_raft_amd.RAFT(drop_rate=0.1, weights=wts, iters=2, iters_pred=2)
        model.compile(beta=12.0, trainable='all', **common)
    else:
        model = tf_raft_amd.RAFT(weights=wts, iters=2, iters_pred=2)
        model.compile(beta=12.0, trainable='all', tape_dtype='bf16', **common)
    i1 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
    i2 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
    res = model.train_step((i1, i2))
    assert list(res) == ['loss', 'photometric', 'smoothness', 'occluded', 'selfsup', 'selfsup_used']
    vals = losses.to_floats(res)
    assert all(np.isfinite(v) for v in vals.values()) and all(vals[k] > 0 for k in ('loss', 'photometric', 'smoothness', 'selfsup')), vals
    sv = _np(model.last_student_visibility)
    assert sv.shape == (2 * N, H - 16, W - 16) and set(np.unique(sv)) <= {0, 1}
    assert np.float32(vals['selfsup_used']) == np.float32(np.float64(int((sv == 0).sum())) / sv.size)     # teacher mask all ones, finite flows
    assert 0.02 < vals['selfsup_used'] < 0.98
    assert _np(model.last_visibility).shape == (2 * N, H, W)
    new = model.get_weights_dict()
    assert all(not np.array_equal(new[k], wts[k]) for k in new if k.endswith('kernel'))
    out = model([i1, i2])
    assert np.isfinite(_np(out[-1])).all()
    report(f'selfsup train_step {variant}', **vals)


def _pair(rng, N=1, H=80, W=112):
    return rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32), rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)


def _model(wts, **kw):
    import tf_raft_amd
    from tf_raft_amd import losses, training
    m = tf_raft_amd.RAFT(weights=wts, iters=2, iters_pred=2)
    m.compile(optimizer=training.AdamW(1e-4, 4e-4), clip_norm=1.0, loss=losses.PhotometricSequenceLoss(), bidirectional=True,
              alpha=0.0, beta=0.55, **kw)
    return m


def test_weight_zero_is_the_step_without_the_option_bit_for_bit(rng):
    """Two steps, all weights: a model with ``selfsup_weight = 0`` against a model compiled without ``selfsup_crop`` -- the same
    terms and the same weights bit for bit, and nothing fed to the ``selfsup`` means."""
    from tf_raft_amd import losses
    from tf_raft_amd import weights as wm
    wts = wm.condition_weights('raft', wm.init_weights('raft', seed=5))
    batches = [_pair(rng), _pair(rng)]
    plain, zero = _model(wts), _model(wts, selfsup_crop=(8, 8), selfsup_weight=0.0)
    for batch in batches:
        a, b = losses.to_floats(plain.train_step(batch)), losses.to_floats(zero.train_step(batch))
        assert list(a) == ['loss', 'photometric', 'smoothness', 'occluded']
        assert list(b) == list(a) + ['selfsup', 'selfsup_used'] and (b['selfsup'], b['selfsup_used']) == (0.0, 0.0)
        assert all(a[k] == b[k] for k in a)
        assert zero.last_student_visibility is None
    assert zero.flow_metrics['selfsup'].count == 0 and zero.flow_metrics['selfsup_used'].count == 0
    assert zero.flow_metrics['loss'].count == 2
    wa, wb = plain.get_weights_dict(), zero.get_weights_dict()
    for k in wa:
        np.testing.assert_array_equal(wa[k], wb[k], err_msg=k)


def test_the_weight_may_be_changed_between_steps(rng):
    """0 -> 0.3 -> 0: the middle step runs the student pass (its means are fed once, the loss grows by weight * the weighted
    distances), the outer ones do not; a model that never ran it ends with other weights."""
    from tf_raft_amd import losses
    from tf_raft_amd import weights as wm
    wts = wm.condition_weights('raft', wm.init_weights('raft', seed=5))
    batch = _pair(rng)
    # (occlusion off: with these weights the teacher's own test passes only in the outer ring that the crop removes)
    model = _model(wts, trainable='update_block', occlusion=False, selfsup_crop=(8, 8), selfsup_weight=0.0)
    plain = _model(wts, trainable='update_block', occlusion=False)
    counts = []
    for weight in (0.0, 0.3, 0.0):
        model.selfsup_weight = weight
        model.reset_metrics()
        res = losses.to_floats(model.train_step(batch))
        ref = losses.to_floats((plain.reset_metrics(), plain.train_step(batch))[1])
        counts.append(model.flow_metrics['selfsup'].count)
        if weight == 0.0 and len(counts) == 1:
            assert all(res[k] == ref[k] for k in ref)
        if weight > 0:
            assert res['selfsup'] > 0 and 0 < res['selfsup_used'] <= 1
            assert res['loss'] >= ref['loss'] + weight * res['selfsup'] * (1 - 1e-5)    # (the last prediction's share alone)
    assert counts == [0, 1, 0]
    wa, wb = model.get_weights_dict(), plain.get_weights_dict()
    assert any(not np.array_equal(wa[k], wb[k]) for k in wa if k.startswith('update_block'))
    with pytest.raises(ValueError, match='weight'):
        model.selfsup_weight = float('nan')
        model.train_step(batch)

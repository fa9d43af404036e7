"""Second-order smoothness on the GPU: raft_smooth2_loss_f32 and the layers above it against the float64
yardstick of tests/test_smooth2_loss.py.

Tolerances of the parity test, per shape: the float32 restatement's own measured distance to the yardstick times 4, for the loss
(relative) and for the gradient (max |difference|), both taken against the yardstick and never against the kernel.  The gradient
has that bound and nothing else.  The two VALUES have, beside it, the floor of 8 * 2^-24 relative that
tests/test_gpu_photometric_loss.py gives its values.  That floor is the number format's, not the kernel's: a value leaves the
entry as ONE float32, which cannot lie closer to the float64 value than its rounding (up to 2^-24 relative), and a kernel whose
expf differs from NumPy's in the last place may land on the neighbouring float32 (2^-23).  Where the restatement happens to round
within 2.7e-8 of the yardstick, as at 1x2x7x2, four times its distance (1.06e-7) is less than one float32 spacing (1.19e-7); the
kernel measured 1.43e-7 there, one spacing from the restatement.  The cases with a known answer: an affine flow gives a gradient of exactly 0 and a value within 4 ulps of the
closed form, and so does the quadratic flow's value.  The measured distances are in docs/NOTEBOOK.md section 35.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import report
from test_photometric_loss import DEFAULTS, make_case, torch_photometric_loss, ulps
from test_smooth2_loss import (CASE_IDS, CASES, NO_STENCIL, PARAMS, affine_case, np_smooth2_loss, quadratic_case,
                               smooth2_restatement_distance, smooth2_yardstick, torch_smooth2_loss)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MID = (2, 37, 53, 3)


def _np(t):
    return t.detach().cpu().numpy()


def _scalars(terms):
    return {k: _np(v).reshape(()).astype(np.float32)[()] for k, v in terms.items()}


def _entry(image1, preds, smooth2_weight=1.0, upstream=1.0, add_to=None, alias=False, prefill=None, want_grad=True, gap=0, guard=0):
    """raft_smooth2_loss_f32 called directly: ``(out2 as float32 NumPy, d_preds (n, B, H, W, 2) or None, the whole slab)``.
    ``prefill`` (a float or a tensor, with accumulate = 1) fills d_preds before the call; ``gap`` floats lie behind every
    prediction and ``guard`` floats of NaN around d_preds; ``alias``: add_to is out2 itself, holding ``add_to``."""
    from tf_raft_amd import _dev, losses
    from tf_raft_amd._ffi import check
    B, H, W, _ = image1.shape
    n, npix = len(preds), B * H * W
    stride = 2 * npix + gap
    i1 = torch.as_tensor(image1).cuda()
    src = torch.zeros((n * stride,), dtype=torch.float32, device='cuda')
    for i, p in enumerate(preds):
        src[i * stride:i * stride + 2 * npix] = torch.as_tensor(p).cuda().reshape(-1)
    slab = torch.full((n * stride + 2 * guard,), float('nan'), dtype=torch.float32, device='cuda')
    dst = slab[guard:guard + n * stride]
    if prefill is not None:
        dst.reshape(n, stride)[:, :2 * npix] = prefill
    out = torch.full((2,), float('nan'), dtype=torch.float32, device='cuda')
    add = None
    if add_to is not None:
        if alias:
            out[0] = add_to
            add = out
        else:
            add = torch.tensor([add_to], dtype=torch.float32, device='cuda')
    lib = _dev.lib()
    ws = losses._workspace(out.device, 8 * int(lib.raft_smooth2_loss_workspace_doubles()))
    check(lib.raft_smooth2_loss_f32(_dev.ptr(i1), _dev.ptr(src), stride, n, B, H, W, PARAMS['gamma'], smooth2_weight,
                                    PARAMS['edge_weight'], PARAMS['eps'], upstream, None if add is None else _dev.ptr(add),
                                    _dev.ptr(out), _dev.ptr(dst) if want_grad else None, 0 if prefill is None else 1, _dev.ptr(ws),
                                    _dev.stream_ptr()), 'smooth2_loss')
    torch.cuda.synchronize()
    d = _np(dst.reshape(n, stride)[:, :2 * npix]).reshape(n, B, H, W, 2) if want_grad else None
    return _np(out), d, slab


@functools.lru_cache(maxsize=None)
def _yardstick(shape):
    image1, _, _, preds = make_case(*shape)
    return smooth2_yardstick(image1, preds, **PARAMS)


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize('shape', CASES, ids=CASE_IDS)
def test_the_entry_alone_matches_the_float64_yardstick(shape):
    """add_to = NULL and accumulate = 0: nothing of the other terms hides a distance."""
    image1, _, _, preds = make_case(*shape)
    out, d, _ = _entry(image1, preds)
    assert d.shape == (shape[3],) + tuple(shape[:3]) + (2,) and d.dtype == np.float32
    if shape == NO_STENCIL:
        assert out.tolist() == [0.0, 0.0]
        assert not d.any() and not np.signbit(d).any()                  # all +0.0
        return
    want, want_last, want_g = _yardstick(shape)
    base_loss, base_g, max_g = smooth2_restatement_distance(*shape)
    rel = abs(float(out[0]) - want) / want
    diff = max(float(np.abs(d[i].astype(np.float64) - w).max()) for i, w in enumerate(want_g))
    report(f'smooth2 entry alone {shape}', base_loss_rel=base_loss, loss_rel=rel, base_grad_over_max=base_g / max_g,
           grad_over_max=diff / max_g)
    assert rel <= max(4 * base_loss, 8 * U)
    assert diff <= 4 * base_g
    own = np_smooth2_loss(image1, preds, **PARAMS)[0][1]
    assert abs(float(out[1]) - want_last) <= max(4 * abs(float(own) - want_last), 8 * U * want_last)      # the last prediction's term


# ------------------------------------------------------------------ cases with a known answer
EXACT = (2, 37, 53, 2)


def test_an_affine_flow_has_a_gradient_of_exactly_zero_and_the_closed_form_value():
    image1, preds, closed = affine_case(*EXACT)
    out, d, _ = _entry(image1, preds)
    assert not d.any()
    report('smooth2, affine flow', value=float(out[1]), closed=closed, ulps=ulps(out[1], closed))
    assert ulps(out[1], closed) <= 4
    assert ulps(out[0], (0.8 + 1.0) * closed) <= 4


@pytest.mark.parametrize('constant_image', [False, True], ids=['noise', 'constant'])
def test_the_quadratic_flow_has_the_closed_form_value(constant_image):
    image1, preds, closed = quadratic_case(*EXACT, constant_image=constant_image)
    out, d, _ = _entry(image1, preds)
    report(f'smooth2, quadratic flow, constant image {constant_image}', value=float(out[1]), closed=closed, ulps=ulps(out[1], closed))
    assert ulps(out[1], closed) <= 4
    if constant_image:                      # all edge weights exactly 1: q is constant along its axis away from the borders
        assert not d[:, :, 2:-2, 2:-2].any() and d[:, :, :, :2].any()


# ------------------------------------------------------------------ structure
def test_accumulate_guard_bands_value_only_and_repeats():
    B, H, W, n = MID
    image1, _, _, preds = make_case(*MID)
    out, stored, _ = _entry(image1, preds, smooth2_weight=0.7, upstream=1.5)
    assert stored.any()
    # accumulate = 1 over a pattern: prefill + the stored result, one float32 addition each; NaN bands around d_preds and in
    # the gaps of a larger pred_stride stay NaN; add_to is added
    pattern = torch.linspace(-1.0, 1.0, n * 2 * B * H * W, dtype=torch.float32, device='cuda').reshape(n, -1)
    out_acc, acc, slab = _entry(image1, preds, smooth2_weight=0.7, upstream=1.5, add_to=0.375, prefill=pattern, gap=10, guard=32)
    np.testing.assert_array_equal(acc, _np(pattern).reshape(acc.shape) + stored)
    stride = 2 * B * H * W + 10
    assert bool(torch.isnan(slab[:32]).all()) and bool(torch.isnan(slab[32 + n * stride:]).all())
    assert bool(torch.isnan(slab[32:32 + n * stride].reshape(n, stride)[:, 2 * B * H * W:]).all())
    assert out_acc[1].tobytes() == out[1].tobytes()
    assert abs(float(out_acc[0]) - (0.375 + float(out[0]))) <= 2 * U
    # add_to aliased to out2: the same bits as a separate add_to
    out_alias, _, _ = _entry(image1, preds, smooth2_weight=0.7, upstream=1.5, add_to=0.375, alias=True)
    assert out_alias.tobytes() == out_acc.tobytes()
    # accumulate = 0 writes every element (a NaN slab underneath), in the gapped layout too
    _, again, slab0 = _entry(image1, preds, smooth2_weight=0.7, upstream=1.5, gap=10, guard=32)
    assert again.tobytes() == stored.tobytes()
    assert bool(torch.isnan(slab0[:32]).all()) and bool(torch.isnan(slab0[32 + n * stride:]).all())
    assert bool(torch.isnan(slab0[32:32 + n * stride].reshape(n, stride)[:, 2 * B * H * W:]).all())
    # value only: the same out2 bits; repeats: the same bits
    only, none, _ = _entry(image1, preds, smooth2_weight=0.7, upstream=1.5, want_grad=False)
    assert none is None and only.tobytes() == out.tobytes()
    out_b, stored_b, _ = _entry(image1, preds, smooth2_weight=0.7, upstream=1.5)
    assert out_b.tobytes() == out.tobytes() and stored_b.tobytes() == stored.tobytes()


@pytest.mark.parametrize('others', [(0.0, 0.0), (0.7, 0.5)], ids=['plain', 'census_ssim'])
@pytest.mark.parametrize('with_mask', [True, False], ids=['mask', 'nomask'])
def test_the_python_layers_add_the_entry_to_the_parent_terms(with_mask, others):
    """``smooth2_weight = 0.5``: the parent's terms plus the entry alone, added in the entry's order; ``terms`` / ``__call__`` agree
    bit for bit; ``smooth2_weight = 0`` is the parent's bytes for every key and gradient."""
    from tf_raft_amd import grad, losses
    cw, sw = others
    image1, image2, mask, preds = make_case(*MID, with_mask=with_mask)
    y_true = (image1, image2) if mask is None else (image1, image2, mask)
    parent_cls = losses.SSIMSequenceLoss if sw else losses.PhotometricSequenceLoss
    parent_extra = dict(census_weight=cw, ssim_weight=sw) if sw else dict(census_weight=cw)
    cls, extra = losses.Smooth2SequenceLoss, dict(census_weight=cw, ssim_weight=sw)
    parent = parent_cls(**DEFAULTS, **parent_extra)
    parent_terms, parent_grads = parent.value_and_grad(y_true, preds)
    keys = ['loss', 'photometric'] + ['census'] * (cw > 0) + ['ssim'] * (sw > 0) + ['smoothness']
    assert list(parent_terms) == keys
    loss = cls(smooth2_weight=0.5, **DEFAULTS, **extra)
    terms, grads = loss.value_and_grad(y_true, preds)
    assert list(terms) == keys + ['smoothness2']
    terms = _scalars(terms)
    out, stored, _ = _entry(image1, preds, smooth2_weight=0.5, add_to=float(_np(parent_terms['loss'])))
    assert out[0].tobytes() == terms['loss'].tobytes() and out[1].tobytes() == terms['smoothness2'].tobytes()
    assert float(terms['smoothness2']) > 0
    for i, g in enumerate(grads):
        np.testing.assert_array_equal(_np(parent_grads[i]) + stored[i], _np(g))
    for k in keys[1:]:
        assert _np(parent_terms[k]).reshape(()).astype(np.float32).tobytes() == terms[k].tobytes(), k
    only = loss.terms(y_true, preds)
    assert list(only) == keys + ['smoothness2']
    assert {k: v.tobytes() for k, v in _scalars(only).items()} == {k: v.tobytes() for k, v in terms.items()}
    assert _np(loss(y_true, preds)).tobytes() == terms['loss'].tobytes()
    again, again_g = grad.smooth2_sequence_loss_value_and_grad(y_true, preds, smooth2_weight=0.5, **DEFAULTS, **extra)
    assert {k: v.tobytes() for k, v in _scalars(again).items()} == {k: v.tobytes() for k, v in terms.items()}
    for a, b, c in zip(grads, again_g, grad.smooth2_sequence_loss_grad(y_true, preds, smooth2_weight=0.5, **DEFAULTS, **extra)):
        assert _np(a).tobytes() == _np(b).tobytes() == _np(c).tobytes()
    assert _np(losses.smooth2_sequence_loss(y_true, preds, smooth2_weight=0.5, **DEFAULTS, **extra)).tobytes() == terms['loss'].tobytes()
    # smooth2_weight = 0: no launch, the parent's bytes
    zero = cls(smooth2_weight=0.0, **DEFAULTS, **extra)
    zero_terms, zero_grads = zero.value_and_grad(y_true, preds)
    assert list(zero_terms) == keys == list(zero.terms(y_true, preds))
    for k in keys:
        assert _np(zero_terms[k]).tobytes() == _np(parent_terms[k]).tobytes() == _np(zero.terms(y_true, preds)[k]).tobytes(), k
    for a, b in zip(parent_grads, zero_grads):
        assert _np(a).tobytes() == _np(b).tobytes()
    # the first-order term off (smooth_weight = 0), the second-order one on: finite, and the entry on top of that parent
    kitti = cls(**dict(DEFAULTS, smooth_weight=0.0), smooth2_weight=2.0, **extra)
    k_terms, k_grads = kitti.value_and_grad(y_true, preds)
    base_terms, base_grads = parent_cls(**dict(DEFAULTS, smooth_weight=0.0), **parent_extra).value_and_grad(y_true, preds)
    out, stored, _ = _entry(image1, preds, smooth2_weight=2.0, add_to=float(_np(base_terms['loss'])))
    assert out[0].tobytes() == _scalars(k_terms)['loss'].tobytes()
    for i, g in enumerate(k_grads):
        np.testing.assert_array_equal(_np(base_grads[i]) + stored[i], _np(g))


# ------------------------------------------------------------------ end to end
def _yardstick_total_loss(i1, i2, mask, preds, smooth2_weight, **params):
    """The photometric yardstick plus the second-order yardstick (float64 torch): what ``Smooth2SequenceLoss`` computes with the census and SSIM terms off."""
    first = torch_photometric_loss(i1, i2, mask, preds, **params)[0]
    return torch_smooth2_loss(i1, preds, gamma=params['gamma'], smooth2_weight=smooth2_weight, edge_weight=params['edge_weight'],
                              eps=params['eps'], add_to=first)[0]


def _reference_train_steps(wts, batches, iters, lr_fn, wd, clip_norm, n_steps, loss_fn):
    """tests/test_gpu_ssim_loss.py::_reference_ssim_train_steps with ``loss_fn(i1, i2, mask, preds)`` as the loss: the reference's
    train_step restricted to the update block, on the oracle in float64 with autograd, tf.clip_by_global_norm and tfa AdamW.
    Returns (losses, updated update-block weights)."""
    import oracle
    from oracle.layers import W, basic_update_block, encoder
    from oracle.model import upsample_flow
    names = sorted(k for k in wts if k.startswith('update_block'))
    var = {k: torch.tensor(wts[k], dtype=torch.float64) for k in names}
    m = {k: torch.zeros_like(v) for k, v in var.items()}
    v2 = {k: torch.zeros_like(v) for k, v in var.items()}
    frozen = W({k: val for k, val in wts.items() if not k.startswith('update_block')}, torch.float64)
    losses = []
    for step in range(n_steps):
        i1, i2 = batches[step][0], batches[step][1]
        mask = batches[step][2] if len(batches[step]) == 3 else None
        with torch.no_grad():
            x1 = 2 * (torch.tensor(i1, dtype=torch.float64) / 255.0) - 1.0
            x2 = 2 * (torch.tensor(i2, dtype=torch.float64) / 255.0) - 1.0
            f1, f2 = encoder(frozen, 'fnet', [x1, x2])
            corr_blk = oracle.CorrBlock(f1, f2, 4, 4)
            cnet = encoder(frozen, 'cnet', x1)
            net, inp = torch.tanh(cnet[..., :128]), torch.relu(cnet[..., 128:])
        ow = W({}, torch.float64)
        ow.t = {k: val.clone().requires_grad_(True) for k, val in var.items()}
        B, h, w, _ = net.shape
        coords0 = oracle.coords_grid(B, h, w, torch.float64)
        coords1, preds = coords0.clone(), []
        for _ in range(iters):
            corr = corr_blk.retrieve(coords1)
            net, up_mask, delta = basic_update_block(ow, 'update_block', net, inp, corr, coords1 - coords0)
            coords1 = coords1 + delta
            preds.append(upsample_flow(coords1 - coords0, up_mask))
        loss = loss_fn(i1, i2, mask, preds)
        loss.backward()
        losses.append(float(loss.detach()))
        g = {k: ow.t[k].grad for k in names}
        gnorm = torch.sqrt(sum((gg ** 2).sum() for gg in g.values()))
        scale = clip_norm / max(float(gnorm), clip_norm)
        t = step + 1
        lr = lr_fn(step)
        lr_t = lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        for k in names:
            gk = g[k] * scale
            w_ = var[k] - wd * var[k]
            m[k] = 0.9 * m[k] + 0.1 * gk
            v2[k] = 0.999 * v2[k] + 0.001 * gk * gk
            var[k] = w_ - lr_t * m[k] / (torch.sqrt(v2[k]) + 1e-7)
    return losses, {k: v.numpy() for k, v in var.items()}


def test_train_step_with_the_second_order_term_matches_reference_semantics(rng):
    """test_gpu_ssim_loss.py::test_train_step_with_the_ssim_term_matches_reference_semantics with
    Smooth2SequenceLoss(smooth_weight=0.1, smooth2_weight=1): two steps at (1, 64, 96), iters = 3, conditioned weights,
    trainable='update_block', cyclical learning rate + AdamW + clip 1.0, against the same procedure on the float64 oracle with the
    float64 yardstick loss, within that test's bounds.  Step 0 carries a mask, step 1 none."""
    import tf_raft_amd
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    B, H, W, iters, n_steps = 1, 64, 96, 3, 2
    wts = wm.condition_weights('raft', wm.init_weights('raft', seed=5))
    batches = []
    for step in range(n_steps):
        i1 = rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32)
        i2 = rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32)
        batches.append((i1, i2, (rng.uniform(size=(B, H, W)) < 0.8).astype(np.uint8)) if step == 0 else (i1, i2))
    lr0, wd, clip = 4e-4, 1e-4, 1.0
    sched = training.CyclicalLearningRate(lr0, 2 * lr0, step_size=1000, scale_fn=training.first_cycle_scaler, scale_mode='cycle')
    model = tf_raft_amd.RAFT(weights=wts, iters=iters, iters_pred=4)
    params = dict(DEFAULTS, smooth_weight=0.1)
    model.compile(optimizer=training.AdamW(wd, sched), clip_norm=clip, loss=losses.Smooth2SequenceLoss(smooth2_weight=1.0, **params),
                  trainable='update_block')
    got_losses = []
    for step in range(n_steps):
        res = model.train_step(batches[step])
        assert list(res) == ['loss', 'photometric', 'smoothness', 'smoothness2']
        got_losses.append(float(model.flow_metrics['loss'].total))
    assert float(res['smoothness2']) > 0
    got_losses = [got_losses[0]] + [b - a for a, b in zip(got_losses, got_losses[1:])]
    loss_fn = lambda i1, i2, mask, preds: _yardstick_total_loss(i1, i2, mask, preds, 1.0, **params)
    want_losses, want_w = _reference_train_steps(wts, batches, iters, sched, wd, clip, n_steps, loss_fn)
    report('smooth2 train_step losses', got0=got_losses[0], want0=want_losses[0], got1=got_losses[1], want1=want_losses[1])
    np.testing.assert_allclose(got_losses, want_losses, rtol=1e-4)
    new_w = model.get_weights_dict()
    total, bad, num, den = 0, 0, 0.0, 0.0
    for k, ref in want_w.items():
        upd_ref = ref - wts[k].astype(np.float64)
        upd_got = new_w[k].astype(np.float64) - wts[k].astype(np.float64)
        total += upd_ref.size
        bad += int((np.abs(upd_got - upd_ref) > 0.25 * lr0).sum())
        num += float(((upd_got - upd_ref) ** 2).sum())
        den += float((upd_ref ** 2).sum())
        assert np.abs(upd_ref).max() > 0.1 * lr0                      # the reference did move this tensor
    for k, v in wts.items():
        if not k.startswith('update_block'):
            np.testing.assert_array_equal(new_w[k], v)                # frozen encoders
    report('smooth2 train_step updated weights', frac_elements_off_by_quarter_lr=bad / total, rel_l2_of_update=float(np.sqrt(num / den)))
    assert bad / total <= 0.02
    assert np.sqrt(num / den) <= 0.1


@pytest.mark.parametrize('variant', ['small', 'raft_all', 'bidirectional_selfsup'])
def test_one_step_of_the_other_configurations(rng, variant):
    """SmallRAFT, RAFT with trainable='all', and a bidirectional step with a student pass on a crop: finite terms, the keys in the
    stated order, the weights moved.  (2, 64, 96) and iters = 2; the step with the student pass takes (2, 80, 112), the smallest
    frames whose crop by (8, 8) leaves the 64 x 96 student the model accepts: it refuses a side under 64.)"""
    import tf_raft_amd
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    B, H, W = (2, 80, 112) if variant == 'bidirectional_selfsup' else (2, 64, 96)
    loss = losses.Smooth2SequenceLoss(smooth2_weight=1.0)
    keys = ['loss', 'photometric', 'smoothness', 'smoothness2']
    if variant == 'small':
        wts = wm.condition_weights('small', wm.init_weights('small', seed=2, perturb=True), 'mid')
        model = tf_raft_amd.SmallRAFT(weights=wts, iters=2, iters_pred=2)
        model.compile(optimizer=training.AdamW(1e-4, 1e-3), clip_norm=1.0, loss=loss)
    else:
        wts = wm.condition_weights('raft', wm.init_weights('raft', seed=2, perturb=True), 'mid')
        model = tf_raft_amd.RAFT(weights=wts, iters=2, iters_pred=2)
        if variant == 'raft_all':
            model.compile(optimizer=training.AdamW(1e-4, 1e-3), clip_norm=1.0, loss=loss, trainable='all')
        else:
            model.compile(optimizer=training.AdamW(1e-4, 1e-3), clip_norm=1.0, loss=loss, trainable='all', bidirectional=True,
                          occlusion=False, selfsup_crop=(8, 8))
            keys = keys + ['occluded', 'selfsup', 'selfsup_used']
    i1 = rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32)
    i2 = rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32)
    res = model.train_step((i1, i2) if variant == 'bidirectional_selfsup' else (i1, i2, rng.uniform(size=(B, H, W)) < 0.8))
    assert list(res) == keys
    vals = losses.to_floats(res)
    assert all(np.isfinite(v) for v in vals.values()), vals
    assert all(vals[k] > 0 for k in ('loss', 'photometric', 'smoothness', 'smoothness2')), vals
    new = model.get_weights_dict()
    moved = [k for k in new if not np.array_equal(new[k], wts[k])]
    assert all(k in moved for k in new if k.endswith('kernel')), [k for k in new if k.endswith('kernel') and k not in moved]
    report(f'smooth2 train_step {variant}', tensors_moved=len(moved), **vals)

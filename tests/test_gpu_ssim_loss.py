"""SSIM term on the GPU: raft_ssim_loss_f32 and the layers above it against the float64 yardstick of
tests/test_ssim_loss.py.

Tolerances of the parity tests, per case: the float32 restatement's own measured distance to the yardstick times 4 (hardware
rounding of a differently associated reduction), with the floors of tests/test_gpu_photometric_loss.py: 8 * 2^-24 relative for the
values and 16 * 2^-24 * max|g| for the gradient.

Measured (MI355X, with mask; the base is what the restatement itself is away from float64, then what the kernel is; loss relative,
gradient over max|g|.  The kernel's distances equal the restatement's to the printed digits in every case, with and without a
mask, from a list of tensors and from views of one buffer alike: the per-pixel arithmetic is the restatement's operation for
operation, only the float64 sums over pixels are associated differently):

    case (B,H,W,n)   all terms, ssim_weight = 1, census off              the SSIM entry alone
                     base and kernel: loss rel, gradient / max|g|        base and kernel: loss rel, gradient / max|g|
    1x2x20x1         2.1e-08, 2.3e-07                                    exactly 0, exactly 0
    1x3x3x1          1.2e-08, 6.8e-08                                    1.9e-08, 2.0e-07
    1x8x9x2          2.9e-08, 4.9e-07                                    3.7e-10, 2.8e-07
    2x37x53x3        6.6e-08, 6.4e-06                                    1.3e-08, 2.5e-06
    1x9x2051x2       1.1e-07, 3.0e-04                                    7.0e-08, 9.6e-05
    2x64x96x12       1.2e-08, 9.7e-06                                    3.5e-09, 3.5e-06
    (without a mask the largest are 1.7e-07, 2.8e-04 and 9.6e-08, 9.1e-05, both at 1x9x2051x2)
    census 0.7 / ssim 0.5:  1x2x20x1  2.1e-08, 2.3e-07 (bit for bit the call without SSIM);  2x37x53x3  2.8e-08, 1.5e-04

Equal frames at zero flow: out2 exactly {0, 0}, the gradient exactly 0 (8.7e-20 from the yardstick's, against a bound of 9.2e-10).
End to end (two steps against the float64 oracle with the yardstick loss, ssim_weight = 1): losses 1.420 / 1.777 on both sides, no
element of the update off by more than 0.25 * lr, relative L2 of the update 5.7e-4.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import report
from windowed_loss import entry
from test_photometric_loss import DEFAULTS, out_of_frame_case
from test_ssim_loss import (CASE_IDS, CASES, NO_INTERIOR, equal_frames_case, np_ssim_loss, np_ssim_total_loss, ssim_case,
                            ssim_only_distance, ssim_restatement_distance, ssim_total_yardstick, ssim_yardstick,
                            torch_ssim_total_loss)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MID = (2, 37, 53, 3)


def _np(t):
    return t.detach().cpu().numpy()


def _as_views(preds):
    """The predictions as views of one (n, B, H, W, 2) device buffer, the way the model returns them."""
    buf = torch.as_tensor(np.stack(preds)).cuda().contiguous()
    return [buf[i] for i in range(buf.shape[0])]


def _scalars(terms):
    return {k: _np(v).reshape(()).astype(np.float32)[()] for k, v in terms.items()}


def _run(case, census_weight=0.0, ssim_weight=1.0, views=False, upstream=1.0, **params):
    """``(terms as float32 NumPy scalars, [gradients as NumPy])`` through grad.ssim_sequence_loss_value_and_grad."""
    from tf_raft_amd import grad
    image1, image2, mask, preds = case
    y_true = (image1, image2) if mask is None else (image1, image2, mask)
    terms, grads = grad.ssim_sequence_loss_value_and_grad(y_true, _as_views(preds) if views else preds, upstream=upstream,
                                                          census_weight=census_weight, ssim_weight=ssim_weight,
                                                          **dict(DEFAULTS, **params))
    assert len(grads) == len(preds)
    return _scalars(terms), [_np(g) for g in grads]


def _entry(case, ssim_weight=1.0, **kwargs):
    """raft_ssim_loss_f32 called directly (windowed_loss.entry)."""
    return entry('ssim', case, ssim_weight, **kwargs)


@functools.lru_cache(maxsize=None)
def _total_yardstick(shape, with_mask, census_weight, ssim_weight):
    return ssim_total_yardstick(ssim_case(shape, with_mask), census_weight, ssim_weight, **DEFAULTS)


def _check_parity(shape, with_mask, views, census_weight, ssim_weight):
    case = ssim_case(shape, with_mask)
    want = _total_yardstick(shape, with_mask, census_weight, ssim_weight)
    want_loss, want_ssim, want_g = want[0], want[3], want[5]
    base_loss, base_g, max_g = ssim_restatement_distance(*shape, with_mask, census_weight, ssim_weight)
    terms, grads = _run(case, census_weight, ssim_weight, views=views)
    assert list(terms) == ['loss', 'photometric'] + ['census'] * (census_weight > 0) + ['ssim', 'smoothness']
    rel = abs(float(terms['loss']) - want_loss) / abs(want_loss)
    diff = max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(grads, want_g))
    report(f'ssim loss, census {census_weight} / ssim {ssim_weight} {shape} mask={with_mask} views={views}', base_loss_rel=base_loss,
           loss_rel=rel, base_grad_over_max=base_g / max_g, grad_over_max=diff / max_g)
    assert rel <= max(4 * base_loss, 8 * U)
    assert diff <= max(4 * base_g, 16 * U * max_g)
    assert all(g.shape == tuple(shape[:3]) + (2,) and g.dtype == np.float32 for g in grads)
    # the reported SSIM term is the last prediction's
    own = np_ssim_total_loss(*case, census_weight, ssim_weight, **DEFAULTS)[3]
    assert abs(float(terms['ssim']) - want_ssim) <= max(4 * abs(float(own) - want_ssim), 8 * U * abs(want_ssim)), (terms['ssim'], want_ssim)
    if shape == NO_INTERIOR:                     # nothing but the other terms, bit for bit
        plain, plain_g = _run(case, census_weight, 0.0, views=views)
        assert 'ssim' not in plain
        assert float(terms['ssim']) == 0.0 and terms['loss'].tobytes() == plain['loss'].tobytes()
        for a, b in zip(grads, plain_g):
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize('views', [False, True], ids=['list', 'views'])
@pytest.mark.parametrize('with_mask', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('shape', CASES, ids=CASE_IDS)
def test_loss_and_gradient_with_the_ssim_term_match_the_float64_yardstick(shape, with_mask, views):
    _check_parity(shape, with_mask, views, 0.0, 1.0)


@pytest.mark.parametrize('views', [False, True], ids=['list', 'views'])
@pytest.mark.parametrize('with_mask', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('shape', [NO_INTERIOR, MID], ids=['1x2x20x1', '2x37x53x3'])
def test_the_total_loss_with_census_weight_0p7_and_ssim_weight_0p5(shape, with_mask, views):
    _check_parity(shape, with_mask, views, 0.7, 0.5)


@pytest.mark.parametrize('with_mask', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('shape', CASES, ids=CASE_IDS)
def test_the_ssim_entry_alone_matches_the_float64_yardstick(shape, with_mask):
    """raft_ssim_loss_f32 with add_to = NULL and accumulate = 0: nothing of the other terms hides a distance."""
    case = ssim_case(shape, with_mask)
    want_total, want_last, want_g = ssim_yardstick(case, DEFAULTS['gamma'])
    base_loss, base_g, max_g = ssim_only_distance(*shape, with_mask)
    out, d, _ = _entry(case)
    if shape == NO_INTERIOR:
        assert out[0] == 0.0 and out[1] == 0.0 and not d.any()
        return
    rel = abs(float(out[0]) - want_total) / want_total
    diff = max(float(np.abs(d[i].astype(np.float64) - w).max()) for i, w in enumerate(want_g))
    report(f'ssim entry alone {shape} mask={with_mask}', base_loss_rel=base_loss, loss_rel=rel, base_grad_over_max=base_g / max_g,
           grad_over_max=diff / max_g)
    assert rel <= max(4 * base_loss, 8 * U)
    assert diff <= max(4 * base_g, 16 * U * max_g)
    own = np_ssim_loss(*case, gamma=DEFAULTS['gamma'])[1]
    assert abs(float(out[1]) - want_last) <= max(4 * abs(float(own) - want_last), 8 * U * want_last)


# ------------------------------------------------------------------ cases with a known answer
EXACT = (2, 37, 53, 2)


def test_equal_frames_at_zero_flow_give_exactly_zero():
    case = equal_frames_case(*EXACT)
    out, d, _ = _entry(case)
    assert out[0] == 0.0 and out[1] == 0.0
    _, _, want_g = ssim_yardstick(case, DEFAULTS['gamma'])
    _, _, own_g = np_ssim_loss(*case, gamma=DEFAULTS['gamma'])
    base = max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(own_g, want_g))
    max_g = ssim_only_distance(*EXACT, True)[2]                       # of make_case at the same shape
    diff = max(float(np.abs(d[i].astype(np.float64) - w).max()) for i, w in enumerate(want_g))
    report('ssim, equal frames', base_grad=base, grad=diff, bound=max(4 * base, 16 * U * max_g))
    assert diff <= max(4 * base, 16 * U * max_g)


def test_vectors_out_of_frame_give_exactly_zero():
    out, d, _ = _entry(out_of_frame_case(*EXACT))
    assert out[0] == 0.0 and out[1] == 0.0
    assert not d.any()


# ------------------------------------------------------------------ structure
def test_accumulate_guard_bands_value_only_and_repeats():
    B, H, W, n = MID
    for with_mask in (True, False):
        case = ssim_case(MID, with_mask)
        out, stored, _ = _entry(case, ssim_weight=0.7, upstream=1.5)
        assert stored.any()
        # accumulate = 1 over a pattern: prefill + the stored result, one float32 addition each; NaN bands around d_preds and in
        # the gaps of a larger pred_stride stay NaN; add_to is added
        pattern = torch.linspace(-1.0, 1.0, n * 2 * B * H * W, dtype=torch.float32, device='cuda').reshape(n, -1)
        out_acc, acc, slab = _entry(case, ssim_weight=0.7, upstream=1.5, add_to=0.375, prefill=pattern, gap=10, guard=32)
        np.testing.assert_array_equal(acc, _np(pattern).reshape(acc.shape) + stored)
        stride = 2 * B * H * W + 10
        assert bool(torch.isnan(slab[:32]).all()) and bool(torch.isnan(slab[32 + n * stride:]).all())
        assert bool(torch.isnan(slab[32:32 + n * stride].reshape(n, stride)[:, 2 * B * H * W:]).all())
        assert out_acc[1].tobytes() == out[1].tobytes()
        assert abs(float(out_acc[0]) - (0.375 + float(out[0]))) <= 2 * U
        # accumulate = 0 writes every element (a NaN slab underneath), in the gapped layout too
        _, again, slab0 = _entry(case, ssim_weight=0.7, upstream=1.5, gap=10, guard=32)
        assert again.tobytes() == stored.tobytes()
        assert bool(torch.isnan(slab0[32:32 + n * stride].reshape(n, stride)[:, 2 * B * H * W:]).all())
        # value only: the same out2 bits; repeats: the same bits
        only, none, _ = _entry(case, ssim_weight=0.7, upstream=1.5, want_grad=False)
        assert none is None and only.tobytes() == out.tobytes()
        out_b, stored_b, _ = _entry(case, ssim_weight=0.7, upstream=1.5)
        assert out_b.tobytes() == out.tobytes() and stored_b.tobytes() == stored.tobytes()


@pytest.mark.parametrize('with_mask', [True, False], ids=['mask', 'nomask'])
def test_python_entries_agree_and_ssim_weight_zero_is_the_parent_loss(with_mask):
    from tf_raft_amd import grad, losses
    image1, image2, mask, preds = ssim_case(MID, with_mask)
    y_true = (image1, image2) if mask is None else (image1, image2, mask)
    for cw in (0.0, 0.5):
        terms, grads = _run((image1, image2, mask, preds), census_weight=cw, ssim_weight=0.25)
        loss = losses.SSIMSequenceLoss(census_weight=cw, ssim_weight=0.25, **DEFAULTS)
        only = loss.terms(y_true, preds)
        assert list(only) == ['loss', 'photometric'] + ['census'] * (cw > 0) + ['ssim', 'smoothness']
        for k in terms:
            assert _np(only[k]).reshape(()).astype(np.float32).tobytes() == terms[k].tobytes(), k
        assert _np(loss(y_true, preds)).tobytes() == terms['loss'].tobytes()
        both, both_g = loss.value_and_grad(y_true, preds)
        assert {k: v.tobytes() for k, v in _scalars(both).items()} == {k: v.tobytes() for k, v in terms.items()}
        for a, b, c in zip(grads, grad.ssim_sequence_loss_grad(y_true, preds, census_weight=cw, ssim_weight=0.25), both_g):
            assert a.tobytes() == _np(b).tobytes() == _np(c).tobytes()
        # ssim_weight = 0 is the parent class bit for bit, in terms and gradients
        parent_terms, parent_grads = grad.photometric_sequence_loss_value_and_grad(y_true, preds, census_weight=cw, **DEFAULTS)
        zero = losses.SSIMSequenceLoss(census_weight=cw, ssim_weight=0.0, **DEFAULTS)
        zero_terms, zero_grads = zero.value_and_grad(y_true, preds)
        assert list(zero_terms) == list(parent_terms) == list(zero.terms(y_true, preds))
        assert list(parent_terms) == list(losses.PhotometricSequenceLoss(census_weight=cw, **DEFAULTS).terms(y_true, preds))
        for k in parent_terms:
            assert _np(parent_terms[k]).tobytes() == _np(zero_terms[k]).tobytes() == _np(zero.terms(y_true, preds)[k]).tobytes(), k
        for a, b, c in zip(parent_grads, zero_grads, grad.ssim_sequence_loss_grad(y_true, preds, census_weight=cw, **DEFAULTS)):
            assert _np(a).tobytes() == _np(b).tobytes() == _np(c).tobytes()
        for k in parent_terms:
            if k != 'loss':
                assert _np(parent_terms[k]).reshape(()).astype(np.float32).tobytes() == terms[k].tobytes(), k
        # the entry on top of the launches before it is the entry alone on top of their results
        out, stored, _ = _entry((image1, image2, mask, preds), ssim_weight=0.25, add_to=float(_np(parent_terms['loss'])))
        assert out[0].tobytes() == terms['loss'].tobytes() and out[1].tobytes() == terms['ssim'].tobytes()
        for i, g in enumerate(grads):
            np.testing.assert_array_equal(_np(parent_grads[i]) + stored[i], g)


# ------------------------------------------------------------------ end to end
def _reference_ssim_train_steps(wts, batches, iters, lr_fn, wd, clip_norm, n_steps, params, census_weight, ssim_weight):
    """tests/test_gpu_census_loss.py::_reference_census_train_steps with the SSIM yardstick added to the loss: the reference's
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
        loss = torch_ssim_total_loss(i1, i2, mask, preds, census_weight, ssim_weight, **params)[0]
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


def test_train_step_with_the_ssim_term_matches_reference_semantics(rng):
    """test_gpu_census_loss.py::test_train_step_with_the_census_term_matches_reference_semantics with
    SSIMSequenceLoss(ssim_weight=1): two steps at (1, 64, 96), iters = 3, conditioned weights, trainable='update_block', cyclical
    learning rate + AdamW + clip 1.0, against the same procedure on the float64 oracle with the float64 yardstick loss, within that
    test's bounds.  Step 0 carries a mask, step 1 none."""
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
    model.compile(optimizer=training.AdamW(wd, sched), clip_norm=clip, loss=losses.SSIMSequenceLoss(ssim_weight=1.0, **DEFAULTS),
                  trainable='update_block')
    with pytest.raises(ValueError, match='image1, image2, mask'):
        model.train_step(batches[0] + (batches[0][2],))
    got_losses = []
    for step in range(n_steps):
        res = model.train_step(batches[step])
        assert list(res) == ['loss', 'photometric', 'ssim', 'smoothness']
        got_losses.append(float(model.flow_metrics['loss'].total))
    assert float(res['ssim']) > 0
    got_losses = [got_losses[0]] + [b - a for a, b in zip(got_losses, got_losses[1:])]
    want_losses, want_w = _reference_ssim_train_steps(wts, batches, iters, sched, wd, clip, n_steps, DEFAULTS, 0.0, 1.0)
    report('ssim train_step losses', got0=got_losses[0], want0=want_losses[0], got1=got_losses[1], want1=want_losses[1])
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
    report('ssim train_step updated weights', frac_elements_off_by_quarter_lr=bad / total, rel_l2_of_update=float(np.sqrt(num / den)))
    assert bad / total <= 0.02
    assert np.sqrt(num / den) <= 0.1
    out = model([batches[0][0], batches[0][1]])
    assert len(out) == 4 and np.isfinite(out[-1].numpy()).all()


@pytest.mark.parametrize('variant', ['small', 'raft_all'])
def test_one_ssim_step_of_the_other_configurations(rng, variant):
    """SmallRAFT, and RAFT with trainable='all': finite terms, exactly the four keys, the weights moved."""
    import tf_raft_amd
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    B, H, W = 2, 64, 96
    loss = losses.SSIMSequenceLoss(ssim_weight=1.0)
    if variant == 'small':
        wts = wm.condition_weights('small', wm.init_weights('small', seed=2, perturb=True), 'mid')
        model = tf_raft_amd.SmallRAFT(weights=wts, iters=2, iters_pred=2)
        model.compile(optimizer=training.AdamW(1e-4, 1e-3), clip_norm=1.0, loss=loss)
    else:
        wts = wm.condition_weights('raft', wm.init_weights('raft', seed=2, perturb=True), 'mid')
        model = tf_raft_amd.RAFT(weights=wts, iters=2, iters_pred=2)
        model.compile(optimizer=training.AdamW(1e-4, 1e-3), clip_norm=1.0, loss=loss, trainable='all')
    i1 = rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32)
    i2 = rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32)
    res = model.train_step((i1, i2, rng.uniform(size=(B, H, W)) < 0.8))
    assert list(res) == ['loss', 'photometric', 'ssim', 'smoothness']
    vals = losses.to_floats(res)
    assert all(np.isfinite(v) and v > 0 for v in vals.values()), vals
    new = model.get_weights_dict()
    moved = [k for k in new if not np.array_equal(new[k], wts[k])]
    assert all(k in moved for k in new if k.endswith('kernel')), [k for k in new if k.endswith('kernel') and k not in moved]
    report(f'ssim train_step {variant}', tensors_moved=len(moved), **vals)

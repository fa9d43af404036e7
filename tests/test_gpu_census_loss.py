"""Soft census term on the GPU: raft_census_loss_f32 and the layers above it against the float64 yardstick
of tests/test_census_loss.py.

Tolerances of the parity tests, per case: the float32 restatement's own measured distance to the yardstick times 4 (a different
summation order over the 48 pairs, hardware rounding of a differently associated reduction), with the floors of
tests/test_gpu_photometric_loss.py: 8 * 2^-24 relative for the values and 16 * 2^-24 * max|g| for the gradient.

Measured (MI355X, with mask; the base is what the restatement itself is away from float64, then what the kernel is.  The kernel's
distances equal the restatement's to the printed digits in every case, with and without a mask, from a list of tensors and from
views of one buffer alike: the per-pixel arithmetic is the restatement's operation for operation, only the float64 sums over
pixels are associated differently):

    case (B,H,W,n)   all terms, census_weight = 1                        the census entry alone
                     base and kernel: loss rel, gradient / max|g|        base and kernel: loss rel, gradient / max|g|
    1x6x20x1         8.2e-08, 1.3e-06                                    exactly 0, exactly 0
    1x8x9x2          4.8e-08, 8.8e-06                                    5.4e-08, 8.9e-06
    2x37x53x3        3.6e-08, 1.8e-04                                    7.2e-09, 1.9e-04
    1x9x2051x2       3.8e-07, 4.8e-03                                    4.5e-07, 4.9e-03
    2x64x96x12       1.2e-08, 7.5e-04                                    4.7e-09, 7.7e-04
    1x100x150x2      4.0e-08, 1.1e-03                                    8.7e-09, 1.1e-03
    (without a mask the largest are 4.0e-07, 7.5e-03 and 6.3e-07, 7.7e-03, both at 1x9x2051x2)

image2 = image1 + 20 at zero flow: census 3.7e-12 against a photometric term of 0.063.  End to end (two steps against the float64
oracle with the yardstick loss, census_weight = 1): losses 1.354 / 1.710 on both sides, 7.3e-5 of the update's elements off by more
than 0.25 * lr, relative L2 of the update 1.3e-2.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import report
from test_census_loss import (BRIGHTER_BOUND, CASE_IDS, CASES, NO_INTERIOR, brighter_case, census_only_distance,
                              census_restatement_distance, census_yardstick, equal_frames_case, np_census_loss, np_total_loss,
                              torch_total_loss, total_yardstick)
from windowed_loss import entry
from test_photometric_loss import DEFAULTS, make_case, out_of_frame_case

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
KEYS = {'loss', 'photometric', 'census', 'smoothness'}


def _np(t):
    return t.detach().cpu().numpy()


def _as_views(preds):
    """The predictions as views of one (n, B, H, W, 2) device buffer, the way the model returns them."""
    buf = torch.as_tensor(np.stack(preds)).cuda().contiguous()
    return [buf[i] for i in range(buf.shape[0])]


def _run(case, census_weight=1.0, views=False, upstream=1.0, **params):
    """``(terms as float32 NumPy scalars, [gradients as NumPy])`` through grad.photometric_sequence_loss_value_and_grad."""
    from tf_raft_amd import grad
    image1, image2, mask, preds = case
    y_true = (image1, image2) if mask is None else (image1, image2, mask)
    terms, grads = grad.photometric_sequence_loss_value_and_grad(y_true, _as_views(preds) if views else preds, upstream=upstream,
                                                                 census_weight=census_weight, **dict(DEFAULTS, **params))
    assert len(grads) == len(preds)
    return {k: _np(v).reshape(()).astype(np.float32)[()] for k, v in terms.items()}, [_np(g) for g in grads]


def _entry(case, census_weight=1.0, **kwargs):
    """raft_census_loss_f32 called directly (windowed_loss.entry)."""
    return entry('census', case, census_weight, **kwargs)


@functools.lru_cache(maxsize=None)
def _total_yardstick(shape, with_mask):
    return total_yardstick(make_case(*shape, with_mask=with_mask), 1.0, **DEFAULTS)


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize('views', [False, True], ids=['list', 'views'])
@pytest.mark.parametrize('with_mask', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('shape', CASES, ids=CASE_IDS)
def test_loss_and_gradient_with_the_census_term_match_the_float64_yardstick(shape, with_mask, views):
    case = make_case(*shape, with_mask=with_mask)
    want_loss, _, want_cen, _, want_g = _total_yardstick(shape, with_mask)
    base_loss, base_g, max_g = census_restatement_distance(*shape, with_mask)
    terms, grads = _run(case, views=views)
    assert set(terms) == KEYS
    rel = abs(float(terms['loss']) - want_loss) / abs(want_loss)
    diff = max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(grads, want_g))
    report(f'census loss, all terms {shape} mask={with_mask} views={views}', base_loss_rel=base_loss, loss_rel=rel,
           base_grad_over_max=base_g / max_g, grad_over_max=diff / max_g)
    assert rel <= max(4 * base_loss, 8 * U)
    assert diff <= max(4 * base_g, 16 * U * max_g)
    assert all(g.shape == tuple(shape[:3]) + (2,) and g.dtype == np.float32 for g in grads)
    # the reported census term is the last prediction's
    own = np_total_loss(*case, 1.0, **DEFAULTS)[2]
    assert abs(float(terms['census']) - want_cen) <= max(4 * abs(float(own) - want_cen), 8 * U * abs(want_cen)), (terms['census'], want_cen)
    if shape == NO_INTERIOR:                     # nothing but the other two terms, bit for bit
        plain, plain_g = _run(case, census_weight=0.0, views=views)
        assert float(terms['census']) == 0.0 and terms['loss'].tobytes() == plain['loss'].tobytes()
        for a, b in zip(grads, plain_g):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('with_mask', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('shape', CASES, ids=CASE_IDS)
def test_the_census_entry_alone_matches_the_float64_yardstick(shape, with_mask):
    """raft_census_loss_f32 with add_to = NULL and accumulate = 0: nothing of the other terms hides a distance."""
    case = make_case(*shape, with_mask=with_mask)
    want_total, want_cen, want_g = census_yardstick(case, DEFAULTS['gamma'])
    base_loss, base_g, max_g = census_only_distance(*shape, with_mask)
    out, d, _ = _entry(case)
    if shape == NO_INTERIOR:
        assert out[0] == 0.0 and out[1] == 0.0 and not d.any()
        return
    rel = abs(float(out[0]) - want_total) / want_total
    diff = max(float(np.abs(d[i].astype(np.float64) - w).max()) for i, w in enumerate(want_g))
    report(f'census entry alone {shape} mask={with_mask}', base_loss_rel=base_loss, loss_rel=rel, base_grad_over_max=base_g / max_g,
           grad_over_max=diff / max_g)
    assert rel <= max(4 * base_loss, 8 * U)
    assert diff <= max(4 * base_g, 16 * U * max_g)
    own = np_census_loss(*case, gamma=DEFAULTS['gamma'])[1]
    assert abs(float(out[1]) - want_cen) <= max(4 * abs(float(own) - want_cen), 8 * U * want_cen)


def test_the_total_loss_with_census_weight_0p7():
    shape = (2, 37, 53, 3)
    case = make_case(*shape)
    want = total_yardstick(case, 0.7, **DEFAULTS)
    base_loss, base_g, max_g = census_restatement_distance(*shape, True, 0.7)
    terms, grads = _run(case, census_weight=0.7)
    plain, _, _ = np_total_loss(*case, 0.0, **DEFAULTS)[:3]
    # yardstick photometric + smoothness + float32(0.7) * census, assembled here from its parts
    ph_sm = total_yardstick(case, 0.0, **DEFAULTS)[0]
    cen_sum = census_yardstick(case, DEFAULTS['gamma'])[0]
    assert abs(want[0] - (ph_sm + float(np.float32(0.7)) * cen_sum)) <= 1e-14
    rel = abs(float(terms['loss']) - want[0]) / want[0]
    diff = max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(grads, want[4]))
    report('census loss, census_weight 0.7', base_loss_rel=base_loss, loss_rel=rel, base_grad_over_max=base_g / max_g, grad_over_max=diff / max_g)
    assert rel <= max(4 * base_loss, 8 * U)
    assert diff <= max(4 * base_g, 16 * U * max_g)
    assert float(terms['loss']) > float(plain)                       # the term is there


# ------------------------------------------------------------------ cases with a known answer
EXACT = (2, 37, 53, 2)


def test_equal_frames_at_zero_flow_give_exactly_zero():
    out, d, _ = _entry(equal_frames_case(*EXACT))
    assert out[0] == 0.0 and out[1] == 0.0
    assert not d.any()


def test_a_brighter_second_frame_costs_next_to_nothing():
    case = brighter_case(*EXACT)
    out, d, _ = _entry(case)
    terms, _ = _run(case)
    report('census, image2 = image1 + 20', census=float(out[1]), photometric=float(terms['photometric']))
    assert 0.0 <= float(out[1]) < BRIGHTER_BOUND and 0.0 <= float(out[0]) < 2 * BRIGHTER_BOUND
    assert float(terms['census']) == float(out[1])
    assert float(terms['photometric']) > 0.05                       # the Charbonnier term pays about 20/255 on every pixel it sees


def test_vectors_out_of_frame_give_exactly_zero():
    out, d, _ = _entry(out_of_frame_case(*EXACT))
    assert out[0] == 0.0 and out[1] == 0.0
    assert not d.any()


# ------------------------------------------------------------------ structure
def test_accumulate_guard_bands_value_only_and_repeats():
    shape = (2, 37, 53, 3)
    B, H, W, n = shape
    for with_mask in (True, False):
        case = make_case(*shape, with_mask=with_mask)
        out, stored, _ = _entry(case, census_weight=0.7, upstream=1.5)
        assert stored.any()
        # accumulate = 1 over a pattern: prefill + the stored result, one float32 addition each; NaN bands around d_preds and in
        # the gaps of a larger pred_stride stay NaN; add_to is added
        pattern = torch.linspace(-1.0, 1.0, n * 2 * B * H * W, dtype=torch.float32, device='cuda').reshape(n, -1)
        out_acc, acc, slab = _entry(case, census_weight=0.7, upstream=1.5, add_to=0.375, prefill=pattern, gap=10, guard=32)
        np.testing.assert_array_equal(acc, _np(pattern).reshape(acc.shape) + stored)
        stride = 2 * B * H * W + 10
        assert bool(torch.isnan(slab[:32]).all()) and bool(torch.isnan(slab[32 + n * stride:]).all())
        assert bool(torch.isnan(slab[32:32 + n * stride].reshape(n, stride)[:, 2 * B * H * W:]).all())
        assert out_acc[1].tobytes() == out[1].tobytes()
        assert abs(float(out_acc[0]) - (0.375 + float(out[0]))) <= 2 * U
        # accumulate = 0 writes every element (a NaN slab underneath), in the gapped layout too
        _, again, slab0 = _entry(case, census_weight=0.7, upstream=1.5, gap=10, guard=32)
        assert again.tobytes() == stored.tobytes()
        assert bool(torch.isnan(slab0[32:32 + n * stride].reshape(n, stride)[:, 2 * B * H * W:]).all())
        # value only: the same out2 bits; repeats: the same bits
        only, none, _ = _entry(case, census_weight=0.7, upstream=1.5, want_grad=False)
        assert none is None and only.tobytes() == out.tobytes()
        out_b, stored_b, _ = _entry(case, census_weight=0.7, upstream=1.5)
        assert out_b.tobytes() == out.tobytes() and stored_b.tobytes() == stored.tobytes()


def test_python_entries_agree_and_census_weight_zero_is_the_call_without_it():
    from tf_raft_amd import grad, losses
    image1, image2, mask, preds = make_case(2, 37, 53, 3)
    y_true = (image1, image2, mask)
    terms, grads = _run((image1, image2, mask, preds), census_weight=0.5)
    loss = losses.PhotometricSequenceLoss(census_weight=0.5, **DEFAULTS)
    only = loss.terms(y_true, preds)
    assert list(only) == ['loss', 'photometric', 'census', 'smoothness']
    for k in terms:
        assert _np(only[k]).reshape(()).astype(np.float32).tobytes() == terms[k].tobytes(), k
    assert _np(losses.photometric_sequence_loss(y_true, preds, census_weight=0.5)).tobytes() == terms['loss'].tobytes()
    assert _np(loss(y_true, preds)).tobytes() == terms['loss'].tobytes()
    for a, b in zip(grads, grad.photometric_sequence_loss_grad(y_true, preds, census_weight=0.5)):
        assert a.tobytes() == _np(b).tobytes()
    # the entry on top of the photometric launch is the entry alone on top of the photometric results
    plain_terms, plain_grads = grad.photometric_sequence_loss_value_and_grad(y_true, preds, **DEFAULTS)
    zero_terms, zero_grads = grad.photometric_sequence_loss_value_and_grad(y_true, preds, census_weight=0.0, **DEFAULTS)
    assert set(plain_terms) == set(zero_terms) == {'loss', 'photometric', 'smoothness'}
    for k in plain_terms:
        assert _np(plain_terms[k]).tobytes() == _np(zero_terms[k]).tobytes(), k
    for a, b in zip(plain_grads, zero_grads):
        assert _np(a).tobytes() == _np(b).tobytes()
    for k in ('photometric', 'smoothness'):
        assert _np(plain_terms[k]).reshape(()).astype(np.float32).tobytes() == terms[k].tobytes(), k
    out, stored, _ = _entry((image1, image2, mask, preds), census_weight=0.5, add_to=float(_np(plain_terms['loss'])))
    assert out[0].tobytes() == terms['loss'].tobytes() and out[1].tobytes() == terms['census'].tobytes()
    for i, g in enumerate(grads):
        np.testing.assert_array_equal(_np(plain_grads[i]) + stored[i], g)


# ------------------------------------------------------------------ end to end
def _reference_census_train_steps(wts, batches, iters, lr_fn, wd, clip_norm, n_steps, params, census_weight):
    """tests/test_gpu_photometric_loss.py::_reference_photometric_train_steps with the census yardstick added to the loss: the
    reference's train_step restricted to the update block, on the oracle in float64 with autograd, tf.clip_by_global_norm and
    tfa AdamW.  Returns (losses, updated update-block weights)."""
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
        loss = torch_total_loss(i1, i2, mask, preds, census_weight, **params)[0]
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


def test_train_step_with_the_census_term_matches_reference_semantics(rng):
    """test_gpu_photometric_loss.py::test_train_step_with_the_photometric_loss_matches_reference_semantics with census_weight = 1:
    two steps at (1, 64, 96), iters = 3, conditioned weights, trainable='update_block', cyclical learning rate + AdamW + clip 1.0,
    against the same procedure on the float64 oracle with the float64 yardstick loss, within that test's bounds.  Step 0 carries
    a mask, step 1 none."""
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
    model.compile(optimizer=training.AdamW(wd, sched), clip_norm=clip, loss=losses.PhotometricSequenceLoss(census_weight=1.0, **DEFAULTS),
                  trainable='update_block')
    with pytest.raises(ValueError, match='image1, image2, mask'):
        model.train_step(batches[0] + (batches[0][2],))
    got_losses = []
    for step in range(n_steps):
        res = model.train_step(batches[step])
        assert list(res) == ['loss', 'photometric', 'census', 'smoothness']
        got_losses.append(float(model.flow_metrics['loss'].total))
    assert float(res['census']) > 0
    got_losses = [got_losses[0]] + [b - a for a, b in zip(got_losses, got_losses[1:])]
    want_losses, want_w = _reference_census_train_steps(wts, batches, iters, sched, wd, clip, n_steps, DEFAULTS, 1.0)
    report('census train_step losses', got0=got_losses[0], want0=want_losses[0], got1=got_losses[1], want1=want_losses[1])
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
    report('census train_step updated weights', frac_elements_off_by_quarter_lr=bad / total, rel_l2_of_update=float(np.sqrt(num / den)))
    assert bad / total <= 0.02
    assert np.sqrt(num / den) <= 0.1
    out = model([batches[0][0], batches[0][1]])
    assert len(out) == 4 and np.isfinite(out[-1].numpy()).all()


@pytest.mark.parametrize('variant', ['small', 'raft_all'])
def test_one_census_step_of_the_other_configurations(rng, variant):
    """SmallRAFT, and RAFT with trainable='all': finite terms, exactly the four keys, the weights moved."""
    import tf_raft_amd
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    B, H, W = 2, 64, 96
    loss = losses.PhotometricSequenceLoss(census_weight=1.0)
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
    assert list(res) == ['loss', 'photometric', 'census', 'smoothness']
    vals = losses.to_floats(res)
    assert all(np.isfinite(v) and v > 0 for v in vals.values()), vals
    new = model.get_weights_dict()
    moved = [k for k in new if not np.array_equal(new[k], wts[k])]
    assert all(k in moved for k in new if k.endswith('kernel')), [k for k in new if k.endswith('kernel') and k not in moved]
    report(f'census train_step {variant}', tensors_moved=len(moved), **vals)

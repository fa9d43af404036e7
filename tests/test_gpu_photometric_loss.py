"""Self-supervised sequence loss on the GPU: raft_photometric_loss_f32 and the layers above it against the
float64 yardstick of tests/test_photometric_loss.py.

Tolerances of the parity test, per case: the float32 restatement's own measured distance to the yardstick times 4 (a different
summation order over the three channels and the four smoothness terms, hardware exp / sqrt / division), with the floors
8 * 2^-24 relative for the values and 16 * 2^-24 * max|g| for the gradient.

Measured (MI355X, with mask; the base is what the restatement itself is away from float64, then what the kernel is.  The kernel's
distances equal the restatement's to the printed digits, from a list of tensors and from views of one buffer alike; without a mask the
orders are the same and 1x3x5x1 is the one case that differs: kernel 5.1e-08, 9.8e-08 against base 4.3e-08, 1.3e-07):

    case (B,H,W,n)   base: loss rel, gradient / max|g|     kernel: loss rel, gradient / max|g|
    1x3x5x1          3.7e-08, 6.9e-08                      3.7e-08, 6.9e-08
    1x1x7x2          5.5e-09, 5.3e-07                      5.5e-09, 5.3e-07
    1x6x1x2          4.1e-08, 2.2e-07                      4.1e-08, 2.2e-07
    2x37x53x3        7.2e-08, 4.2e-05                      7.2e-08, 4.2e-05
    1x3x2051x2       6.5e-09, 8.2e-04                      6.5e-09, 8.2e-04
    2x64x96x12       3.5e-08, 7.4e-05                      3.5e-08, 7.4e-05
    1x100x150x2      4.3e-08, 1.0e-04                      4.3e-08, 1.0e-04

End to end (two steps against the float64 oracle with the yardstick loss): losses 0.5325 / 0.6697 on both sides, 1.3e-6 of the update's
elements off by more than 0.25 * lr, relative L2 of the update 6.1e-3.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import report
from test_photometric_loss import (CASE_IDS, CASES, DEFAULTS, make_case, np_photometric_loss, out_of_frame_case, restatement_distance,
                                   shift_case, torch_photometric_loss, ulps, yardstick, zero_flow_case)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _np(t):
    return t.detach().cpu().numpy()


def _as_views(preds):
    """The predictions as views of one (n, B, H, W, 2) device buffer, the way the model returns them."""
    buf = torch.as_tensor(np.stack(preds)).cuda().contiguous()
    return [buf[i] for i in range(buf.shape[0])]


def _run(case, views=False, upstream=1.0, **params):
    """``(terms as floats32 NumPy scalars, [gradients as NumPy])`` through grad.photometric_sequence_loss_value_and_grad."""
    from tf_raft_amd import grad
    image1, image2, mask, preds = case
    y_true = (image1, image2) if mask is None else (image1, image2, mask)
    terms, grads = grad.photometric_sequence_loss_value_and_grad(y_true, _as_views(preds) if views else preds, upstream=upstream,
                                                                 **dict(DEFAULTS, **params))
    assert set(terms) == {'loss', 'photometric', 'smoothness'} and len(grads) == len(preds)
    return {k: _np(v).reshape(()).astype(np.float32)[()] for k, v in terms.items()}, [_np(g) for g in grads]


@functools.lru_cache(maxsize=None)
def _yardstick(shape, with_mask):
    return yardstick(make_case(*shape, with_mask=with_mask), **DEFAULTS)


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize('views', [False, True], ids=['list', 'views'])
@pytest.mark.parametrize('with_mask', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('shape', CASES, ids=CASE_IDS)
def test_value_and_gradient_match_the_float64_yardstick(shape, with_mask, views):
    case = make_case(*shape, with_mask=with_mask)
    want_loss, want_ph, want_sm, want_g = _yardstick(shape, with_mask)
    base_loss, base_g, max_g = restatement_distance(*shape, with_mask)
    terms, grads = _run(case, views=views)
    rel = abs(float(terms['loss']) - want_loss) / abs(want_loss)
    diff = max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(grads, want_g))
    report(f'photometric loss {shape} mask={with_mask} views={views}', base_loss_rel=base_loss, loss_rel=rel,
           base_grad_over_max=base_g / max_g, grad_over_max=diff / max_g)
    assert rel <= max(4 * base_loss, 8 * U)
    assert diff <= max(4 * base_g, 16 * U * max_g)
    assert all(g.shape == tuple(shape[:3]) + (2,) and g.dtype == np.float32 for g in grads)
    # the two reported terms are the last prediction's: against the yardstick at the values' floor or 4 x the restatement's distance
    _, ph32, sm32, _ = np_photometric_loss(*case, **DEFAULTS)
    for got, want, own in ((terms['photometric'], want_ph, ph32), (terms['smoothness'], want_sm, sm32)):
        assert abs(float(got) - want) <= max(4 * abs(float(own) - want), 8 * U * abs(want)), (got, want)


# ------------------------------------------------------------------ cases with a known answer
EXACT = (2, 37, 53, 2)


def test_zero_flow_between_equal_frames():
    case, closed = zero_flow_case(*EXACT)
    terms, grads = _run(case)
    assert all(not g.any() for g in grads)
    assert ulps(terms['photometric'], closed['photometric']) <= 4
    assert ulps(terms['smoothness'], closed['smoothness']) <= 4


@pytest.mark.parametrize('d', [(3, -2), (-5, 1)], ids=['3,-2', '-5,1'])
def test_constant_integer_flow_between_shifted_frames(d):
    case, closed = shift_case(*EXACT, d)
    terms, grads = _run(case)
    assert all(not g.any() for g in grads)
    report(f'photometric shift {d}', photometric_ulps=ulps(terms['photometric'], closed['photometric']),
           smoothness_ulps=ulps(terms['smoothness'], closed['smoothness']))
    assert ulps(terms['photometric'], closed['photometric']) <= 4
    assert ulps(terms['smoothness'], closed['smoothness']) <= 4


def test_vectors_out_of_frame_and_masked_pixels():
    case = out_of_frame_case(*EXACT)
    terms, grads = _run(case, smooth_weight=0.0)
    assert float(terms['loss']) == 0.0 and float(terms['photometric']) == 0.0
    assert all(not g.any() for g in grads)
    # masked pixels receive exactly the smoothness-only gradient: whatever image2 holds does not reach them
    image1, image2, mask, preds = make_case(*EXACT)
    noise = np.random.default_rng(9).integers(0, 256, size=image2.shape).astype(np.float32)
    _, g_a = _run((image1, image2, mask, preds))
    _, g_b = _run((image1, noise, mask, preds))
    for a, b in zip(g_a, g_b):
        np.testing.assert_array_equal(a[mask == 0], b[mask == 0])
        assert (a[mask != 0] != b[mask != 0]).any()


# ------------------------------------------------------------------ structure
def test_the_gradient_is_written_only_inside_its_extent():
    """NaN guard bands around d_preds, and a pred_stride larger than 2 * npix whose gaps stay untouched."""
    from tf_raft_amd import _dev, losses
    from tf_raft_amd._ffi import check
    B, H, W, n = 2, 37, 53, 3
    image1, image2, mask, preds = make_case(B, H, W, n)
    npix = B * H * W
    stride = 2 * npix + 10                                          # even, with a gap of 10 floats behind every prediction
    i1, i2, m = (torch.as_tensor(a).cuda() for a in (image1, image2, mask))
    src = torch.zeros((n * stride,), dtype=torch.float32, device='cuda')
    for i, p in enumerate(preds):
        src[i * stride:i * stride + 2 * npix] = torch.as_tensor(p).cuda().reshape(-1)
    slab = torch.full((n * stride + 64,), float('nan'), dtype=torch.float32, device='cuda')
    dst = slab[32:32 + n * stride]
    out = torch.empty((3,), dtype=torch.float32, device='cuda')
    ws = losses._photometric_workspace(out.device)
    check(_dev.lib().raft_photometric_loss_f32(_dev.ptr(i1), _dev.ptr(i2), _dev.ptr(m), _dev.ptr(src), stride, n, B, H, W, 0.8, 0.1, 10.0, 0.01,
                                               1.0, _dev.ptr(out), _dev.ptr(dst), _dev.ptr(ws), _dev.stream_ptr()), 'photometric_loss')
    torch.cuda.synchronize()
    assert bool(torch.isnan(slab[:32]).all()) and bool(torch.isnan(slab[32 + n * stride:]).all())
    got = dst.reshape(n, stride)
    assert bool(torch.isnan(got[:, 2 * npix:]).all())               # the gaps
    assert not bool(torch.isnan(got[:, :2 * npix]).any())           # every element of the gradient was written
    terms, grads = _run((image1, image2, mask, preds))
    for i in range(n):
        np.testing.assert_array_equal(_np(got[i, :2 * npix]).reshape(B, H, W, 2), grads[i])
    np.testing.assert_array_equal(_np(out), np.array([terms['loss'], terms['photometric'], terms['smoothness']], np.float32))


def test_value_only_repeat_gamma_one_and_upstream():
    from tf_raft_amd import grad, losses
    image1, image2, mask, preds = make_case(2, 37, 53, 3)
    for m in (mask, None):
        case = (image1, image2, m, preds)
        y_true = (image1, image2) if m is None else (image1, image2, m)
        terms, grads = _run(case)
        # value-only and value + gradient: the same three floats, bit for bit; two runs are bit-identical
        only = losses.PhotometricSequenceLoss(**DEFAULTS).terms(y_true, preds)
        for k in terms:
            assert _np(only[k]).reshape(()).astype(np.float32).tobytes() == terms[k].tobytes(), k
        assert _np(losses.photometric_sequence_loss(y_true, preds)).tobytes() == terms['loss'].tobytes()
        again, grads2 = _run(case)
        assert all(again[k].tobytes() == terms[k].tobytes() for k in terms)
        for a, b in zip(grads, grads2):
            assert a.tobytes() == b.tobytes()
        only_g = grad.photometric_sequence_loss_grad(y_true, preds)
        for a, b in zip(grads, only_g):
            assert a.tobytes() == _np(b).tobytes()
        # upstream = 2 doubles the gradient, bit for bit
        _, doubled = _run(case, upstream=2.0)
        for a, b in zip(grads, doubled):
            np.testing.assert_array_equal(2 * a, b)
        # gamma = 1 over n predictions: the sum of the single-prediction losses
        total = float(_run(case, gamma=1.0)[0]['loss'])
        parts = sum(float(_run((image1, image2, m, [p]), gamma=1.0)[0]['loss']) for p in preds)
        assert abs(total - parts) <= 1e-6 * abs(parts)


# ------------------------------------------------------------------ end to end
def _reference_photometric_train_steps(wts, batches, iters, lr_fn, wd, clip_norm, n_steps, params):
    """tests/test_gpu_backward.py::_reference_train_steps with the float64 yardstick loss in the place of sequence_loss: the
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
        loss = torch_photometric_loss(i1, i2, mask, preds, **params)[0]
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


def test_train_step_with_the_photometric_loss_matches_reference_semantics(rng):
    """test_gpu_backward.py::test_train_step_update_block_matches_reference_semantics with unlabelled pairs: two steps at
    (1, 64, 96), iters = 3, conditioned weights, trainable='update_block', cyclical learning rate + AdamW + clip 1.0, against the
    same procedure on the float64 oracle with the float64 yardstick loss, within that test's bounds.  Step 0 carries a mask,
    step 1 none."""
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
    model.compile(optimizer=training.AdamW(wd, sched), clip_norm=clip, loss=losses.PhotometricSequenceLoss(**DEFAULTS),
                  trainable='update_block')
    with pytest.raises(ValueError, match='image1, image2, mask'):
        model.train_step(batches[0] + (batches[0][2],))
    got_losses = []
    for step in range(n_steps):
        res = model.train_step(batches[step])
        assert set(res) == {'loss', 'photometric', 'smoothness'}
        got_losses.append(float(model.flow_metrics['loss'].total))
    got_losses = [got_losses[0]] + [b - a for a, b in zip(got_losses, got_losses[1:])]
    want_losses, want_w = _reference_photometric_train_steps(wts, batches, iters, sched, wd, clip, n_steps, DEFAULTS)
    report('photometric train_step losses', got0=got_losses[0], want0=want_losses[0], got1=got_losses[1], want1=want_losses[1])
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
    report('photometric train_step updated weights', frac_elements_off_by_quarter_lr=bad / total,
           rel_l2_of_update=float(np.sqrt(num / den)))
    assert bad / total <= 0.02
    assert np.sqrt(num / den) <= 0.1
    out = model([batches[0][0], batches[0][1]])
    assert len(out) == 4 and np.isfinite(out[-1].numpy()).all()


@pytest.mark.parametrize('variant', ['small', 'raft_all_bf16_dropout'])
def test_one_photometric_step_of_the_other_configurations(rng, variant):
    """SmallRAFT, and RAFT with trainable='all', the bf16 tape and dropout: finite terms, exactly the three keys, the weights
    moved, the model still predicts."""
    import tf_raft_amd
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    B, H, W = 2, 64, 96
    if variant == 'small':
        wts = wm.condition_weights('small', wm.init_weights('small', seed=2, perturb=True), 'mid')
        model = tf_raft_amd.SmallRAFT(weights=wts, iters=2, iters_pred=2)
        model.compile(optimizer=training.AdamW(1e-4, 1e-3), clip_norm=1.0, loss=losses.PhotometricSequenceLoss())
    else:
        wts = wm.condition_weights('raft', wm.init_weights('raft', seed=2, perturb=True), 'mid')
        model = tf_raft_amd.RAFT(drop_rate=0.1, weights=wts, iters=2, iters_pred=2)
        model.compile(optimizer=training.AdamW(1e-4, 1e-3), clip_norm=1.0, loss=losses.PhotometricSequenceLoss(), trainable='all',
                      tape_dtype='bf16')
    i1 = rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32)
    i2 = rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32)
    res = model.train_step((i1, i2, rng.uniform(size=(B, H, W)) < 0.8))
    assert list(res) == ['loss', 'photometric', 'smoothness']
    vals = losses.to_floats(res)
    assert all(np.isfinite(v) and v > 0 for v in vals.values()), vals
    new = model.get_weights_dict()
    moved = [k for k in new if not np.array_equal(new[k], wts[k])]
    assert all(k in moved for k in new if k.endswith('kernel')), [k for k in new if k.endswith('kernel') and k not in moved]
    out = model([i1, i2])
    assert np.isfinite(_np(out[-1])).all()
    report(f'photometric train_step {variant}', tensors_moved=len(moved), **vals)


# loss of the supervised step below on the parent commit (the commit before the photometric loss existed), as float32 bits
PARENT_SUPERVISED_LOSS_BITS = 0x40637c50          # 3.554462432861328


def test_the_supervised_step_is_what_it_was(rng):
    """compile(loss=sequence_loss) and train_step on a labelled batch: the keys and the bits of the loss the parent commit gave for
    this seed."""
    import tf_raft_amd
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    B, H, W = 1, 64, 96
    wts = wm.condition_weights('raft', wm.init_weights('raft', seed=5))
    model = tf_raft_amd.RAFT(weights=wts, iters=3, iters_pred=4)
    model.compile(optimizer=training.AdamW(1e-4, 4e-4), clip_norm=1.0, loss=losses.sequence_loss, epe=losses.end_point_error,
                  trainable='update_block')
    data = (rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32), rng.uniform(0, 255, (B, H, W, 3)).astype(np.float32),
            (rng.normal(size=(B, H, W, 2)) * 2).astype(np.float32), rng.uniform(size=(B, H, W)) < 0.9)
    res = model.train_step(data)
    assert list(res) == ['loss', 'epe', 'u1', 'u3', 'u5']
    bits = int(np.float32(float(res['loss'])).view(np.uint32))
    print(f'[photometric] supervised loss {float(res["loss"])!r} bits 0x{bits:08x}')
    assert bits == PARENT_SUPERVISED_LOSS_BITS

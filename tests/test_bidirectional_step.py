"""Bidirectional training step with in-step occlusion masks, host side (no GPU): the NumPy restatement of
``raft_flow_visibility_f32`` built on tests/test_consistency.py's restatement of the consistency test, the two C entries'
declarations and argument checks, ``compile``'s validation, ``train_step``'s tuple errors, and the float64 oracle of the
update-block step with the check that its visibility mask is stable against float32 arithmetic for the inputs and the ``beta``
that tests/test_gpu_bidirectional_step.py uses.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tf_raft_amd import _ffi
from test_consistency import analytic_case, np_bilinear, np_flow_consistency, parity_flows
from test_photometric_loss import DEFAULTS, torch_photometric_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement
def np_flow_visibility(flows, N, mask=None, alpha=0.01, beta=0.5, apply=True):
    """``(visible uint8 (2N, H, W), occluded_fraction float32, occluded bool)``: slice ``s < N`` tested against ``s + N`` and the
    other way round by ``np_flow_consistency``, inverted, ANDed with ``mask``; the share counts every occluded pixel whatever
    ``apply`` and ``mask`` are, divided in double and rounded once."""
    flows = np.asarray(flows)
    assert flows.shape[0] == 2 * N
    fwd, bwd = flows[:N], flows[N:]
    occ = np.concatenate([np_flow_consistency(fwd, bwd, alpha, beta)[0], np_flow_consistency(bwd, fwd, alpha, beta)[0]])
    use = np.ones(occ.shape, bool) if mask is None else np.asarray(mask) != 0
    visible = use & ~(occ & bool(apply))
    return visible.astype(np.uint8), np.float32(np.float64(occ.sum()) / np.float64(occ.size)), occ


def np_visibility_f64(flows, N, alpha, beta):
    """The same test with EVERYTHING in float64, sample positions included (the oracle's own mask): ``(occluded, margin)``."""
    flows = np.asarray(flows, np.float64)
    _, H, W, _ = flows.shape
    out, margins = [], []
    for own, other in ((flows[:N], flows[N:]), (flows[N:], flows[:N])):
        sx = np.arange(W, dtype=np.float64)[None, None, :] + own[..., 0]
        sy = np.arange(H, dtype=np.float64)[None, :, None] + own[..., 1]
        inside = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
        s = np_bilinear(other, sx, sy, inside)
        lhs = ((own + s) ** 2).sum(-1)
        rhs = alpha * ((own ** 2).sum(-1) + (s ** 2).sum(-1)) + beta
        out.append(~(inside & (lhs <= rhs)))
        margins.append(lhs - rhs)
    return np.concatenate(out), np.concatenate(margins)


def visibility_flows(N, H, W, seed):
    """(2N, H, W, 2) float32: sub-pixel vectors, whole-pixel disagreement between the directions, vectors that leave the frame,
    and one NaN vector."""
    rng = np.random.default_rng(seed)
    if W >= 12 and H >= 12:
        fwd, bwd = parity_flows(H, W, N, seed)
    else:
        fwd = rng.uniform(-0.4, 0.4, (N, H, W, 2)).astype(np.float32)
        fwd[:, 1:, :, 1] = -np.abs(fwd[:, 1:, :, 1])              # (three rows: no vector of one direction reaches the NaN below)
        bwd = (-fwd + rng.uniform(-0.1, 0.1, (N, H, W, 2))).astype(np.float32)
        for f in (fwd, bwd):                                       # sub-pixel vectors that stay in the frame
            f[:, 0, :, 1], f[:, -1, :, 1] = np.abs(f[:, 0, :, 1]), -np.abs(f[:, -1, :, 1])
            f[:, :, 0, 0], f[:, :, -1, 0] = np.abs(f[:, :, 0, 0]), -np.abs(f[:, :, -1, 0])
            if W == 1:
                f[..., 0] = 0
        if W > 1:
            bwd[:, H // 2, W // 2] = (0.0, -1.0)                   # whole-pixel disagreement between the directions
        fwd[:, 0, 0] = (0.0, -1.5)                                 # leaves the frame
    flows = np.ascontiguousarray(np.concatenate([fwd, bwd]), np.float32)
    flows[-1, -1, -1] = (np.nan, 0.25)
    return flows


@pytest.mark.parametrize('H,W', [(37, 53), (64, 96)])
def test_the_restatement_on_a_moving_square(H, W):
    """The analytic case of tests/test_consistency.py: the occluded pixels are the background the square covers (forward) and
    uncovers (backward); visibility is their complement ANDed with the mask, and the share is their count."""
    N = 2
    _, _, fwd, bwd, sq1, sq2 = analytic_case(H, W, N=N)
    flows = np.concatenate([fwd, bwd])
    covered, uncovered = sq2 & ~sq1, sq1 & ~sq2
    want_occ = np.stack([covered] * N + [uncovered] * N)
    mask = (np.random.default_rng(0).uniform(size=(2 * N, H, W)) < 0.7).astype(np.uint8) * 3       # (nonzero = use)
    count = np.float32(np.float64(want_occ.sum()) / (2 * N * H * W))
    for m in (None, mask):
        use = np.ones_like(want_occ) if m is None else m != 0
        vis, frac, occ = np_flow_visibility(flows, N, m, apply=True)
        np.testing.assert_array_equal(occ, want_occ)
        np.testing.assert_array_equal(vis, (use & ~want_occ).astype(np.uint8))
        assert frac == count and frac.dtype == np.float32
        vis, frac, _ = np_flow_visibility(flows, N, m, apply=False)
        np.testing.assert_array_equal(vis, use.astype(np.uint8))
        assert frac == count
    occ64, _ = np_visibility_f64(flows, N, 0.01, 0.5)
    np.testing.assert_array_equal(occ64, want_occ)


@pytest.mark.parametrize('shape', [(1, 3, 1), (1, 5, 7), (2, 37, 53)])
def test_the_test_flows_exercise_every_branch(shape):
    N, H, W = shape
    flows = visibility_flows(N, H, W, seed=H + W)
    _, frac, occ = np_flow_visibility(flows, N)
    assert occ[-1, -1, -1] and occ[0, 0, 0] and 0.0 < float(frac) < 1.0
    assert occ[:N].any() and occ[N:].any() and not occ[:N].all() and not occ[N:].all()
    assert np.isnan(flows).sum() == 1


# ------------------------------------------------------------------ the C entries
def test_the_header_declares_and_the_library_exports_the_entries():
    with open(os.path.join(ROOT, 'include', 'raft_hip.h')) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    assert re.search(r'int64_t\s+raft_flow_visibility_workspace_doubles\s*\(\s*void\s*\)', header)
    assert re.search(r'int\s+raft_flow_visibility_f32\s*\(', header)
    sigs = _ffi.header_signatures(header)
    P, I, F = C.c_void_p, C.c_int, C.c_float
    assert sigs['raft_flow_visibility_workspace_doubles'] == (C.c_int64, [])
    assert sigs['raft_flow_visibility_f32'] == (I, [P, P, P, P, I, I, I, F, F, I, P, P])
    assert _ffi.ABI_VERSION == 222                                   # entries were added, no signature changed
    lib = _ffi.load_library()
    assert lib.raft_flow_visibility_workspace_doubles() >= 1
    assert len(lib.raft_flow_visibility_f32.argtypes) == 12


def test_visibility_argument_errors_are_returned_before_any_device_work():
    """No GPU here: a call that got past its checks would fail in the launch (a positive hipError_t) or crash.  The order is the
    header's: NULL, then sizes, alpha / beta, apply, then alignment."""
    lib = _ffi.load_library()
    fn = lib.raft_flow_visibility_f32
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off = C.c_void_p(p.value + 4)
    #       flows mask visible fraction N  H  W  alpha beta apply ws stream
    good = [p, p, p, p, 1, 4, 5, 0.01, 0.5, 1, p, None]
    for k in (0, 3, 10):                                                    # (mask and visible may be NULL)
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    for k in (4, 5, 6):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for bad in ((1, 1 << 14, 1 << 15), (1 << 9, 1 << 10, 1 << 10), (1, 1, 1 << 29), ((1 << 30) + 1, 1, 1), (1 << 29, 1, 1)):   # 2N*H*W*2 reaches 2^31
        args = list(good)
        args[4:7] = bad
        assert fn(*args) == -2, bad
    for k in (7, 8):
        for v in (-1e-3, float('nan'), float('inf'), -float('inf')):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for v in (-1, 2):
        args = list(good)
        args[9] = v
        assert fn(*args) == -2, v
    for k in (0, 10):
        for m, vis in ((p, p), (None, None)):
            args = list(good)
            args[k], args[1], args[2] = off, m, vis
            assert fn(*args) == -4, (k, m)
    # precedence: NULL before shape before alignment
    args = list(good)
    args[0], args[4], args[10] = None, 0, off
    assert fn(*args) == -1
    args[0] = off
    assert fn(*args) == -2
    args[4], args[9] = 1, 7
    assert fn(*args) == -2
    args[9] = 0
    assert fn(*args) == -4


# ------------------------------------------------------------------ compile and train_step, nothing reaches the device
def test_compile_validates_the_bidirectional_arguments():
    import inspect
    from tf_raft_amd import image_ops, losses
    from tf_raft_amd.model import RAFT, SmallRAFT
    sig = inspect.signature(RAFT.compile).parameters
    assert sig['bidirectional'].default is False and sig['occlusion'].default is True
    assert (sig['alpha'].default, sig['beta'].default) == (image_ops.CONSISTENCY_ALPHA, image_ops.CONSISTENCY_BETA) == (0.01, 0.5)
    for cls in (RAFT, SmallRAFT):
        model = cls.__new__(cls)
        for loss in (None, losses.sequence_loss, lambda y_true, y_pred: 0.0):
            with pytest.raises(ValueError, match='PhotometricSequenceLoss'):
                model.compile(optimizer=None, loss=loss, bidirectional=True)
        for bad in (-0.01, float('nan'), float('inf'), 'x', None, True):
            with pytest.raises(ValueError, match='alpha'):
                model.compile(optimizer=None, loss=losses.PhotometricSequenceLoss(), bidirectional=True, alpha=bad)
            with pytest.raises(ValueError, match='beta'):
                model.compile(optimizer=None, loss=losses.PhotometricSequenceLoss(), bidirectional=True, beta=bad)
        with pytest.raises(ValueError, match='bidirectional'):
            model.compile(optimizer=None, loss=losses.PhotometricSequenceLoss(), bidirectional=1)
        model.compile(optimizer=None, loss=losses.SSIMSequenceLoss(census_weight=0.5, ssim_weight=0.5), bidirectional=True, occlusion=False,
                      alpha=0, beta=np.float32(2))
        assert model.bidirectional is True and model.occlusion is False and model.consistency == (0.0, 2.0)
        assert model.last_visibility is None
        assert model._unlabelled_keys() == ('loss', 'photometric', 'census', 'ssim', 'smoothness', 'occluded')
        assert 'occluded' in model.flow_metrics
        # the default stays what it was: no 'occluded' mean, the keys of the unidirectional step
        for kw in ({}, {'bidirectional': False}):
            model.compile(optimizer=None, loss=losses.PhotometricSequenceLoss(), **kw)
            assert model.bidirectional is False and model.occlusion is True
            assert model._unlabelled_keys() == ('loss', 'photometric', 'smoothness')
            assert 'occluded' not in model.flow_metrics
        model.compile(optimizer=None)
        assert list(model.flow_metrics) == ['loss', 'epe', 'u1', 'u3', 'u5'] and model.bidirectional is False


def test_train_step_names_the_two_forms_before_any_device_work():
    from tf_raft_amd import losses
    from tf_raft_amd.model import RAFT, SmallRAFT
    x = np.zeros((2, 64, 96, 3), np.float32)
    m, flow = np.ones((2, 64, 96), np.uint8), np.zeros((2, 64, 96, 2), np.float32)
    forms = r'\(image1, image2\) or \(image1, image2, \(mask1, mask2\)\)'
    for cls in (RAFT, SmallRAFT):
        model = cls.__new__(cls)                                             # (no device: anything enqueued would fail)
        model.compile(optimizer=None, loss=losses.PhotometricSequenceLoss(), bidirectional=True)
        for data in ((), (x,), (x, x, flow, m), (x, x, m), (x, x, (m,)), (x, x, (m, m, m)), (x, x, (m, m[:1])), (x, x, (m[:, :5], m)),
                     (x, x[:1]), (x[..., :2], x[..., :2]), (x, x, (m, None)), 5):
            with pytest.raises(ValueError, match=forms):
                model.train_step(data)


# ------------------------------------------------------------------ the float64 oracle of the update-block step
# alpha = 0 and beta just under the median of the float64 oracle's |f + s|^2 at step 0.  With these inputs that quantity has two
# modes at step 0 (quartiles 0.81 / 1.69 / 1.80); 1.4 lies in the valley between them, where no pixel is within 1e-4 of the
# threshold, and marks 62 % of the pixels.  (UnFlow's beta = 0.5 would mark nearly all of them.)  At step 1 the updated weights
# give |f + s|^2 of 23 and more, so every pixel is marked and the step's data term is empty: the mask comparison there is of
# two all-zero masks, the loss is the smoothness term.  Derived with `PYTHONPATH=. python tests/test_bidirectional_step.py`,
# which prints the quantiles; test_the_oracle_mask_is_stable_in_float32 keeps the choice honest.
ORACLE_ALPHA, ORACLE_BETA = 0.0, 1.4
ORACLE_SHAPE, ORACLE_ITERS, ORACLE_STEPS = (1, 64, 96), 3, 2
ORACLE_LR0, ORACLE_WD, ORACLE_CLIP = 4e-4, 1e-4, 1.0


def oracle_case():
    """Weights and the two batches of the update-block test: step 0 carries a mask pair, step 1 none."""
    from tf_raft_amd import weights as wm
    N, H, W = ORACLE_SHAPE
    rng = np.random.default_rng(20)
    wts = wm.condition_weights('raft', wm.init_weights('raft', seed=5))
    batches = []
    for step in range(ORACLE_STEPS):
        i1 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
        i2 = rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32)
        masks = tuple((rng.uniform(size=(N, H, W)) < 0.8).astype(np.uint8) for _ in range(2))
        batches.append((i1, i2, masks) if step == 0 else (i1, i2))
    return wts, batches


def oracle_schedule():
    from tf_raft_amd import training
    return training.CyclicalLearningRate(ORACLE_LR0, 2 * ORACLE_LR0, step_size=1000, scale_fn=training.first_cycle_scaler, scale_mode='cycle')


def reference_bidirectional_train_steps(wts, batches, iters, lr_fn, wd, clip_norm, n_steps, params, alpha, beta, occlusion=True,
                                        loss_masks=None, dtype=torch.float64):
    """tests/test_gpu_photometric_loss.py::_reference_photometric_train_steps on the doubled batch [i1 | i2], [i2 | i1]: the
    update block trained on the oracle under autograd with the yardstick loss, clip_by_global_norm and AdamW.  Every step
    computes its own visibility from its own last prediction in float64 (``np_visibility_f64``).  The mask of the loss is
    ``loss_masks[step]`` when given (the device's, so that a pixel on the threshold cannot move the loss), else the oracle's
    own, ANDed with the user's.  Returns (losses, updated weights, [occluded per step], [margin per step])."""
    import oracle
    from oracle.layers import W, basic_update_block, encoder
    from oracle.model import upsample_flow
    names = sorted(k for k in wts if k.startswith('update_block'))
    var = {k: torch.tensor(wts[k], dtype=dtype) for k in names}
    m = {k: torch.zeros_like(v) for k, v in var.items()}
    v2 = {k: torch.zeros_like(v) for k, v in var.items()}
    frozen = W({k: val for k, val in wts.items() if not k.startswith('update_block')}, dtype)
    losses, occs, margins = [], [], []
    for step in range(n_steps):
        N = batches[step][0].shape[0]
        i1 = np.concatenate([batches[step][0], batches[step][1]])
        i2 = np.concatenate([batches[step][1], batches[step][0]])
        user = np.concatenate(batches[step][2]) != 0 if len(batches[step]) == 3 else np.ones(i1.shape[:3], bool)
        with torch.no_grad():
            x1 = 2 * (torch.tensor(i1, dtype=dtype) / 255.0) - 1.0
            x2 = 2 * (torch.tensor(i2, dtype=dtype) / 255.0) - 1.0
            f1, f2 = encoder(frozen, 'fnet', [x1, x2])
            corr_blk = oracle.CorrBlock(f1, f2, 4, 4)
            cnet = encoder(frozen, 'cnet', x1)
            net, inp = torch.tanh(cnet[..., :128]), torch.relu(cnet[..., 128:])
        ow = W({}, dtype)
        ow.t = {k: val.clone().requires_grad_(True) for k, val in var.items()}
        B, h, w, _ = net.shape
        coords0 = oracle.coords_grid(B, h, w, dtype)
        coords1, preds = coords0.clone(), []
        for _ in range(iters):
            corr = corr_blk.retrieve(coords1)
            net, up_mask, delta = basic_update_block(ow, 'update_block', net, inp, corr, coords1 - coords0)
            coords1 = coords1 + delta
            preds.append(upsample_flow(coords1 - coords0, up_mask))
        if dtype == torch.float64:
            occ, margin = np_visibility_f64(preds[-1].detach().numpy(), N, alpha, beta)
        else:                                       # (the stability check: float32 flows and sample positions)
            occ, margin = np_flow_visibility(preds[-1].detach().numpy(), N, None, alpha, beta)[2], None
        occs.append(occ)
        margins.append(margin)
        mask = loss_masks[step] if loss_masks is not None else (user & ~(occ & bool(occlusion)))
        loss = torch_photometric_loss(i1, i2, np.asarray(mask), [p.double() for p in preds], **params)[0]
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
    return losses, {k: v.detach().numpy() for k, v in var.items()}, occs, margins


def _oracle_run(dtype):
    wts, batches = oracle_case()
    return reference_bidirectional_train_steps(wts, batches, ORACLE_ITERS, oracle_schedule(), ORACLE_WD, ORACLE_CLIP, ORACLE_STEPS, DEFAULTS,
                                               ORACLE_ALPHA, ORACLE_BETA, dtype=dtype)


def test_the_oracle_mask_is_stable_in_float32():
    """The condition the GPU test's cap rests on: with the committed inputs and ``beta`` the float64 oracle marks between 20 % and
    80 % of the pixels at step 0, and the same procedure in float32 disagrees with it on at most 1e-3 of the pixels at either
    step."""
    _, _, occ64, _ = _oracle_run(torch.float64)
    _, _, occ32, _ = _oracle_run(torch.float32)
    share = [float(o.mean()) for o in occ64]
    differ = [float((a != b).mean()) for a, b in zip(occ64, occ32)]
    print(f'[bidirectional] oracle occluded share per step {share}, float32 against float64 disagreement {differ}')
    assert 0.2 <= share[0] <= 0.8
    assert max(differ) <= 1e-3


if __name__ == '__main__':      # how ORACLE_BETA was derived
    ORACLE_BETA = 1.0
    for step, marg in enumerate(_oracle_run(torch.float64)[3]):
        lhs = marg + ORACLE_BETA                                           # (alpha = 0: margin = |f + s|^2 - beta)
        print(f'step {step}: quantiles of |f + s|^2 at 10/25/50/75/90 %:', np.quantile(lhs[np.isfinite(lhs)], [0.1, 0.25, 0.5, 0.75, 0.9]))

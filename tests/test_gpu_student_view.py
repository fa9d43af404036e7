"""The student's view on the GPU: raft_view_frames_f32 and raft_view_flow_f32 against the float32 restatement
(bit for bit) and the float64 yardstick of tests/test_student_view.py, their memory discipline, the known answers on the device,
and ``train_step`` under ``selfsup_transform``: the identity view against the crop step bit for bit, a fixed dyadic view against
the float64 two-pass oracle, and a generic drawn view.

Tolerances of the parity test, per case: four times the float32 restatement's own distance to the yardstick (the table in
tests/test_student_view.py); masks equal outside the band defined there.
"""
import numpy as np
import pytest
import torch

from conftest import report
from test_gpu_bidirectional_step import _update_errors
from test_gpu_selfsup_loss import _model, _pair
from test_photometric_loss import DEFAULTS, torch_photometric_loss
from test_selfsup_loss import (ORACLE_ALPHA, ORACLE_BETA, ORACLE_CLIP, ORACLE_CROP, ORACLE_ITERS, ORACLE_LR0, ORACLE_OCCLUSION,
                               ORACLE_SELFSUP, ORACLE_STEPS, ORACLE_WD, oracle_case, oracle_schedule, torch_selfsup_loss)
from test_student_view import (CASE_IDS, CASES, GENERIC_DRAW, GEOMS, check_affine_teacher, check_constant_teacher,
                               check_identity_is_the_window, check_one_zero_and_one_nan, check_out_of_frame_is_zero, compare_outside_band,
                               flow_f64, frames_f64, np_view_flow, np_view_frames, records_of, restatement_distance, view_case)

pytestmark = pytest.mark.gpu

GUARD = 64


def _np(t):
    return t.detach().as_subclass(torch.Tensor).cpu().numpy()


def _entries(frames, flow, tv, records, size, prefill=0xFF):
    """Both entries called directly with the ``records``: ``(frames out, target, target_visible, intact)``.  Each output lies in
    a slab with ``GUARD`` elements around it -- NaN for the floats, 0xA5 for the bytes, and the mask itself prefilled with
    ``prefill``; ``intact`` says that every guard still holds what it was filled with."""
    from tf_raft_amd import _dev
    from tf_raft_amd._ffi import ViewParams, check
    H, W = size
    B, Ht, Wt, Cn = frames.shape
    dev = _dev.require_gpu()
    up = lambda a: None if a is None else torch.tensor(np.array(a)).to(dev)
    fr, fl, tvd = up(frames), up(flow), up(tv)
    recs = torch.frombuffer(bytearray(bytes((ViewParams * len(records))(*records))), dtype=torch.uint8).to(dev)
    nf, nt, nv = B * H * W * Cn, B * H * W * 2, B * H * W
    slab_f = torch.full((nf + 2 * GUARD,), float('nan'), dtype=torch.float32, device=dev)
    slab_t = torch.full((nt + 2 * GUARD,), float('nan'), dtype=torch.float32, device=dev)
    slab_v = torch.full((nv + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    slab_v[GUARD:GUARD + nv] = prefill
    lib, ptr = _dev.lib(), lambda t: None if t is None else _dev.ptr(t)
    check(lib.raft_view_frames_f32(ptr(fr), ptr(recs), ptr(slab_f[GUARD:]), B, Ht, Wt, H, W, Cn, _dev.stream_ptr()), 'view_frames')
    check(lib.raft_view_flow_f32(ptr(fl), ptr(tvd), ptr(recs), ptr(slab_t[GUARD:]), ptr(slab_v[GUARD:]), B, Ht, Wt, H, W,
                                 _dev.stream_ptr()), 'view_flow')
    torch.cuda.synchronize()
    sf, st, sv = _np(slab_f), _np(slab_t), _np(slab_v)
    intact = bool(np.isnan(sf[:GUARD]).all() and np.isnan(sf[-GUARD:]).all() and np.isnan(st[:GUARD]).all() and np.isnan(st[-GUARD:]).all()
                  and (sv[:GUARD] == 0xA5).all() and (sv[-GUARD:] == 0xA5).all())
    return (sf[GUARD:-GUARD].reshape(B, H, W, Cn).copy(), st[GUARD:-GUARD].reshape(B, H, W, 2).copy(),
            sv[GUARD:-GUARD].reshape(B, H, W).copy(), intact)


class Device:
    """The two gathers through the public ops, as the known answers of tests/test_student_view.py call them."""

    @staticmethod
    def frames(src, view, size):
        from tf_raft_amd import image_ops
        return _np(image_ops.view_frames(np.array(src, np.float32), view, size))       # (a copy: the shared cases are read-only)

    @staticmethod
    def flow(flow, view, size, visible=None):
        from tf_raft_amd import image_ops
        target, vis = image_ops.view_flow(np.array(flow, np.float32), view, size, None if visible is None else np.array(visible))
        assert vis.dtype == torch.uint8
        return _np(target), _np(vis)


# ------------------------------------------------------------------ kernel parity
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_the_kernels_equal_the_restatement_bit_for_bit_and_stay_near_the_yardstick(case):
    (_, (_, H, W)), kind = case
    frames, flow, tv, view = view_case(case)
    recs = records_of(view)
    base_f, base_t, _ = restatement_distance(case)
    out, _ = compare_outside_band(case)
    want_f64, _ = frames_f64(frames, view, (H, W))
    worst_t = 0.0
    for mask in (None, tv):
        got_f, got_t, got_v, intact = _entries(frames, flow, mask, recs, (H, W))
        assert intact
        assert set(np.unique(got_v)) <= {0, 1}                                   # the 0xFF prefill is fully overwritten
        own_t, own_v = np_view_flow(flow, mask, recs, (H, W))
        differing = (int((np_view_frames(frames, recs, (H, W)).view(np.uint32) != got_f.view(np.uint32)).sum()),
                     int((own_t.view(np.uint32) != got_t.view(np.uint32)).sum()), int((own_v != got_v).sum()))
        assert differing == (0, 0, 0), differing
        want_t, want_v = flow_f64(flow, mask, view, (H, W))
        assert np.array_equal(got_v[~out] != 0, want_v[~out])
        worst_t = max(worst_t, float(np.abs(got_t - want_t)[~out].max()))
    worst_f = float(np.abs(got_f - want_f64)[~out].max())
    report(f'student view kernels {CASE_IDS[CASES.index(case)]}', base_frames=base_f, frames=worst_f, base_target=base_t, target=worst_t,
           left_out=float(out.mean()))
    assert worst_f <= 4 * base_f
    assert worst_t <= 4 * base_t
    if kind != 'colour':                                                         # the public ops launch the same: the same bits
        np.testing.assert_array_equal(Device.frames(frames, view, (H, W)).view(np.uint32), got_f.view(np.uint32))
        dt, dv = Device.flow(flow, view, (H, W), tv)
        np.testing.assert_array_equal(dt.view(np.uint32), got_t.view(np.uint32))
        np.testing.assert_array_equal(dv, got_v)


def test_a_teacher_one_pixel_wide_takes_the_unpaired_loads(rng):
    """The flow kernel reads the two taps of a row as one load where the teacher has two columns or more; a teacher of width 1 takes
    the other path.  Teacher (2, 6, 1), student (2, 5, 3): half-pixel rows, two of the three columns out of frame."""
    from tf_raft_amd.augment import StudentView
    frames = rng.uniform(0, 255, (2, 6, 1, 3)).astype(np.float32)
    flow = rng.normal(0, 2, (2, 6, 1, 2)).astype(np.float32)
    tv = (rng.uniform(size=(2, 6, 1)) < 0.7).astype(np.uint8)
    recs = records_of(StudentView(np.array([[[1.0, 0.0, -1.0], [0.0, 1.0, 0.5]], [[-1.0, 0.0, 2.0], [0.0, 0.75, 0.25]]])))
    for mask in (None, tv):
        got_f, got_t, got_v, intact = _entries(frames, flow, mask, recs, (5, 3))
        want_t, want_v = np_view_flow(flow, mask, recs, (5, 3))
        assert intact and 0 < got_v.sum() < got_v.size
        np.testing.assert_array_equal(got_f.view(np.uint32), np_view_frames(frames, recs, (5, 3)).view(np.uint32))
        np.testing.assert_array_equal(got_t.view(np.uint32), want_t.view(np.uint32))
        np.testing.assert_array_equal(got_v, want_v)


def test_repeats_give_the_same_bits_and_other_channel_counts_run():
    case = (GEOMS[2], 'generic')
    frames, flow, tv, view = view_case(case)
    size, recs = GEOMS[2][1][1:], records_of(view)
    first = _entries(frames, flow, tv, recs, size)
    for prefill in (0x00, 0x7F):
        again = _entries(frames, flow, tv, recs, size, prefill=prefill)
        assert again[3] and all(a.tobytes() == b.tobytes() for a, b in zip(first[:3], again[:3]))
    colour = records_of(view_case((GEOMS[2], 'colour'))[3])
    for Cn in (1, 2, 5):                                                         # 5: the loop over any channel count
        src = np.ascontiguousarray(np.resize(frames, frames.shape[:3] + (Cn,)))
        for r in (recs, colour):
            got, _, _, intact = _entries(src, flow, None, r, size)
            assert intact
            np.testing.assert_array_equal(got.view(np.uint32), np_view_frames(src, r, size).view(np.uint32))


# ------------------------------------------------------------------ the known answers on the device
@pytest.mark.parametrize('geom', GEOMS, ids=['x'.join(map(str, g[0])) for g in GEOMS])
def test_the_identity_view_is_window_copy_on_the_device(geom):
    from tf_raft_amd import image_ops
    check_identity_is_the_window(Device, geom)
    frames, _, _, view = view_case((geom, 'identity'))
    size = geom[1][1:]
    np.testing.assert_array_equal(Device.frames(frames, view, size), _np(image_ops.resize_with_crop_or_pad(np.array(frames), *size)))


def test_known_answers_on_the_device():
    check_constant_teacher(Device)
    check_affine_teacher(Device)
    check_one_zero_and_one_nan(Device)
    check_out_of_frame_is_zero(Device)


# ------------------------------------------------------------------ train_step
def test_the_identity_view_is_the_crop_step_bit_for_bit(rng):
    """Two steps, all weights: a model whose ``selfsup_transform`` returns ``StudentView.identity`` against a model compiled
    without the option -- the same terms and the same weights bit for bit."""
    from tf_raft_amd import losses
    from tf_raft_amd import weights as wm
    from tf_raft_amd.augment import StudentTransform, StudentView
    wts = wm.condition_weights('raft', wm.init_weights('raft', seed=5))
    batches = [_pair(rng), _pair(rng)]
    calls = []

    def fixed(N, frame, student):
        calls.append((N, frame, student))
        return StudentView.identity(N, (8, 8))
    plain = _model(wts, occlusion=False, selfsup_crop=(8, 8))
    models = [_model(wts, occlusion=False, selfsup_crop=(8, 8), selfsup_transform=fixed),
              _model(wts, occlusion=False, selfsup_crop=(8, 8), selfsup_transform=StudentTransform())]      # (the default draws it too)
    for batch in batches:
        a = losses.to_floats(plain.train_step(batch))
        assert list(a) == ['loss', 'photometric', 'smoothness', 'occluded', 'selfsup', 'selfsup_used'] and a['selfsup_used'] > 0
        for m in models:
            b = losses.to_floats(m.train_step(batch))
            assert a == b, (a, b)
            assert isinstance(m.last_student_view, StudentView) and len(m.last_student_view) == 1
            assert tuple(m.last_target_visibility.shape) == (2, 64, 96)
    assert calls == [(1, (80, 112), (64, 96))] * 2
    assert plain.last_student_view is None and plain.last_target_visibility is None
    wa = plain.get_weights_dict()
    for m in models:
        wb = m.get_weights_dict()
        for k in wa:
            np.testing.assert_array_equal(wa[k], wb[k], err_msg=k)


ORACLE_THETA = np.array([[[-1.25, 0.0, 55.5 + 1.25 * 47.5], [0.0, 1.25, 39.5 - 1.25 * 31.5]]])     # flip_x and M-scale 1.25 about the centres


def reference_view_train_steps(wts, batches, iters, lr_fn, wd, clip_norm, n_steps, params, crop, selfsup, view, teacher_masks, target_masks):
    """tests/test_selfsup_loss.py::reference_selfsup_train_steps with the student under ``view``: per step the update block runs on
    the doubled batch of the full frames and again on the float64 yardstick view of those frames, and ``loss1 + weight *
    selfsup(student predictions, yardstick view_flow of the teacher's last prediction, detached)`` is differentiated by autograd,
    then clip_by_global_norm and AdamW.  ``teacher_masks[step]`` is the device's visible1 and ``target_masks[step]`` its
    target_visible, both constants.  Returns (losses, [(loss1, selfsup_last, used share)], updated weights, [the yardstick's
    target masks])."""
    import oracle
    from oracle.layers import W, basic_update_block, encoder
    from oracle.model import upsample_flow
    dtype = torch.float64
    names = sorted(k for k in wts if k.startswith('update_block'))
    var = {k: torch.tensor(wts[k], dtype=dtype) for k in names}
    m = {k: torch.zeros_like(v) for k, v in var.items()}
    v2 = {k: torch.zeros_like(v) for k, v in var.items()}
    frozen = W({k: val for k, val in wts.items() if not k.startswith('update_block')}, dtype)
    cy, cx = crop
    losses, parts, own_masks = [], [], []
    for step in range(n_steps):
        N, H, Wd = batches[step][0].shape[:3]
        size = (H - 2 * cy, Wd - 2 * cx)
        i1 = np.concatenate([batches[step][0], batches[step][1]])
        i2 = np.concatenate([batches[step][1], batches[step][0]])
        ow = W({}, dtype)
        ow.t = {k: val.clone().requires_grad_(True) for k, val in var.items()}

        def run(a, b):
            with torch.no_grad():
                x1 = 2 * (torch.tensor(a, dtype=dtype) / 255.0) - 1.0
                x2 = 2 * (torch.tensor(b, dtype=dtype) / 255.0) - 1.0
                f1, f2 = encoder(frozen, 'fnet', [x1, x2])
                corr_blk = oracle.CorrBlock(f1, f2, 4, 4)
                cnet = encoder(frozen, 'cnet', x1)
                net, inp = torch.tanh(cnet[..., :128]), torch.relu(cnet[..., 128:])
            B, h, w, _ = net.shape
            coords0 = oracle.coords_grid(B, h, w, dtype)
            coords1, preds = coords0.clone(), []
            for _ in range(iters):
                corr = corr_blk.retrieve(coords1)
                net, up_mask, delta = basic_update_block(ow, 'update_block', net, inp, corr, coords1 - coords0)
                coords1 = coords1 + delta
                preds.append(upsample_flow(coords1 - coords0, up_mask))
            return preds

        preds1 = run(i1, i2)
        mask1 = np.asarray(teacher_masks[step]) != 0
        loss1 = torch_photometric_loss(i1, i2, mask1, [p.double() for p in preds1], **params)[0]
        s1 = frames_f64(i1, view, size)[0]                                     # the 2N distinct frames under the pairs' views
        s2 = np.concatenate([s1[N:], s1[:N]])
        preds2 = run(s1, s2)
        target, own = flow_f64(preds1[-1].detach().numpy(), mask1.astype(np.uint8), view, size)
        own_masks.append(own)
        loss, dist, share = torch_selfsup_loss(target, np.asarray(target_masks[step]), (0, 0), None, [p.double() for p in preds2],
                                               gamma=params['gamma'], add_to=loss1, **selfsup)
        loss.backward()
        losses.append(float(loss.detach()))
        parts.append((float(loss1.detach()), float(dist.detach()), share))
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
    return losses, parts, {k: v.detach().numpy() for k, v in var.items()}, own_masks


def test_the_update_block_steps_under_a_fixed_view_match_the_two_pass_oracle():
    """Two steps at N = 1, frames 80 x 112, selfsup_crop = (8, 8) (student 64 x 96), iters = 3, the constants of
    tests/test_selfsup_loss.py, under the fixed view M = diag(-1.25, 1.25) about the centres (a mirror and a scale, dyadic: the
    float32 coordinates are exact, so the device's target mask must equal the yardstick's exactly; the student's outer columns
    fall outside the teacher).  Bounds as in tests/test_gpu_selfsup_loss.py: losses and ``selfsup`` at rtol 1e-4, ``selfsup_used``
    exact, no element of the update off by 0.25 lr, relative L2 of the update at most 0.1.

    Measured (MI355X): see DESIGN.md section 23."""
    import tf_raft_amd
    from tf_raft_amd import losses, training
    from tf_raft_amd.augment import StudentView
    wts, batches = oracle_case()
    N, H, W = batches[0][0].shape[:3]
    view = StudentView(ORACLE_THETA)
    sched = oracle_schedule()
    model = tf_raft_amd.RAFT(weights=wts, iters=ORACLE_ITERS, iters_pred=4)
    model.compile(optimizer=training.AdamW(ORACLE_WD, sched), clip_norm=ORACLE_CLIP, loss=losses.PhotometricSequenceLoss(**DEFAULTS),
                  trainable='update_block', bidirectional=True, occlusion=ORACLE_OCCLUSION[0], alpha=ORACLE_ALPHA, beta=ORACLE_BETA,
                  selfsup_crop=ORACLE_CROP, selfsup_transform=lambda n, frame, student: view,
                  **{'selfsup_' + k: v for k, v in ORACLE_SELFSUP.items()})
    got, masks1, masks_t = [], [], []
    for step in range(ORACLE_STEPS):
        model.occlusion = ORACLE_OCCLUSION[step]
        model.reset_metrics()
        res = model.train_step(batches[step])
        assert list(res) == ['loss', 'photometric', 'smoothness', 'occluded', 'selfsup', 'selfsup_used']
        got.append(losses.to_floats(res))
        masks1.append(_np(model.last_visibility).copy())
        masks_t.append(_np(model.last_target_visibility).copy())
        assert model.last_student_view is view and masks_t[-1].shape == (2 * N, H - 16, W - 16)
    want_losses, parts, want_w, own_masks = reference_view_train_steps(
        wts, batches, ORACLE_ITERS, sched, ORACLE_WD, ORACLE_CLIP, ORACLE_STEPS, DEFAULTS, ORACLE_CROP, ORACLE_SELFSUP, view, masks1, masks_t)
    for step in range(ORACLE_STEPS):
        np.testing.assert_array_equal(masks_t[step] != 0, own_masks[step])      # exactly the yardstick's
        report(f'student view update-block step {step}', got_loss=got[step]['loss'], want_loss=want_losses[step],
               got_selfsup=got[step]['selfsup'], want_selfsup=parts[step][1], got_used=got[step]['selfsup_used'], want_used=parts[step][2])
        assert np.float32(got[step]['selfsup_used']) == np.float32(parts[step][2])
        assert 0.3 < got[step]['selfsup_used'] < 1.0                            # out-of-frame columns (and, at step 0, the user's mask)
    np.testing.assert_allclose([g['loss'] for g in got], want_losses, rtol=1e-4)
    np.testing.assert_allclose([g['selfsup'] for g in got], [p[1] for p in parts], rtol=1e-4)
    new_w = model.get_weights_dict()
    assert all(np.abs(ref - wts[k].astype(np.float64)).max() > 0 for k, ref in want_w.items())
    for k, v in wts.items():
        if not k.startswith('update_block'):
            np.testing.assert_array_equal(new_w[k], v)                           # frozen encoders, bit for bit
    frac, rel = _update_errors(want_w, new_w, wts, ORACLE_LR0)
    report('student view update-block updated weights', frac_elements_off_by_quarter_lr=frac, rel_l2_of_update=rel)
    assert frac == 0.0
    assert rel <= 0.1


@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_one_step_under_a_generic_drawn_view(rng, variant):
    """RAFT with all weights, and SmallRAFT with UFlow's mask rule, under the same seeded draw with flips, zoom, rotation, shift,
    gain and bias: exactly the documented keys, finite terms, a used share in (0, 1], the view and both masks kept, weights
    changed."""
    import tf_raft_amd
    from tf_raft_amd import losses, training
    from tf_raft_amd import weights as wm
    from tf_raft_amd.augment import StudentTransform, StudentView
    N, H, W, crop = 2, 80, 112, (8, 8)
    wts = wm.condition_weights(variant, wm.init_weights(variant, seed=2, perturb=True), 'mid')
    transform = StudentTransform(rng=np.random.RandomState(23), **GENERIC_DRAW)
    common = dict(optimizer=training.AdamW(1e-4, 1e-3), clip_norm=1.0, loss=losses.PhotometricSequenceLoss(), bidirectional=True,
                  occlusion=False, alpha=0.0, selfsup_crop=crop, selfsup_transform=transform)
    if variant == 'small':
        model = tf_raft_amd.SmallRAFT(weights=wts, iters=2, iters_pred=2)
        model.compile(beta=58.0, selfsup_mask='occluded', **common)
    else:
        model = tf_raft_amd.RAFT(weights=wts, iters=2, iters_pred=2)
        model.compile(beta=12.0, trainable='all', **common)
    i1, i2 = _pair(rng, N, H, W)
    res = model.train_step((i1, i2))
    assert list(res) == ['loss', 'photometric', 'smoothness', 'occluded', 'selfsup', 'selfsup_used']
    vals = losses.to_floats(res)
    assert all(np.isfinite(v) for v in vals.values()), vals
    assert 0 < vals['selfsup_used'] <= 1 and vals['selfsup'] > 0
    view = model.last_student_view
    want = StudentTransform(rng=np.random.RandomState(23), **GENERIC_DRAW).draw(N, (H, W), (H - 16, W - 16))
    assert isinstance(view, StudentView) and view.theta.tobytes() == want.theta.tobytes() and view.gain.tobytes() == want.gain.tobytes()
    tvis = _np(model.last_target_visibility)
    assert tvis.shape == (2 * N, H - 16, W - 16) and set(np.unique(tvis)) <= {0, 1}
    np.testing.assert_array_equal(tvis[:N], tvis[N:])                           # one spatial map per pair, finite flows, no masks
    if variant == 'small':
        sv = _np(model.last_student_visibility)
        assert np.float32(vals['selfsup_used']) == np.float32(np.float64(int(((sv == 0) & (tvis != 0)).sum())) / sv.size)
    else:
        assert model.last_student_visibility is None
        assert np.float32(vals['selfsup_used']) == np.float32(np.float64(int((tvis != 0).sum())) / tvis.size)
    new = model.get_weights_dict()
    assert all(not np.array_equal(new[k], wts[k]) for k in new if k.endswith('kernel'))
    report(f'student view train_step {variant}', **vals)

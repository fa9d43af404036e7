"""Device mirror of reference ``tf_raft/losses/losses.py`` -- the evaluation side of the forward pass.

    sequence_loss(y_true, y_pred, gamma=0.8, max_flow=400)        losses.py:4-21
    end_point_error(y_true, y_pred, max_flow=400)                 losses.py:24-43
    EndPointError(max_flow=400)                                   losses.py:46-90

and the self-supervised loss the reference does not have (csrc/photometric_loss.hip):

    PhotometricSequenceLoss(gamma=0.8, smooth_weight=0.1, edge_weight=10.0, eps=0.01, census_weight=0.0)
    SSIMSequenceLoss(gamma=0.8, smooth_weight=0.1, edge_weight=10.0, eps=0.01, census_weight=0.0, ssim_weight=0.0)
    Smooth2SequenceLoss(gamma=0.8, smooth_weight=0.1, edge_weight=10.0, eps=0.01, census_weight=0.0, ssim_weight=0.0,
                        smooth2_weight=0.0)                       second-order smoothness as well (section 24)
    smooth2_sequence_loss(y_true, y_pred, ...)                    the same as a function
    photometric_sequence_loss(y_true, y_pred, ...)                y_true = (image1, image2) or (image1, image2, mask)
    SelfSupervisionLoss(gamma=0.8, weight=0.3, eps=0.001)         student predictions on a crop against a teacher flow (section 22)

``y_true = (flow_gt, valid)`` with ``flow_gt`` (bs, H, W, 2) float and ``valid`` (bs, H, W) bool; ``y_pred`` is the list
of flow predictions the model returns (``sequence_loss``) or one prediction (``end_point_error``).  Arrays may be
NumPy or torch, host or device.  The reductions run as single-pass HIP kernels (csrc/metrics.hip) on the current
stream; results are 0-d fp32 device tensors that answer ``.numpy()`` / ``float()`` like TF eager scalars.  There is no
CPU fallback.
"""
from __future__ import annotations

import functools
import math
import numbers

import torch

from . import _dev
from ._ffi import check

_WORKSPACES = {}


def _workspace(device, nbytes):
    """The kernels' partial records (and the census planes): one grow-only buffer per device AND stream.  The launches of one
    stream are ordered, so one buffer serves all of them in turn; two streams of a device would overwrite each other's records.
    ``nbytes`` comes from the library's ``raft_*_workspace_*`` entry points."""
    key = (device.index, _dev.stream_ptr())
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=device)
        _WORKSPACES[key] = ws
    return ws


def _metrics_workspace(device):
    return _workspace(device, 8 * int(_dev.lib().raft_metrics_workspace_doubles()))


def _photometric_workspace(device):
    return _workspace(device, 8 * int(_dev.lib().raft_photometric_loss_workspace_doubles()))


_census_workspace = _workspace      # (device, raft_census_loss_workspace_bytes(...)): the name the direct callers of the entry use


def _stacked(preds, stride):
    """The device fp32 predictions as ONE buffer with ``stride`` floats from one to the next.  The model returns views of one
    (iters, bs, H, W, 2) buffer: those are used in place (the first view is returned); any other list is gathered once."""
    base = preds[0]
    if all(p.is_contiguous() and p.data_ptr() == base.data_ptr() + 4 * stride * i for i, p in enumerate(preds)):
        return base
    return torch.stack([p.contiguous() for p in preds])


def _truth(y_true):
    try:
        flow_gt, valid = y_true
    except (TypeError, ValueError) as exc:
        raise ValueError('y_true must be the pair (flow_gt, valid)') from exc
    flow_gt = _dev.to_device(flow_gt).as_subclass(torch.Tensor).to(torch.float32).contiguous()
    if flow_gt.dim() < 2 or flow_gt.shape[-1] != 2:
        raise ValueError(f'flow_gt must be (..., 2), got {tuple(flow_gt.shape)}')
    valid = torch.as_tensor(valid) if not isinstance(valid, torch.Tensor) else valid.as_subclass(torch.Tensor)
    if tuple(valid.shape) != tuple(flow_gt.shape[:-1]):
        raise ValueError(f'valid must be {tuple(flow_gt.shape[:-1])}, got {tuple(valid.shape)}')
    valid = (valid != 0).to(device=flow_gt.device, dtype=torch.uint8).contiguous()
    return flow_gt, valid


def _prediction(p, flow_gt):
    p = _dev.to_device(p).as_subclass(torch.Tensor).to(torch.float32)
    if tuple(p.shape) != tuple(flow_gt.shape):
        raise ValueError(f'prediction must be {tuple(flow_gt.shape)}, got {tuple(p.shape)}')
    return p


def sequence_loss(y_true, y_pred, gamma=0.8, max_flow=400):
    """reference losses.py:4-21: sum_i gamma**(n-i-1) * mean(valid * |y_pred[i] - flow_gt|)."""
    flow_gt, valid = _truth(y_true)
    preds = [_prediction(p, flow_gt) for p in y_pred]
    n = len(preds)
    if n == 0:
        return _dev.wrap(torch.zeros((), dtype=torch.float32, device=flow_gt.device))   # flow_loss = 0.0
    if n > 64:
        raise ValueError(f'sequence_loss: at most 64 predictions, got {n}')
    npix = flow_gt.numel() // 2
    stride = npix * 2
    stacked = _stacked(preds, stride)
    out = torch.empty((), dtype=torch.float32, device=flow_gt.device)
    check(_dev.lib().raft_sequence_loss_f32(_dev.ptr(flow_gt), _dev.ptr(valid), _dev.ptr(stacked), stride, n, npix,
                                            float(gamma), float(max_flow), _dev.ptr(out), _dev.ptr(_metrics_workspace(out.device)),
                                            _dev.stream_ptr()), 'sequence_loss')
    return _dev.wrap(out)


# ---------------------------------------------------------------- self-supervised: photometric + smoothness
_F32_MAX = 3.402823466e38


def _real(name, v):
    if isinstance(v, bool) or isinstance(v, (str, bytes, complex)):
        raise ValueError(f'{name} must be a real number, got {v!r}')
    try:
        return float(v)
    except (TypeError, ValueError) as exc:
        raise ValueError(f'{name} must be a real number, got {v!r}') from exc


def _term_weight(name, weight):
    """The weight of a further term as its entry (raft_census_loss_f32, raft_ssim_loss_f32, raft_smooth2_loss_f32) checks it: finite
    and >= 0."""
    v = _real(name, weight)
    if not 0.0 <= v <= _F32_MAX:
        raise ValueError(f'{name} must be finite and >= 0, got {v!r}')
    return v


_census_weight = functools.partial(_term_weight, 'census_weight')
_ssim_weight = functools.partial(_term_weight, 'ssim_weight')
_smooth2_weight = functools.partial(_term_weight, 'smooth2_weight')


def _photometric_params(gamma, smooth_weight, edge_weight, eps, upstream=1.0):
    """The checks raft_photometric_loss_f32 makes on its parameters: finite non-negative weights, ``eps > 0``, finite upstream."""
    out = []
    for name, v in (('gamma', gamma), ('smooth_weight', smooth_weight), ('edge_weight', edge_weight)):
        v = _real(name, v)
        if not 0.0 <= v <= _F32_MAX:
            raise ValueError(f'{name} must be finite and >= 0, got {v!r}')
        out.append(v)
    eps = _real('eps', eps)
    eps2 = float(torch.tensor(eps, dtype=torch.float32) ** 2) if 0.0 < eps <= _F32_MAX else 0.0
    if not 0.0 < eps2 <= _F32_MAX:
        raise ValueError(f'eps and eps * eps must be finite and > 0 in float32, got {eps!r}')
    upstream = _real('upstream', upstream)
    if not math.isfinite(upstream) or abs(upstream) > _F32_MAX:
        raise ValueError(f'upstream must be finite, got {upstream!r}')
    return (*out, eps, upstream)


def _shape_of(x):
    shape = getattr(x, 'shape', None)
    if shape is None:
        import numpy as np
        shape = np.shape(x)
    return tuple(int(d) for d in shape)


def _check_unlabelled(y_true, y_pred):
    """Shapes of ``(image1, image2[, mask])`` and of the predictions, checked BEFORE anything moves to the device.  Returns
    ``(image1, image2, mask or None, (B, H, W))``."""
    try:
        items = tuple(y_true)
    except TypeError as exc:
        raise ValueError('y_true must be (image1, image2) or (image1, image2, mask)') from exc
    if len(items) not in (2, 3):
        raise ValueError(f'y_true must be (image1, image2) or (image1, image2, mask), got {len(items)} items')
    image1, image2 = items[0], items[1]
    mask = items[2] if len(items) == 3 else None
    s1 = _shape_of(image1)
    if len(s1) != 4 or s1[-1] != 3 or min(s1) < 1:
        raise ValueError(f'image1 must be (B, H, W, 3), got {s1}')
    if _shape_of(image2) != s1:
        raise ValueError(f'image2 must be {s1}, got {_shape_of(image2)}')
    if mask is not None and _shape_of(mask) != s1[:3]:
        raise ValueError(f'mask must be {s1[:3]}, got {_shape_of(mask)}')
    if s1[0] * s1[1] * s1[2] * 3 >= 2 ** 31:
        raise ValueError(f'B*H*W*3 must stay below 2^31, got {s1}')
    preds = list(y_pred)
    if len(preds) > 64:
        raise ValueError(f'at most 64 predictions, got {len(preds)}')
    want = s1[:3] + (2,)
    for p in preds:
        if _shape_of(p) != want:
            raise ValueError(f'prediction must be {want}, got {_shape_of(p)}')
    return image1, image2, mask, preds, s1[:3]


_BIDIRECTIONAL_FORMS = '(image1, image2) or (image1, image2, (mask1, mask2))'


def _check_bidirectional(data):
    """What a bidirectional ``train_step`` takes, checked BEFORE anything moves to the device: ``(image1,
    image2)`` or ``(image1, image2, (mask1, mask2))``, each mask ``(N, H, W)`` -- ``mask1`` over frame 1's pixels for the forward
    direction, ``mask2`` over frame 2's for the backward one.  Returns ``None`` or ``(mask1, mask2)``."""
    try:
        items = tuple(data)
    except TypeError as exc:
        raise ValueError(f'a bidirectional train_step expects {_BIDIRECTIONAL_FORMS}') from exc
    if len(items) not in (2, 3):
        raise ValueError(f'a bidirectional train_step expects {_BIDIRECTIONAL_FORMS}, got {len(items)} items')
    try:
        s1 = _check_unlabelled(items[:2], ())[4]
    except ValueError as exc:
        raise ValueError(f'a bidirectional train_step expects {_BIDIRECTIONAL_FORMS}: {exc}') from exc
    if 2 * s1[0] * s1[1] * s1[2] * 3 >= 2 ** 31:
        raise ValueError(f'2*N*H*W*3 must stay below 2^31, got {s1}')
    if len(items) == 2:
        return None
    masks = items[2]
    if not isinstance(masks, (tuple, list)) or len(masks) != 2:
        raise ValueError(f'a bidirectional train_step expects {_BIDIRECTIONAL_FORMS}: the masks come as a pair, one per direction')
    for name, m in zip(('mask1', 'mask2'), masks):
        if _shape_of(m) != s1:
            raise ValueError(f'a bidirectional train_step expects {_BIDIRECTIONAL_FORMS} with {name} {s1}, got {_shape_of(m)}')
    return tuple(masks)


def _mask_to_device(mask, device):
    """nonzero = use the pixel -> contiguous uint8 0/1 on ``device``."""
    mask = mask.as_subclass(torch.Tensor) if isinstance(mask, torch.Tensor) else torch.as_tensor(mask)
    if mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous():
        return mask                                 # the kernel tests != 0 itself
    return (mask != 0).to(device=device, dtype=torch.uint8).contiguous()


def _photometric_launch(y_true, y_pred, gamma, smooth_weight, edge_weight, eps, upstream=1.0, want_grad=False, census_weight=0.0,
                        ssim_weight=0.0, smooth2_weight=0.0):
    """One raft_photometric_loss_f32 call: ``(out, d_preds)`` -- ``out`` maps 'loss', 'photometric', 'smoothness' to elements of
    one device buffer (the last two of the LAST prediction), d_preds is the stacked gradients ``(n, B, H, W, 2)`` or None.
    With ``census_weight > 0`` a raft_census_loss_f32 call follows on the same stream: it adds its term
    to the loss and its gradient to d_preds on the device, and ``out`` gains 'census'.  With ``ssim_weight > 0`` a
    raft_ssim_loss_f32 call follows those in the same way (section 19), and ``out`` gains 'ssim'.  With ``smooth2_weight > 0`` a
    raft_smooth2_loss_f32 call follows all of them (section 24): the second-order smoothness, with the first-order term's
    ``edge_weight`` and ``eps``; ``out`` gains 'smoothness2' behind 'smoothness'."""
    gamma, smooth_weight, edge_weight, eps, upstream = _photometric_params(gamma, smooth_weight, edge_weight, eps, upstream)
    census_weight = _census_weight(census_weight)
    ssim_weight = _ssim_weight(ssim_weight)
    smooth2_weight = _smooth2_weight(smooth2_weight)
    image1, image2, mask, preds, (B, H, W) = _check_unlabelled(y_true, y_pred)
    image1 = _dev.to_device(image1).as_subclass(torch.Tensor)
    image2 = _dev.to_device(image2).as_subclass(torch.Tensor)
    if mask is not None:
        mask = _mask_to_device(mask, image1.device)
    n = len(preds)
    # buf = [loss, photometric, smoothness], and behind them, per windowed term that is on, its out2 = [loss with that term too,
    # the term]; a term's add_to is the loss so far: the out2 of the term before it, or buf[0].  One row per term that is on, in
    # launch order: (key of raft_<key>_loss_f32 / raft_<key>_loss_workspace_bytes, weight, where its add_to sits, where its out2)
    on = [(key, weight) for key, weight in (('census', census_weight), ('ssim', ssim_weight)) if weight > 0.0]
    windowed = [(key, weight, 1 + 2 * j if j else 0, 3 + 2 * j) for j, (key, weight) in enumerate(on)]
    # the second-order smoothness comes last: its add_to is the loss so far, its out2 the last two elements
    second = smooth2_weight > 0.0
    at_loss, at_second = windowed[-1][3] if windowed else 0, 3 + 2 * len(windowed)
    buf = torch.zeros((at_second + 2 * second,), dtype=torch.float32, device=image1.device)
    out = {'loss': buf[at_second if second else at_loss], 'photometric': buf[1]}
    for key, _, _, at_out2 in windowed:
        out[key] = buf[at_out2 + 1]
    out['smoothness'] = buf[2]
    if second:
        out['smoothness2'] = buf[at_second + 1]
    if n == 0:
        return out, None
    preds = [_dev.to_device(p).as_subclass(torch.Tensor).to(torch.float32) for p in preds]
    stride = B * H * W * 2
    stacked = _stacked(preds, stride)
    d_preds = torch.empty((n, B, H, W, 2), dtype=torch.float32, device=image1.device) if want_grad else None
    lib = _dev.lib()
    # one buffer for all entries: the census, SSIM and second-order launches follow the photometric ones on the stream
    need = max([8 * int(lib.raft_photometric_loss_workspace_doubles())]
               + [int(getattr(lib, f'raft_{key}_loss_workspace_bytes')(n, B, H, W)) for key, _, _, _ in windowed]
               + [8 * int(lib.raft_smooth2_loss_workspace_doubles()) * second])
    ws = _workspace(buf.device, need)
    check(lib.raft_photometric_loss_f32(_dev.ptr(image1), _dev.ptr(image2), _dev.ptr(mask) if mask is not None else None,
                                        _dev.ptr(stacked), stride, n, B, H, W, gamma, smooth_weight, edge_weight, eps,
                                        upstream, _dev.ptr(buf), _dev.ptr(d_preds) if want_grad else None,
                                        _dev.ptr(ws), _dev.stream_ptr()),
          'photometric_loss')
    for key, weight, at_add_to, at_out2 in windowed:
        check(getattr(lib, f'raft_{key}_loss_f32')(_dev.ptr(image1), _dev.ptr(image2), _dev.ptr(mask) if mask is not None else None,
                                                   _dev.ptr(stacked), stride, n, B, H, W, gamma, weight, upstream,
                                                   _dev.ptr(buf[at_add_to:]), _dev.ptr(buf[at_out2:]),
                                                   _dev.ptr(d_preds) if want_grad else None, 1, _dev.ptr(ws), _dev.stream_ptr()),
              f'{key}_loss')
    if second:
        check(lib.raft_smooth2_loss_f32(_dev.ptr(image1), _dev.ptr(stacked), stride, n, B, H, W, gamma, smooth2_weight, edge_weight, eps,
                                        upstream, _dev.ptr(buf[at_loss:]), _dev.ptr(buf[at_second:]),
                                        _dev.ptr(d_preds) if want_grad else None, 1, _dev.ptr(ws), _dev.stream_ptr()),
              'smooth2_loss')
    return out, d_preds


def _photometric_terms(out):
    return {k: _dev.wrap(v) for k, v in out.items()}


class PhotometricSequenceLoss:
    """Self-supervised sequence loss: ``sum_i gamma**(n-i-1) * (ph_i + smooth_weight * sm_i)`` with
    ``ph_i`` the Charbonnier difference between frame 1 and frame 2 sampled under prediction i (over the pixels that are in
    frame and, if given, in ``mask``) and ``sm_i`` the edge-aware first-order smoothness of prediction i.
    ``y_true = (image1, image2)`` or ``(image1, image2, mask)``: images ``(B, H, W, 3)`` in 0..255, ``mask`` ``(B, H, W)``,
    nonzero = use the pixel (e.g. ``predict_step_bidirectional(...).occluded_forward == 0``).
    ``census_weight > 0`` adds ``census_weight * cen_i`` to every prediction's term: the soft census distance (7x7 patches of
    gray values, UnFlow's constants) between frame 1 and the warped frame 2, a data term that does not assume brightness
    constancy.
    ``smooth_weight``, ``edge_weight`` and ``eps`` are choices, not tuned values, and ``census_weight`` has no tuned default
    either (0 = the term is off): nothing here was trained on real footage.  ``RAFT.compile(loss=PhotometricSequenceLoss())``
    makes ``train_step`` take unlabelled pairs."""

    def __init__(self, gamma=0.8, smooth_weight=0.1, edge_weight=10.0, eps=0.01, census_weight=0.0):
        self.gamma, self.smooth_weight, self.edge_weight, self.eps, _ = _photometric_params(gamma, smooth_weight, edge_weight, eps)
        self.census_weight = _census_weight(census_weight)

    def _params(self):
        return dict(gamma=self.gamma, smooth_weight=self.smooth_weight, edge_weight=self.edge_weight, eps=self.eps,
                    census_weight=self.census_weight)

    def terms(self, y_true, y_pred):
        """``{'loss', 'photometric', 'smoothness'}``, with ``census_weight > 0`` also ``'census'``: the loss, and the terms of the
        LAST prediction (0-d device scalars).  (The subclasses add ``'ssim'`` and ``'smoothness2'``.)"""
        return _photometric_terms(_photometric_launch(y_true, y_pred, **self._params())[0])

    def __call__(self, y_true, y_pred):
        return self.terms(y_true, y_pred)['loss']

    def value_and_grad(self, y_true, y_pred, upstream=1.0):
        """``(terms, grads)`` from one pass: ``terms()`` and ``grads[i] = upstream * d loss / d y_pred[i]``, shaped like the
        predictions.  What ``train_step`` calls, so that a subclass with further terms serves it unchanged."""
        out, d = _photometric_launch(y_true, y_pred, upstream=upstream, want_grad=True, **self._params())
        return _photometric_terms(out), [] if d is None else [_dev.wrap(d[i]) for i in range(d.shape[0])]


class SSIMSequenceLoss(PhotometricSequenceLoss):
    """``PhotometricSequenceLoss`` with a structural-similarity data term, the third part of the data term of
    ARFlow-style recipes: ``ssim_weight > 0`` adds ``ssim_weight * ssim_i`` to every prediction's term, ``ssim_i`` the mean over all
    pixels of ``(1 - SSIM) / 2`` between frame 1 and the warped frame 2 (3x3 windows of gray values on 0..255, Wang et al.'s
    constants for L = 255) where the pixel is in ``mask``, its vector in frame and its window in the picture.
    ``ssim_weight`` has no tuned default (0 = the term is off, and the loss is the parent's launch for launch and bit for bit),
    and nothing is claimed about accuracy on real footage: nothing here was trained on any."""

    def __init__(self, gamma=0.8, smooth_weight=0.1, edge_weight=10.0, eps=0.01, census_weight=0.0, ssim_weight=0.0):
        super().__init__(gamma, smooth_weight, edge_weight, eps, census_weight)
        self.ssim_weight = _ssim_weight(ssim_weight)

    def _params(self):
        return dict(super()._params(), ssim_weight=self.ssim_weight)


class Smooth2SequenceLoss(SSIMSequenceLoss):
    """``SSIMSequenceLoss`` with the edge-aware SECOND-order smoothness, the regulariser UFlow, ARFlow and
    SMURF name: ``smooth2_weight > 0`` adds ``smooth2_weight * sm2_i`` to every prediction's term, ``sm2_i`` the Charbonnier penalty
    of the second differences of prediction i along x and y.  It leaves an affine flow -- a zoom, a rotation, a receding ground
    plane -- alone, where the first-order term pulls it towards a constant.  Its edge weight is the central difference of frame 1
    over two pixels under the SAME ``edge_weight`` as the first-order term, and its penalty has the same ``eps``: a choice, not a
    tuned value.  ``smooth_weight=0`` with ``smooth2_weight > 0`` is the second-order term alone (UFlow's KITTI setting).
    ``smooth2_weight`` is the last keyword and has no tuned default (0 = the term is off: no launch, and the loss is the parent's bit
    for bit); the parents keep their signatures, as ``SSIMSequenceLoss`` kept its parent's.  Nothing is claimed about accuracy on
    real footage: nothing here was trained on any."""

    def __init__(self, gamma=0.8, smooth_weight=0.1, edge_weight=10.0, eps=0.01, census_weight=0.0, ssim_weight=0.0, smooth2_weight=0.0):
        super().__init__(gamma, smooth_weight, edge_weight, eps, census_weight, ssim_weight)
        self.smooth2_weight = _smooth2_weight(smooth2_weight)

    def _params(self):
        return dict(super()._params(), smooth2_weight=self.smooth2_weight)


def smooth2_sequence_loss(y_true, y_pred, gamma=0.8, smooth_weight=0.1, edge_weight=10.0, eps=0.01, census_weight=0.0, ssim_weight=0.0,
                          smooth2_weight=0.0):
    """``Smooth2SequenceLoss(gamma, smooth_weight, edge_weight, eps, census_weight, ssim_weight, smooth2_weight)(y_true, y_pred)``."""
    return Smooth2SequenceLoss(gamma, smooth_weight, edge_weight, eps, census_weight, ssim_weight, smooth2_weight)(y_true, y_pred)


def photometric_sequence_loss(y_true, y_pred, gamma=0.8, smooth_weight=0.1, edge_weight=10.0, eps=0.01, census_weight=0.0):
    """``PhotometricSequenceLoss(gamma, smooth_weight, edge_weight, eps, census_weight)(y_true, y_pred)``."""
    return PhotometricSequenceLoss(gamma, smooth_weight, edge_weight, eps, census_weight)(y_true, y_pred)


# ---------------------------------------------------------------- self-supervision: student against teacher
def _selfsup_params(gamma, weight, eps, upstream=1.0):
    """The checks raft_selfsup_loss_f32 makes on its parameters: finite non-negative ``gamma`` / ``weight``, ``eps > 0``, finite
    upstream."""
    gamma, _, _, eps, upstream = _photometric_params(gamma, 0.0, 0.0, eps, upstream)
    weight = _real('weight', weight)
    if not 0.0 <= weight <= _F32_MAX:
        raise ValueError(f'weight must be finite and >= 0, got {weight!r}')
    return gamma, weight, eps, upstream


def _index(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):          # (NumPy's integer scalars are Integral)
        raise ValueError(f'{name} must be an int, got {v!r}')
    return int(v)


def _check_selfsup(teacher, preds, origin, teacher_visible, student_visible):
    """Shapes of the teacher, the student's predictions, the window and the masks, checked BEFORE anything moves to the device.
    Returns ``(preds, (B, H, W), (Ht, Wt), (oy, ox))``."""
    ts = _shape_of(teacher)
    if len(ts) != 4 or ts[-1] != 2 or min(ts) < 1:
        raise ValueError(f'teacher must be (B, Ht, Wt, 2), got {ts}')
    if ts[0] * ts[1] * ts[2] * 3 >= 2 ** 31:
        raise ValueError(f'B*Ht*Wt*3 must stay below 2^31, got {ts}')
    preds = list(preds)
    if not preds:
        raise ValueError('self-supervision needs at least one student prediction')
    if len(preds) > 64:
        raise ValueError(f'at most 64 predictions, got {len(preds)}')
    ps = _shape_of(preds[0])
    if len(ps) != 4 or ps[-1] != 2 or min(ps) < 1 or ps[0] != ts[0]:
        raise ValueError(f'prediction must be ({ts[0]}, H, W, 2), got {ps}')
    for p in preds[1:]:
        if _shape_of(p) != ps:
            raise ValueError(f'prediction must be {ps}, got {_shape_of(p)}')
    try:
        oy, ox = origin
    except (TypeError, ValueError) as exc:
        raise ValueError(f'origin must be the pair (oy, ox), got {origin!r}') from exc
    oy, ox = _index('origin[0]', oy), _index('origin[1]', ox)
    if oy < 0 or ox < 0 or oy + ps[1] > ts[1] or ox + ps[2] > ts[2]:
        raise ValueError(f'the window {ps[1]} x {ps[2]} at origin ({oy}, {ox}) does not lie inside the teacher {ts[1]} x {ts[2]}')
    if teacher_visible is not None and _shape_of(teacher_visible) != ts[:3]:
        raise ValueError(f'teacher_visible must be {ts[:3]}, got {_shape_of(teacher_visible)}')
    if student_visible is not None and _shape_of(student_visible) != ps[:3]:
        raise ValueError(f'student_visible must be {ps[:3]}, got {_shape_of(student_visible)}')
    return preds, ps[:3], ts[1:3], (oy, ox)


def _selfsup_launch(teacher, preds, origin, teacher_visible, student_visible, gamma, weight, eps, upstream=1.0, want_grad=False,
                    add_to=None):
    """One raft_selfsup_loss_f32 call: ``(out, d_preds)`` -- ``out`` maps 'loss', 'selfsup', 'selfsup_used' to the elements of one
    device buffer, d_preds is the stacked gradients ``(n, B, H, W, 2)`` or None.  ``add_to``: a 0-d float32 device tensor the
    loss is added to on the device (``train_step``: the first pass's loss)."""
    gamma, weight, eps, upstream = _selfsup_params(gamma, weight, eps, upstream)
    preds, (B, H, W), (Ht, Wt), (oy, ox) = _check_selfsup(teacher, preds, origin, teacher_visible, student_visible)
    teacher = _dev.to_device(teacher).as_subclass(torch.Tensor).to(torch.float32).contiguous()
    tv = _mask_to_device(teacher_visible, teacher.device) if teacher_visible is not None else None
    sv = _mask_to_device(student_visible, teacher.device) if student_visible is not None else None
    preds = [_dev.to_device(p).as_subclass(torch.Tensor).to(torch.float32) for p in preds]
    n, stride = len(preds), B * H * W * 2
    stacked = _stacked(preds, stride)
    buf = torch.empty((3,), dtype=torch.float32, device=teacher.device)
    d_preds = torch.empty((n, B, H, W, 2), dtype=torch.float32, device=teacher.device) if want_grad else None
    lib = _dev.lib()
    ws = _workspace(buf.device, 8 * int(lib.raft_selfsup_loss_workspace_doubles()))
    check(lib.raft_selfsup_loss_f32(_dev.ptr(teacher), _dev.ptr(tv) if tv is not None else None, Ht, Wt, oy, ox,
                                    _dev.ptr(sv) if sv is not None else None, _dev.ptr(stacked), stride, n, B, H, W, gamma, weight,
                                    eps, upstream, _dev.ptr(add_to) if add_to is not None else None, _dev.ptr(buf),
                                    _dev.ptr(d_preds) if want_grad else None, 0, _dev.ptr(ws), _dev.stream_ptr()), 'selfsup_loss')
    return {'loss': buf[0], 'selfsup': buf[1], 'selfsup_used': buf[2]}, d_preds


class SelfSupervisionLoss:
    """Self-supervision, also called self-distillation: the predictions of a *student* pass over a crop of
    the frames are trained to reproduce the flow of the *teacher* pass over the full frames, read through the crop's window and
    held constant: ``weight * sum_i gamma**(n-i-1) * dist_i`` with ``dist_i`` the Charbonnier distance ``sqrt(d*d + eps*eps)``
    between prediction i and the teacher, summed over the used pixels and both components and divided by ALL ``B*H*W*2``
    elements.  A pixel is used where ``teacher_visible`` (if given) is nonzero, ``student_visible`` (if given) is ZERO -- nonzero
    says the student sees the pixel itself, UFlow's rule -- and the teacher's vector is finite.
    ``weight = 0.3`` and ``eps = 0.001`` are UFlow's constants, not tuned here: nothing here was trained on real footage.
    ``RAFT.compile(..., selfsup_crop=(cy, cx))`` makes ``train_step`` use it."""

    def __init__(self, gamma=0.8, weight=0.3, eps=0.001):
        self.gamma, self.weight, self.eps, _ = _selfsup_params(gamma, weight, eps)

    def _params(self):
        return dict(gamma=self.gamma, weight=self.weight, eps=self.eps)

    def terms(self, teacher, preds, origin=(0, 0), teacher_visible=None, student_visible=None):
        """``{'loss', 'selfsup', 'selfsup_used'}``: the weighted loss, the distance of the LAST prediction, and the share of
        used pixels (0-d device scalars).  ``teacher`` is ``(B, Ht, Wt, 2)``, ``preds`` flows ``(B, H, W, 2)``; student pixel
        ``(y, x)`` faces teacher pixel ``(y + origin[0], x + origin[1])``."""
        return _photometric_terms(_selfsup_launch(teacher, preds, origin, teacher_visible, student_visible, **self._params())[0])

    def __call__(self, teacher, preds, origin=(0, 0), teacher_visible=None, student_visible=None):
        return self.terms(teacher, preds, origin, teacher_visible, student_visible)['loss']

    def value_and_grad(self, teacher, preds, origin=(0, 0), teacher_visible=None, student_visible=None, upstream=1.0, _add_to=None):
        """``(terms, grads)`` from one launch: ``terms()`` and ``grads[i] = upstream * d loss / d preds[i]``, shaped like the
        predictions.  The teacher and both masks are constants."""
        out, d = _selfsup_launch(teacher, preds, origin, teacher_visible, student_visible, upstream=upstream, want_grad=True,
                                 add_to=_add_to, **self._params())
        return _photometric_terms(out), [_dev.wrap(d[i]) for i in range(d.shape[0])]


def _metrics(y_true, y_pred, max_flow):
    flow_gt, valid = _truth(y_true)
    pred = _prediction(y_pred, flow_gt).contiguous()
    out = torch.empty((5,), dtype=torch.float32, device=flow_gt.device)
    check(_dev.lib().raft_flow_metrics_f32(_dev.ptr(flow_gt), _dev.ptr(valid), _dev.ptr(pred), flow_gt.numel() // 2,
                                           float(max_flow), _dev.ptr(out), _dev.ptr(_metrics_workspace(out.device)),
                                           _dev.stream_ptr()), 'flow_metrics')
    return out


def end_point_error(y_true, y_pred, max_flow=400):
    """reference losses.py:24-43: {'epe', 'u1', 'u3', 'u5'} over the valid pixels with |flow_gt| < max_flow."""
    out = _metrics(y_true, y_pred, max_flow)
    return {k: _dev.wrap(out[i]) for i, k in enumerate(('epe', 'u1', 'u3', 'u5'))}


class EndPointError:
    """reference losses.py:46-90 (a keras Metric): running means of the per-batch EPE / u1 / u3 / u5 of ``y_pred[-1]``."""

    def __init__(self, max_flow=400, **kwargs):
        self.name = kwargs.pop('name', 'end_point_error')
        if kwargs:
            raise TypeError(f'unexpected keyword arguments {sorted(kwargs)}')
        self.max_flow = max_flow
        self.reset_states()

    def reset_states(self):
        self._sum = None      # device tensor [epe, u1, u3, u5]
        self.count = 0

    def update_state(self, y_true, y_pred):
        out = _metrics(y_true, y_pred[-1], self.max_flow)[:4]       # losses.py:68: the last prediction
        self._sum = out.clone() if self._sum is None else self._sum + out
        self.count += 1

    def result(self):
        if self._sum is None:
            nan = float('nan')                                       # 0 / 0 in the reference
            return {'epe': nan, 'u1': nan, 'u3': nan, 'u5': nan}
        mean = self._sum / float(self.count)
        return {k: _dev.wrap(mean[i]) for i, k in enumerate(('epe', 'u1', 'u3', 'u5'))}


class Mean:
    """The part of ``tf.keras.metrics.Mean`` the reference uses (model.py:118-124): a running mean of scalars."""

    def __init__(self, name='mean'):
        self.name = name
        self.reset_states()

    def reset_states(self):
        self.total = 0.0
        self.count = 0

    def update_state(self, value):
        # a device scalar stays on the device (no host synchronisation inside a training step: the caller converts the result
        # when it wants the number, as with the Keras metric's tensor)
        if isinstance(value, torch.Tensor) and value.is_cuda:
            v = value.detach().as_subclass(torch.Tensor).to(torch.float32).reshape(())
            self.total = v.clone() if self.count == 0 else self.total + v
        else:
            self.total = self.total + float(value)
        self.count += 1

    def result(self):
        """Running mean.  Fed device scalars (train_step / test_step) it is a 0-dim DEVICE tensor -- like the Keras metric's
        tensor, no host synchronisation inside a step -- otherwise a Python float (0.0 when nothing was fed: keras
        divide_no_nan).  ``float(m.result())`` works on both (and synchronises); logging code that wants plain numbers
        (``json.dumps``, formatting) uses ``result_float()`` or ``losses.to_floats(logs)``."""
        if not self.count:
            return 0.0                                              # keras: divide_no_nan
        mean = self.total / self.count
        return _dev.wrap(mean) if isinstance(mean, torch.Tensor) else mean

    def result_float(self) -> float:
        """``result()`` as a Python float (one device synchronisation when the mean lives on the device)."""
        return float(self.result())


def to_floats(logs):
    """The dict a ``train_step`` / ``test_step`` returns (0-dim device tensors) as plain Python floats: ONE device-to-host copy
    for all entries.  For logging / ``json.dumps``; the step functions themselves never synchronise."""
    keys = list(logs)
    dev = [k for k in keys if isinstance(logs[k], torch.Tensor)]
    out = {k: float(logs[k]) for k in keys if k not in dev}
    if dev:
        vals = torch.stack([logs[k].detach().as_subclass(torch.Tensor).to(torch.float32).reshape(()) for k in dev]).cpu().tolist()
        out.update(dict(zip(dev, vals)))
    return {k: out[k] for k in keys}

"""``tf.image.resize_with_crop_or_pad`` on the device: the step between a frame of any size and the model's input size.

The reference never feeds a raw frame to the model: ``CropOrPadder`` (tf_raft/datasets/dataset.py:323-334) maps the
validation set to a fixed size, and ``VisFlowCallback`` (tf_raft/training.py:72-84) pads both frames, runs the model and
crops the flow back, all with this one call.  The rule, per axis, with ``d = target - source`` (floor division):

    crop offset in the source = max(-d // 2, 0)
    pad  offset in the target = max( d // 2, 0)
    copied extent             = min(source, target)

so an odd surplus goes to the bottom / right, and everything outside the window is zero in the input's own scale.
The copy is one launch of the window-copy kernel (``raft_crop_or_pad_*``, tf_raft_amd/csrc/image_ops.hip) on the current
stream; there is no host fallback.

``resize`` / ``resize_flow`` are the other way between the two sizes: bilinear interpolation with half-pixel centres
(``tf.image.resize(method='bilinear', antialias=...)``), for frames much larger than the model's size.
The taps of an axis are derived here, on the host, in float64 (``resize_taps``) and each weight is rounded once to float32; the
kernel (``raft_resize_*``) only applies tables, so no source coordinate is ever computed in float32.

``tile_gather`` / ``tile_blend`` are the third way, for large frames at their OWN resolution: the frame is covered
by a product grid of overlapping tiles of the model's size (``tile_origins``: one tile placed by the crop-or-pad rule where the frame
is no longer than the tile, else the fewest tiles sharing at least ``overlap`` pixels, spread evenly), every tile is predicted on its
own, and the predictions are cross-faded with tent weights normalised per pixel (``tile_taps``, float64 on the host, each weight
rounded once; separable on a product grid).  One launch each (``raft_tile_gather_*`` / ``raft_tile_blend_f32``); flow vectors are not
scaled.

``flow_to_image`` is the reference's flow colour coding (tf_raft/datasets/flow_viz.py) as two launches
(``raft_flow_rad_max_f32`` / ``raft_flow_to_image_u8``, tf_raft_amd/csrc/flow_viz.hip), optionally seen
through the same crop-or-pad window, so a prediction leaves the device as a 3-byte picture instead of an 8-byte flow.

``warp`` / ``flow_consistency`` say where a prediction can be trusted: the backward warp of frames along a
flow, and the forward-backward test of two flows that marks occluded and out-of-frame pixels, one launch each (``raft_warp_*`` /
``raft_flow_consistency_f32``, tf_raft_amd/csrc/flow_check.hip).  ``flow_visibility_launch`` is that test inside a bidirectional
training step: the 2N flows of the doubled batch in, the mask of the loss and the occluded share out
(``raft_flow_visibility_f32``).  ``range_map`` / ``range_occlusion`` are the second occlusion test: every
vector splatted forward with integer bilinear weights, a pixel that receives too little is occluded (``raft_flow_range_*``,
tf_raft_amd/csrc/flow_splat.hip); ``range_visibility_launch`` is its in-step form.

``splat`` / ``interpolate`` carry FRAMES forward along a flow: the range map's integer accumulator with
``C + 1`` sums per pixel, for uint8 frames and float32 frames on 0 .. 255, and the frame at a time ``t`` between two frames from
both flows of a bidirectional prediction (``raft_splat_frames_*`` / ``raft_interpolate_frames_*``, tf_raft_amd/csrc/frame_splat.hip).

``track`` follows points through the flows of consecutive frame pairs: the forward flow sampled at the
point, the point moved, the backward flow sampled there and tested against it, all steps of all points in one launch
(``raft_track_points_f32``, tf_raft_amd/csrc/flow_track.hip); ``point_grid`` makes the points of a dense long-range flow and
``tf_raft_amd.video.FlowTracker`` is the tracker above the model.

``fit_motion`` says what the camera did between two frames: one 2 x 3 matrix per slice -- a translation, a
similarity or an affine map -- fitted to the vectors of a flow by iteratively reweighted least squares, float64 sums in a fixed order
(``raft_flow_fit_motion_f32``, tf_raft_amd/csrc/flow_motion.hip); ``residual_flow`` is the flow with that motion taken away and the
mask of what moves on its own, ``motion_flow`` the dense flow of a motion, and ``MotionViews`` hands corrections to ``view_frames``
(``tf_raft_amd.video.stabilize_video``).

``fuse_frames`` is motion-compensated temporal filtering: K neighbours aligned onto a centre frame along
their flows (or at ``track``'s positions) and averaged under a patch-based Cauchy weight, occluded and out-of-frame pixels left
out, in ONE launch that repeats bit for bit (``raft_fuse_frames_*``, tf_raft_amd/csrc/frame_fuse.hip); ``RAFT.fuse_step`` and
``tf_raft_amd.video.denoise_video`` are burst fusion and video denoising above the model.

``detect_points`` finds the points worth following: a Shi-Tomasi / Harris corner score from Sobel
derivatives (``corner_score``), non-maximum suppression over a ``(2 * min_distance + 1)^2`` window and the ``max_points`` strongest
survivors per image, strongest first, all on the device and bit for bit the same every run (``raft_detect_points``,
tf_raft_amd/csrc/point_detect.hip); ``refill_points_launch`` puts new points into the slots a tracker has lost
(``raft_refill_points``).  ``tf_raft_amd.video.FlowTracker`` uses both: ``points=None`` and ``replenish=True``.

``label_components`` / ``find_objects`` / ``remove_small_components`` turn a mask into a list: the connected
components of a ``moving`` or an occlusion mask under 4- or 8-connectivity, labelled by their smallest raster index, and the
``max_objects`` largest of at least ``min_area`` pixels with area, box, centroid and mean flow, largest first -- a union-find over
tiles in which no workgroup waits for another, integer atomics throughout, so the result repeats bit for bit
(``raft_label_components`` / ``raft_find_objects`` / ``raft_remove_small_components``, tf_raft_amd/csrc/components.hip);
``RAFT.moving_objects_step`` is the list of what moves on its own above the model.

``match_objects`` says which object of one such list is which object of the next: the labels of the first are
carried along the flow to the nearest pixel of the next frame and counted against the labels there (``object_overlap_launch``),
slots are matched one to one, most shared pixels first (``match_objects_launch``), and ``chain_object_ids_launch`` hands identities on
through any number of steps in one launch -- integer sums and maxima only (``raft_object_overlap`` / ``raft_match_objects`` /
``raft_chain_object_ids``, tf_raft_amd/csrc/object_track.hip); ``tf_raft_amd.video.ObjectTracker`` is the tracker above the model.

``forward_interpolate`` projects a low-resolution flow forward along itself: the start of the next pair's
recurrence in a video stream (``raft_forward_interpolate_f32``, tf_raft_amd/csrc/flow_init.hip; ``tf_raft_amd.video``).

``view_frames`` / ``view_flow`` cut the student's view of a self-supervised step out of the frames and carry the teacher's flow
and trust mask into it, under one affine map per slice (``raft_view_frames_f32`` / ``raft_view_flow_f32``,
tf_raft_amd/csrc/student_view.hip; the views are ``tf_raft_amd.augment.StudentView``).

The model reaches the three ways through ONE object per call (``fit_route``: a ``CropOrPadRoute``, a ``ResizeRoute`` or a
``TilePlan``), which answers the same four questions whichever way it is: ``frames_in(t)`` (a frame batch -> the float32 batch
the model runs on, one launch), ``result_size(B)`` (batch and size of the result for a model batch ``B``), ``flow_back(pred,
into)`` (predictions over any leading axes -> the frames' own size, one launch) and ``tensors()`` (the device tables a launch
on another stream reads).  Making the object makes -- the first time: uploads -- both directions' tables on the current stream.
"""
from __future__ import annotations

import collections
import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _dev
from . import _ffi
from ._ffi import check


def crop_or_pad_offsets(source: int, target: int):
    """One axis of ``resize_with_crop_or_pad``: ``(crop_offset, pad_offset, extent)``."""
    source, target = int(source), int(target)
    if source < 1 or target < 1:
        raise ValueError(f'sizes must be >= 1, got {source} -> {target}')
    d = target - source
    return max(-d // 2, 0), max(d // 2, 0), min(source, target)


def _on_device(x) -> torch.Tensor:
    """NumPy / torch, host or device -> contiguous device tensor in the type it arrived in (float64 narrows to float32)."""
    if isinstance(x, torch.Tensor):
        t = x.detach().as_subclass(torch.Tensor)       # (joins a pending result)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if t.dtype == torch.float64:
        t = t.to(torch.float32)
    if not t.is_cuda:
        t = t.to(_dev.require_gpu())
    return t.contiguous()


_FRAME_TYPES = (torch.float32, torch.uint8, torch.bool)


def _entry(x, what, dtypes=_FRAME_TYPES, lead=False):
    """What every public op asks of its input before any launch: ``(H, W, C)`` or ``(N, H, W, C)`` (``lead``: any leading axes),
    not empty, of one of ``dtypes`` (None: the caller judges).  Returns the contiguous device tensor and its 4-D view."""
    t = _on_device(x)
    if t.dim() < 3 or (t.dim() > 4 and not lead):
        raise ValueError(f'{what} expects {"(..., H, W, C)" if lead else "(H, W, C) or (N, H, W, C)"}, got {tuple(t.shape)}')
    if 0 in t.shape:
        raise ValueError(f'empty input {tuple(t.shape)}')
    if dtypes is not None and t.dtype not in dtypes:
        raise TypeError(f'{what} takes {" / ".join(str(d)[6:] for d in dtypes)}, got {t.dtype}')
    return t, t.reshape((-1,) + tuple(t.shape[-3:]))


def _check_out(out, shape, dtype, device, alloc=True):
    """The tensor a launch writes: the caller's ``out`` as a plain tensor if it is a contiguous one of exactly this shape, type and
    device (anything else is a ``ValueError``), without one a new tensor (``alloc=False``: None, for a check ahead of the launch)."""
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype) if alloc else None
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device
            or not out.is_contiguous()):
        raise ValueError(f'out must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}')
    return out if type(out) is torch.Tensor else out.as_subclass(torch.Tensor)


def _over_leading(launch, t, keep, out=None):
    """``launch(t', out')`` with all axes of ``t`` in front of its last ``keep`` folded into one (``out`` likewise): ONE launch over
    any leading axes.  Returns ``out``, or the new result with ``t``'s leading axes back."""
    res = launch(t.reshape((-1,) + tuple(t.shape[-keep:])), None if out is None else out.view((-1,) + tuple(out.shape[-keep:])))
    return out if out is not None else res.view(tuple(t.shape[:-keep]) + tuple(res.shape[1:]))


def _source_entry(t, what):
    """``raft_<what>_f32`` or ``raft_<what>_u8_f32`` for a float32 or uint8 / bool source, and the tensor to read it through."""
    if t.dtype == torch.float32:
        return getattr(_dev.lib(), f'raft_{what}_f32'), t
    if t.dtype in (torch.uint8, torch.bool):
        return getattr(_dev.lib(), f'raft_{what}_u8_f32'), t.view(torch.uint8)
    raise TypeError(f'{what} takes uint8, bool or float32, got {t.dtype}')


def window_copy(t: torch.Tensor, target_height: int, target_width: int, dtype=None, out=None) -> torch.Tensor:
    """The launch itself: contiguous device ``(N, H, W, C)`` of uint8 / bool / float32 -> a new ``(N, Ht, Wt, C)`` tensor on the
    CURRENT stream (plain ``torch.Tensor``; the callers wrap it).  ``out``: a contiguous tensor of the result's shape and type to
    write into instead (a caller that allocates under another stream than the one it launches on)."""
    N, H, W, Cn = t.shape
    lib = _dev.lib()
    if t.dtype == torch.float32 and dtype in (None, torch.float32):
        fn, src, out_dtype = lib.raft_crop_or_pad_f32, t, torch.float32
    elif t.dtype in (torch.uint8, torch.bool) and dtype == torch.float32:
        fn, src, out_dtype = lib.raft_crop_or_pad_u8_f32, t.view(torch.uint8), torch.float32
    elif t.dtype in (torch.uint8, torch.bool) and dtype in (None, t.dtype):
        fn, src, out_dtype = lib.raft_crop_or_pad_u8, t.view(torch.uint8), torch.uint8
    else:
        raise TypeError(f'resize_with_crop_or_pad takes uint8, bool or float32 (optionally uint8 -> float32), got {t.dtype} -> {dtype}')
    out = _check_out(out, (N, int(target_height), int(target_width), Cn), out_dtype, t.device)
    with torch.cuda.device(t.device):
        check(fn(_dev.ptr(src), _dev.ptr(out), N, H, W, int(target_height), int(target_width), Cn, _dev.stream_ptr()), 'crop_or_pad')
    return out.view(torch.bool) if (t.dtype == torch.bool and dtype is None) else out


def resize_with_crop_or_pad(x, target_height: int, target_width: int, dtype=None) -> torch.Tensor:
    """``tf.image.resize_with_crop_or_pad(x, target_height, target_width)`` for ``(H, W, C)`` or ``(N, H, W, C)``.

    ``x``: NumPy or torch, host or device, uint8 / bool / float32.  Returns a contiguous device tensor of the input's type, or
    float32 when ``dtype=torch.float32`` is asked of a uint8 input (cast and window in one pass).  Runs on the current stream.
    A source that already has the target size is returned unchanged (no launch)."""
    target_height, target_width = int(target_height), int(target_width)
    if target_height < 1 or target_width < 1:
        raise ValueError(f'target size must be >= 1, got {target_height} x {target_width}')
    t, _ = _entry(x, 'resize_with_crop_or_pad', dtypes=None)      # (the PAIR of types is window_copy's to judge)
    if tuple(t.shape[-3:-1]) == (target_height, target_width):
        if dtype is not None and dtype != t.dtype:
            if not (t.dtype in (torch.uint8, torch.bool) and dtype == torch.float32):
                raise TypeError(f'resize_with_crop_or_pad takes uint8, bool or float32 (optionally uint8 -> float32), got {t.dtype} -> {dtype}')
            t = t.to(dtype)
        return _dev.wrap(t)
    return _dev.wrap(_over_leading(lambda s, o: window_copy(s, target_height, target_width, dtype), t, 3))


# ---------------------------------------------------------------------------------------------------------------- resize
RESIZE_MAX_TAPS = 64          # csrc/image_ops.hip kResizeMaxTaps
_RESIZE_LDS_FLOATS = 2048     # csrc/image_ops.hip kResizeCap


def resize_taps(n_in: int, n_out: int, antialias: bool = False):
    """One axis of the bilinear resize ``n_in -> n_out`` with half-pixel centres, in float64: ``(first, count, weights)`` with
    ``first[i]`` the first source index of output ``i``, ``count[i]`` its number of taps and ``weights[i, :count[i]]`` their
    weights (non-negative, summing to 1; the rest of the row is 0).  ``antialias`` widens the triangle by ``n_in / n_out`` on an
    axis that shrinks and changes nothing on one that grows."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f'sizes must be >= 1, got {n_in} -> {n_out}')
    scale = np.float64(n_in) / np.float64(n_out)
    support = max(scale, 1.0) if antialias else np.float64(1.0)
    inv = 1.0 / support
    center = scale * (np.arange(n_out, dtype=np.float64) + 0.5)
    first = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    last = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in)
    count = last - first
    j = first[:, None] + np.arange(int(count.max()), dtype=np.int64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs((j - center[:, None] + 0.5) * inv))
    w[j >= last[:, None]] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    return first.astype(np.int32), count.astype(np.int32), w


class _DeviceTable:
    """Device arrays uploaded once, with what a use on another stream than the one they were made under needs."""
    __slots__ = ('tensors', 'host', 'stream', 'event', 'max_taps')

    def __init__(self, arrays, device, max_taps=0):
        self.host = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in arrays]     # alive as long as the copies may run
        self.stream = torch.cuda.current_stream(device)
        self.tensors = [h.to(device, non_blocking=True) for h in self.host]
        self.event = torch.cuda.Event()
        self.event.record(self.stream)
        self.max_taps = max_taps

    def use(self, device):
        cur = torch.cuda.current_stream(device)
        if cur != self.stream:
            cur.wait_event(self.event)              # behind the upload
            for t in self.tensors:
                t.record_stream(cur)                # an evicted table is not handed out again under a launch that reads it
        return self.tensors


_TABLES = {}                  # device index -> OrderedDict(key -> _DeviceTable), least recently used first
_TABLES_PER_DEVICE = 32


def _table(device, key, make):
    cache = _TABLES.setdefault(device.index, collections.OrderedDict())
    ent = cache.get(key)
    if ent is None:
        with torch.cuda.device(device):
            ent = cache[key] = make()
        while len(cache) > _TABLES_PER_DEVICE:
            cache.popitem(last=False)
    else:
        cache.move_to_end(key)
    return ent


def _taps_table(device, key, taps, limit, too_many):
    """The cached device table of one axis: ``taps()`` gives ``(first, count, weights)``; rows wider than ``limit`` are a
    ``ValueError`` saying ``too_many(width)``."""
    def make():
        first, count, w = taps()
        if w.shape[1] > limit:
            raise ValueError(f'{too_many(w.shape[1])}, the kernel takes up to {limit}')
        return _DeviceTable([np.stack([first, count]), w.astype(np.float32)], device, w.shape[1])
    return _table(device, key, make)


def _axis_table(device, n_in, n_out, antialias):
    return _taps_table(device, (int(n_in), int(n_out), bool(antialias)), lambda: resize_taps(n_in, n_out, antialias), RESIZE_MAX_TAPS,
                       lambda k: f'resize {n_in} -> {n_out} needs {k} taps per output')


class ResizePlan:
    """The device tables of one ``(Hs, Ws) -> (Ht, Wt)`` resize: both axes' taps and, for a flow, the two channel factors
    (``u * Wt / Ws``, ``v * Ht / Hs``: float64 ratios rounded once).  Made (and, the first time, uploaded) on the CURRENT stream."""

    def __init__(self, device, Hs, Ws, Ht, Wt, antialias=False, flow=False):
        self.device = device
        self.source, self.target, self.antialias = (int(Hs), int(Ws)), (int(Ht), int(Wt)), bool(antialias)
        self.ys = _axis_table(device, Hs, Ht, antialias)
        self.xs = _axis_table(device, Ws, Wt, antialias)
        self.factors = (np.float32(np.float64(Wt) / np.float64(Ws)), np.float32(np.float64(Ht) / np.float64(Hs))) if flow else None
        self.scale = None
        if flow:
            self.scale = _table(device, ('factors',) + self.source + self.target,
                                lambda: _DeviceTable([np.array(self.factors, np.float32)], device))

    def tensors(self):
        return self.ys.tensors + self.xs.tensors + (self.scale.tensors if self.scale is not None else [])

    def check(self, channels, itemsize):
        """What ``raft_resize_*`` cannot take is an error here, before any launch."""
        if self.scale is not None and channels != 2:
            raise ValueError(f'a flow has 2 channels, got {channels}')
        group = 16 // itemsize
        if (_RESIZE_LDS_FLOATS - 2 * (group - 1)) // channels - self.xs.max_taps - 1 < 0:
            raise ValueError(f'{self.xs.max_taps} taps of {channels} channels do not fit the resize kernel')


def resize_launch(t: torch.Tensor, plan: ResizePlan, out=None) -> torch.Tensor:
    """The launch itself: contiguous device ``(N, Hs, Ws, C)`` of uint8 / bool / float32 -> float32 ``(N, Ht, Wt, C)`` on the
    CURRENT stream (plain ``torch.Tensor``), written into ``out`` when given (contiguous, of the result's shape)."""
    N, H, W, Cn = t.shape
    if (H, W) != plan.source or t.device != plan.device:
        raise ValueError(f'plan of {plan.source} on {plan.device} used on {(H, W)} on {t.device}')
    fn, src = _source_entry(t, 'resize')
    plan.check(Cn, src.element_size())
    out = _check_out(out, (N,) + plan.target + (Cn,), torch.float32, t.device)
    with torch.cuda.device(t.device):
        (yi, yw), (xi, xw) = plan.ys.use(t.device), plan.xs.use(t.device)
        cs = plan.scale.use(t.device)[0] if plan.scale is not None else None
        Ht, Wt = plan.target
        check(fn(_dev.ptr(src), _dev.ptr(out), N, H, W, Ht, Wt, Cn,
                 _dev.ptr(yi), _dev.ptr(yi) + 4 * Ht, _dev.ptr(yw), plan.ys.max_taps,
                 _dev.ptr(xi), _dev.ptr(xi) + 4 * Wt, _dev.ptr(xw), plan.xs.max_taps,
                 _dev.ptr(cs) if cs is not None else None, _dev.stream_ptr()), 'resize')
    return out


def _resize(x, height, width, antialias, out, flow):
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError(f'target size must be >= 1, got {height} x {width}')
    t, _ = _entry(x, 'resize_flow' if flow else 'resize', (torch.float32,) if flow else _FRAME_TYPES, lead=flow)
    if flow and t.shape[-1] != 2:
        raise ValueError(f'a flow has 2 channels, got {tuple(t.shape)}')
    out = _check_out(out, tuple(t.shape[:-3]) + (height, width, t.shape[-1]), torch.float32, t.device, alloc=False)
    if tuple(t.shape[-3:-1]) == (height, width):
        t = t if t.dtype == torch.float32 else t.to(torch.float32)
        return _dev.wrap(t if out is None else out.copy_(t))
    plan = ResizePlan(t.device, t.shape[-3], t.shape[-2], height, width, antialias, flow)
    return _dev.wrap(_over_leading(lambda s, o: resize_launch(s, plan, o), t, 3, out))


def resize(x, height: int, width: int, antialias: bool = False, out=None) -> torch.Tensor:
    """Bilinear resize with half-pixel centres (``tf.image.resize(x, (height, width), 'bilinear', antialias=antialias)``) of
    ``(H, W, C)`` or ``(N, H, W, C)``: NumPy or torch, host or device, uint8 / bool / float32 (float64 narrows).  Returns a
    contiguous float32 device tensor (``out`` when given), computed by one launch on the current stream.  A source that already
    has the target size is returned unchanged, cast to float32 if needed (no launch).  A shrink ratio beyond what the kernel
    takes (``RESIZE_MAX_TAPS`` taps per output) raises ``ValueError``."""
    return _resize(x, height, width, antialias, out, False)


def resize_flow(flow, height: int, width: int, antialias: bool = False, out=None) -> torch.Tensor:
    """``resize`` of a float32 flow field ``(..., H, W, 2)`` over any leading axes in one launch, with ``u`` multiplied by
    ``width / W`` and ``v`` by ``height / H`` in the same pass."""
    return _resize(flow, height, width, antialias, out, True)


# ----------------------------------------------------------------------------------------------------------------- tiles
TILE_MAX_PER_AXIS = _ffi.TILE_MAX_PER_AXIS      # include/raft_hip.h RAFT_TILE_MAX_PER_AXIS
TILE_MAX_TAPS = _ffi.TILE_MAX_TAPS              # include/raft_hip.h RAFT_TILE_MAX_TAPS


def _check_overlap(tile, overlap):
    if isinstance(overlap, (bool, np.bool_)) or not isinstance(overlap, (int, np.integer)):
        raise ValueError(f'overlap must be an int, got {overlap!r}')
    if not 0 <= int(overlap) <= int(tile) // 2:
        raise ValueError(f'overlap must be between 0 and half the tile ({int(tile) // 2} for tiles of {int(tile)}), got {overlap}')
    return int(overlap)


def _overlap_pair(overlap, Ht, Wt):
    """``overlap`` as an int or ``(oy, ox)`` -> both, each validated against its axis."""
    if isinstance(overlap, (tuple, list)):
        if len(overlap) != 2:
            raise ValueError(f'overlap must be an int or (overlap_y, overlap_x), got {overlap!r}')
        oy, ox = overlap
    else:
        oy = ox = overlap
    return _check_overlap(Ht, oy), _check_overlap(Wt, ox)


def tile_origins(length: int, tile: int, overlap: int):
    """One axis of the tiling rule: the origins, in frame coordinates, of the tiles of length ``tile`` that
    cover ``length`` with consecutive tiles sharing at least ``overlap`` pixels.  A frame no longer than the tile takes one tile
    with the frame where ``resize_with_crop_or_pad`` puts it (origin ``-((tile - length) // 2)``); a longer one takes
    ``ceil((length - tile) / (tile - overlap)) + 1`` tiles spread evenly from 0 to ``length - tile``, rounded half up."""
    L, T = int(length), int(tile)
    if L < 1 or T < 1:
        raise ValueError(f'sizes must be >= 1, got a frame of {L} and tiles of {T}')
    o = _check_overlap(T, overlap)
    if L <= T:
        return [-((T - L) // 2)]
    n = -(-(L - T) // (T - o)) + 1
    return [(2 * i * (L - T) + (n - 1)) // (2 * (n - 1)) for i in range(n)]


def tile_taps(length: int, tile: int, origins):
    """The blend table of one axis, in float64: ``(first, count, weights)`` with ``first[p]`` the first tile that covers frame
    coordinate ``p``, ``count[p]`` how many consecutive tiles do and ``weights[p, :count[p]]`` their tent weights
    ``min(t + 1, tile - t)`` at the tile-local coordinate ``t = p - origin``, normalised to sum 1 (the rest of the row is 0)."""
    L, T = int(length), int(tile)
    org = np.asarray(list(origins), np.int64)
    if L < 1 or T < 1 or org.ndim != 1 or org.size < 1:
        raise ValueError(f'expected sizes >= 1 and at least one origin, got {L}, {T}, {origins!r}')
    if np.any(np.diff(org) < 1):
        raise ValueError(f'origins must increase, got {origins!r}')
    t = np.arange(L, dtype=np.int64)[:, None] - org[None, :]
    cover = (t >= 0) & (t < T)
    count = cover.sum(axis=1)
    if np.any(count < 1):
        raise ValueError(f'tiles of {T} at {origins!r} do not cover a frame of {L}')
    first = cover.argmax(axis=1)
    w = np.where(cover, np.minimum(t + 1, T - t), 0).astype(np.float64)
    j = first[:, None] + np.arange(int(count.max()), dtype=np.int64)[None, :]
    inside = j < (first + count)[:, None]                    # (tiles of one length with increasing origins cover a run)
    w = np.where(inside, np.take_along_axis(w, np.minimum(j, org.size - 1), axis=1), 0.0)
    w /= w.sum(axis=1, keepdims=True)
    return first.astype(np.int32), count.astype(np.int32), w


def _tile_axis_table(device, length, tile, overlap):
    return _taps_table(device, ('tile', int(length), int(tile), int(overlap)), lambda: tile_taps(length, tile, tile_origins(length, tile, overlap)),
                       TILE_MAX_TAPS, lambda k: f'{k} tiles of {tile} overlap in one coordinate of {length}')


class TilePlan:
    """The tile grid of ``(H, W)`` frames under ``(Ht, Wt)`` tiles (``tile_origins`` per axis, ``K = ny * nx`` tiles per frame,
    tile ``ky * nx + kx`` at ``(origins_y[ky], origins_x[kx])``) and the two device tables of the blend.  ``overlap``: an int or
    ``(overlap_y, overlap_x)``.  Made (and, the first time, uploaded) on the CURRENT stream.  What the kernels cannot take -- more
    than ``TILE_MAX_PER_AXIS`` tiles per axis, more than ``TILE_MAX_TAPS`` tiles over one coordinate -- is a ``ValueError`` here."""

    def __init__(self, device, H, W, Ht, Wt, overlap):
        self.device = device
        self.frame, self.tile = (int(H), int(W)), (int(Ht), int(Wt))
        self.overlap = _overlap_pair(overlap, Ht, Wt)
        self.origins_y = tile_origins(H, Ht, self.overlap[0])
        self.origins_x = tile_origins(W, Wt, self.overlap[1])
        self.ny, self.nx = len(self.origins_y), len(self.origins_x)
        self.K = self.ny * self.nx
        if max(self.ny, self.nx) > TILE_MAX_PER_AXIS:
            raise ValueError(f'{self.frame} frames take {self.ny} x {self.nx} tiles of {self.tile}, the kernels take up to '
                             f'{TILE_MAX_PER_AXIS} per axis')
        self.origins = _ffi.TileOrigins(self.ny, self.nx)
        self.origins.oy[:self.ny] = self.origins_y
        self.origins.ox[:self.nx] = self.origins_x
        self.ys = _tile_axis_table(device, H, Ht, self.overlap[0])
        self.xs = _tile_axis_table(device, W, Wt, self.overlap[1])

    def tensors(self):
        return self.ys.tensors + self.xs.tensors

    # the route of fit='tile' (see ``fit_route``): the tiles of a frame batch are a model batch of N * K
    def frames_in(self, t):
        return tile_gather_launch(t, self)

    def result_size(self, B):
        return (B // self.K,) + self.frame

    def flow_back(self, pred, into=None):
        return _over_leading(lambda s, o: tile_blend_launch(s, self, o), pred, 4, into)


def tile_gather_launch(t: torch.Tensor, plan: TilePlan, out=None) -> torch.Tensor:
    """The launch itself: contiguous device ``(N, H, W, C)`` of uint8 / bool / float32 -> float32 ``(N * K, Ht, Wt, C)`` on the
    CURRENT stream (plain ``torch.Tensor``), written into ``out`` when given (contiguous, of the result's shape)."""
    N, H, W, Cn = t.shape
    if (H, W) != plan.frame or t.device != plan.device:
        raise ValueError(f'plan of {plan.frame} on {plan.device} used on {(H, W)} on {t.device}')
    fn, src = _source_entry(t, 'tile_gather')
    out = _check_out(out, (N * plan.K,) + plan.tile + (Cn,), torch.float32, t.device)
    with torch.cuda.device(t.device):
        check(fn(_dev.ptr(src), _dev.ptr(out), N, H, W, plan.tile[0], plan.tile[1], Cn, plan.origins, _dev.stream_ptr()), 'tile_gather')
    return out


def tile_blend_launch(t: torch.Tensor, plan: TilePlan, out=None) -> torch.Tensor:
    """The launch itself: contiguous float32 device ``(M, N * K, Ht, Wt, 2)`` -> ``(M, N, H, W, 2)`` on the CURRENT stream (plain
    ``torch.Tensor``), written into ``out`` when given (contiguous, of the result's shape)."""
    M, NK, Ht, Wt, Cn = t.shape
    if (Ht, Wt) != plan.tile or t.device != plan.device:
        raise ValueError(f'plan of {plan.tile} tiles on {plan.device} used on {(Ht, Wt)} on {t.device}')
    if t.dtype != torch.float32:
        raise TypeError(f'tile_blend takes float32, got {t.dtype}')
    if Cn != 2:
        raise ValueError(f'a flow has 2 channels, got {Cn}')
    if NK % plan.K:
        raise ValueError(f'{NK} tiles are no whole number of frames of {plan.ny} x {plan.nx} tiles')
    H, W = plan.frame
    shape = (M, NK // plan.K, H, W, 2)
    out = _check_out(out, shape, torch.float32, t.device)
    if t.data_ptr() % 8 or out.data_ptr() % 8:
        raise ValueError('tile_blend reads and writes whole flow vectors: tiles and out must be 8-byte aligned')
    with torch.cuda.device(t.device):
        (yi, yw), (xi, xw) = plan.ys.use(t.device), plan.xs.use(t.device)
        check(_dev.lib().raft_tile_blend_f32(_dev.ptr(t), _dev.ptr(out), M, shape[1], H, W, Ht, Wt, plan.origins,
                                             _dev.ptr(yi), _dev.ptr(yi) + 4 * H, _dev.ptr(yw), plan.ys.max_taps,
                                             _dev.ptr(xi), _dev.ptr(xi) + 4 * W, _dev.ptr(xw), plan.xs.max_taps, _dev.stream_ptr()), 'tile_blend')
    return out


def tile_gather(x, height: int, width: int, overlap=64, out=None) -> torch.Tensor:
    """The tiles of ``(H, W, C)`` or ``(N, H, W, C)`` frames under the tiling rule (``tile_origins`` per axis with tiles of
    ``height x width``; ``overlap`` an int or ``(overlap_y, overlap_x)``): NumPy or torch, host or device, uint8 / bool / float32
    (float64 narrows) -> a contiguous float32 device tensor ``(N * K, height, width, C)`` (``out`` when given) with frame ``n``'s
    tile ``(ky, kx)`` at index ``(n * ny + ky) * nx + kx``, zero outside the frame.  One launch on the current stream.  Frames
    that already have the tile's size are returned unchanged, cast to float32 if needed (no launch)."""
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError(f'tile size must be >= 1, got {height} x {width}')
    pair = _overlap_pair(overlap, height, width)
    t, t4 = _entry(x, 'tile_gather')
    if tuple(t4.shape[1:3]) == (height, width):
        out = _check_out(out, tuple(t4.shape), torch.float32, t.device, alloc=False)
        t4 = t4 if t4.dtype == torch.float32 else t4.to(torch.float32)
        return _dev.wrap(t4 if out is None else out.copy_(t4))
    plan = TilePlan(t.device, t4.shape[1], t4.shape[2], height, width, pair)
    return _dev.wrap(tile_gather_launch(t4, plan, out))


def tile_blend(tiles, H: int, W: int, overlap=64, out=None) -> torch.Tensor:
    """The way back: float32 predictions ``(..., N * K, Ht, Wt, 2)`` on the tiles of ``tile_gather`` (same ``overlap``) ->
    ``(..., N, H, W, 2)`` at the frames' own size (``out`` when given), every pixel the tent-weighted mean of the tiles that cover
    it (``tile_taps``), over any leading axes in one launch on the current stream.  Flow vectors are not scaled: the tiles are at
    the frame's resolution.  Tiles of the frame's own size are returned unchanged (no launch)."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f'frame size must be >= 1, got {H} x {W}')
    shape = tuple(tiles.shape) if hasattr(tiles, 'shape') else np.shape(tiles)
    if len(shape) < 4:
        raise ValueError(f'expected (..., N * K, Ht, Wt, 2), got {shape}')
    if 0 in shape:
        raise ValueError(f'empty input {shape}')
    if shape[-1] != 2:
        raise ValueError(f'a flow has 2 channels, got {shape}')
    Ht, Wt = (int(v) for v in shape[-3:-1])
    pair = _overlap_pair(overlap, Ht, Wt)
    t = _on_device(tiles)
    if t.dtype != torch.float32:
        raise TypeError(f'tile_blend takes float32, got {t.dtype}')
    if (Ht, Wt) == (H, W):
        out = _check_out(out, tuple(t.shape), torch.float32, t.device, alloc=False)
        return _dev.wrap(t if out is None else out.copy_(t))
    plan = TilePlan(t.device, H, W, Ht, Wt, pair)
    if t.shape[-4] % plan.K:
        raise ValueError(f'{t.shape[-4]} tiles are no whole number of frames of {plan.ny} x {plan.nx} tiles')
    out = _check_out(out, tuple(t.shape[:-4]) + plan.result_size(t.shape[-4]) + (2,), torch.float32, t.device, alloc=False)
    return _dev.wrap(plan.flow_back(t, out))


# ---------------------------------------------------------------------------------------------------------------- routes
class CropOrPadRoute:
    """``fit='crop_or_pad'`` between ``(H, W)`` frames and a model of ``(Ht, Wt)``: the window copy both ways, no tables."""

    def __init__(self, H, W, Ht, Wt):
        self.frame, self.model = (int(H), int(W)), (int(Ht), int(Wt))

    def frames_in(self, t):
        return window_copy(t, *self.model, torch.float32)

    def result_size(self, B):
        return (B,) + self.frame

    def flow_back(self, pred, into=None):
        return _over_leading(lambda s, o: window_copy(s, *self.frame, out=o), pred, 3, into)

    def tensors(self):
        return []


class ResizeRoute:
    """``fit='resize'``: the plan of the frames' way in and the plan of the flow's way back (``u``, ``v`` scaled), both made here."""

    def __init__(self, device, H, W, Ht, Wt, antialias):
        self.fwd = ResizePlan(device, H, W, Ht, Wt, antialias)
        self.back = ResizePlan(device, Ht, Wt, H, W, antialias, flow=True)

    def frames_in(self, t):
        return resize_launch(t, self.fwd)

    def result_size(self, B):
        return (B,) + self.back.target

    def flow_back(self, pred, into=None):
        return _over_leading(lambda s, o: resize_launch(s, self.back, o), pred, 3, into)

    def tensors(self):
        return self.back.tensors()          # (the way in runs on the stream the tables were made on)


def fit_route(fit, device, H, W, Ht, Wt, antialias=False, overlap=None):
    """The route object of one call (module docstring) between ``(H, W)`` frames on ``device`` and a model of ``(Ht, Wt)``.  Both
    directions' tables are made -- the first time: uploaded -- here, on the CURRENT stream, so a ``flow_back`` launched on another
    stream finds everything in place."""
    if fit == 'resize':
        return ResizeRoute(device, H, W, Ht, Wt, antialias)
    if fit == 'tile':
        return TilePlan(device, H, W, Ht, Wt, overlap)
    return CropOrPadRoute(H, W, Ht, Wt)


# ---------------------------------------------------------------------------------------------------------- colour coding
def _viz_args(clip_flow, rad_max):
    clip = -1.0 if clip_flow is None else float(clip_flow)
    if clip_flow is not None and not clip >= 0.0:
        raise ValueError(f'clip_flow must be >= 0, got {clip_flow!r}')
    fixed = 0.0 if rad_max is None else float(rad_max)
    if rad_max is not None and not (fixed > 0.0 and np.isfinite(np.float32(fixed))):
        raise ValueError(f'rad_max must be a positive float, got {rad_max!r}')
    return clip, fixed


def _flow_4d(flow, size):
    t = _on_device(flow)
    if t.dim() not in (3, 4) or t.shape[-1] != 2:
        raise ValueError(f'expected a flow (H, W, 2) or (N, H, W, 2), got {tuple(t.shape)}')
    if 0 in t.shape:
        raise ValueError(f'empty input {tuple(t.shape)}')
    if t.dtype != torch.float32:
        raise TypeError(f'a flow is float32, got {t.dtype}')
    h, w = (int(v) for v in (t.shape[-3:-1] if size is None else size))
    if h < 1 or w < 1:
        raise ValueError(f'size must be >= 1 per axis, got {h} x {w}')
    return t, (t if t.dim() == 4 else t[None]), h, w


def flow_rad_max_launch(t: torch.Tensor, height: int, width: int, clip: float = -1.0) -> torch.Tensor:
    """The first launch of the colour coding (``raft_flow_rad_max_f32``) on the CURRENT stream: contiguous float32 device
    ``(N, H, W, 2)`` -> the partial maxima of every image's flow magnitude inside the crop-or-pad window to ``(height, width)``,
    ``(N, raft_flow_to_image_workspace_floats(1))`` float32, every element written."""
    N, H, W, _ = t.shape
    lib = _dev.lib()
    partial = torch.empty((N, int(lib.raft_flow_to_image_workspace_floats(1))), device=t.device, dtype=torch.float32)
    with torch.cuda.device(t.device):
        check(lib.raft_flow_rad_max_f32(_dev.ptr(t), _dev.ptr(partial), N, H, W, int(height), int(width), clip, _dev.stream_ptr()),
              'flow_rad_max')
    return partial


def flow_to_image_launch(t: torch.Tensor, height: int, width: int, clip: float = -1.0, bgr: bool = False, fixed_rad_max: float = 0.0,
                         out=None) -> torch.Tensor:
    """The launches themselves: contiguous float32 device ``(N, H, W, 2)`` -> uint8 ``(N, height, width, 3)`` on the CURRENT
    stream (plain ``torch.Tensor``), written into ``out`` when given.  Two launches; one when ``fixed_rad_max > 0`` (nothing
    needs the images' own maxima then)."""
    N, H, W, _ = t.shape
    shape = (N, int(height), int(width), 3)
    out = _check_out(out, shape, torch.uint8, t.device)
    partial = flow_rad_max_launch(t, height, width, clip) if not fixed_rad_max > 0.0 else None
    with torch.cuda.device(t.device):
        check(_dev.lib().raft_flow_to_image_u8(_dev.ptr(t), _dev.ptr(partial) if partial is not None else None, _dev.ptr(out), N, H, W,
                                               shape[1], shape[2], clip, int(bool(bgr)), fixed_rad_max, _dev.stream_ptr()), 'flow_to_image')
    return out


def flow_to_image(flow, size=None, clip_flow=None, convert_to_bgr=False, rad_max=None, out=None) -> torch.Tensor:
    """The reference's ``flow_to_image`` (tf_raft/datasets/flow_viz.py:109-132, the Middlebury colour wheel) on the device:
    a flow ``(H, W, 2)`` or ``(N, H, W, 2)`` (NumPy or torch, host or device, float32; float64 narrows) -> a uint8 device
    tensor ``(..., H, W, 3)`` of the same rank (``out`` when given), computed by two launches on the current stream.

    Each image is normalised by its own largest magnitude, as the reference does per call.  ``rad_max`` (a positive float) fixes
    the radius instead -- one scale for all frames of a video -- and vectors beyond it take the reference's out-of-range
    branch, which darkens them: the picture is ``flow_uv_to_colors(u / (R + eps), v / (R + eps))`` with ``R + eps`` in float32.
    ``clip_flow`` is the reference's ``np.clip(flow, 0, clip_flow)`` (negative components become 0) and ``convert_to_bgr`` its
    channel order.  ``size=(h, w)``: the picture of ``resize_with_crop_or_pad(flow, h, w)`` without that copy; flow cropped
    away does not set the scale, padding is zero flow (white).

    Values agree with the reference's NumPy to within one level in at most a few values per million (``atan2`` is computed in
    double and rounded once; NumPy's float32 ``arctan2`` is not correctly rounded -- DESIGN.md section 13).  A NaN or infinite flow
    is outside the contract.  ``tf_raft_amd.io.flow_to_image`` is the host version."""
    clip, fixed = _viz_args(clip_flow, rad_max)
    t, t4, h, w = _flow_4d(flow, size)
    out = _check_out(out, tuple(t.shape[:-3]) + (h, w, 3), torch.uint8, t.device, alloc=False)
    res = flow_to_image_launch(t4, h, w, clip, convert_to_bgr, fixed, None if out is None else (out if t.dim() == 4 else out[None]))
    return _dev.wrap(res if t.dim() == 4 else res[0])


def flow_rad_max(flow, size=None, clip_flow=None) -> torch.Tensor:
    """The radius ``flow_to_image`` normalises each image by: float32 ``(N,)`` (a scalar tensor for ``(H, W, 2)``), bit for bit
    the reference's ``np.max(np.sqrt(np.square(u) + np.square(v)))`` over the window to ``size``.  The first launch alone; its
    partial maxima are folded by a torch reduction here (``flow_to_image`` never calls this: its second kernel folds them itself)."""
    clip, _ = _viz_args(clip_flow, None)
    t, t4, h, w = _flow_4d(flow, size)
    m = flow_rad_max_launch(t4, h, w, clip).amax(dim=1)
    return _dev.wrap(m if t.dim() == 4 else m[0])


# ------------------------------------------------------------------------------------------ warp and consistency check
CONSISTENCY_ALPHA, CONSISTENCY_BETA = 0.01, 0.5      # Meister et al. 2018 (UnFlow)


def check_consistency_args(alpha, beta):
    """``alpha`` and ``beta`` of the forward-backward test as floats: numbers (no bool), finite in float32 and not negative."""
    vals = []
    for name, v in (('alpha', alpha), ('beta', beta)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f'{name} must be a number, got {v!r}')
        if not 0.0 <= float(v) <= float(np.finfo(np.float32).max):
            raise ValueError(f'{name} must be finite and >= 0, got {v!r}')
        vals.append(float(v))
    return tuple(vals)


def _check_flow(f, what):
    if not f.is_contiguous():
        raise ValueError(f'{what}: the flow must be contiguous, got strides {tuple(f.stride())} for {tuple(f.shape)}')
    if f.dtype != torch.float32:
        raise TypeError(f'{what}: a flow is float32, got {f.dtype}')
    if f.data_ptr() % 8:
        raise ValueError(f'{what} reads whole flow vectors: the flow must be 8-byte aligned')


def warp_launch(t: torch.Tensor, flow: torch.Tensor, out=None, inside=None) -> torch.Tensor:
    """The launch itself: contiguous device ``(N, H, W, C)`` of uint8 / bool / float32 sampled along the contiguous float32 flow
    ``(N, H, W, 2)`` -> float32 ``(N, H, W, C)`` on the CURRENT stream (plain ``torch.Tensor``), written into ``out`` when given;
    ``inside``: a contiguous uint8 ``(N, H, W)`` tensor to receive the in-frame map."""
    N, H, W, Cn = t.shape
    if tuple(flow.shape) != (N, H, W, 2) or flow.device != t.device:
        raise ValueError(f'frames {tuple(t.shape)} on {t.device} need a flow {(N, H, W, 2)}, got {tuple(flow.shape)} on {flow.device}')
    _check_flow(flow, 'warp')
    if not t.is_contiguous():
        raise ValueError(f'warp: the frames must be contiguous, got strides {tuple(t.stride())} for {tuple(t.shape)}')
    fn, src = _source_entry(t, 'warp')
    out = _check_out(out, (N, H, W, Cn), torch.float32, t.device)
    inside = _check_out(inside, (N, H, W), torch.uint8, t.device, alloc=False)
    with torch.cuda.device(t.device):
        check(fn(_dev.ptr(src), _dev.ptr(flow), _dev.ptr(out), _dev.ptr(inside) if inside is not None else None, N, H, W, Cn,
                 _dev.stream_ptr()), 'warp')
    return out


def flow_consistency_launch(flow_a: torch.Tensor, flow_b: torch.Tensor, alpha: float = CONSISTENCY_ALPHA, beta: float = CONSISTENCY_BETA,
                            both: bool = True):
    """The launch itself: two contiguous float32 device flows ``(N, H, W, 2)`` -> the uint8 masks ``(occluded_a, occluded_b)``,
    each ``(N, H, W)`` with 1 = occluded, by ONE launch on the CURRENT stream (plain tensors; ``both=False``: direction a alone,
    ``occluded_b`` is None)."""
    if flow_a.dim() != 4 or flow_a.shape[-1] != 2 or flow_a.shape != flow_b.shape or flow_a.device != flow_b.device:
        raise ValueError(f'expected two flows (N, H, W, 2) of one shape and device, got {tuple(flow_a.shape)} on {flow_a.device} / '
                         f'{tuple(flow_b.shape)} on {flow_b.device}')
    _check_flow(flow_a, 'flow_consistency')
    _check_flow(flow_b, 'flow_consistency')
    N, H, W, _ = flow_a.shape
    masks = torch.empty((2 if both else 1, N, H, W), device=flow_a.device, dtype=torch.uint8)
    with torch.cuda.device(flow_a.device):
        check(_dev.lib().raft_flow_consistency_f32(_dev.ptr(flow_a), _dev.ptr(flow_b), _dev.ptr(masks[0]), _dev.ptr(masks[1]) if both else None,
                                                   N, H, W, alpha, beta, _dev.stream_ptr()), 'flow_consistency')
    return masks[0], (masks[1] if both else None)


def flow_visibility_launch(flows: torch.Tensor, N: int, mask=None, alpha: float = CONSISTENCY_ALPHA, beta: float = CONSISTENCY_BETA,
                           apply: bool = True, want_visible: bool = True):
    """The launch itself (``raft_flow_visibility_f32``): contiguous float32 device flows ``(2N, H, W, 2)``,
    the N forward flows in front of the N backward ones, and an optional contiguous uint8 ``mask`` ``(2N, H, W)`` ->
    ``(visible, occluded_fraction)`` on the CURRENT stream (plain tensors).  ``visible`` is uint8 ``(2N, H, W)``,
    ``mask != 0 and not (apply and occluded)`` (None with ``want_visible=False``); ``occluded_fraction`` is the 0-d float32 share
    of occluded pixels among all ``2N * H * W``, whatever ``apply`` and ``mask`` are."""
    from . import losses
    if flows.dim() != 4 or flows.shape[-1] != 2 or flows.shape[0] != 2 * int(N) or int(N) < 1:
        raise ValueError(f'expected flows (2N, H, W, 2) with N = {N}, got {tuple(flows.shape)}')
    _check_flow(flows, 'flow_visibility')
    B, H, W, _ = flows.shape
    if mask is not None:
        mask = _check_out(mask, (B, H, W), torch.uint8, flows.device)
    visible = torch.empty((B, H, W), device=flows.device, dtype=torch.uint8) if want_visible else None
    fraction = torch.empty((), device=flows.device, dtype=torch.float32)
    lib = _dev.lib()
    with torch.cuda.device(flows.device):
        ws = losses._workspace(flows.device, 8 * int(lib.raft_flow_visibility_workspace_doubles()))
        check(lib.raft_flow_visibility_f32(_dev.ptr(flows), _dev.ptr(mask) if mask is not None else None,
                                           _dev.ptr(visible) if visible is not None else None, _dev.ptr(fraction), int(N), H, W,
                                           float(alpha), float(beta), int(bool(apply)), _dev.ptr(ws), _dev.stream_ptr()),
              'flow_visibility')
    return visible, fraction


def _flow_like(flow, lead_shape, what):
    f = _on_device(flow)
    if tuple(f.shape) != tuple(lead_shape) + (2,):
        raise ValueError(f'{what} expects a flow {tuple(lead_shape) + (2,)}, got {tuple(f.shape)}')
    if f.dtype != torch.float32:
        raise TypeError(f'a flow is float32, got {f.dtype}')
    return f


def warp(x, flow, return_inside=False, out=None):
    """Backward warp: ``(H, W, C)`` or ``(N, H, W, C)`` frames (NumPy or torch, host or device, uint8 / bool / float32; float64
    narrows) sampled bilinearly at every pixel's end point under ``flow`` (same leading shape, 2 channels, float32) -> a contiguous
    float32 device tensor of the frames' shape (``out`` when given): ``result[y, x] = frames[y + v, x + u]``, so ``warp(image2,
    flow_forward)`` reconstructs frame 1 from frame 2.  A pixel whose end point ``(float32(x) + u, float32(y) + v)`` lies outside
    ``[0, W - 1] x [0, H - 1]`` (or is NaN) is 0 in every channel; ``return_inside=True`` also returns the uint8 map of the
    pixels that are not.  One launch on the current stream."""
    t, t4 = _entry(x, 'warp')
    f = _flow_like(flow, t.shape[:-1], 'warp')
    out = _check_out(out, tuple(t.shape), torch.float32, t.device, alloc=False)
    inside = torch.empty(tuple(t4.shape[:3]), device=t.device, dtype=torch.uint8) if return_inside else None
    res = warp_launch(t4, f.reshape(t4.shape[:3] + (2,)), None if out is None else out.view(t4.shape), inside)
    res = _dev.wrap(out if out is not None else res.view(t.shape))
    return (res, _dev.wrap(inside.view(t.shape[:-1]))) if return_inside else res


def flow_consistency(flow_forward, flow_backward, alpha=CONSISTENCY_ALPHA, beta=CONSISTENCY_BETA):
    """Forward-backward consistency of two float32 flows ``(H, W, 2)`` or ``(N, H, W, 2)`` (NumPy or torch, host or device):
    ``(occluded_forward, occluded_backward)``, uint8 device tensors ``(..., H, W)`` with 1 where a vector cannot be trusted.  With
    ``s`` the other direction's flow sampled bilinearly at the vector's end point, a pixel is occluded unless the end point lies
    in the frame and ``|f + s|^2 <= alpha * (|f|^2 + |s|^2) + beta`` (Meister et al. 2018, whose values the defaults are); a
    non-finite vector marks its pixel.  Both masks come from ONE launch on the current stream."""
    alpha, beta = check_consistency_args(alpha, beta)
    t, f4, _, _ = _flow_4d(flow_forward, None)
    b = _flow_like(flow_backward, t.shape[:-1], 'flow_consistency')
    occ_f, occ_b = flow_consistency_launch(f4, b.reshape(f4.shape), alpha, beta)
    return _dev.wrap(occ_f.view(t.shape[:-1])), _dev.wrap(occ_b.view(t.shape[:-1]))


# ------------------------------------------------------------------------------------------ range map: the second occlusion test
RANGE_THRESHOLD = 0.5      # a choice, not a tuned value
OCCLUSION_TESTS = ('consistency', 'range')


def check_range_threshold(threshold):
    """``threshold`` of the range-map test as a float: a number (no bool) whose float32 value lies in ``(0, 1]``."""
    if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise ValueError(f'threshold must be a number, got {threshold!r}')
    try:
        with np.errstate(over='ignore'):
            t = float(np.float32(threshold))
    except OverflowError:
        t = float('inf')
    if not 0.0 < t <= 1.0:
        raise ValueError(f'threshold must lie in (0, 1] as a float32, got {threshold!r}')
    return t


def check_occlusion_test(occlusion_test):
    """``'consistency'`` (the forward-backward test) or ``'range'`` (the range map, section 21)."""
    if not isinstance(occlusion_test, str) or occlusion_test not in OCCLUSION_TESTS:
        raise ValueError(f"occlusion_test must be 'consistency' or 'range', got {occlusion_test!r}")
    return occlusion_test


def _range_workspace(device, slices, H, W, records=0):
    """The uint64 sums of ``slices`` frames (and ``records`` doubles behind them) in the stream's grow-only workspace."""
    from . import losses
    nbytes = int(_dev.lib().raft_flow_range_workspace_bytes(int(slices), int(H), int(W)))
    if nbytes <= 0:
        raise ValueError(f'the range map takes frames of up to 2^28 pixels and flows of fewer than 2^31 floats, got {slices} x {H} x {W}')
    ws = losses._workspace(device, nbytes + 8 * int(records))
    return ws, _dev.ptr(ws) + nbytes


def range_map_launch(flow: torch.Tensor, out=None) -> torch.Tensor:
    """The launches themselves (``raft_flow_range_map_f32``): a contiguous float32 device flow ``(N, H, W, 2)`` -> its range map,
    float32 ``(N, H, W)`` on the CURRENT stream (a plain tensor), written into ``out`` when given."""
    if flow.dim() != 4 or flow.shape[-1] != 2:
        raise ValueError(f'expected a flow (N, H, W, 2), got {tuple(flow.shape)}')
    _check_flow(flow, 'range_map')
    N, H, W, _ = flow.shape
    out = _check_out(out, (N, H, W), torch.float32, flow.device)
    with torch.cuda.device(flow.device):
        ws, _ = _range_workspace(flow.device, N, H, W)
        check(_dev.lib().raft_flow_range_map_f32(_dev.ptr(flow), _dev.ptr(out), N, H, W, _dev.ptr(ws), _dev.stream_ptr()), 'range_map')
    return out


def range_occlusion_launch(flow_a: torch.Tensor, flow_b: torch.Tensor, threshold: float = RANGE_THRESHOLD, both: bool = True):
    """The launches themselves (``raft_flow_range_occlusion_f32``): two contiguous float32 device flows ``(N, H, W, 2)`` -> the
    uint8 masks ``(occluded_a, occluded_b)``, each ``(N, H, W)`` with 1 = occluded, on the CURRENT stream (plain tensors;
    ``both=False``: direction a alone, only ``flow_b`` is splatted and ``occluded_b`` is None)."""
    if flow_a.dim() != 4 or flow_a.shape[-1] != 2 or flow_a.shape != flow_b.shape or flow_a.device != flow_b.device:
        raise ValueError(f'expected two flows (N, H, W, 2) of one shape and device, got {tuple(flow_a.shape)} on {flow_a.device} / '
                         f'{tuple(flow_b.shape)} on {flow_b.device}')
    _check_flow(flow_a, 'range_occlusion')
    _check_flow(flow_b, 'range_occlusion')
    N, H, W, _ = flow_a.shape
    masks = torch.empty((2 if both else 1, N, H, W), device=flow_a.device, dtype=torch.uint8)
    with torch.cuda.device(flow_a.device):
        ws, _ = _range_workspace(flow_a.device, 2 * N if both else N, H, W)
        check(_dev.lib().raft_flow_range_occlusion_f32(_dev.ptr(flow_a), _dev.ptr(flow_b), _dev.ptr(masks[0]),
                                                       _dev.ptr(masks[1]) if both else None, N, H, W, float(threshold), _dev.ptr(ws),
                                                       _dev.stream_ptr()), 'range_occlusion')
    return masks[0], (masks[1] if both else None)


def range_visibility_launch(flows: torch.Tensor, N: int, mask=None, threshold: float = RANGE_THRESHOLD, apply: bool = True,
                            want_visible: bool = True):
    """``flow_visibility_launch`` with the range-map test (``raft_flow_range_visibility_f32``): contiguous
    float32 device flows ``(2N, H, W, 2)``, the N forward flows in front of the N backward ones, and an optional contiguous uint8
    ``mask`` ``(2N, H, W)`` -> ``(visible, occluded_fraction)`` on the CURRENT stream (plain tensors), with the same meaning."""
    if flows.dim() != 4 or flows.shape[-1] != 2 or flows.shape[0] != 2 * int(N) or int(N) < 1:
        raise ValueError(f'expected flows (2N, H, W, 2) with N = {N}, got {tuple(flows.shape)}')
    _check_flow(flows, 'range_visibility')
    B, H, W, _ = flows.shape
    if mask is not None:
        mask = _check_out(mask, (B, H, W), torch.uint8, flows.device)
    visible = torch.empty((B, H, W), device=flows.device, dtype=torch.uint8) if want_visible else None
    fraction = torch.empty((), device=flows.device, dtype=torch.float32)
    lib = _dev.lib()
    with torch.cuda.device(flows.device):
        ws, records = _range_workspace(flows.device, B, H, W, lib.raft_flow_visibility_workspace_doubles())
        check(lib.raft_flow_range_visibility_f32(_dev.ptr(flows), _dev.ptr(mask) if mask is not None else None,
                                                 _dev.ptr(visible) if visible is not None else None, _dev.ptr(fraction), int(N), H, W,
                                                 float(threshold), int(bool(apply)), _dev.ptr(ws), records, _dev.stream_ptr()),
              'range_visibility')
    return visible, fraction


def range_map(flow) -> torch.Tensor:
    """The range map of a float32 flow ``(..., H, W, 2)`` (NumPy or torch, host or device; Wang et al. 2018):
    a float32 device tensor ``(..., H, W)`` that says how much of the flow's own grid lands on each pixel when every vector is
    splatted forward with bilinear weights -- 1 under zero flow, 0 where no vector ends, above 1 where several do.  The weights are
    quantised to 1 / 4096 per axis and summed as integers, so the result does not depend on the order of the adds: it repeats bit for
    bit.  A vector that ends outside ``(-1, W) x (-1, H)`` or is not finite contributes nothing."""
    shape = tuple(flow.shape) if hasattr(flow, 'shape') else np.shape(flow)
    if len(shape) < 3 or shape[-1] != 2:
        raise ValueError(f'range_map expects a flow (..., H, W, 2), got {shape}')
    if 0 in shape:
        raise ValueError(f'empty input {shape}')
    t = _on_device(flow)
    if t.dtype != torch.float32:
        raise TypeError(f'a flow is float32, got {t.dtype}')
    return _dev.wrap(range_map_launch(t.reshape((-1,) + shape[-3:])).view(shape[:-1]))


def range_occlusion(flow_forward, flow_backward, threshold=RANGE_THRESHOLD):
    """The range-map occlusion test of two float32 flows ``(H, W, 2)`` or ``(N, H, W, 2)`` (NumPy or torch, host or device):
    ``(occluded_forward, occluded_backward)``, uint8 device tensors ``(..., H, W)`` with 1 where a vector cannot be trusted.  A pixel
    of frame 1 is occluded when less than ``threshold`` of frame 2's grid lands on it under ``flow_backward`` (``range_map``; no
    pixel of frame 2 came from there) or when its own vector leaves the frame, so the masks mean what ``flow_consistency``'s do.
    ``threshold`` lies in ``(0, 1]``; the comparison is made on the integer sums.  A local expansion by a factor ``s`` thins the
    range to about ``1 / s^2``: under a zoom of more than about 1.4 the default marks everything."""
    threshold = check_range_threshold(threshold)
    t, f4, _, _ = _flow_4d(flow_forward, None)
    b = _flow_like(flow_backward, t.shape[:-1], 'range_occlusion')
    occ_f, occ_b = range_occlusion_launch(f4, b.reshape(f4.shape), threshold)
    return _dev.wrap(occ_f.view(t.shape[:-1])), _dev.wrap(occ_b.view(t.shape[:-1]))


# ------------------------------------------------------------------------------------------ forward splat of frames, the frame in between
FRAME_SPLAT_MAX_PIXELS = 1 << 24      # csrc/frame_splat.hip kFrameMaxPixels: every uint64 sum stays below 2^64
FRAME_SPLAT_MAX_CHANNELS = 4


def check_splat_time(t, unit=False):
    """A splat's time as a float: a number (no bool) whose float32 value is finite (``unit``: lies in ``[0, 1]``)."""
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, np.integer, np.floating)):
        raise ValueError(f't must be a number, got {t!r}')
    try:
        with np.errstate(over='ignore'):
            v = float(np.float32(t))
    except OverflowError:
        v = float('inf')
    if not np.isfinite(v) or (unit and not 0.0 <= v <= 1.0):
        raise ValueError(f't must {"lie in [0, 1]" if unit else "be finite"} as a float32, got {t!r}')
    return v


def _check_frame_sizes(slices, H, W, C, what):
    if not 1 <= C <= FRAME_SPLAT_MAX_CHANNELS:
        raise ValueError(f'{what} takes frames of 1 to {FRAME_SPLAT_MAX_CHANNELS} channels, got {C}')
    if H * W > FRAME_SPLAT_MAX_PIXELS or slices * H * W * FRAME_SPLAT_MAX_CHANNELS >= 1 << 31:
        raise ValueError(f'{what} takes frames of up to 2^24 pixels and fewer than 2^29 pixels in all, got {slices} x {H} x {W}: too large')


def _shape_and_type(x, what):
    """Shape and torch type of a NumPy / torch argument as ``_on_device`` will deliver it, read without touching a device."""
    if isinstance(x, torch.Tensor):
        return tuple(x.shape), (torch.float32 if x.dtype == torch.float64 else x.dtype)
    a = x if isinstance(x, np.ndarray) else np.asarray(x)
    kinds = {np.dtype(np.uint8): torch.uint8, np.dtype(np.bool_): torch.bool, np.dtype(np.float32): torch.float32,
             np.dtype(np.float64): torch.float32}
    if a.dtype not in kinds:
        raise TypeError(f'{what}: unsupported type {a.dtype}')
    return tuple(a.shape), kinds[a.dtype]


def _check_frames_flow_mask(frames, flow, mask, what):
    """``(N, H, W, C)`` uint8 / float32 frames, their flow ``(N, H, W, 2)`` and an optional uint8 mask ``(N, H, W)``: plain
    contiguous tensors of one device."""
    if frames.dim() != 4:
        raise ValueError(f'{what}: expected frames (N, H, W, C), got {tuple(frames.shape)}')
    if frames.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f'{what} takes uint8 or float32 frames, got {frames.dtype}')
    N, H, W, Cn = frames.shape
    if tuple(flow.shape) != (N, H, W, 2) or flow.device != frames.device:
        raise ValueError(f'frames {tuple(frames.shape)} on {frames.device} need a flow {(N, H, W, 2)}, got {tuple(flow.shape)} on {flow.device}')
    _check_flow(flow, what)
    if not frames.is_contiguous():
        raise ValueError(f'{what}: the frames must be contiguous, got strides {tuple(frames.stride())} for {tuple(frames.shape)}')
    if mask is not None:
        _check_out(mask, (N, H, W), torch.uint8, frames.device)


def _frame_workspace(device, slices, H, W, C):
    """The uint64 sums of ``slices`` frames of ``C`` channels in the stream's grow-only workspace."""
    from . import losses
    nbytes = int(_dev.lib().raft_frame_splat_workspace_bytes(int(slices), int(H), int(W), int(C)))
    if nbytes <= 0:
        raise ValueError(f'a frame splat takes frames of up to 2^24 pixels and 1 to 4 channels, got {slices} x {H} x {W} x {C}: too large')
    return losses._workspace(device, nbytes)


def frame_splat_launch(frames: torch.Tensor, flow: torch.Tensor, t: float = 1.0, mask=None, want_weight: bool = False, out=None):
    """The launches themselves (``raft_splat_frames_*``): contiguous device frames ``(N, H, W, C)`` of
    uint8 / float32, their contiguous float32 flow ``(N, H, W, 2)`` and an optional contiguous uint8 ``mask`` ``(N, H, W)`` ->
    ``(splatted, weight)`` on the CURRENT stream (plain tensors): float32 ``(N, H, W, C)`` (``out`` when given) and float32
    ``(N, H, W)`` (None without ``want_weight``)."""
    t = check_splat_time(t)
    _check_frames_flow_mask(frames, flow, mask, 'splat')
    N, H, W, Cn = frames.shape
    _check_frame_sizes(N, H, W, Cn, 'splat')
    fn, src = _source_entry(frames, 'splat_frames')
    out = _check_out(out, (N, H, W, Cn), torch.float32, frames.device)
    weight = torch.empty((N, H, W), device=frames.device, dtype=torch.float32) if want_weight else None
    with torch.cuda.device(frames.device):
        ws = _frame_workspace(frames.device, N, H, W, Cn)
        check(fn(_dev.ptr(src), _dev.ptr(flow), _dev.ptr(mask) if mask is not None else None, t, _dev.ptr(out),
                 _dev.ptr(weight) if weight is not None else None, N, H, W, Cn, _dev.ptr(ws), _dev.stream_ptr()), 'splat_frames')
    return out, weight


def _interpolate_entry(in_dtype, dtype):
    """The entry's name and the result's type for frames of ``in_dtype`` and the result type asked for (None: float32)."""
    if in_dtype not in (torch.uint8, torch.float32):
        raise TypeError(f'interpolate takes uint8 or float32 frames, got {in_dtype}')
    if dtype in (None, torch.float32):
        return ('raft_interpolate_frames_f32' if in_dtype == torch.float32 else 'raft_interpolate_frames_u8_f32'), torch.float32
    if dtype == torch.uint8 and in_dtype == torch.uint8:
        return 'raft_interpolate_frames_u8', torch.uint8
    raise TypeError(f'interpolate returns float32, or uint8 for uint8 frames, got {in_dtype} -> {dtype}')


def interpolate_launch(image1: torch.Tensor, image2: torch.Tensor, flow_forward: torch.Tensor, flow_backward: torch.Tensor,
                       t: float = 0.5, mask1=None, mask2=None, want_holes: bool = False, dtype=None, out=None, holes=None):
    """The launches themselves (``raft_interpolate_frames_*``): two contiguous device frame batches
    ``(N, H, W, C)`` of one type (uint8 / float32), the contiguous float32 flows ``(N, H, W, 2)`` from frame 1 to frame 2 and
    back, optional contiguous uint8 masks ``(N, H, W)`` (non-zero = this pixel is splatted) -> ``(frame, holes)`` on the CURRENT
    stream (plain tensors): the frame at time ``t`` in ``[0, 1]``, ``(N, H, W, C)`` of ``dtype`` (float32, or uint8 for uint8
    frames; written into ``out`` when given), and the uint8 map ``(N, H, W)`` of the pixels nothing landed on (None without
    ``want_holes``; ``holes``: a tensor to write it into)."""
    t = check_splat_time(t, unit=True)
    _check_frames_flow_mask(image1, flow_forward, mask1, 'interpolate')
    _check_frames_flow_mask(image2, flow_backward, mask2, 'interpolate')
    if image1.shape != image2.shape or image1.dtype != image2.dtype or image1.device != image2.device:
        raise ValueError(f'expected two frame batches of one shape, type and device, got {tuple(image1.shape)} {image1.dtype} on '
                         f'{image1.device} / {tuple(image2.shape)} {image2.dtype} on {image2.device}')
    name, out_dtype = _interpolate_entry(image1.dtype, dtype)
    N, H, W, Cn = image1.shape
    _check_frame_sizes(2 * N, H, W, Cn, 'interpolate')
    out = _check_out(out, (N, H, W, Cn), out_dtype, image1.device)
    holes = _check_out(holes, (N, H, W), torch.uint8, image1.device, alloc=bool(want_holes))
    with torch.cuda.device(image1.device):
        ws = _frame_workspace(image1.device, 2 * N, H, W, Cn)
        check(getattr(_dev.lib(), name)(_dev.ptr(image1), _dev.ptr(image2), _dev.ptr(flow_forward), _dev.ptr(flow_backward),
                                        _dev.ptr(mask1) if mask1 is not None else None, _dev.ptr(mask2) if mask2 is not None else None,
                                        t, _dev.ptr(out), _dev.ptr(holes) if holes is not None else None, N, H, W, Cn, _dev.ptr(ws),
                                        _dev.stream_ptr()), 'interpolate_frames')
    return out, holes


def _frames_ahead(x, what):
    """Shape and type of a frames argument ``(H, W, C)`` / ``(N, H, W, C)``, checked before anything reaches a device."""
    shape, dtype = _shape_and_type(x, what)
    if len(shape) not in (3, 4):
        raise ValueError(f'{what} expects (H, W, C) or (N, H, W, C), got {shape}')
    if 0 in shape:
        raise ValueError(f'empty input {shape}')
    if dtype not in (torch.uint8, torch.float32):
        raise TypeError(f'{what} takes uint8 or float32 frames, got {dtype}')
    return shape, dtype


def _flow_ahead(flow, lead_shape, what):
    shape, dtype = _shape_and_type(flow, what)
    if shape != tuple(lead_shape) + (2,):
        raise ValueError(f'{what} expects a flow {tuple(lead_shape) + (2,)}, got {shape}')
    if dtype != torch.float32:
        raise TypeError(f'a flow is float32, got {dtype}')


def _mask_ahead(mask, lead_shape, what):
    if mask is None:
        return
    shape, dtype = _shape_and_type(mask, what)
    if shape != tuple(lead_shape):
        raise ValueError(f'{what} expects a mask {tuple(lead_shape)}, got {shape}')
    if dtype not in (torch.uint8, torch.bool):
        raise TypeError(f'a mask is uint8 or bool, got {dtype}')


def _mask_on_device(mask, shape3):
    return None if mask is None else _on_device(mask).view(torch.uint8).reshape(shape3)


def splat(frames, flow, t=1.0, mask=None, return_weight=False):
    """Forward splat: ``(H, W, C)`` or ``(N, H, W, C)`` frames (NumPy or torch, host or device, uint8, or
    float32 on 0 .. 255; float64 narrows; 1 to 4 channels) carried along ``flow`` (same leading shape, 2 channels, float32) to
    time ``t`` -> a contiguous float32 device tensor of the frames' shape: every pixel travels to ``(x + t * u, y + t * v)`` and
    hands its value to the four pixels around that point with bilinear weights; the result is the weighted mean of what landed,
    0 where nothing did.  ``return_weight=True`` also returns how much landed, float32 ``(..., H, W)``: at ``t = 1`` the flow's
    ``range_map``.  ``mask`` (uint8 / bool, the frames' leading shape): only pixels where it is non-zero travel.  Weights are
    quantised to 1 / 4096 per axis, float32 values to 1 / 256 (and clamped to 0 .. 255), and everything is summed as integers:
    the result does not depend on the order of the adds and repeats bit for bit.  A vector that ends outside ``(-1, W) x (-1, H)``
    or is not finite contributes nothing."""
    t = check_splat_time(t)
    shape, _ = _frames_ahead(frames, 'splat')
    _flow_ahead(flow, shape[:-1], 'splat')
    _mask_ahead(mask, shape[:-1], 'splat')
    shape4 = ((1,) + shape) if len(shape) == 3 else shape
    _check_frame_sizes(shape4[0], shape4[1], shape4[2], shape4[3], 'splat')
    x = _on_device(frames).reshape(shape4)
    f = _on_device(flow).reshape(shape4[:3] + (2,))
    out, weight = frame_splat_launch(x, f, t, _mask_on_device(mask, shape4[:3]), return_weight)
    out = _dev.wrap(out.view(shape))
    return (out, _dev.wrap(weight.view(shape[:-1]))) if return_weight else out


def _times(t):
    """``t`` of ``interpolate``: ``(list of checked floats, whether a sequence was given)``."""
    if isinstance(t, (list, tuple, np.ndarray)) and np.ndim(t) == 1:
        if len(t) == 0:
            raise ValueError('t must not be empty')
        return [check_splat_time(v, unit=True) for v in (t.tolist() if isinstance(t, np.ndarray) else t)], True
    return [check_splat_time(t, unit=True)], False


def interpolate(image1, image2, flow_forward, flow_backward, t=0.5, mask1=None, mask2=None, return_holes=False, dtype=None):
    """The frame at time ``t`` between two frames: ``(H, W, C)`` or ``(N, H, W, C)`` frames of one type
    (NumPy or torch, host or device, uint8, or float32 on 0 .. 255; 1 to 4 channels), the flow from frame 1 to frame 2 and the flow
    back (float32, the frames' leading shape) -> a contiguous device tensor of the frames' shape, float32 or -- ``dtype=
    torch.uint8``, for uint8 frames only -- uint8.  Frame 1 is splatted forward to ``t`` along ``flow_forward`` and frame 2 to
    ``1 - t`` along ``flow_backward`` (``splat``), and every pixel is the mean of what landed on it, frame 1's share weighted by
    ``1 - t`` and frame 2's by ``t``.  A pixel nothing landed on is a hole: it takes the cross-fade ``(1 - t) * image1 + t *
    image2`` of its own two values; ``return_holes=True`` also returns their uint8 map ``(..., H, W)``.  ``mask1`` / ``mask2``
    (uint8 / bool): only pixels where the mask is non-zero are splatted, e.g. ``occluded == 0`` of a bidirectional prediction.
    ``t`` in ``[0, 1]`` may be a sequence: the result then has a leading axis of that length (one pair of launches per time).
    Integer sums: the result repeats bit for bit."""
    times, many = _times(t)
    shape, in_dtype = _frames_ahead(image1, 'interpolate')
    shape2, in_dtype2 = _frames_ahead(image2, 'interpolate')
    if shape2 != shape or in_dtype2 != in_dtype:
        raise ValueError(f'expected two frames of one shape and type, got {shape} {in_dtype} / {shape2} {in_dtype2}')
    _, out_dtype = _interpolate_entry(in_dtype, dtype)
    _flow_ahead(flow_forward, shape[:-1], 'interpolate')
    _flow_ahead(flow_backward, shape[:-1], 'interpolate')
    _mask_ahead(mask1, shape[:-1], 'interpolate')
    _mask_ahead(mask2, shape[:-1], 'interpolate')
    shape4 = ((1,) + shape) if len(shape) == 3 else shape
    _check_frame_sizes(2 * shape4[0], shape4[1], shape4[2], shape4[3], 'interpolate')
    i1, i2 = _on_device(image1).reshape(shape4), _on_device(image2).reshape(shape4)
    ff, fb = _on_device(flow_forward).reshape(shape4[:3] + (2,)), _on_device(flow_backward).reshape(shape4[:3] + (2,))
    m1, m2 = _mask_on_device(mask1, shape4[:3]), _mask_on_device(mask2, shape4[:3])
    out = torch.empty((len(times),) + shape4, device=i1.device, dtype=out_dtype)
    holes = torch.empty((len(times),) + shape4[:3], device=i1.device, dtype=torch.uint8) if return_holes else None
    for k, tk in enumerate(times):
        interpolate_launch(i1, i2, ff, fb, tk, m1, m2, return_holes, out_dtype, out[k], holes[k] if return_holes else None)
    lead = (len(times),) if many else ()
    res = _dev.wrap(out.view(lead + shape))
    return (res, _dev.wrap(holes.view(lead + shape[:-1]))) if return_holes else res


# ------------------------------------------------------------------------------------------ points followed through a video
def point_grid(H, W, stride=1, N=1):
    """Every ``stride``-th pixel of an ``H x W`` frame as points: a host array ``(N, P, 2)`` float32 of ``(x, y)``, rows first
    (``P = ceil(H / stride) * ceil(W / stride)``), the same for each of the ``N`` videos.  With ``stride=1`` it is the start of
    a dense long-range flow: ``positions - point_grid(H, W)`` after ``track`` is that flow, ``lost`` its occlusion flag."""
    for name, v in (('H', H), ('W', W), ('stride', stride), ('N', N)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f'{name} must be an integer >= 1, got {v!r}')
    ys, xs = np.arange(0, int(H), int(stride), dtype=np.float32), np.arange(0, int(W), int(stride), dtype=np.float32)
    grid = np.stack(np.broadcast_arrays(xs[None, :], ys[:, None]), axis=-1).reshape(1, -1, 2)
    return np.ascontiguousarray(np.broadcast_to(grid, (int(N),) + grid.shape[1:]))


def check_track_time(t0, steps=0):
    """``t0`` of a track as an int: an integer (no bool) >= 0 with ``t0 + steps`` below 2^31."""
    if isinstance(t0, (bool, np.bool_)) or not isinstance(t0, (int, np.integer)) or t0 < 0 or int(t0) + int(steps) >= 1 << 31:
        raise ValueError(f't0 must be an integer >= 0 (with t0 + S below 2^31), got {t0!r}')
    return int(t0)


def _points_ahead(points, lost, start, what, lead=2):
    """Shapes and types of ``points`` ``(N, P, 2)`` float32 (``lead=1``: ``(P, 2)``), ``lost`` (uint8 / bool, the points' leading
    shape) and ``start`` (integers >= 0 below 2^31, the same shape), checked before anything reaches a device.  Returns the
    points' leading shape."""
    shape, dtype = _shape_and_type(points, what)
    if len(shape) != lead + 1 or shape[-1] != 2:
        raise ValueError(f'{what} expects points {"(N, P, 2)" if lead == 2 else "(P, 2)"}, got {shape}')
    if 0 in shape:
        raise ValueError(f'empty input {shape}')
    if dtype != torch.float32:
        raise TypeError(f'points are float32, got {dtype}')
    if lost is not None:
        lshape, ldtype = _shape_and_type(lost, what)
        if lshape != shape[:-1]:
            raise ValueError(f'{what} expects lost {shape[:-1]}, got {lshape}')
        if ldtype not in (torch.uint8, torch.bool):
            raise TypeError(f'lost is uint8 or bool, got {ldtype}')
    if start is not None:
        if isinstance(start, torch.Tensor):
            sshape, integral = tuple(start.shape), start.dtype in (torch.int32, torch.int64)
            host = start if start.device.type == 'cpu' else None
        else:
            host = np.asarray(start)
            sshape, integral = host.shape, host.dtype.kind in 'iu'
        if not integral:
            raise TypeError(f'start holds integers (frame indices), got {start.dtype if hasattr(start, "dtype") else type(start)}')
        if tuple(sshape) != shape[:-1]:
            raise ValueError(f'{what} expects start {shape[:-1]}, got {tuple(sshape)}')
        if host is not None and (int(host.min()) < 0 or int(host.max()) >= 1 << 31):
            raise ValueError('start holds frame indices >= 0 (below 2^31)')
    return shape[:-1]


def _start_on_device(start, shape):
    if start is None:
        return None
    t = start.detach() if isinstance(start, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(start).astype(np.int32)))
    return t.to(device=_dev.require_gpu(), dtype=torch.int32).reshape(shape).contiguous()


def _check_track_sizes(S, N, P, H, W):
    if S * N * H * W * 2 >= 1 << 31 or S * N * P * 2 >= 1 << 31:
        raise ValueError(f'a track takes fewer than 2^31 elements of flow and of positions, got (S, N, H, W) = {(S, N, H, W)} and '
                         f'P = {P}: too large')


def track_launch(points: torch.Tensor, forward: torch.Tensor, backward=None, lost=None, start=None, t0: int = 0,
                 alpha: float = CONSISTENCY_ALPHA, beta: float = CONSISTENCY_BETA, out=None):
    """The launch itself (``raft_track_points_f32``): contiguous float32 device points ``(N, P, 2)`` as
    ``(x, y)`` in pixels, the contiguous float32 flows ``forward`` ``(S, N, H, W, 2)`` of the pairs ``t0 + s -> t0 + s + 1`` and
    ``backward`` (the same shape, the other direction; None: only the frame borders are tested), optional contiguous ``lost``
    (uint8 ``(N, P)``, nonzero = already lost) and ``start`` (int32 ``(N, P)``: a point is copied through until its frame) ->
    ``(positions (S, N, P, 2) float32, lost (S, N, P) uint8)``, the state after every step, by ONE launch on the CURRENT stream
    (plain tensors).  ``out``: a pair of tensors to write them into; with ``S = 1`` it may be ``(points.view(1, N, P, 2),
    lost.view(1, N, P))`` -- the in-place step of a stream."""
    alpha, beta = check_consistency_args(alpha, beta)
    if points.dim() != 3 or points.shape[-1] != 2 or points.dtype != torch.float32 or not points.is_contiguous() or 0 in points.shape:
        raise ValueError(f'expected contiguous float32 points (N, P, 2), got {tuple(points.shape)} {points.dtype}')
    N, P, _ = points.shape
    if forward.dim() != 5 or forward.shape[1] != N or forward.shape[-1] != 2 or forward.device != points.device or 0 in forward.shape:
        raise ValueError(f'points {tuple(points.shape)} on {points.device} need flows (S, {N}, H, W, 2), got {tuple(forward.shape)} on '
                         f'{forward.device}')
    _check_flow(forward, 'track')
    S, _, H, W, _ = forward.shape
    if backward is not None:
        if backward.shape != forward.shape or backward.device != forward.device:
            raise ValueError(f'expected a backward flow {tuple(forward.shape)} on {forward.device}, got {tuple(backward.shape)} on '
                             f'{backward.device}')
        _check_flow(backward, 'track')
    t0 = check_track_time(t0, S)
    _check_track_sizes(S, N, P, H, W)
    if points.data_ptr() % 8:
        raise ValueError('track reads whole points: they must be 8-byte aligned')
    if lost is not None:
        lost = _check_out(lost, (N, P), torch.uint8, points.device)
    if start is not None:
        start = _check_out(start, (N, P), torch.int32, points.device)
    if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
        raise ValueError('out must be a pair (positions (S, N, P, 2), lost (S, N, P))')
    pos_out = _check_out(None if out is None else out[0], (S, N, P, 2), torch.float32, points.device)
    lost_out = _check_out(None if out is None else out[1], (S, N, P), torch.uint8, points.device)
    if pos_out.data_ptr() % 8:
        raise ValueError('track writes whole points: the positions must be 8-byte aligned')
    with torch.cuda.device(points.device):
        check(_dev.lib().raft_track_points_f32(_dev.ptr(points), _dev.ptr(lost) if lost is not None else None,
                                               _dev.ptr(start) if start is not None else None, t0, _dev.ptr(forward),
                                               _dev.ptr(backward) if backward is not None else None, _dev.ptr(pos_out),
                                               _dev.ptr(lost_out), S, N, P, H, W, alpha, beta, _dev.stream_ptr()), 'track_points')
    return pos_out, lost_out


def track(points, forward, backward=None, lost=None, start=None, t0=0, alpha=CONSISTENCY_ALPHA, beta=CONSISTENCY_BETA):
    """Points followed along flows: ``points`` ``(N, P, 2)`` float32 as ``(x, y)`` in pixels (NumPy or
    torch, host or device; float64 narrows), ``forward`` the flows ``(S, N, H, W, 2)`` of ``S`` consecutive frame pairs of ``N``
    videos, or ``(N, H, W, 2)`` for one step, and ``backward`` the flows of the same pairs in the other direction ->
    ``(positions, lost)``, device tensors ``(S, N, P, 2)`` float32 and ``(S, N, P)`` uint8: where every point is after every
    step (without the step axis for a 4-D ``forward``).  A step samples the forward flow bilinearly at the point, moves the point
    by it, samples the backward flow there and applies ``flow_consistency``'s test with ``alpha`` / ``beta`` (Meister et al.
    2018, whose values the defaults are).  ``lost``: 0 = tracked, 1 = the point or its new position lies outside ``[0, W - 1] x
    [0, H - 1]`` (or is NaN), 2 = the two flows disagree (an occlusion); a lost point stays lost and keeps the position it was
    last tracked at.  ``backward=None``: only the frame borders are tested.  ``lost`` (uint8 / bool ``(N, P)``): the codes to
    begin with; ``start`` (integers ``(N, P)``) with ``t0``, the frame index of the first pair's first frame: a point waits,
    untouched, until the step that begins at its frame.  ONE launch on the current stream, whatever ``S`` is; the result equals
    its float32 NumPy restatement bit for bit."""
    alpha, beta = check_consistency_args(alpha, beta)
    lead = _points_ahead(points, lost, start, 'track')
    N, P = lead
    fshape, fdtype = _shape_and_type(forward, 'track')
    if len(fshape) not in (4, 5) or fshape[-1] != 2 or fshape[-4] != N or 0 in fshape:
        raise ValueError(f'track expects flows (S, N, H, W, 2) or (N, H, W, 2) with N = {N}, got {fshape}')
    if fdtype != torch.float32:
        raise TypeError(f'a flow is float32, got {fdtype}')
    if backward is not None:
        _flow_ahead(backward, fshape[:-1], 'track')
    shape5 = ((1,) + fshape) if len(fshape) == 4 else fshape
    t0 = check_track_time(t0, shape5[0])
    _check_track_sizes(shape5[0], N, P, shape5[2], shape5[3])
    p = _on_device(points)
    f = _on_device(forward).reshape(shape5)
    b = None if backward is None else _on_device(backward).reshape(shape5)
    pos, codes = track_launch(p, f, b, _mask_on_device(lost, lead), _start_on_device(start, lead), t0, alpha, beta)
    if len(fshape) == 4:
        pos, codes = pos[0], codes[0]
    return _dev.wrap(pos), _dev.wrap(codes)


# ------------------------------------------------------------------------------------------ corner detection
DETECT_MAX_POINTS = _ffi._CONSTANTS['RAFT_DETECT_MAX_POINTS']
DETECT_MAX_MIN_DISTANCE = _ffi._CONSTANTS['RAFT_DETECT_MAX_MIN_DISTANCE']
DETECT_MAX_BLOCK_RADIUS = 3                                           # csrc/point_detect.hip kMaxBlockRadius
# choices, not tuned values: OpenCV's qualityLevel convention and blockSize = 3, Harris' usual k
DETECT_MIN_DISTANCE, DETECT_QUALITY_LEVEL, DETECT_BLOCK_RADIUS, DETECT_HARRIS_K, DETECT_BORDER = 7, 0.01, 1, 0.04, 8
DETECT_METHODS = {'min_eig': 0, 'harris': 1}
LOST_EMPTY = 3                                                        # the code of a slot that never held a point


def _int_in(v, name, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f'{name} must be an integer in {lo} .. {hi}, got {v!r}')
    return int(v)


def check_score_args(block_radius=DETECT_BLOCK_RADIUS, method='min_eig', harris_k=DETECT_HARRIS_K, border=DETECT_BORDER):
    """The corner score's parameters as ``(block_radius, method code, harris_k, border)``: ``block_radius`` an integer in 1 .. 3,
    ``method`` 'min_eig' or 'harris', ``harris_k`` a number (no bool) that is finite and >= 0 as a float32, ``border`` an integer
    >= ``block_radius + 1``."""
    r = _int_in(block_radius, 'block_radius', 1, DETECT_MAX_BLOCK_RADIUS)
    if not isinstance(method, str) or method not in DETECT_METHODS:
        raise ValueError(f'method must be one of {sorted(DETECT_METHODS)}, got {method!r}')
    k = _float32_value(harris_k, 'harris_k')
    if not (np.isfinite(k) and k >= 0):
        raise ValueError(f'harris_k must be finite and >= 0 as a float32, got {harris_k!r}')
    if isinstance(border, (bool, np.bool_)) or not isinstance(border, (int, np.integer)) or not r + 1 <= border <= 1 << 29:
        raise ValueError(f'border must be an integer >= block_radius + 1 = {r + 1}, got {border!r}')
    return r, DETECT_METHODS[method], k, int(border)


def check_detect_args(max_points, min_distance=DETECT_MIN_DISTANCE, quality_level=DETECT_QUALITY_LEVEL):
    """``(max_points, min_distance, quality_level)`` of a detection: integers in 1 .. 4096 and 1 .. 15, and a number (no bool)
    whose float32 value lies in ``[0, 1)``."""
    K = _int_in(max_points, 'max_points', 1, DETECT_MAX_POINTS)
    m = _int_in(min_distance, 'min_distance', 1, DETECT_MAX_MIN_DISTANCE)
    q = _float32_value(quality_level, 'quality_level')
    if not 0.0 <= q < 1.0:
        raise ValueError(f'quality_level must lie in [0, 1) as a float32, got {quality_level!r}')
    return K, m, q


DETECT_OPTIONS = ('min_distance', 'quality_level', 'block_radius', 'method', 'harris_k', 'border', 'mask')


def check_detect_options(detect, max_points=1):
    """``detect=dict(...)`` of the tracker: a dict (None: empty) of ``DETECT_OPTIONS`` whose values pass the checks of
    ``detect_points``; returns a copy."""
    if detect is None:
        return {}
    if not isinstance(detect, dict) or not set(detect) <= set(DETECT_OPTIONS):
        raise ValueError(f'detect must be a dict of {", ".join(DETECT_OPTIONS)}, got {detect!r}')
    detect = dict(detect)
    check_detect_args(max_points, detect.get('min_distance', DETECT_MIN_DISTANCE), detect.get('quality_level', DETECT_QUALITY_LEVEL))
    check_score_args(detect.get('block_radius', DETECT_BLOCK_RADIUS), detect.get('method', 'min_eig'),
                     detect.get('harris_k', DETECT_HARRIS_K), detect.get('border', DETECT_BORDER))
    if detect.get('mask') is not None:
        shape, dtype = _shape_and_type(detect['mask'], 'detect')
        if len(shape) != 3 or dtype not in (torch.uint8, torch.bool):
            raise ValueError(f'the mask of detect is uint8 or bool (N, H, W), got {shape} {dtype}')
    return detect


def _check_detect_sizes(N, H, W, C, border, what):
    if C not in (1, 3):
        raise ValueError(f'{what} takes frames of 1 or 3 channels, got {C}')
    if H <= 2 * border or W <= 2 * border:
        raise ValueError(f'{what}: H and W must be greater than 2 * border = {2 * border}, got {H} x {W}')
    if H * W >= 1 << 32 or N * H * W >= 1 << 31:
        raise ValueError(f'{what} takes fewer than 2^31 pixels in all, got {N} x {H} x {W}: too large')


def _check_detect_frames(frames, what):
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or 0 in frames.shape or not frames.is_contiguous():
        raise ValueError(f'{what}: expected contiguous frames (N, H, W, C), got '
                         f'{tuple(frames.shape) if hasattr(frames, "shape") else type(frames)}')
    if frames.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f'{what} takes uint8 or float32 frames, got {frames.dtype}')


def corner_score_launch(frames: torch.Tensor, block_radius: int = DETECT_BLOCK_RADIUS, method: str = 'min_eig',
                        harris_k: float = DETECT_HARRIS_K, border: int = DETECT_BORDER, want_max: bool = False, out=None):
    """The launch itself (``raft_corner_score_*``): contiguous device frames ``(N, H, W, C)``, uint8 or
    float32, ``C`` 1 or 3 -> ``(score (N, H, W) float32, smax (N,) float32 or None)`` on the CURRENT stream (plain tensors)."""
    r, code, k, border = check_score_args(block_radius, method, harris_k, border)
    _check_detect_frames(frames, 'corner_score')
    N, H, W, Cn = frames.shape
    _check_detect_sizes(N, H, W, Cn, border, 'corner_score')
    out = _check_out(out, (N, H, W), torch.float32, frames.device)
    smax = torch.empty((N,), device=frames.device, dtype=torch.float32) if want_max else None
    fn, src = _source_entry(frames, 'corner_score')
    with torch.cuda.device(frames.device):
        check(fn(_dev.ptr(src), _dev.ptr(out), _dev.ptr(smax) if smax is not None else None, N, H, W, Cn, r, code, k, border,
                 _dev.stream_ptr()), 'corner_score')
    return out, smax


def corner_score(frames, block_radius=DETECT_BLOCK_RADIUS, method='min_eig', harris_k=DETECT_HARRIS_K, border=DETECT_BORDER,
                 return_max=False):
    """The corner score of every pixel: ``(H, W, C)`` or ``(N, H, W, C)`` frames (NumPy or torch, host or
    device, uint8, or float32 on 0 .. 255; float64 narrows; 1 or 3 channels) -> a float32 device tensor of the frames' leading
    shape.  ``method='min_eig'`` is the smaller eigenvalue of the structure tensor (Shi-Tomasi), ``'harris'`` ``det - harris_k *
    trace^2``, of Sobel derivatives summed over a ``(2 * block_radius + 1)^2`` window; negative responses and NaNs are 0, and so
    are the pixels closer than ``border`` to a frame edge.  ``return_max=True`` also returns the per-image maximum.  Every operation
    is one float32 operation in a fixed order: the map equals its NumPy restatement bit for bit."""
    r, _, k, border = check_score_args(block_radius, method, harris_k, border)
    shape, _ = _frames_ahead(frames, 'corner_score')
    shape4 = ((1,) + shape) if len(shape) == 3 else shape
    _check_detect_sizes(shape4[0], shape4[1], shape4[2], shape4[3], border, 'corner_score')
    score, smax = corner_score_launch(_on_device(frames).reshape(shape4), r, method, k, border, return_max)
    score = _dev.wrap(score.view(shape[:-1]))
    return (score, _dev.wrap(smax.view(shape[:-3]))) if return_max else score


def detect_workspace_bytes(N, H, W, min_distance=DETECT_MIN_DISTANCE):
    """``raft_detect_points_workspace_bytes``: the bytes a detection on ``(N, H, W)`` frames needs (host arithmetic only)."""
    nbytes = int(_ffi.load_library().raft_detect_points_workspace_bytes(int(N), int(H), int(W), int(min_distance)))
    if nbytes <= 0:
        raise ValueError(f'a detection takes fewer than 2^31 pixels in all and min_distance in 1 .. {DETECT_MAX_MIN_DISTANCE}, got '
                         f'{N} x {H} x {W}, min_distance = {min_distance}: too large')
    return nbytes


def _check_avoid(avoid, N, device=None):
    """``avoid=(points (N, P, 2) float32, lost (N, P) uint8 / bool)`` by shape and type alone; returns P."""
    if not isinstance(avoid, (tuple, list)) or len(avoid) != 2:
        raise ValueError('avoid must be a pair (points (N, P, 2), lost (N, P))')
    (N2, P) = _points_ahead(avoid[0], avoid[1], None, 'avoid')
    if avoid[1] is None:
        raise ValueError('avoid must be a pair (points (N, P, 2), lost (N, P))')
    if N2 != N:
        raise ValueError(f'avoid holds points of {N2} videos, the frames are {N}')
    if N * P * 2 >= 1 << 31:
        raise ValueError(f'avoid takes fewer than 2^30 points, got {N} x {P}: too large')
    return P


def detect_points_launch(frames: torch.Tensor, max_points: int, min_distance: int = DETECT_MIN_DISTANCE,
                         quality_level: float = DETECT_QUALITY_LEVEL, block_radius: int = DETECT_BLOCK_RADIUS, method: str = 'min_eig',
                         harris_k: float = DETECT_HARRIS_K, border: int = DETECT_BORDER, mask=None, avoid=None, want_lost: bool = False,
                         out=None, workspace=None):
    """The launches themselves (``raft_detect_points``): contiguous device frames ``(N, H, W, C)``, uint8 or
    float32, ``C`` 1 or 3; an optional contiguous uint8 ``mask`` ``(N, H, W)`` (nonzero = allowed); an optional pair ``avoid =
    (points (N, P, 2) float32, lost (N, P) uint8)`` of contiguous device tensors -> ``(points (N, K, 2) float32, scores (N, K)
    float32, count (N,) int32, lost (N, K) uint8 or None)`` on the CURRENT stream (plain tensors).  ``out``: a tuple of four tensors
    to write them into (the last may be None without ``want_lost``); ``workspace``: a contiguous uint8 device tensor of at least
    ``detect_workspace_bytes(N, H, W, min_distance)`` bytes, 8-byte aligned (None: the stream's grow-only workspace)."""
    K, m, q = check_detect_args(max_points, min_distance, quality_level)
    r, code, k, border = check_score_args(block_radius, method, harris_k, border)
    _check_detect_frames(frames, 'detect_points')
    N, H, W, Cn = frames.shape
    _check_detect_sizes(N, H, W, Cn, border, 'detect_points')
    dev = frames.device
    if mask is not None:
        mask = _check_out(mask, (N, H, W), torch.uint8, dev)
    P = 0
    if avoid is not None:
        P = _check_avoid(avoid, N)
        avoid = (_check_out(avoid[0], (N, P, 2), torch.float32, dev), _check_out(avoid[1], (N, P), torch.uint8, dev))
    if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 4):
        raise ValueError('out must be a tuple (points (N, K, 2), scores (N, K), count (N,), lost (N, K) or None)')
    out = (None,) * 4 if out is None else out
    points = _check_out(out[0], (N, K, 2), torch.float32, dev)
    scores = _check_out(out[1], (N, K), torch.float32, dev)
    count = _check_out(out[2], (N,), torch.int32, dev)
    lost = _check_out(out[3], (N, K), torch.uint8, dev, alloc=bool(want_lost))
    nbytes = detect_workspace_bytes(N, H, W, m)
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1
                                  or workspace.numel() < nbytes or workspace.device != dev or not workspace.is_contiguous()
                                  or workspace.data_ptr() % 8):
        raise ValueError(f'workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}, 8-byte aligned')
    with torch.cuda.device(dev):
        if workspace is None:
            from . import losses
            workspace = losses._workspace(dev, nbytes)
        check(_dev.lib().raft_detect_points(_dev.ptr(frames), int(frames.dtype == torch.uint8), _dev.ptr(mask) if mask is not None else None,
                                            _dev.ptr(avoid[0]) if avoid is not None else None,
                                            _dev.ptr(avoid[1]) if avoid is not None else None, P, _dev.ptr(points), _dev.ptr(scores),
                                            _dev.ptr(count), _dev.ptr(lost) if lost is not None else None, N, H, W, Cn, K, m, q, r, code,
                                            k, border, _dev.ptr(workspace), _dev.stream_ptr()), 'detect_points')
    return points, scores, count, lost


def detect_points(frames, max_points, min_distance=DETECT_MIN_DISTANCE, quality_level=DETECT_QUALITY_LEVEL,
                  block_radius=DETECT_BLOCK_RADIUS, method='min_eig', harris_k=DETECT_HARRIS_K, border=DETECT_BORDER, mask=None,
                  avoid=None, return_lost=False):
    """Good features to track: ``(N, H, W, C)`` frames (NumPy or torch, host or device, uint8, or float32 on
    0 .. 255; 1 or 3 channels) -> ``(points (N, K, 2) float32, scores (N, K) float32, count (N,) int32)`` as device tensors, ``K =
    max_points`` (1 .. 4096): per image the up to ``K`` strongest corners as ``(x, y)``, STRONGEST FIRST; the slots from
    ``count[n]`` on hold ``(-1, -1)`` and score 0.  ``return_lost=True`` also returns ``lost (N, K)`` uint8, 0 for a filled slot
    and 3 for an empty one: with ``points`` it is the state a tracker starts from (``track`` carries code 3 through untouched).

    A pixel is taken iff its ``corner_score`` is the largest in its ``(2 * min_distance + 1)^2`` window (of equal scores the
    earlier pixel in raster order wins), positive, and at least ``quality_level`` times the image's largest score; ``mask`` (uint8
    / bool ``(N, H, W)``, nonzero = allowed) and ``avoid = (points (N, P, 2), lost (N, P))`` -- no new point within ``min_distance``
    (Chebyshev) of a point whose code is 0 -- are applied after that suppression.  The window replaces OpenCV's greedy
    minimum-distance rule: any two points are more than ``min_distance`` apart in both methods, but the sets differ.  The result
    equals its NumPy restatement bit for bit and repeats bit for bit."""
    K, m, q = check_detect_args(max_points, min_distance, quality_level)
    r, _, k, border = check_score_args(block_radius, method, harris_k, border)
    shape, _ = _frames_ahead(frames, 'detect_points')
    if len(shape) != 4:
        raise ValueError(f'detect_points expects frames (N, H, W, C), got {shape}')
    _check_detect_sizes(shape[0], shape[1], shape[2], shape[3], border, 'detect_points')
    _mask_ahead(mask, shape[:3], 'detect_points')
    if avoid is not None:
        _check_avoid(avoid, shape[0])
    detect_workspace_bytes(shape[0], shape[1], shape[2], m)
    x = _on_device(frames)
    if avoid is not None:
        avoid = (_on_device(avoid[0]), _on_device(avoid[1]).view(torch.uint8))
    res = detect_points_launch(x, K, m, q, r, method, k, border, _mask_on_device(mask, shape[:3]), avoid, return_lost)
    return tuple(_dev.wrap(t) for t in (res if return_lost else res[:3]))


def refill_points_launch(pos: torch.Tensor, lost: torch.Tensor, new_points: torch.Tensor, new_count: torch.Tensor, t: int,
                         born: torch.Tensor, ids: torch.Tensor, next_id: torch.Tensor, out=None):
    """The launch itself (``raft_refill_points``): a tracker's state ``pos (N, P, 2)`` float32 and ``lost
    (N, P)`` uint8, a detection's ``new_points (N, K, 2)`` float32 (strongest first) with ``new_count (N,)`` int32, and the frame
    index ``t`` -> ``(positions, lost)`` (``out``: a pair to write them into; ``out=(pos, lost)`` refills in place).  Per video
    the slots with a nonzero code take the new points in ascending slot order until either side runs out: such a slot gets the
    new position, code 0, ``born = t`` and the next id of the video.  ``born``, ``ids`` ``(N, P)`` and ``next_id`` ``(N,)``
    (int32) are updated in place.  One launch on the CURRENT stream; all tensors contiguous on one device."""
    t = check_track_time(t)
    if not isinstance(pos, torch.Tensor) or pos.dim() != 3 or pos.shape[-1] != 2 or pos.dtype != torch.float32 or not pos.is_contiguous() \
            or 0 in pos.shape:
        raise ValueError(f'expected contiguous float32 positions (N, P, 2), got '
                         f'{(tuple(pos.shape), pos.dtype) if isinstance(pos, torch.Tensor) else type(pos)}')
    N, P, _ = pos.shape
    dev = pos.device
    if N * P * 2 >= 1 << 31:
        raise ValueError(f'a refill takes fewer than 2^30 points, got {N} x {P}: too large')
    lost = _check_out(lost, (N, P), torch.uint8, dev)
    if not isinstance(new_points, torch.Tensor) or new_points.dim() != 3 or new_points.shape[0] != N or new_points.shape[2] != 2 \
            or not 1 <= new_points.shape[1] <= DETECT_MAX_POINTS:
        raise ValueError(f'expected new points ({N}, K, 2) with K in 1 .. {DETECT_MAX_POINTS}, got '
                         f'{tuple(new_points.shape) if isinstance(new_points, torch.Tensor) else type(new_points)}')
    K = new_points.shape[1]
    new_points = _check_out(new_points, (N, K, 2), torch.float32, dev)
    new_count = _check_out(new_count, (N,), torch.int32, dev)
    born = _check_out(born, (N, P), torch.int32, dev)
    ids = _check_out(ids, (N, P), torch.int32, dev)
    next_id = _check_out(next_id, (N,), torch.int32, dev)
    if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
        raise ValueError('out must be a pair (positions (N, P, 2), lost (N, P))')
    pos_out = _check_out(None if out is None else out[0], (N, P, 2), torch.float32, dev)
    lost_out = _check_out(None if out is None else out[1], (N, P), torch.uint8, dev)
    with torch.cuda.device(dev):
        check(_dev.lib().raft_refill_points(_dev.ptr(pos), _dev.ptr(lost), _dev.ptr(new_points), _dev.ptr(new_count), t, _dev.ptr(pos_out),
                                            _dev.ptr(lost_out), _dev.ptr(born), _dev.ptr(ids), _dev.ptr(next_id), N, P, K,
                                            _dev.stream_ptr()), 'refill_points')
    return pos_out, lost_out


def tracker_ids(lost: torch.Tensor, start=None):
    """What a replenishing tracker starts from for the state ``lost (N, P)``: ``(born, ids, next_id)`` int32 device tensors --
    ``born`` the slot's ``start`` (or 0), ``ids`` ``0 .. P - 1``, both -1 for an empty slot (code 3); ``next_id`` ``P``."""
    N, P = lost.shape
    empty = lost == LOST_EMPTY
    minus = torch.full((N, P), -1, device=lost.device, dtype=torch.int32)
    born = torch.zeros((N, P), device=lost.device, dtype=torch.int32) if start is None else start.to(torch.int32)
    ids = torch.arange(P, device=lost.device, dtype=torch.int32).expand(N, P)
    return (torch.where(empty, minus, born).contiguous(), torch.where(empty, minus, ids).contiguous(),
            torch.full((N,), P, device=lost.device, dtype=torch.int32))


# ------------------------------------------------------------------------------------------ connected components
OBJECTS_MAX = _ffi._CONSTANTS['RAFT_OBJECTS_MAX']
OBJECTS_MIN_AREA, OBJECTS_CONNECTIVITY = 64, 8                        # choices, not tuned values
OBJECTS_MAX_AREA = (1 << 31) - 2                                      # H * W of one image


class Objects(NamedTuple):
    """What ``find_objects`` returns: per image the up to ``K`` largest components, LARGEST FIRST -- ``labels`` ``(N, H, W)`` int32
    (slot + 1, 0 elsewhere), ``count`` ``(N,)`` int32, ``area`` ``(N, K)`` int32, ``boxes`` ``(N, K, 4)`` int32 as inclusive
    ``x0, y0, x1, y1``, ``centroid`` ``(N, K, 2)`` float32 as ``(x, y)`` and ``mean_flow`` ``(N, K, 2)`` float32.  Fields that
    were not asked for are None."""
    labels: object
    count: object
    area: object
    boxes: object
    centroid: object
    mean_flow: object


def check_objects_args(max_objects=1, min_area=OBJECTS_MIN_AREA, connectivity=OBJECTS_CONNECTIVITY):
    """``(max_objects, min_area, connectivity)`` of a component search: integers (no bool) in 1 .. ``OBJECTS_MAX`` and 1 .. 2^31 - 2,
    and 4 or 8."""
    K = _int_in(max_objects, 'max_objects', 1, OBJECTS_MAX)
    a = _int_in(min_area, 'min_area', 1, OBJECTS_MAX_AREA)
    if isinstance(connectivity, (bool, np.bool_)) or not isinstance(connectivity, (int, np.integer)) or connectivity not in (4, 8):
        raise ValueError(f'connectivity must be 4 or 8, got {connectivity!r}')
    return K, a, int(connectivity)


def _check_objects_sizes(N, H, W, what):
    if H * W > OBJECTS_MAX_AREA or N * H * W >= 1 << 31:
        raise ValueError(f'{what} takes fewer than 2^31 pixels in all, got {N} x {H} x {W}: too large')


def components_workspace_bytes(N, H, W, connectivity=OBJECTS_CONNECTIVITY, min_area=1):
    """``raft_components_workspace_bytes``: the bytes a component search on ``(N, H, W)`` masks needs (host arithmetic only)."""
    nbytes = int(_ffi.load_library().raft_components_workspace_bytes(int(N), int(H), int(W), int(connectivity), int(min_area)))
    if nbytes <= 0:
        raise ValueError(f'a component search takes fewer than 2^31 pixels in all, connectivity 4 or 8 and min_area >= 1, got '
                         f'{N} x {H} x {W}, connectivity = {connectivity}, min_area = {min_area}: too large')
    return nbytes


def _check_objects_masks(mask, exclude, what):
    if not isinstance(mask, torch.Tensor) or mask.dim() != 3 or 0 in mask.shape:
        raise ValueError(f'{what}: expected a contiguous uint8 mask (N, H, W), got '
                         f'{tuple(mask.shape) if hasattr(mask, "shape") else type(mask)}')
    N, H, W = mask.shape
    _check_objects_sizes(N, H, W, what)
    mask = _check_out(mask, (N, H, W), torch.uint8, mask.device)
    if exclude is not None:
        exclude = _check_out(exclude, (N, H, W), torch.uint8, mask.device)
    return mask, exclude, N, H, W


def _objects_workspace(workspace, dev, nbytes):
    """The caller's workspace, checked, or the stream's grow-only one (inside ``torch.cuda.device(dev)``)."""
    if workspace is None:
        from . import losses
        return losses._workspace(dev, nbytes)
    if (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or workspace.numel() < nbytes
            or workspace.device != dev or not workspace.is_contiguous() or workspace.data_ptr() % 8):
        raise ValueError(f'workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}, 8-byte aligned')
    return workspace


def label_components_launch(mask: torch.Tensor, exclude=None, connectivity: int = OBJECTS_CONNECTIVITY, out=None, workspace=None):
    """The launches themselves (``raft_label_components``): a contiguous uint8 device ``mask`` ``(N, H, W)``
    and an optional ``exclude`` of the same kind -> ``labels`` ``(N, H, W)`` int32 on the CURRENT stream (a plain tensor): 0 for
    background, ``1 +`` the smallest raster index ``y * W + x`` of its component for a foreground pixel.  Three launches."""
    _, _, conn = check_objects_args(1, 1, connectivity)
    mask, exclude, N, H, W = _check_objects_masks(mask, exclude, 'label_components')
    labels = _check_out(out, (N, H, W), torch.int32, mask.device)
    nbytes = components_workspace_bytes(N, H, W, conn, 1)
    with torch.cuda.device(mask.device):
        ws = _objects_workspace(workspace, mask.device, nbytes)
        check(_dev.lib().raft_label_components(_dev.ptr(mask), _dev.ptr(exclude) if exclude is not None else None, _dev.ptr(labels), N, H,
                                               W, conn, _dev.ptr(ws), _dev.stream_ptr()), 'label_components')
    return labels


def find_objects_launch(mask: torch.Tensor, max_objects: int, min_area: int = OBJECTS_MIN_AREA, connectivity: int = OBJECTS_CONNECTIVITY,
                        exclude=None, flow=None, want_labels: bool = True, workspace=None):
    """The launches themselves (``raft_find_objects``): a contiguous uint8 device ``mask`` ``(N, H, W)``, an
    optional ``exclude`` of the same kind and an optional contiguous float32 ``flow`` ``(N, H, W, 2)`` -> ``Objects`` of plain
    tensors on the CURRENT stream (``labels`` None without ``want_labels``, ``mean_flow`` None without a flow).  One memset and
    seven launches enqueued by one call, nothing synchronised."""
    K, a, conn = check_objects_args(max_objects, min_area, connectivity)
    mask, exclude, N, H, W = _check_objects_masks(mask, exclude, 'find_objects')
    dev = mask.device
    if flow is not None:
        if not isinstance(flow, torch.Tensor) or tuple(flow.shape) != (N, H, W, 2) or flow.device != dev:
            raise ValueError(f'find_objects: a mask {(N, H, W)} on {dev} needs a flow {(N, H, W, 2)}, got '
                             f'{tuple(flow.shape) if hasattr(flow, "shape") else type(flow)}')
        _check_flow(flow, 'find_objects')
        flow = flow if type(flow) is torch.Tensor else flow.as_subclass(torch.Tensor)
    labels = torch.empty((N, H, W), device=dev, dtype=torch.int32) if want_labels else None
    count = torch.empty((N,), device=dev, dtype=torch.int32)
    area = torch.empty((N, K), device=dev, dtype=torch.int32)
    boxes = torch.empty((N, K, 4), device=dev, dtype=torch.int32)
    centroid = torch.empty((N, K, 2), device=dev, dtype=torch.float32)
    mean_flow = torch.empty((N, K, 2), device=dev, dtype=torch.float32) if flow is not None else None
    nbytes = components_workspace_bytes(N, H, W, conn, a)
    ptr = lambda t: None if t is None else _dev.ptr(t)       # noqa: E731
    with torch.cuda.device(dev):
        ws = _objects_workspace(workspace, dev, nbytes)
        check(_dev.lib().raft_find_objects(_dev.ptr(mask), ptr(exclude), ptr(flow), ptr(labels), _dev.ptr(count), _dev.ptr(area),
                                           _dev.ptr(boxes), _dev.ptr(centroid), ptr(mean_flow), N, H, W, conn, a, K, _dev.ptr(ws),
                                           _dev.stream_ptr()), 'find_objects')
    return Objects(labels, count, area, boxes, centroid, mean_flow)


def remove_small_components_launch(mask: torch.Tensor, min_area: int, connectivity: int = OBJECTS_CONNECTIVITY, exclude=None, out=None,
                                   workspace=None):
    """The launches themselves (``raft_remove_small_components``): a contiguous uint8 device ``mask``
    ``(N, H, W)`` and an optional ``exclude`` -> the uint8 mask ``(N, H, W)`` (a plain tensor) that is 1 where the pixel is
    foreground and its component has at least ``min_area`` pixels.  ``out=mask`` cleans in place.  One memset and four launches on
    the CURRENT stream."""
    _, a, conn = check_objects_args(1, min_area, connectivity)
    mask, exclude, N, H, W = _check_objects_masks(mask, exclude, 'remove_small_components')
    out = _check_out(out, (N, H, W), torch.uint8, mask.device)
    nbytes = components_workspace_bytes(N, H, W, conn, a)
    with torch.cuda.device(mask.device):
        ws = _objects_workspace(workspace, mask.device, nbytes)
        check(_dev.lib().raft_remove_small_components(_dev.ptr(mask), _dev.ptr(exclude) if exclude is not None else None, _dev.ptr(out), N,
                                                      H, W, conn, a, _dev.ptr(ws), _dev.stream_ptr()), 'remove_small_components')
    return out


def _objects_ahead(mask, exclude, what):
    """Shape of a mask argument ``(..., H, W)`` with its leading axes folded, ``(shape, (N, H, W))``, checked ahead with ``exclude``."""
    shape, dtype = _shape_and_type(mask, what)
    if len(shape) < 2:
        raise ValueError(f'{what} expects a mask (..., H, W), got {shape}')
    if 0 in shape:
        raise ValueError(f'empty input {shape}')
    if dtype not in (torch.uint8, torch.bool):
        raise TypeError(f'a mask is uint8 or bool, got {dtype}')
    _mask_ahead(exclude, shape, what)
    N, H, W = int(np.prod(shape[:-2], dtype=np.int64)), shape[-2], shape[-1]
    _check_objects_sizes(N, H, W, what)
    return shape, (N, H, W)


def label_components(mask, exclude=None, connectivity=OBJECTS_CONNECTIVITY):
    """Connected-component labelling: a uint8 / bool mask ``(..., H, W)`` (NumPy or torch, host or device;
    nonzero = foreground) -> int32 labels of the same shape on the device: 0 for background, and for a foreground pixel ``1 +`` the
    smallest raster index ``y * W + x`` of its component -- a function of the mask alone.  ``exclude`` (same shape and kind):
    pixels where it is nonzero are background, so a ``moving`` mask and an ``occluded_forward`` mask go in as they are.
    ``connectivity`` 4 or 8; every ``(H, W)`` slice is labelled on its own."""
    _, _, conn = check_objects_args(1, 1, connectivity)
    shape, shape3 = _objects_ahead(mask, exclude, 'label_components')
    labels = label_components_launch(_mask_on_device(mask, shape3), _mask_on_device(exclude, shape3), conn)
    return _dev.wrap(labels.view(shape))


def find_objects(mask, max_objects, min_area=OBJECTS_MIN_AREA, connectivity=OBJECTS_CONNECTIVITY, exclude=None, flow=None,
                 return_labels=True):
    """The objects of a mask: a uint8 / bool mask ``(..., H, W)`` (NumPy or torch, host or device) ->
    ``Objects(labels, count, area, boxes, centroid, mean_flow)`` of device tensors with the mask's leading axes: per slice the up to
    ``K = max_objects`` (1 .. 1024) connected components of at least ``min_area`` pixels, LARGEST FIRST (of equal areas the one
    that starts earlier in raster order); the slots from ``count`` on hold area 0, box ``(0, 0, -1, -1)``, centroid ``(-1, -1)``
    and mean flow 0.  ``boxes`` are inclusive ``x0, y0, x1, y1``, ``centroid`` is ``(x, y)``; ``labels`` (``return_labels``) holds
    ``slot + 1`` on the pixels of a chosen component and 0 elsewhere.  With a float32 ``flow`` ``(..., H, W, 2)``, ``mean_flow`` is
    the mean vector over the object's pixels, quantised to 1/256 pixel per vector (vectors that are not finite or longer than 2^20
    per component are left out); without one it is None.  ``exclude``: as in ``label_components``.  ``min_area=64`` and
    ``connectivity=8`` are choices, not tuned values.  Integer sums throughout: the result equals its NumPy restatement bit for bit
    and repeats bit for bit."""
    K, a, conn = check_objects_args(max_objects, min_area, connectivity)
    shape, shape3 = _objects_ahead(mask, exclude, 'find_objects')
    if flow is not None:
        _flow_ahead(flow, shape, 'find_objects')
    f = None if flow is None else _on_device(flow).reshape(shape3 + (2,))
    res = find_objects_launch(_mask_on_device(mask, shape3), K, a, conn, _mask_on_device(exclude, shape3), f, bool(return_labels))
    lead = shape[:-2]
    return Objects(*(None if t is None else _dev.wrap(t.view(lead + tuple(t.shape[1:]))) for t in res))


def remove_small_components(mask, min_area, connectivity=OBJECTS_CONNECTIVITY, exclude=None):
    """A mask without its specks: a uint8 / bool mask ``(..., H, W)`` (NumPy or torch, host or device) -> the
    uint8 device mask of the same shape that is 1 where the pixel is foreground and its connected component has at least
    ``min_area`` pixels, else 0.  ``exclude`` and ``connectivity``: as in ``label_components``."""
    _, a, conn = check_objects_args(1, min_area, connectivity)
    shape, shape3 = _objects_ahead(mask, exclude, 'remove_small_components')
    out = remove_small_components_launch(_mask_on_device(mask, shape3), a, conn, _mask_on_device(exclude, shape3))
    return _dev.wrap(out.view(shape))


# ------------------------------------------------------------------------------------------ object identity
OBJECT_TRACK_MAX = _ffi._CONSTANTS['RAFT_TRACK_OBJECTS_MAX']
OBJECT_MIN_OVERLAP = 0.25                                             # a choice, not a tuned value


class ObjectMatch(NamedTuple):
    """What ``match_objects`` returns, per slot ``b`` of the NEXT side, ``(..., K)`` int32: ``match`` the previous slot it took
    (-1: none), ``overlap`` the pixels of that previous object that landed on it (0 where unmatched), ``origin`` the previous slot
    most of whose pixels landed on it whatever the threshold and whoever was matched (-1: nothing landed on it)."""
    match: object
    overlap: object
    origin: object


def check_object_track_args(max_objects=1, min_overlap=OBJECT_MIN_OVERLAP):
    """``(max_objects, min_overlap)`` of an object matching: an integer (no bool) in 1 .. ``OBJECT_TRACK_MAX`` and a number whose
    float32 value lies in (0, 1]."""
    K = _int_in(max_objects, 'max_objects', 1, OBJECT_TRACK_MAX)
    s = _float32_value(min_overlap, 'min_overlap')
    if not 0.0 < s <= 1.0:
        raise ValueError(f'min_overlap must lie in (0, 1] as a float32, got {min_overlap!r}')
    return K, s


def _int32_table(t, shape, device, what):
    if (not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != torch.int32 or t.device != device
            or not t.is_contiguous()):
        raise ValueError(f'{what} must be a contiguous int32 tensor of shape {tuple(shape)} on {device}, got '
                         f'{(tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t)}')
    return t if type(t) is torch.Tensor else t.as_subclass(torch.Tensor)


def object_overlap_launch(labels_prev: torch.Tensor, flow: torch.Tensor, labels_next: torch.Tensor, K: int):
    """The launch itself (``raft_object_overlap``): contiguous int32 device label maps ``(M, H, W)`` of two
    consecutive ``find_objects`` results (slot + 1, 0 = background) and the contiguous float32 ``flow`` ``(M, H, W, 2)`` from the
    frame of the first into the frame of the second -> ``(overlap (M, K, K), landed (M, K))`` int32 on the CURRENT stream:
    ``landed[m, a]`` counts the pixels of previous slot ``a`` whose vector is finite and lands, rounded to the nearest pixel (ties
    to even), inside the frame, ``overlap[m, a, b]`` those of them that land on next slot ``b``.  Two memsets and one launch."""
    K, _ = check_object_track_args(K)
    if not isinstance(labels_prev, torch.Tensor) or labels_prev.dim() != 3 or 0 in labels_prev.shape:
        raise ValueError(f'object_overlap: expected int32 labels (M, H, W), got '
                         f'{tuple(labels_prev.shape) if hasattr(labels_prev, "shape") else type(labels_prev)}')
    M, H, W = labels_prev.shape
    dev = labels_prev.device
    _check_objects_sizes(M, H, W, 'object_overlap')
    labels_prev = _int32_table(labels_prev, (M, H, W), dev, 'labels_prev')
    labels_next = _int32_table(labels_next, (M, H, W), dev, 'labels_next')
    if not isinstance(flow, torch.Tensor) or tuple(flow.shape) != (M, H, W, 2) or flow.device != dev:
        raise ValueError(f'object_overlap: labels {(M, H, W)} on {dev} need a flow {(M, H, W, 2)}, got '
                         f'{tuple(flow.shape) if hasattr(flow, "shape") else type(flow)}')
    _check_flow(flow, 'object_overlap')
    flow = flow if type(flow) is torch.Tensor else flow.as_subclass(torch.Tensor)
    overlap = torch.empty((M, K, K), device=dev, dtype=torch.int32)
    landed = torch.empty((M, K), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        check(_dev.lib().raft_object_overlap(_dev.ptr(labels_prev), _dev.ptr(flow), _dev.ptr(labels_next), _dev.ptr(overlap),
                                             _dev.ptr(landed), M, H, W, K, _dev.stream_ptr()), 'object_overlap')
    return overlap, landed


def match_objects_launch(overlap: torch.Tensor, landed: torch.Tensor, area_next: torch.Tensor, min_overlap: float = OBJECT_MIN_OVERLAP,
                         want_overlap: bool = True, want_origin: bool = True):
    """The launch itself (``raft_match_objects``): ``overlap`` ``(M, K, K)`` and ``landed`` ``(M, K)`` of
    ``object_overlap_launch`` and the next side's ``area`` ``(M, K)``, contiguous int32 device tensors -> ``ObjectMatch`` of
    ``(M, K)`` int32 tensors on the CURRENT stream.  A pair is admissible iff its count is at least ``min_overlap`` times the
    smaller of ``landed[a]`` and ``area_next[b]`` (and at least 1); the admissible pairs are taken greedily, most pixels first (of
    equal counts the smaller previous slot, then the smaller next slot), each slot once.  One launch, one workgroup per image."""
    if not isinstance(overlap, torch.Tensor) or overlap.dim() != 3 or overlap.shape[1] != overlap.shape[2] or 0 in overlap.shape:
        raise ValueError(f'match_objects: expected an int32 overlap table (M, K, K), got '
                         f'{tuple(overlap.shape) if hasattr(overlap, "shape") else type(overlap)}')
    M, K, _ = overlap.shape
    K, share = check_object_track_args(K, min_overlap)
    dev = overlap.device
    overlap = _int32_table(overlap, (M, K, K), dev, 'overlap')
    landed = _int32_table(landed, (M, K), dev, 'landed')
    area_next = _int32_table(area_next, (M, K), dev, 'area_next')
    match = torch.empty((M, K), device=dev, dtype=torch.int32)
    count = torch.empty((M, K), device=dev, dtype=torch.int32) if want_overlap else None
    origin = torch.empty((M, K), device=dev, dtype=torch.int32) if want_origin else None
    ptr = lambda t: None if t is None else _dev.ptr(t)       # noqa: E731
    with torch.cuda.device(dev):
        check(_dev.lib().raft_match_objects(_dev.ptr(overlap), _dev.ptr(landed), _dev.ptr(area_next), share, _dev.ptr(match), ptr(count),
                                            ptr(origin), M, K, _dev.stream_ptr()), 'match_objects')
    return ObjectMatch(match, count, origin)


def chain_object_ids_launch(match: torch.Tensor, count: torch.Tensor, t0: int, ids: torch.Tensor, born: torch.Tensor,
                            next_id: torch.Tensor, out=None):
    """The launch itself (``raft_chain_object_ids``): ``match`` ``(S, N, K)`` and ``count`` ``(S, N)`` of ``S``
    consecutive steps of ``N`` videos, the state before them ``ids``, ``born`` ``(N, K)`` and ``next_id`` ``(N,)``, all contiguous
    int32 device tensors, and the index ``t0`` of the first step -> ``(ids, born)`` ``(S, N, K)`` after every step (``out``: a pair
    to write them into; with ``S == 1``, ``out=(ids[None], born[None])`` updates the state in place).  A matched slot inherits the
    id and birth step of the previous slot it took; an unmatched filled slot takes the next id of its video, in ascending slot
    order, and is born at ``t0 + s``; an empty slot holds -1 / -1.  ``next_id`` is updated in place.  One launch on the CURRENT
    stream, one workgroup per video."""
    t0 = check_track_time(t0)
    if not isinstance(match, torch.Tensor) or match.dim() != 3 or 0 in match.shape:
        raise ValueError(f'chain_object_ids: expected int32 matches (S, N, K), got '
                         f'{tuple(match.shape) if hasattr(match, "shape") else type(match)}')
    S, N, K = match.shape
    check_object_track_args(K)
    if S * N * K >= 1 << 31 or t0 + S >= 1 << 31:
        raise ValueError(f'chain_object_ids takes fewer than 2^31 slots in all, got {S} x {N} x {K}: too large')
    dev = match.device
    match = _int32_table(match, (S, N, K), dev, 'match')
    count = _int32_table(count, (S, N), dev, 'count')
    ids = _int32_table(ids, (N, K), dev, 'ids')
    born = _int32_table(born, (N, K), dev, 'born')
    next_id = _int32_table(next_id, (N,), dev, 'next_id')
    if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
        raise ValueError('out must be a pair (ids (S, N, K), born (S, N, K))')
    ids_out = _check_out(None if out is None else out[0], (S, N, K), torch.int32, dev)
    born_out = _check_out(None if out is None else out[1], (S, N, K), torch.int32, dev)
    with torch.cuda.device(dev):
        check(_dev.lib().raft_chain_object_ids(_dev.ptr(match), _dev.ptr(count), t0, _dev.ptr(ids), _dev.ptr(born), _dev.ptr(next_id),
                                               _dev.ptr(ids_out), _dev.ptr(born_out), S, N, K, _dev.stream_ptr()), 'chain_object_ids')
    return ids_out, born_out


def _int32_ahead(x, what):
    """Shape of an int32 argument (NumPy or torch), read without touching a device."""
    if not isinstance(x, torch.Tensor):
        x = x if isinstance(x, np.ndarray) else np.asarray(x)
    if x.dtype not in (torch.int32, np.dtype(np.int32)):
        raise TypeError(f'{what} is int32, got {x.dtype}')
    return tuple(x.shape)


def match_objects(prev, flow, next, min_overlap=OBJECT_MIN_OVERLAP):       # noqa: A002
    """Which object of one frame pair is which object of the next: ``prev`` and ``next`` are the ``Objects``
    of two consecutive ``find_objects`` calls (``prev`` needs ``labels`` ``(..., H, W)``, ``next`` ``labels`` and ``area`` ``(..., K)``,
    all int32), NumPy or torch, host or device, and ``flow`` ``(..., H, W, 2)`` float32 leads from the frame of
    ``prev.labels`` into the frame of ``next.labels`` -> ``ObjectMatch(match, overlap, origin)`` of ``(..., K)`` int32 device
    tensors, ``K = next.area.shape[-1]`` (at most 128; labels above ``K`` count as background).  Every pixel of a previous object
    is carried along its vector to the nearest pixel (vectors that are not finite or leave the frame drop out); a pair of slots is
    admissible iff the pixels of ``a`` that landed on ``b`` are at least ``min_overlap`` times the smaller of ``a``'s landed pixels
    and ``b``'s area; admissible pairs are taken greedily, most pixels first, each slot once.  ``min_overlap=0.25``, the nearest
    pixel and the greedy one-to-one rule are choices, not tuned values.  Integer sums throughout: the result equals its NumPy
    restatement bit for bit and repeats bit for bit."""
    if getattr(prev, 'labels', None) is None or getattr(next, 'labels', None) is None or getattr(next, 'area', None) is None:
        raise ValueError('match_objects needs prev.labels, next.labels and next.area: call find_objects with return_labels=True')
    shape = _int32_ahead(prev.labels, 'prev.labels')
    if len(shape) < 2 or 0 in shape:
        raise ValueError(f'match_objects expects labels (..., H, W), got {shape}')
    if _int32_ahead(next.labels, 'next.labels') != shape:
        raise ValueError(f'match_objects expects next.labels {shape}, got {_int32_ahead(next.labels, "next.labels")}')
    lead = shape[:-2]
    area_shape = _int32_ahead(next.area, 'next.area')
    if len(area_shape) != len(lead) + 1 or area_shape[:-1] != lead or area_shape[-1] < 1:
        raise ValueError(f'match_objects expects next.area {lead + ("K",)}, got {area_shape}')
    K, share = check_object_track_args(area_shape[-1], min_overlap)
    _flow_ahead(flow, shape, 'match_objects')
    M, H, W = int(np.prod(lead, dtype=np.int64)), shape[-2], shape[-1]
    _check_objects_sizes(M, H, W, 'match_objects')
    overlap, landed = object_overlap_launch(_on_device(prev.labels).reshape(M, H, W), _on_device(flow).reshape(M, H, W, 2),
                                            _on_device(next.labels).reshape(M, H, W), K)
    res = match_objects_launch(overlap, landed, _on_device(next.area).reshape(M, K), share)
    return ObjectMatch(*(_dev.wrap(t.view(lead + (K,))) for t in res))


# ------------------------------------------------------------------------------------------ temporal fusion
FUSE_SIGMA, FUSE_PATCH_RADIUS, FUSE_CENTER_WEIGHT = 10.0, 1, 1.0      # choices, not tuned values
FUSE_MAX_NEIGHBOURS, FUSE_MAX_PATCH_RADIUS, FUSE_MAX_CHANNELS = 16, 3, 4      # csrc/frame_fuse.hip
FUSE_MAX_PIXELS = 1 << 26                                             # N * H * W of one call


def check_fuse_args(sigma=FUSE_SIGMA, patch_radius=FUSE_PATCH_RADIUS, center_weight=FUSE_CENTER_WEIGHT):
    """``(sigma, patch_radius, center_weight)`` of a fusion as two floats around an int: numbers (no bool) whose float32 values
    are positive and finite (``sigma * sigma`` too, in float32), and an integer radius in 0 .. 3."""
    vals = []
    for name, v in (('sigma', sigma), ('center_weight', center_weight)):
        f = _float32_value(v, name)
        if not (np.isfinite(f) and f > 0.0):
            raise ValueError(f'{name} must be positive and finite as a float32, got {v!r}')
        vals.append(f)
    with np.errstate(over='ignore', under='ignore'):
        s2 = float(np.float32(vals[0]) * np.float32(vals[0]))
    if not (np.isfinite(s2) and s2 > 0.0):
        raise ValueError(f'sigma * sigma must be positive and finite as a float32, got sigma = {sigma!r}')
    if isinstance(patch_radius, (bool, np.bool_)) or not isinstance(patch_radius, (int, np.integer)) or \
            not 0 <= patch_radius <= FUSE_MAX_PATCH_RADIUS:
        raise ValueError(f'patch_radius must be an integer in 0 .. {FUSE_MAX_PATCH_RADIUS}, got {patch_radius!r}')
    return vals[0], int(patch_radius), vals[1]


def _check_fuse_sizes(K, N, H, W, C, what):
    if not 1 <= K <= FUSE_MAX_NEIGHBOURS:
        raise ValueError(f'{what} takes 1 to {FUSE_MAX_NEIGHBOURS} neighbours, got {K}')
    if not 1 <= C <= FUSE_MAX_CHANNELS:
        raise ValueError(f'{what} takes frames of 1 to {FUSE_MAX_CHANNELS} channels, got {C}')
    if N * H * W > FUSE_MAX_PIXELS:
        raise ValueError(f'{what} takes up to 2^26 pixels in a frame batch, got {N} x {H} x {W}: too large')


def _fuse_entry(in_dtype, dtype):
    """The entry's name and the result's type for frames of ``in_dtype`` and the result type asked for (None: the frames')."""
    if in_dtype not in (torch.uint8, torch.float32):
        raise TypeError(f'fuse_frames takes uint8 or float32 frames, got {in_dtype}')
    if dtype is None:
        dtype = in_dtype
    if dtype == torch.float32:
        return ('raft_fuse_frames_f32' if in_dtype == torch.float32 else 'raft_fuse_frames_u8_f32'), torch.float32
    if dtype == torch.uint8 and in_dtype == torch.uint8:
        return 'raft_fuse_frames_u8', torch.uint8
    raise TypeError(f'fuse_frames returns float32, or uint8 for uint8 frames, got {in_dtype} -> {dtype}')


def _check_fuse_index(index, M):
    """``index`` of a fusion (None: every block of the stack in order) as a list of ints in ``0 .. M - 1``; repeats are allowed."""
    if index is None:
        return list(range(M))
    if isinstance(index, (str, bytes)) or not hasattr(index, '__iter__'):
        raise ValueError(f'index must be a sequence of integers, got {index!r}')
    out = []
    for i in (index.tolist() if isinstance(index, np.ndarray) else index):
        if isinstance(i, (bool, np.bool_)) or not isinstance(i, (int, np.integer)) or not 0 <= i < M:
            raise ValueError(f'index holds integers in 0 .. {M - 1} (blocks of the stack), got {i!r}')
        out.append(int(i))
    return out


def fuse_frames_launch(center: torch.Tensor, stack: torch.Tensor, vectors: torch.Tensor, index=None, skip=None,
                       absolute: bool = False, sigma: float = FUSE_SIGMA, patch_radius: int = FUSE_PATCH_RADIUS,
                       center_weight: float = FUSE_CENTER_WEIGHT, want_weight: bool = False, dtype=None, out=None, weight=None):
    """The launch itself (``raft_fuse_frames_*``): a contiguous device centre ``(N, H, W, C)`` of uint8 /
    float32, a contiguous ``stack`` ``(M, N, H, W, C)`` of the same type on the same device and ``index``, a sequence of K block
    numbers of the stack (None: all M in order; repeats allowed) -- so ``video.view(T, 1, H, W, C)`` with the indices of a
    frame's neighbours fuses a window where it lies --, contiguous float32 ``vectors`` ``(K, N, H, W, 2)`` (flows centre ->
    neighbour k, or with ``absolute`` the sample positions themselves, e.g. ``track_launch``'s) and an optional contiguous uint8
    ``skip`` ``(K, N, H, W)`` (nonzero = not used) -> ``(fused, weight)`` by ONE launch on the CURRENT stream (plain tensors):
    ``(N, H, W, C)`` of ``dtype`` (None: the frames' type; float32, or uint8 for uint8 frames; ``out`` when given) and float32
    ``(N, H, W)`` (None without ``want_weight``; ``weight``: a tensor to write it into).  The outputs may overlap no input."""
    sigma, patch_radius, center_weight = check_fuse_args(sigma, patch_radius, center_weight)
    if center.dim() != 4 or 0 in center.shape or not center.is_contiguous():
        raise ValueError(f'fuse_frames: expected a contiguous centre (N, H, W, C), got {tuple(center.shape)}')
    name, out_dtype = _fuse_entry(center.dtype, dtype)
    N, H, W, Cn = center.shape
    if (stack.dim() != 5 or tuple(stack.shape[1:]) != (N, H, W, Cn) or stack.shape[0] < 1 or stack.dtype != center.dtype
            or stack.device != center.device or not stack.is_contiguous()):
        raise ValueError(f'a centre {tuple(center.shape)} {center.dtype} on {center.device} needs a contiguous stack (M, {N}, {H}, {W}, '
                         f'{Cn}) of its type, got {tuple(stack.shape)} {stack.dtype} on {stack.device}')
    index = _check_fuse_index(index, stack.shape[0])
    K = len(index)
    _check_fuse_sizes(K, N, H, W, Cn, 'fuse_frames')
    if tuple(vectors.shape) != (K, N, H, W, 2) or vectors.device != center.device:
        raise ValueError(f'{K} neighbours of {tuple(center.shape)} need vectors {(K, N, H, W, 2)}, got {tuple(vectors.shape)} on {vectors.device}')
    _check_flow(vectors, 'fuse_frames')
    if skip is not None:
        skip = _check_out(skip, (K, N, H, W), torch.uint8, center.device)
    out = _check_out(out, (N, H, W, Cn), out_dtype, center.device)
    weight = _check_out(weight, (N, H, W), torch.float32, center.device, alloc=bool(want_weight))
    with torch.cuda.device(center.device):
        check(getattr(_dev.lib(), name)(_dev.ptr(center), _dev.ptr(stack), (ctypes.c_int64 * K)(*index), _dev.ptr(vectors),
                                        _dev.ptr(skip) if skip is not None else None, 1 if absolute else 0, sigma, center_weight,
                                        patch_radius, _dev.ptr(out), _dev.ptr(weight) if weight is not None else None, K, N, H, W, Cn,
                                        _dev.stream_ptr()), 'fuse_frames')
    return out, weight


def _stacked(neighbours):
    """A list / tuple of K frame batches as one array ``(K, ...)`` (anything else is returned as it is)."""
    if isinstance(neighbours, (list, tuple)) and neighbours and all(hasattr(a, 'shape') for a in neighbours):
        if all(isinstance(a, torch.Tensor) for a in neighbours):
            return torch.stack(list(neighbours), dim=0)
        return np.stack([a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in neighbours], axis=0)
    return neighbours


def _fuse_ahead(center, neighbours, vectors, skip, what):
    """Shapes and types of a fusion's arrays, checked before anything reaches a device: ``(frame shape, frame type, K)``."""
    shape, in_dtype = _frames_ahead(center, what)
    nshape, ndtype = _shape_and_type(neighbours, what)
    if len(nshape) != len(shape) + 1 or nshape[1:] != shape or ndtype != in_dtype:
        raise ValueError(f'{what} expects neighbours (K,) + {shape} of the centre\'s type {in_dtype}, got {nshape} {ndtype}')
    K = nshape[0]
    shape4 = ((1,) + shape) if len(shape) == 3 else shape
    _check_fuse_sizes(K, shape4[0], shape4[1], shape4[2], shape4[3], what)
    _flow_ahead(vectors, (K,) + shape[:-1], what)
    _mask_ahead(skip, (K,) + shape[:-1], what)
    return shape, in_dtype, K


def fuse_frames(center, neighbours, flows=None, positions=None, skip=None, sigma=FUSE_SIGMA, patch_radius=FUSE_PATCH_RADIUS,
                center_weight=FUSE_CENTER_WEIGHT, return_weight=False, dtype=None):
    """Motion-compensated temporal filtering: a centre frame ``(H, W, C)`` or ``(N, H, W, C)`` (NumPy or
    torch, host or device, uint8, or float32 on 0 .. 255; float64 narrows; 1 to 4 channels) fused with ``neighbours`` ``(K, ...)``
    of the same shape and type (an array, or a list of K frames; K in 1 .. 16) -> a contiguous device tensor of the centre's shape,
    uint8 for uint8 frames unless ``dtype=torch.float32``, float32 otherwise.  Exactly one of ``flows`` (``(K, ..., H, W, 2)``
    float32: the flow centre -> neighbour k, as ``predict_step_bidirectional`` gives it for the pair (centre, neighbour k)) and
    ``positions`` (the same shape: where every pixel of the centre lies in neighbour k, as ``track`` gives it for
    ``point_grid(H, W)``) says where to sample.  Every neighbour is sampled bilinearly there (``warp``'s rule) and averaged with
    the centre under the weight ``sigma^2 / (sigma^2 + m)``, ``m`` the mean squared difference to the centre per channel over the
    ``(2 * patch_radius + 1)^2`` window of pixels that see the neighbour; the centre weighs ``center_weight``.  A neighbour is not
    used at a pixel whose sample leaves the frame, is NaN, or where ``skip`` (uint8 / bool ``(K, ..., H, W)``: an ``occluded_*``
    mask, ``track``'s ``lost``) is nonzero.  ``return_weight=True`` also returns the sum of the weights, float32 ``(..., H, W)``
    (``center_weight`` where nothing was used).  ``sigma`` is on the 0 .. 255 scale; it, ``patch_radius`` and ``center_weight``
    are choices, not tuned values.  ONE launch; float32 in a fixed order without transcendental functions, so the result equals
    its NumPy restatement and repeats bit for bit."""
    check_fuse_args(sigma, patch_radius, center_weight)
    if (flows is None) == (positions is None):
        raise ValueError('fuse_frames takes exactly one of flows and positions')
    neighbours = _stacked(neighbours)
    vectors = flows if flows is not None else positions
    shape, in_dtype, K = _fuse_ahead(center, neighbours, vectors, skip, 'fuse_frames')
    _fuse_entry(in_dtype, dtype)
    shape4 = ((1,) + shape) if len(shape) == 3 else shape
    c = _on_device(center).reshape(shape4)
    stack = _on_device(neighbours).reshape((K,) + shape4)
    v = _on_device(vectors).reshape((K,) + shape4[:3] + (2,))
    s = _mask_on_device(skip, (K,) + shape4[:3])
    out, weight = fuse_frames_launch(c, stack, v, None, s, positions is not None, sigma, patch_radius, center_weight, return_weight, dtype)
    out = _dev.wrap(out.view(shape))
    return (out, _dev.wrap(weight.view(shape[:-1]))) if return_weight else out


# ------------------------------------------------------------------------------------------ the camera's motion
MOTION_MODELS = ('translation', 'similarity', 'affine')      # the C entry's model 0, 1, 2
MOTION_ITERATIONS, MOTION_SCALE = 5, 1.0                     # choices, not tuned values
MOTION_MAX_ITERATIONS = 32                                   # include/raft_hip.h raft_flow_fit_motion_f32
MOTION_MAX_SLICES = 65535                                    # csrc/flow_motion.hip kMotionMaxSlices


def _float32_value(v, name):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f'{name} must be a number, got {v!r}')
    try:
        with np.errstate(over='ignore'):
            return float(np.float32(v))
    except OverflowError:
        return float('inf')


def check_motion_args(model='affine', iterations=MOTION_ITERATIONS, scale=MOTION_SCALE):
    """``(model index, iterations, scale)`` of a motion fit: ``model`` one of ``MOTION_MODELS``, ``iterations`` an integer (no
    bool) in 1 .. 32, ``scale`` a number whose float32 value is positive and finite (pixels)."""
    if not isinstance(model, str) or model not in MOTION_MODELS:
        raise ValueError(f"model must be 'translation', 'similarity' or 'affine', got {model!r}")
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or not 1 <= iterations <= MOTION_MAX_ITERATIONS:
        raise ValueError(f'iterations must be an integer in 1 .. {MOTION_MAX_ITERATIONS}, got {iterations!r}')
    s = _float32_value(scale, 'scale')
    if not (s > 0.0 and np.isfinite(s)):
        raise ValueError(f'scale must be positive and finite as a float32, got {scale!r}')
    return MOTION_MODELS.index(model), int(iterations), s


def check_motion_threshold(threshold):
    """``threshold`` of ``residual_flow`` as a float, or None: a number (no bool) whose float32 value is finite and >= 0."""
    if threshold is None:
        return None
    t = _float32_value(threshold, 'threshold')
    if not (t >= 0.0 and np.isfinite(t)):
        raise ValueError(f'threshold must be finite and >= 0 as a float32, got {threshold!r}')
    return t


def _check_motion_sizes(N, H, W, fit, what):
    if N * H * W * 2 >= 1 << 31 or (fit and N > MOTION_MAX_SLICES):
        raise ValueError(f'{what} takes flows of fewer than 2^31 floats{" in at most 65535 slices" if fit else ""}, got {N} x {H} x {W}: '
                         'too large')


def _check_motion(motion, N, device, what):
    if (not isinstance(motion, torch.Tensor) or tuple(motion.shape) != (N, 2, 3) or motion.dtype != torch.float32 or motion.device != device
            or not motion.is_contiguous()):
        raise ValueError(f'{what}: motion must be a contiguous float32 tensor {(N, 2, 3)} on {device}')
    return motion if type(motion) is torch.Tensor else motion.as_subclass(torch.Tensor)


def fit_motion_launch(flow: torch.Tensor, mask=None, invert: bool = False, model: str = 'affine', iterations: int = MOTION_ITERATIONS,
                      scale: float = MOTION_SCALE):
    """The launches themselves (``raft_flow_fit_motion_f32``): a contiguous float32 device flow ``(N, H, W, 2)``
    and an optional contiguous uint8 ``mask`` ``(N, H, W)`` -- a pixel is used where it is nonzero, with ``invert=True`` where it
    is zero -> ``(motion (N, 2, 3), stats (N, 4))`` float32 on the CURRENT stream (plain tensors), ``2 * iterations + 2``
    launches enqueued by one call, nothing synchronised."""
    from . import losses
    model, iterations, scale = check_motion_args(model, iterations, scale)
    if flow.dim() != 4 or flow.shape[-1] != 2 or 0 in flow.shape:
        raise ValueError(f'expected a flow (N, H, W, 2), got {tuple(flow.shape)}')
    _check_flow(flow, 'fit_motion')
    N, H, W, _ = flow.shape
    _check_motion_sizes(N, H, W, True, 'fit_motion')
    if mask is not None:
        mask = _check_out(mask, (N, H, W), torch.uint8, flow.device)
    motion = torch.empty((N, 2, 3), device=flow.device, dtype=torch.float32)
    stats = torch.empty((N, 4), device=flow.device, dtype=torch.float32)
    lib = _dev.lib()
    with torch.cuda.device(flow.device):
        ws = losses._workspace(flow.device, 8 * int(lib.raft_flow_motion_workspace_doubles(N, H, W)))
        check(lib.raft_flow_fit_motion_f32(_dev.ptr(flow), _dev.ptr(mask) if mask is not None else None, int(bool(invert)), _dev.ptr(motion),
                                           _dev.ptr(stats), N, H, W, model, iterations, scale, _dev.ptr(ws), _dev.stream_ptr()),
              'fit_motion')
    return motion, stats


def residual_flow_launch(flow: torch.Tensor, motion: torch.Tensor, threshold=None, want_residual: bool = True):
    """The launch itself (``raft_flow_residual_f32``): a contiguous float32 device flow ``(N, H, W, 2)`` and the motions ``(N, 2, 3)``
    -> ``(residual (N, H, W, 2) float32, moving (N, H, W) uint8)`` on the CURRENT stream (plain tensors): the flow minus the
    motion's own, and 1 where what is left is longer than ``threshold`` (``moving`` is None without a threshold, ``residual`` with
    ``want_residual=False``)."""
    threshold = check_motion_threshold(threshold)
    if flow.dim() != 4 or flow.shape[-1] != 2 or 0 in flow.shape:
        raise ValueError(f'expected a flow (N, H, W, 2), got {tuple(flow.shape)}')
    _check_flow(flow, 'residual_flow')
    N, H, W, _ = flow.shape
    _check_motion_sizes(N, H, W, False, 'residual_flow')
    motion = _check_motion(motion, N, flow.device, 'residual_flow')
    if threshold is None and not want_residual:
        raise ValueError('residual_flow: nothing to compute without a threshold and without the residual')
    residual = torch.empty((N, H, W, 2), device=flow.device, dtype=torch.float32) if want_residual else None
    moving = torch.empty((N, H, W), device=flow.device, dtype=torch.uint8) if threshold is not None else None
    with torch.cuda.device(flow.device):
        check(_dev.lib().raft_flow_residual_f32(_dev.ptr(flow), _dev.ptr(motion), _dev.ptr(residual) if residual is not None else None,
                                                _dev.ptr(moving) if moving is not None else None, N, H, W,
                                                0.0 if threshold is None else threshold, _dev.stream_ptr()), 'residual_flow')
    return residual, moving


def motion_flow_launch(motion: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """The launch itself (``raft_motion_flow_f32``): contiguous float32 device motions ``(N, 2, 3)`` -> their dense flows
    ``(N, H, W, 2)`` float32 on the CURRENT stream (a plain tensor)."""
    H, W = _view_size((H, W))
    if not isinstance(motion, torch.Tensor) or motion.dim() != 3 or 0 in motion.shape:
        raise ValueError(f'expected motions (N, 2, 3), got {tuple(getattr(motion, "shape", ()))}')
    N = motion.shape[0]
    motion = _check_motion(motion, N, motion.device, 'motion_flow')
    _check_motion_sizes(N, H, W, False, 'motion_flow')
    flow = torch.empty((N, H, W, 2), device=motion.device, dtype=torch.float32)
    with torch.cuda.device(motion.device):
        check(_dev.lib().raft_motion_flow_f32(_dev.ptr(motion), _dev.ptr(flow), N, H, W, _dev.stream_ptr()), 'motion_flow')
    return flow


def _flow_lead(flow, what):
    """Shape of a flow argument ``(..., H, W, 2)`` with its leading axes folded: ``(shape, (N, H, W))``, checked ahead."""
    shape, dtype = _shape_and_type(flow, what)
    if len(shape) < 3 or shape[-1] != 2:
        raise ValueError(f'{what} expects a flow (..., H, W, 2), got {shape}')
    if 0 in shape:
        raise ValueError(f'empty input {shape}')
    if dtype != torch.float32:
        raise TypeError(f'a flow is float32, got {dtype}')
    return shape, (int(np.prod(shape[:-3], dtype=np.int64)),) + shape[-3:-1]


def _motion_ahead(motion, lead, what):
    shape, dtype = _shape_and_type(motion, what)
    if shape != tuple(lead) + (2, 3):
        raise ValueError(f'{what} expects motions {tuple(lead) + (2, 3)}, got {shape}')
    if dtype != torch.float32:
        raise TypeError(f'a motion is float32, got {dtype}')


def fit_motion(flow, mask=None, occluded=None, model='affine', iterations=MOTION_ITERATIONS, scale=MOTION_SCALE, return_stats=False):
    """What the camera did between two frames, from their flow: a float32 flow ``(..., H, W, 2)`` (NumPy or
    torch, host or device; float64 narrows) -> the motions ``(..., 2, 3)`` as a float32 device tensor, one per leading index: the
    map ``p2 = M (x, y, 1)`` from frame 1 to frame 2 in pixel coordinates whose own flow fits the given one best.  ``model``:
    ``'translation'``, ``'similarity'`` (rotation, uniform zoom, shift) or ``'affine'``.  ``mask`` (uint8 / bool ``(..., H, W)``):
    only pixels where it is nonzero are fitted; ``occluded``: the same with the other polarity, so the ``occluded_*`` masks of a
    bidirectional prediction go in as they are (one of the two at most).  Vectors that are not finite are left out.

    Iteratively reweighted least squares: the first of ``iterations`` solves is plain least squares, every later one weights a
    pixel ``1 / (1 + r^2 / scale^2)`` with ``r`` its residual under the solve before (Cauchy), so whatever moves on its own loses
    its say.  ``iterations=5`` and ``scale=1.0`` pixel are choices, not tuned values.  ``return_stats=True`` also returns
    ``(..., 4)`` float32: the share of used pixels, the inlier share (mean weight), the weighted RMS residual in pixels, and the
    status (0 fitted, 1 the vectors do not determine the model: translation only, 2 no pixel to fit: identity).  Float64 sums in a
    fixed order: the result repeats bit for bit and a slice does not depend on the rest of the batch."""
    check_motion_args(model, iterations, scale)
    shape, (N, H, W) = _flow_lead(flow, 'fit_motion')
    if mask is not None and occluded is not None:
        raise ValueError('fit_motion takes mask or occluded, not both')
    chosen = mask if mask is not None else occluded
    _mask_ahead(chosen, shape[:-1], 'fit_motion')
    _check_motion_sizes(N, H, W, True, 'fit_motion')
    f = _on_device(flow).reshape(N, H, W, 2)
    motion, stats = fit_motion_launch(f, _mask_on_device(chosen, (N, H, W)), occluded is not None, model, iterations, scale)
    motion = _dev.wrap(motion.view(shape[:-3] + (2, 3)))
    return (motion, _dev.wrap(stats.view(shape[:-3] + (4,)))) if return_stats else motion


def residual_flow(flow, motion, threshold=None):
    """The flow with the camera's motion taken away: a float32 flow ``(..., H, W, 2)`` and motions ``(..., 2, 3)`` (NumPy or torch,
    host or device) -> ``flow - motion_flow(motion, H, W)`` as a float32 device tensor of the flow's shape, formed in float64 and
    rounded once.  With a ``threshold`` (pixels, finite and >= 0) it returns ``(residual, moving)``, ``moving`` the uint8 mask
    ``(..., H, W)`` of the pixels whose residual is longer than the threshold or not finite: what moves on its own.  One launch."""
    threshold = check_motion_threshold(threshold)
    shape, (N, H, W) = _flow_lead(flow, 'residual_flow')
    _motion_ahead(motion, shape[:-3], 'residual_flow')
    _check_motion_sizes(N, H, W, False, 'residual_flow')
    f = _on_device(flow).reshape(N, H, W, 2)
    residual, moving = residual_flow_launch(f, _on_device(motion).reshape(N, 2, 3), threshold)
    residual = _dev.wrap(residual.view(shape))
    return residual if threshold is None else (residual, _dev.wrap(moving.view(shape[:-1])))


def motion_flow(motion, H, W):
    """The dense flow of motions ``(..., 2, 3)`` float32 (NumPy or torch, host or device) on an ``H x W`` frame: a float32 device
    tensor ``(..., H, W, 2)`` with ``M (x, y, 1) - (x, y)`` at pixel ``(y, x)``, formed in float64 and rounded once.  One launch."""
    H, W = _view_size((H, W))
    shape, dtype = _shape_and_type(motion, 'motion_flow')
    if len(shape) < 2 or shape[-2:] != (2, 3) or 0 in shape:
        raise ValueError(f'motion_flow expects motions (..., 2, 3), got {shape}')
    if dtype != torch.float32:
        raise TypeError(f'a motion is float32, got {dtype}')
    N = int(np.prod(shape[:-2], dtype=np.int64))
    _check_motion_sizes(N, H, W, False, 'motion_flow')
    return _dev.wrap(motion_flow_launch(_on_device(motion).reshape(N, 2, 3), H, W).view(shape[:-2] + (H, W, 2)))


class MotionViews:
    """Motions ``(N, 2, 3)`` (host, float64) as the views of ``view_host_records``: slice ``n`` is resampled at ``p = M q + o`` with
    ``M = motions[n, :, :2]`` and ``o = motions[n, :, 2]``, each number rounded to float32 once; no colour change."""

    def __init__(self, motions):
        m = np.asarray(motions, dtype=np.float64)
        if m.ndim != 3 or m.shape[1:] != (2, 3) or m.shape[0] < 1:
            raise ValueError(f'expected motions (N, 2, 3), got {m.shape}')
        self.motions = m

    def __len__(self):
        return self.motions.shape[0]

    def records(self, doubled=False):
        recs = (_ffi.ViewParams * (len(self) * (2 if doubled else 1)))()
        for b, r in enumerate(recs):
            m = self.motions[b % len(self)]
            # (a map without an inverse gets one that is not finite: view_host_records refuses the record)
            inv = np.linalg.inv(m[:, :2]) if np.isfinite(m).all() and np.linalg.det(m[:, :2]) != 0 else np.full((2, 2), np.nan)
            with np.errstate(over='ignore'):
                r.m[:], r.o[:], r.inv[:] = (a.astype(np.float32).tolist() for a in (m[:, :2].reshape(4), m[:, 2], inv.reshape(4)))
            r.gain[:], r.bias[:], r.colour = [1.0] * 3, [0.0] * 3, 0
        return recs


# ------------------------------------------------------------------------------------------ forward projection of a flow
def forward_interpolate_launch(t: torch.Tensor, out=None) -> torch.Tensor:
    """The launch itself: contiguous float32 device ``(B, h, w, 2)`` -> its forward projection, a new tensor of the same shape
    (``out`` when given; it must not overlap ``t``) on the CURRENT stream (plain ``torch.Tensor``)."""
    if t.dim() != 4 or t.shape[-1] != 2:
        raise ValueError(f'expected a flow (B, h, w, 2), got {tuple(t.shape)}')
    _check_flow(t, 'forward_interpolate')
    B, h, w, _ = t.shape
    out = _check_out(out, (B, h, w, 2), torch.float32, t.device)
    with torch.cuda.device(t.device):
        check(_dev.lib().raft_forward_interpolate_f32(_dev.ptr(t), B, h, w, _dev.ptr(out), _dev.stream_ptr()), 'forward_interpolate')
    return out


def forward_interpolate(flow) -> torch.Tensor:
    """A flow projected forward along itself (the authors' ``forward_interpolate``, the warm start of RAFT's video protocol;
    DESIGN.md section 16): ``(..., h, w, 2)`` float32 (NumPy or torch, host or device; float64 narrows) -> a contiguous float32
    device tensor of the same shape.  Per image, the vector at ``(x0, y0)`` travels to ``(x0 + u, y0 + v)``; every cell takes the
    vector of the nearest end point that lies strictly inside ``(0, w) x (0, h)``, ties to the first source in row-major order,
    zeros where an image has none.  Float32 throughout, bit for bit the rule in ``include/raft_hip.h``.  One launch on the current
    stream.  Meant for low-resolution flows: the search is exhaustive, ``(h * w)^2`` candidates per image."""
    shape = tuple(flow.shape) if hasattr(flow, 'shape') else np.shape(flow)
    dtype = flow.dtype if hasattr(flow, 'dtype') else np.asarray(flow).dtype
    if len(shape) < 3 or shape[-1] != 2:
        raise ValueError(f'forward_interpolate expects a flow (..., h, w, 2), got {shape}')
    if 0 in shape:
        raise ValueError(f'empty input {shape}')
    floats = (torch.float32, torch.float64) if isinstance(dtype, torch.dtype) else (np.dtype(np.float32), np.dtype(np.float64))
    if dtype not in floats:
        raise TypeError(f'a flow is float32, got {dtype}')
    t = _on_device(flow)
    return _dev.wrap(forward_interpolate_launch(t.reshape((-1,) + shape[-3:])).view(shape))


# ------------------------------------------------------------------------------------------ the student's view
def _view_size(size):
    try:
        Hs, Ws = size
    except (TypeError, ValueError) as exc:
        raise ValueError(f'size must be the pair (H, W), got {size!r}') from exc
    for v in (Hs, Ws):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f'size must be a pair of ints >= 1, got {size!r}')
    return int(Hs), int(Ws)


def view_host_records(views, slices: int) -> bytes:
    """The ``RaftViewParams`` records of ``slices`` slices as bytes, checked on the host: ``views`` is an ``augment.StudentView`` of
    N views -- ``slices == N`` gives every view with frame 1's colour, ``slices == 2N`` the doubled form of a training step, slices
    ``n`` and ``n + N`` carrying view ``n`` with frame 1's and frame 2's colour.  Every number of a record must be finite."""
    if not hasattr(views, 'records'):
        raise ValueError(f'views must be an augment.StudentView, got {views!r}')
    n = len(views)
    if slices not in (n, 2 * n):
        raise ValueError(f'{n} views serve {n} or {2 * n} slices, got {slices}')
    recs = views.records(doubled=slices == 2 * n)
    for b, r in enumerate(recs):
        vals = [*r.m, *r.o, *r.inv] + ([*r.gain, *r.bias] if r.colour else [])
        if not np.isfinite(np.array(vals, dtype=np.float64)).all():
            raise ValueError(f'view record {b} holds a number that is not finite: {vals}')
    return bytes(recs)


_VIEW_STAGING = None          # pinned host buffers of the records' uploads (augment._Staging), made on first use


def view_records(views, slices: int, device) -> torch.Tensor:
    """``view_host_records`` uploaded on the current stream: the uint8 device tensor the launch forms below take (one upload serves
    both).  The copy leaves from pinned memory and does not wait for what is queued, so the host of a training loop stays ahead."""
    global _VIEW_STAGING
    raw = view_host_records(views, int(slices))
    if _VIEW_STAGING is None:
        from .augment import _Staging
        _VIEW_STAGING = _Staging()
    with torch.cuda.device(device):
        return _VIEW_STAGING.upload(raw, device)


def _check_records(records, slices, device):
    if (not isinstance(records, torch.Tensor) or records.dtype != torch.uint8 or records.device != device or not records.is_contiguous()
            or records.numel() != slices * _ffi.C.sizeof(_ffi.ViewParams)):
        raise ValueError(f'records must be the uint8 tensor of view_records() for {slices} slices on {device}')


def view_frames_launch(t: torch.Tensor, records: torch.Tensor, size, out=None) -> torch.Tensor:
    """The launch itself (``raft_view_frames_f32``): contiguous float32 device frames ``(B, Ht, Wt, C)`` seen through the ``B``
    device records of ``view_records`` -> float32 ``(B, H, W, C)`` with ``size = (H, W)``, on the CURRENT stream (plain tensor)."""
    Hs, Ws = _view_size(size)
    if t.dim() != 4 or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f'view_frames takes contiguous float32 frames (B, Ht, Wt, C), got {t.dtype} {tuple(t.shape)}')
    B, Ht, Wt, Cn = t.shape
    _check_records(records, B, t.device)
    out = _check_out(out, (B, Hs, Ws, Cn), torch.float32, t.device)
    with torch.cuda.device(t.device):
        check(_dev.lib().raft_view_frames_f32(_dev.ptr(t), _dev.ptr(records), _dev.ptr(out), B, Ht, Wt, Hs, Ws, Cn, _dev.stream_ptr()),
              'view_frames')
    return out


def view_flow_launch(flow: torch.Tensor, records: torch.Tensor, size, visible=None):
    """The launch itself (``raft_view_flow_f32``): a contiguous float32 device flow ``(B, Ht, Wt, 2)`` and an optional contiguous
    uint8 trust mask ``(B, Ht, Wt)`` seen through the ``B`` device records -> ``(target (B, H, W, 2) float32, target_visible
    (B, H, W) uint8)`` on the CURRENT stream (plain tensors)."""
    Hs, Ws = _view_size(size)
    if flow.dim() != 4 or flow.shape[-1] != 2:
        raise ValueError(f'view_flow takes a flow (B, Ht, Wt, 2), got {tuple(flow.shape)}')
    _check_flow(flow, 'view_flow')
    B, Ht, Wt, _ = flow.shape
    _check_records(records, B, flow.device)
    if visible is not None:
        visible = _check_out(visible, (B, Ht, Wt), torch.uint8, flow.device)
    target = torch.empty((B, Hs, Ws, 2), device=flow.device, dtype=torch.float32)
    target_visible = torch.empty((B, Hs, Ws), device=flow.device, dtype=torch.uint8)
    with torch.cuda.device(flow.device):
        check(_dev.lib().raft_view_flow_f32(_dev.ptr(flow), _dev.ptr(visible) if visible is not None else None, _dev.ptr(records),
                                            _dev.ptr(target), _dev.ptr(target_visible), B, Ht, Wt, Hs, Ws, _dev.stream_ptr()), 'view_flow')
    return target, target_visible


def _shape_dtype(x):
    if isinstance(x, torch.Tensor):
        return tuple(x.shape), x.dtype
    x = np.asarray(x)
    return tuple(x.shape), x.dtype


def view_frames(images, views, size):
    """Frames ``(B, Ht, Wt, C)`` (NumPy or torch, host or device, float32; float64 narrows) cut out under the affine views
    ``views`` (an ``augment.StudentView`` of B views, or of B / 2: the doubled batch of a training step) -> a float32 device tensor ``(B, H, W, C)`` with ``size = (H, W)``: pixel ``(y, x)`` of slice ``b`` is the
    bilinear sample of the frame at ``M (x, y) + o``, 0 out of frame, then ``clip(v * gain + bias, 0, 255)`` where the view has a
    gain.  One launch on the current stream; shapes and records are checked before anything moves."""
    Hs, Ws = _view_size(size)
    shape, dtype = _shape_dtype(images)
    if len(shape) != 4 or 0 in shape:
        raise ValueError(f'view_frames expects (B, Ht, Wt, C), got {shape}')
    if str(dtype).replace('torch.', '') not in ('float32', 'float64'):
        raise TypeError(f'view_frames takes float32 frames, got {dtype}')
    view_host_records(views, shape[0])
    t = _on_device(images)
    recs = view_records(views, shape[0], t.device)
    return _dev.wrap(view_frames_launch(t, recs, (Hs, Ws)))


def view_flow(flow, views, size, visible=None):
    """A flow ``(B, Ht, Wt, 2)`` float32 and an optional trust mask ``visible`` ``(B, Ht, Wt)`` (nonzero = trusted) seen through
    the views (as for ``view_frames``) -> ``(target, target_visible)``: the float32 flow ``(B, H, W, 2)`` in the student's own
    coordinates, ``Minv f(M q + o)``, and the uint8 mask ``(B, H, W)`` that is 1 where the pixel is in frame, every tap of
    nonzero weight is trusted and the vector is finite; the target is (0, 0) elsewhere.  One launch on the current stream
    (DESIGN.md section 23); shapes and records are checked before anything moves."""
    from . import losses
    Hs, Ws = _view_size(size)
    shape, dtype = _shape_dtype(flow)
    if len(shape) != 4 or shape[-1] != 2 or 0 in shape:
        raise ValueError(f'view_flow expects a flow (B, Ht, Wt, 2), got {shape}')
    if str(dtype).replace('torch.', '') not in ('float32', 'float64'):
        raise TypeError(f'a flow is float32, got {dtype}')
    if visible is not None and _shape_dtype(visible)[0] != shape[:3]:
        raise ValueError(f'visible must be {shape[:3]}, got {_shape_dtype(visible)[0]}')
    view_host_records(views, shape[0])
    f = _on_device(flow)
    recs = view_records(views, shape[0], f.device)
    mask = losses._mask_to_device(visible, f.device) if visible is not None else None
    target, target_visible = view_flow_launch(f, recs, (Hs, Ws), mask)
    return _dev.wrap(target), _dev.wrap(target_visible)

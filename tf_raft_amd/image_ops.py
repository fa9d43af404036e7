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
"""
from __future__ import annotations

import numpy as np
import torch

from . import _dev
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
    shape = (N, int(target_height), int(target_width), Cn)
    if out is None:
        out = torch.empty(shape, device=t.device, dtype=out_dtype)
    elif tuple(out.shape) != shape or out.dtype != out_dtype or out.device != t.device or not out.is_contiguous():
        raise ValueError(f'out must be a contiguous {out_dtype} tensor of shape {shape} on {t.device}')
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
    t = _on_device(x)
    if t.dim() not in (3, 4):
        raise ValueError(f'expected (H, W, C) or (N, H, W, C), got {tuple(t.shape)}')
    if 0 in t.shape:
        raise ValueError(f'empty input {tuple(t.shape)}')
    if tuple(t.shape[-3:-1]) == (target_height, target_width):
        if dtype is not None and dtype != t.dtype:
            if not (t.dtype in (torch.uint8, torch.bool) and dtype == torch.float32):
                raise TypeError(f'resize_with_crop_or_pad takes uint8, bool or float32 (optionally uint8 -> float32), got {t.dtype} -> {dtype}')
            t = t.to(dtype)
        return _dev.wrap(t)
    out = window_copy(t if t.dim() == 4 else t[None], target_height, target_width, dtype)
    return _dev.wrap(out if t.dim() == 4 else out[0])

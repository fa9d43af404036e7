"""What the forward schedule of ``tf_raft_amd.model`` keeps between calls: the plan of one call's loop, the lanes that loops
run on and the ring of loop states that lets several of them be in flight."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _dev
from ._ffi import check
from .layers.update import UpdateState


class LoopPlan(NamedTuple):
    """How one forward call schedules its recurrent loop, fixed when the call starts and passed down to the launcher."""
    lane: int                   # whose flow / mask streams and raft_loop_ctx the loop uses
    three_stream: bool          # flow / mask branches on side streams; False = the single-stream schedule
    pre_hint: Optional[int]     # launch-shape hint of the encoders and volume build; None = the calling thread's own
    loop_hint: int              # launch-shape hint of the loop


class Lane:
    """Lane ``index`` of one model on ``device``: the streams a loop of this lane runs on and its caller-owned ``raft_loop_ctx``
    (the cross-stream events of the three-stream loops).  Loops of different lanes run concurrently; loops of one lane follow each
    other in stream order and share the context.  The streams are the process-wide side streams (``_dev.side_stream``: one set
    per device, hardware queues by creation order), asked for when first used."""

    def __init__(self, device, index: int):
        self.device, self.index, self._streams, self._ctx = device, index, {}, None

    def stream(self, role):
        """This lane's ``'loop'``, ``'flow'`` or ``'mask'`` stream."""
        s = self._streams.get(role)
        if s is None:
            s = self._streams[role] = _dev.side_stream(self.device, role if self.index == 0 else f'{role}{self.index}')
        return s

    def loop_args(self, plan: LoopPlan):
        """``(s0, s1, s2, ctx)`` of a loop launched now under ``plan``: the current stream and, on the three-stream schedule, this
        lane's flow and mask streams (events inside the library); otherwise the current stream three times = the single-stream
        schedule.  ``ctx`` is the lane's loop context, created at its first use."""
        s0 = _dev.stream_ptr()
        s1, s2 = (self.stream('flow').cuda_stream, self.stream('mask').cuda_stream) if plan.three_stream else (s0, s0)
        if self._ctx is None:
            handle = C.c_void_p()
            with torch.cuda.device(self.device):
                check(_dev.lib().raft_loop_ctx_create(C.byref(handle)), 'loop_ctx_create')
            self._ctx = handle
        return s0, s1, s2, self._ctx

    def close(self):
        """Destroy the loop context once every loop that uses its events has finished."""
        ctx, self._ctx = self._ctx, None
        if ctx is not None:
            try:
                torch.cuda.synchronize(self.device)
                _dev.lib().raft_loop_ctx_destroy(ctx)
            except Exception:   # noqa: BLE001  (interpreter shutdown)
                pass


class RingSlot:
    """One slot of the pipelined forward's ring: the ``UpdateState`` a loop reads and the done-event of the last loop that did."""

    def __init__(self):
        self.state, self.done = None, None

    def fit(self, variant, B, h, w, device) -> UpdateState:
        """The slot's state for a ``(B, h, w)`` call on ``device``, reallocated where either changed."""
        st = self.state
        if st is None or (st.B, st.h, st.w) != (B, h, w) or st.net.device != device:
            if self.done is not None:
                self.done.synchronize()                  # the old buffers are about to be freed: their last loop must be done
            self.state, self.done = UpdateState(variant, B, h, w, device), None
        return self.state

    def join(self):
        """Make the current stream wait for the last loop that read this slot."""
        if self.done is not None:
            torch.cuda.current_stream(self.state.net.device).wait_event(self.done)

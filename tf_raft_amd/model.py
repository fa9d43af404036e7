"""Device mirror of reference ``tf_raft/model.py`` -- ``RAFT`` / ``SmallRAFT`` forward prediction.

Same constructor and call signature as the reference (model.py:11, 68, 174, 190):

    model = RAFT(drop_rate=0, iters=12, iters_pred=24)
    flow_predictions = model([image1, image2], training=False)   # list of (bs, H, W, 2)

``image1/2`` are ``(bs, H, W, 3)`` float arrays in 0..255 (NumPy or torch, host or device);
the result is a Python list of ``iters_pred`` (``iters`` when ``training=True``) fp32 device
tensors, ``[-1]`` the finest, each answering ``.numpy()`` like a TF eager tensor.

Execution: everything runs on hand-written HIP kernels behind the C ABI (``include/raft_hip.h``): the two
encoders (``raft_encoder_f32``), the correlation volume build, and the whole recurrent loop
(lookup -> update block -> coords update -> upsampling) enqueued by ONE ``raft_iterate_*`` call (``RAFT._iterate``
picks which) with no host synchronisation.  There is no CPU fallback.  One body enqueues the forward pass for the serial
schedule (the caller's stream) and the pipelined one (loops of consecutive calls on lanes of their own, results joined lazily):
section "the forward schedule" below; what it keeps between calls is in ``tf_raft_amd.schedule``.

Callers of the forward pass (reference model.py:111-170): ``compile``, ``test_step`` (EPE / u1 / u3 / u5 of the final
prediction against ground truth, reduced on the device: ``tf_raft_amd.losses``), ``predict_step``, ``reset_metrics``,
``load_weights`` / ``save_weights`` (TensorFlow tensor-bundle checkpoints, read and written without TensorFlow) are
provided.  ``train_step`` (model.py:126-144) is functional for RAFT: training-mode forward, backward, global-norm clipping
and AdamW on HIP kernels (``tf_raft_amd.grad`` / ``tf_raft_amd.training``), orchestrated from Python -- not yet a tuned
path.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import itertools
import os
from collections import OrderedDict
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import _dev
from . import image_ops
from . import weights as weights_mod
from . import _ffi
from ._ffi import check
from .layers.corr import CorrBlock, coords_grid, upflow8
from .layers.extractor import BasicEncoder, SmallEncoder
from .layers.update import BasicUpdateBlock, SmallUpdateBlock, UpdateState
from .schedule import Lane, LoopPlan, RingSlot


def _rank_of_this_process() -> int:
    """Data-parallel rank (0 without torch.distributed)."""
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _dropout_seed(model_seed: int, rank: int, step: int) -> int:
    """Even 62-bit seed of a training step's two dropout masks (the second uses seed + 1): a splitmix64-style mix of the
    model seed, the data-parallel rank and the step, so that ranks, models and steps draw independent masks."""
    x = (int(model_seed) * 0x9E3779B97F4A7C15 + int(rank) * 0xBF58476D1CE4E5B9 + int(step) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 31
    return int(x >> 2) & ~1


DEFAULT_LANES = 3          # profiles/r12b_lanes_ab_per_process.txt: 1 / 2 / 3 / 4 / 6 lanes = 332 / 352 / 362 / 347-352 / 353-362 pairs/s at 4 pairs


class BidirectionalFlow(NamedTuple):
    """What ``predict_step_bidirectional`` / ``predict_bidirectional`` return: both flows ``(N, H, W, 2)`` float32 and, per
    direction, the uint8 mask ``(N, H, W)`` of the pixels whose vector fails the forward-backward test (1 = occluded or out of frame)."""
    forward: object
    backward: object
    occluded_forward: object
    occluded_backward: object


class CameraMotion(NamedTuple):
    """What ``camera_motion_step`` returns: the motions ``(N, 2, 3)`` float32 (frame 1 to frame 2 in pixels) with their statistics
    ``(N, 4)``, the forward flow with the motion's own taken away ``(N, H, W, 2)``, the uint8 mask ``(N, H, W)`` of what moves on its
    own, and the forward flow and occlusion mask they were computed from."""
    motion: object
    stats: object
    residual: object
    moving: object
    forward: object
    occluded_forward: object


class MovingObjects(NamedTuple):
    """What ``moving_objects_step`` returns: ``CameraMotion``'s six fields, then the objects of ``moving`` outside
    ``occluded_forward`` (``image_ops.Objects``): ``labels`` ``(N, H, W)`` int32 (slot + 1, 0 elsewhere), ``count`` ``(N,)`` int32,
    ``area`` ``(N, K)`` int32, ``boxes`` ``(N, K, 4)`` int32 as inclusive ``x0, y0, x1, y1``, ``centroid`` ``(N, K, 2)`` float32 as
    ``(x, y)`` and ``mean_flow`` ``(N, K, 2)`` float32, the object's mean motion relative to the camera in pixels per frame pair."""
    motion: object
    stats: object
    residual: object
    moving: object
    forward: object
    occluded_forward: object
    labels: object
    count: object
    area: object
    boxes: object
    centroid: object
    mean_flow: object


def _hinted(hint):
    return _ffi.thread_concurrency(hint) if hint is not None else contextlib.nullcontext()


class RAFT:
    """reference model.py:10-109.  A model object is driven by one host thread at a time."""

    variant = 'raft'

    def __init__(self, drop_rate=0, iters=12, iters_pred=24, weights: Optional[Dict[str, np.ndarray]] = None,
                 seed=0, alternate_corr=False, overlap=None, pipeline=None, lanes=None, loop_concurrency=None, target_size=None,
                 fit='crop_or_pad', antialias=True, tile_overlap=None, **kwargs):
        # reference model.py:11-12 forwards **kwargs to tf.keras.Model, whose constructor takes `name` (and nothing a
        # forward pass depends on): accept it, reject the rest
        self.name = kwargs.pop('name', type(self).__name__.lower())
        if kwargs:
            raise TypeError(f'unexpected keyword arguments {sorted(kwargs)}')
        self.hidden_dim = 128
        self.context_dim = 128
        self.corr_levels = 4
        self.corr_radius = 4
        self.drop_rate = drop_rate
        self.seed = int(seed)                       # also mixed into the dropout mask seeds of train_step
        self.iters = iters
        self.iters_pred = iters_pred
        self.alternate_corr = alternate_corr
        # Inference on frames of any size (reference train_sintel.py:72-75 CropOrPadder, training.py:72-84 VisFlowCallback): None =
        # frames must already be multiples of 8; 'auto' = every inference call zero-pads its frames to the next multiples of 8, at
        # least MIN_SIDE per axis; (Ht, Wt) = the reference's fixed target, larger frames are centre-cropped.  The returned flow
        # is cropped / zero-padded back to the frames' own size.  Training-mode calls and train_step are not affected.
        self.target_size = self._check_target_size(target_size)
        # How the frames reach the model's size: 'crop_or_pad' = the reference's rule above; 'resize' = bilinear interpolation with
        # half-pixel centres (tf.image.resize; `antialias` widens the triangle where an axis shrinks), the returned flow resized
        # back with u scaled by W / Wt and v by H / Ht -- for frames much larger than the model's size.
        # 'tile' = overlapping tiles of the model's size at the frame's own resolution, run as one batch and cross-faded back
        # (`tile_overlap` pixels, an int or (overlap_y, overlap_x), at least shared by neighbouring tiles).
        # Whichever it is, a call whose frames differ from the model's size builds ONE route object (_fit_frames) and asks it alone.
        self.fit, self.antialias = self._check_fit(fit, antialias, self.target_size)
        self.tile_overlap = self._check_tile_overlap(self.fit, tile_overlap, self.target_size)
        # three-stream schedule of the loop (RAFT only); RAFT_OVERLAP=0 forces the single-stream loop.  With several lanes
        # (below) the loops of a pipelined call default to the single-stream schedule: the other lanes fill the chain's idle CUs
        # and gaps better than a loop's own side branches do (profiles/r12b_lanes_ab_per_process.txt).
        env_ov = os.environ.get('RAFT_OVERLAP')
        self._overlap_given = overlap is not None or env_ov is not None
        self.overlap = (env_ov != '0') if overlap is None else bool(overlap)
        # Consecutive inference calls overlap (section "the forward schedule" below).  OPT-IN (pipeline=True or RAFT_PIPELINE=1):
        # a pipelined call returns before its loop has finished and its results join the consuming stream lazily, which
        # consumers that bypass torch's dispatch (C++ extensions taking at::Tensor, the legacy torch.utils.dlpack.to_dlpack)
        # cannot see -- the default is the serial schedule, where stream order alone makes every route to the bytes safe.
        # ``predict()`` pipelines regardless: it consumes its own results.
        self.pipeline = (os.environ.get('RAFT_PIPELINE', '0') == '1') if pipeline is None else bool(pipeline)
        # Pipelined forward: how many recurrent loops may be in flight at once (each on streams of its own; RAFT_LANES).
        self.lanes = max(1, int(os.environ.get('RAFT_LANES', str(DEFAULT_LANES))) if lanes is None else int(lanes))
        self._state = None                       # serial schedule: the one UpdateState, reused by stream order
        self._ring = []                          # pipelined forward: one RingSlot per state in flight (lanes + 1 slots)
        self._calls = 0
        # which launches of a multi-lane call get the library's concurrency hint (launch shapes of a lanes-times larger batch):
        # 'loop' = the recurrent loop, 'all' = encoders and volume build as well, 'none'
        self._shape_hint = os.environ.get('RAFT_LANE_SHAPES', 'all')      # profiles/r12e_hint_ab.txt: 361 / 374 / 375 pairs/s with none / loop / all at 4 pairs
        # serial schedule: the hint its loops are launched with (1 = latency shapes; tests give a serial model the lanes of a
        # pipelined one to obtain the same kernels, hence the same bits)
        self.loop_concurrency = 1 if loop_concurrency is None else max(1, int(loop_concurrency))
        self._open_lanes = {}                    # lane index -> Lane, made at the lane's first loop
        _dev.reserve_streams(_dev.require_gpu())
        _dev.lib()
        if weights is None:
            weights = weights_mod.init_weights(self.variant, seed)     # Keras default initialisers
        weights_mod.check_weights(self.variant, weights)
        self._weights = dict(weights)
        self._dw, self._host_stale, self._train_vars = None, False, None     # device master copies of train_step
        self._inference_stale = False            # train_step updated them: the inference kernels' packed copies are behind
        self._last_correlation = None
        self._build(weights)

    MIN_SIDE = 64      # the four-level pyramid pools an H/8 x W/8 map three times: below 8 rows or columns its last level is empty

    @classmethod
    def _check_target_size(cls, target_size):
        if target_size is None or target_size == 'auto':
            return target_size
        try:
            th, tw = (int(v) for v in target_size)
        except (TypeError, ValueError):
            raise ValueError(f"target_size must be None, 'auto' or (height, width), got {target_size!r}") from None
        if th % 8 or tw % 8 or th < cls.MIN_SIDE or tw < cls.MIN_SIDE:
            raise ValueError(f'target_size must be multiples of 8 and at least {cls.MIN_SIDE} per axis, got {th} x {tw}')
        return (th, tw)

    @staticmethod
    def _check_fit(fit, antialias, target_size):
        if fit not in ('crop_or_pad', 'resize', 'tile'):
            raise ValueError(f"fit must be 'crop_or_pad', 'resize' or 'tile', got {fit!r}")
        if fit == 'tile' and not isinstance(target_size, tuple):
            raise ValueError("fit='tile' needs a target_size (height, width): the size of a tile")
        if fit == 'resize' and target_size is None:
            raise ValueError("fit='resize' needs a target_size ('auto' or (height, width))")
        if not isinstance(antialias, (bool, np.bool_)):
            raise ValueError(f'antialias must be True or False, got {antialias!r}')
        return fit, bool(antialias)

    DEFAULT_TILE_OVERLAP = 64      # eight feature cells of context on each side of a seam: a choice, not a measured optimum

    @classmethod
    def _check_tile_overlap(cls, fit, tile_overlap, target_size):
        if fit != 'tile':
            if tile_overlap is not None:
                raise ValueError(f"tile_overlap belongs to fit='tile', got fit={fit!r}")
            return None
        return image_ops._overlap_pair(cls.DEFAULT_TILE_OVERLAP if tile_overlap is None else tile_overlap, *target_size)

    @classmethod
    def _check_consistency(cls, alpha, beta):
        """``alpha`` / ``beta`` of the forward-backward test (``image_ops.flow_consistency``) as floats; anything but finite
        numbers >= 0 is a ``ValueError``."""
        return image_ops.check_consistency_args(alpha, beta)

    def _model_size(self, H, W):
        """The size the model runs at for frames of H x W under ``target_size``."""
        if self.target_size == 'auto':
            return max(self.MIN_SIDE, -(-H // 8) * 8), max(self.MIN_SIDE, -(-W // 8) * 8)
        return self.target_size

    def _fit_frames(self, *images):
        """``target_size`` set: the frames of a call (both of a pair; the one new batch of a video stream) as float32 device tensors
        of the model's size, and the call's route between the frames' own size and the model's (``image_ops.fit_route``:
        crop-or-pad, resize or tiles behind one interface; None when the sizes are equal and nothing was launched).  uint8 frames
        are cast on their way in, in the same pass; with ``fit='tile'`` each frame becomes its K tiles (batch N * K).  The route's
        ``flow_back`` takes the predictions to the frames' own size."""
        images = [image_ops._on_device(i) for i in images]
        first = images[0]
        if first.dim() != 4 or first.shape[-1] != 3 or 0 in first.shape or any(i.shape != first.shape or i.dtype != first.dtype for i in images):
            raise ValueError('images must %sbe (bs, H, W, 3) of one type, got %s' % ('both ' if len(images) > 1 else '',
                             ' / '.join(f'{tuple(i.shape)} {i.dtype}' for i in images)))
        H, W = first.shape[1:3]
        th, tw = self._model_size(H, W)
        if (H, W) == (th, tw):
            return (*(_dev.to_device(i) for i in images), None)
        if first.dtype not in (torch.uint8, torch.float32):
            images = [i.to(torch.float32) for i in images]
        # both directions' tables are made (the first time: uploaded) here, on the caller's stream: the launch that takes the
        # predictions back, on the loop's stream of a pipelined call, finds everything in place
        route = image_ops.fit_route(self.fit, first.device, H, W, th, tw, self.antialias, self.tile_overlap)
        return (*(route.frames_in(i) for i in images), route)

    def _build(self, weights):
        self.fnet = BasicEncoder(output_dim=256, norm_type='instance', drop_rate=self.drop_rate,
                                 weights=weights, prefix='fnet')
        self.cnet = BasicEncoder(output_dim=self.hidden_dim + self.context_dim, norm_type='batch',
                                 drop_rate=self.drop_rate, weights=weights, prefix='cnet')
        self.update_block = BasicUpdateBlock(filters=self.hidden_dim, weights=weights, prefix='update_block')

    # ---- weights ------------------------------------------------------------------------------
    def set_weights(self, weights: Dict[str, np.ndarray]) -> None:
        weights_mod.check_weights(self.variant, weights)
        self._join_pipeline()                       # the old device blobs are freed below: no loop may still be reading them
        self._weights = dict(weights)
        self._inference_stale = False
        self._train_vars = None                     # train_step re-reads its device master copies
        self._dw, self._host_stale = None, False
        self.fnet.set_weights(weights)
        self.cnet.set_weights(weights)
        self.update_block.set_weights(weights)

    def load_weights(self, path: str) -> None:
        """reference README.md:66-96 / train_sintel.py:117-123: ``model.load_weights('checkpoints/model')``.
        ``path`` is a TensorFlow checkpoint prefix (``<path>.index`` + ``<path>.data-*``, read without TensorFlow by
        ``tf_raft_amd.checkpoint``) or a ``.npz`` written by ``save_weights`` (Keras layout either way)."""
        from . import checkpoint
        if checkpoint.is_tf_checkpoint(path):
            self.set_weights(checkpoint.load_tf_checkpoint(path, self.variant))
        else:
            self.set_weights(weights_mod.load_weights(path))

    def _sync_host(self):
        """``train_step`` keeps the master weights (and the batch-norm moving statistics) on the device and updates them in
        place; the NumPy dictionary is refreshed from them only when somebody asks for it (checkpoint, inference re-pack)."""
        if self._host_stale and self._dw is not None:
            self._weights = {k: v.detach().cpu().numpy() for k, v in self._dw.items()}
            self._host_stale = False

    def get_weights_dict(self) -> Dict[str, np.ndarray]:
        """The current weights in Keras layout under ``tf_raft_amd.weights`` names."""
        self._sync_host()
        return dict(self._weights)

    def save_weights(self, path: str) -> None:
        """reference train_sintel.py:104-107 (ModelCheckpoint(save_weights_only=True)): ``path`` ending in ``.npz``
        writes the NumPy container, anything else a TensorFlow tensor-bundle checkpoint prefix."""
        from . import checkpoint
        self._sync_host()
        if path.endswith('.npz'):
            weights_mod.save_weights(path, self._weights)
        else:
            checkpoint.write_tf_checkpoint(path, self._weights, self.variant)

    # ---- reference helpers ----------------------------------------------------------------------
    def initialize_flow(self, image):
        """reference model.py:32-37."""
        bs, h, w, _ = image.shape
        return coords_grid(bs, h // 8, w // 8), coords_grid(bs, h // 8, w // 8)

    def upsample_flow(self, flow, mask):
        """reference model.py:39-66.  flow (bs, h, w, 2), mask (bs, h, w, 576) -> (bs, 8h, 8w, 2)."""
        flow = _dev.to_device(flow)
        mask = _dev.to_device(mask)
        bs, h, w, _ = flow.shape
        if tuple(mask.shape) != (bs, h, w, 576) or flow.shape[-1] != 2:
            raise ValueError(f'expected flow (bs,h,w,2) and mask (bs,h,w,576), got {tuple(flow.shape)}, {tuple(mask.shape)}')
        out = torch.empty((bs, 8 * h, 8 * w, 2), device=flow.device, dtype=torch.float32)
        check(_dev.lib().raft_upsample_convex_f32(_dev.ptr(flow), _dev.ptr(mask), bs, h, w, _dev.ptr(out),
                                                  _dev.stream_ptr()), 'upsample_convex')
        return _dev.wrap(out)

    # ---- forward ----------------------------------------------------------------------------------
    def _get_state(self, B, h, w, device) -> UpdateState:
        st = self._state
        if st is None or (st.B, st.h, st.w) != (B, h, w) or st.net.device != device:
            st = UpdateState(self.variant, B, h, w, device)
            self._state = st
        return st

    def _prepare(self, cnet, st):
        check(_dev.lib().raft_prepare_state_f32(_dev.ptr(cnet), st.B, st.h, st.w, C.byref(st.c),
                                                _dev.stream_ptr()), 'prepare_state')
        self.update_block.prepare(st)          # GRU terms of `inp`: constant over the loop (model.py:86)

    def _warm_start(self, flow_init, st):
        check(_dev.lib().raft_warm_start_f32(_dev.ptr(flow_init), st.B, st.h, st.w, C.byref(st.c), _dev.stream_ptr()), 'warm_start')

    def _lane(self, dev, index) -> Lane:
        lane = self._open_lanes.get(index)
        if lane is None or lane.device != dev:
            if lane is not None:
                lane.close()
            lane = self._open_lanes[index] = Lane(dev, index)
        return lane

    def __del__(self):
        for lane in getattr(self, '_open_lanes', {}).values():      # (an object made without __init__ has none)
            lane.close()

    def _iterate(self, corr: CorrBlock, st, iters, out, plan=None, final_only=False):
        """model.py:93-109 on the CURRENT stream (+ the lane's flow / mask streams on the three-stream schedule): the ONE place
        that picks the loop's entry point.  ``out`` takes all ``iters`` predictions, ``final_only`` the last one alone."""
        if plan is None:                            # called on its own: lane 0 of the serial schedule
            plan = self._plan(0, self.overlap, 1)
        lib, wts = _dev.lib(), C.byref(self.update_block.c)
        loop_args = lambda: self._lane(out.device, plan.lane).loop_args(plan)      # (s0, s1, s2, ctx) of the entry points that take them
        if final_only:
            # mask head and convex upsampling in the last iteration only (_predict_final says which models take it)
            check(lib.raft_iterate_basic_final_f32(wts, _dev.ptr(corr._pyr), corr._off, st.B, st.h, st.w, iters, C.byref(st.c),
                                                   _dev.ptr(out), *loop_args()), 'iterate_basic_final')
        elif self.alternate_corr and self.variant == 'raft' and self.overlap:
            # the same C loop, lookups computed on demand from fmap1 and the pooled fmap2 pyramid; overlap=False keeps the loop below
            check(lib.raft_iterate_basic_ondemand_f32(wts, _dev.ptr(corr.fmap1), _dev.ptr(corr._f2pyr), corr.fmap1.shape[-1],
                                                      st.B, st.h, st.w, iters, C.byref(st.c), _dev.ptr(out), *loop_args()),
                  'iterate_basic_ondemand')
        elif self.alternate_corr:
            for i in range(iters):
                corr.retrieve(st.coords1, out=st.corr, ld_out=st.g['corr_ld'])
                self.update_block.step(st)
                self._upsample_into(st, out[i])
        elif self.variant == 'small':
            check(lib.raft_iterate_small_f32(wts, _dev.ptr(corr._pyr), corr._off, st.B, st.h, st.w, iters, C.byref(st.c),
                                             _dev.ptr(out), _dev.stream_ptr()), 'iterate_small')
        elif plan.three_stream:
            # flow branch and mask branch of every iteration on two side streams
            check(lib.raft_iterate_basic_overlap_f32(wts, _dev.ptr(corr._pyr), corr._off, st.B, st.h, st.w, iters, C.byref(st.c),
                                                     _dev.ptr(out), *loop_args()), 'iterate_basic_overlap')
        else:
            # (takes no loop context: none is created for a model that only ever runs this one)
            check(lib.raft_iterate_basic_f32(wts, _dev.ptr(corr._pyr), corr._off, st.B, st.h, st.w, iters, C.byref(st.c),
                                             _dev.ptr(out), _dev.stream_ptr()), 'iterate_basic')
        self._last_correlation = corr               # keep buffers alive until the stream drains

    def _upsample_into(self, st, out):
        check(_dev.lib().raft_upsample_convex_f32(_dev.ptr(st.flow), _dev.ptr(st.mask), st.B, st.h, st.w,
                                                  _dev.ptr(out), _dev.stream_ptr()), 'upsample_convex')

    def __call__(self, inputs, training=False):
        return self.call(inputs, training)

    def call(self, inputs, training=False):
        """reference model.py:68-109."""
        return self._forward(inputs, training)

    def _sync_inference_weights(self):
        if self._inference_stale:
            self._sync_host()
            keep = (self._train_vars, self._dw)
            self.set_weights(self._weights)
            self._train_vars, self._dw = keep
            self._inference_stale = False

    # ---- the forward schedule: serial and pipelined forward ---------------------------------------------------------------
    # One inference call = encoders + volume build (2.96 of 12.3 ms at 4 pairs, kernels that fill the chip) followed by the 24
    # iterations of a DEPENDENT chain whose launches leave 32 .. 88 of the 256 CUs idle.  _forward picks the call's plan and the
    # streams of three roles, and ONE body (_run) enqueues the pass on them: the context stream (cnet and the state preparation),
    # the pre-loop stream (fnet and the volume build: always the caller's) and the loop stream.  For a role that has the caller's
    # stream the body does nothing -- no event, no wait, no record_stream, no stream context: the serial schedule does not pay for
    # the pipelined one's plumbing.  Every ordering rule is a comment at the line in _run that enforces it.
    # Serial schedule: all on the caller's stream, with `overlap` the context encoder beside the feature encoder on the 'encoder'
    # side stream.  Stream order alone makes every route to the result's bytes safe.
    # Pipelined schedule: back-to-back calls are independent of each other, so call n + 1's pre-loop work can run under call n's
    # loop.  The loop is enqueued on the loop stream of lane n % lanes, the pre-loop work stays on the caller's stream, and the
    # returned tensors carry a `_dev.Pending`: whichever stream first touches their data waits for the loop then (a caller that
    # consumes the result at once sees the serial schedule).  Why several lanes: the loop's kernels are launched for ONE batch,
    # 7 * 2^k workgroups on 256 CUs, a ~3 us boundary between dependent kernels, one event gap per iteration -- which is why 8
    # pairs per call run 9 % and 16 pairs 17 % faster per pair than 4.  With `lanes` = D > 1 up to D loops of consecutive calls
    # are resident together (schedule.Lane) and each fills the other's gaps and idle CUs; the loop state, which call n + 1 would
    # overwrite, exists D + 1 times (schedule.RingSlot).  Each call still runs exactly the kernels of the serial schedule in the
    # same order on its own buffers: results are bit-identical per call
    # (tests/test_gpu_model.py::test_pipelined_calls_are_bitwise_the_serial_calls).
    def _forward(self, inputs, training=False, final_only=False, pipelined=None, mirror=False, video=None):
        """``mirror`` (inference, serial schedule): ONE pass over the 2B pairs [(image1, image2) | (image2, image1)] with the
        feature encoder run once per frame; the result has batch 2B, the second half the backward direction.  ``video`` (inference,
        serial schedule): the call of a ``tf_raft_amd.video.FlowVideo``, whose frames arrive fitted (``video.route``), whose first
        feature map is carried from the stream's previous call and whose loop may start from ``video.flow_init``."""
        self._sync_inference_weights()
        image1, image2 = inputs
        route = None
        if video is not None:
            route = video.route                         # (the stream fitted each frame once, when it arrived)
        elif self.target_size is not None and not training:
            image1, image2, route = self._fit_frames(image1, image2)
        image1 = _dev.to_device(image1)
        image2 = _dev.to_device(image2)
        if image1.dim() != 4 or image1.shape[-1] != 3 or image1.shape != image2.shape:
            raise ValueError(f'images must both be (bs, H, W, 3), got {tuple(image1.shape)} / {tuple(image2.shape)}')
        B, H, W, _ = image1.shape
        if H % 8 or W % 8:
            raise ValueError(f'H and W must be multiples of 8 (got {H}x{W})')   # model.py:35 uses h//8
        # model.py:70-71 (2 * (image / 255) - 1) is applied by the encoders while they stage the image
        dev = image1.device
        slot = context_stream = loop_stream = None          # None = the caller's stream
        if (self.pipeline if pipelined is None else pipelined) and not training and not mirror:
            # several lanes (and their launch shapes) only for a model that asked for the pipelined schedule: predict() on a serial
            # model overlaps its calls on ONE lane with the serial schedule's kernels, so predict() == predict_step() bit for bit
            lanes = self.lanes if self.pipeline else 1
            n = self._calls
            self._calls += 1
            # with several lanes the loops are single-stream unless overlap was asked for: the lanes are each other's side branches
            plan = self._plan(n % lanes, self.overlap and not (lanes > 1 and not self._overlap_given), lanes)
            while len(self._ring) <= lanes:
                self._ring.append(RingSlot())
            slot, loop_stream = self._ring[n % (lanes + 1)], self._lane(dev, plan.lane).stream('loop')
        else:
            self._join_pipeline()                       # (a training-mode or serial call after pipelined ones)
            plan = self._plan(0, self.overlap, 1 if training else self.loop_concurrency)
            if self.overlap and not training:
                # the context encoder does not depend on the feature encoder or the volume: it runs on a side stream
                # next to them (its one-workgroup-per-CU layers fill the tails of the feature encoder's launches)
                context_stream = _dev.side_stream(dev, 'encoder')
        with _hinted(plan.pre_hint):                    # (the loop's own hint inside; the thread's is restored on the way out)
            return self._run(image1, image2, training, final_only, mirror and not training, plan, route, slot, context_stream, loop_stream,
                             video)

    def _plan(self, lane, three_stream, hint):
        """The loop plan of one call.  ``hint`` is the number of loops that share the chip: the lanes of a pipelined call,
        loop_concurrency of a serial inference call, 1 in training.  RAFT_LANE_SHAPES says whether the loop ('loop', 'all') and the
        pre-loop work ('all') are launched with it; with a hint of 1 the pre-loop work keeps the calling thread's own."""
        return LoopPlan(lane, three_stream, hint if (hint > 1 and self._shape_hint == 'all') else None,
                        hint if self._shape_hint in ('loop', 'all') else 1)

    def _run(self, image1, image2, training, final_only, mirror, plan, route, slot, context_stream, loop_stream, video=None):
        """The forward pass of both schedules.  ``slot`` / ``loop_stream``: the ring slot and the lane's loop stream of a pipelined
        call; ``context_stream``: the side stream of the context encoder; None = the caller's stream, the serial state.
        ``video``: the stream whose call this is (None: a call on a pair)."""
        B, H, W, _ = image1.shape
        dev = image1.device
        cur = torch.cuda.current_stream(dev)
        if mirror:
            # Both directions as one batch of 2B pairs.  The backward direction needs the same two feature maps with their roles
            # swapped and the context of frame 2: fnet still runs on 2B frames (not 4B), cnet on [image1 | image2], and everything
            # from the volume build on sees an ordinary batch of 2B.
            B = 2 * B
        if slot is None:
            st = self._get_state(B, H // 8, W // 8, dev)     # (allocated under the caller's stream, like its other users)
        else:
            st = slot.fit(self.variant, B, H // 8, W // 8, dev)
            if slot.done is not None:
                # a pipelined call never makes the caller's stream wait for a loop, except for the one that read the state this
                # call is about to overwrite (call n - lanes - 1), and that in front of the state preparation
                cur.wait_event(slot.done)

        def context():
            if mirror:
                cnet = self.cnet.forward_device(image1, input_affine=True, images_b=image2)
            else:
                cnet = self.cnet(image1, training=training, _raw_images=True)             # model.py:82
            self._prepare(cnet, st)                                                       # model.py:84-89
            if video is not None and video.flow_init is not None:
                self._warm_start(video.flow_init, st)      # coords1 = grid + init: behind the preparation, on its stream
            return cnet

        if context_stream is not None:
            # net / inp / the GRU's context rows depend on cnet only: prepared there too, beside the feature encoder, instead
            # of behind the volume build (0.1 ms of the step at 4 pairs).  The encoder stream follows the caller's first, which
            # also orders this call's state preparation behind the previous call's loop
            context_stream.wait_stream(cur)
            with torch.cuda.stream(context_stream):
                cnet = context()
        elif not training:
            cnet = context()       # (kept to the end of the call, as the other pre-loop buffers are: one allocation pattern per call)
        if mirror:
            # the encoder's output (B, h, w, C) over [image1 | image2] IS the first operand; the second is its halves swapped
            fmap1 = self.fnet.forward_device(image1, input_affine=True, images_b=image2)
            fmap2 = torch.cat([fmap1[B // 2:], fmap1[:B // 2]], dim=0)
        elif video is not None:
            # fnet on the NEW frames alone (image2), beside the context encoder as ever; the first operand is what the stream
            # carried from its previous call, and the new map is what it carries on
            fmap1, fmap2 = video.feature_maps(self.fnet.forward_device(image2, input_affine=True))
        else:
            fmap1, fmap2 = self.fnet([image1, image2], training=training, _raw_images=True)   # model.py:74
        correlation = CorrBlock(fmap1, fmap2, num_levels=self.corr_levels, radius=self.corr_radius,
                                alternate=self.alternate_corr)                  # model.py:77
        if context_stream is not None:
            cur.wait_stream(context_stream)             # the loop reads what the encoder stream prepared ...
            cnet.as_subclass(torch.Tensor).record_stream(cur)       # ... and cnet, allocated there, is the caller's stream's to reuse
        elif training:
            cnet = context()       # the reference's order: the encoders' dropout draws from one generator, fnet's mask first
        iters = self.iters if training else self.iters_pred
        shape = (B, H, W, 2)
        # from the caller's stream's pool, like every other buffer; the result has the frames' batch and size (the tiles of
        # fit='tile' are a batch of N * K)
        out = torch.empty(shape if final_only else (iters,) + shape, device=dev, dtype=torch.float32)
        res = out if route is None else torch.empty(out.shape[:-4] + route.result_size(B) + (2,), device=dev, dtype=torch.float32)
        if loop_stream is not None:
            # the loop stream waits for ONE event of the caller's stream, behind the volume build and the allocations above
            ready = torch.cuda.Event()
            ready.record(cur)
            loop_stream.wait_event(ready)
        with (torch.cuda.stream(loop_stream) if loop_stream is not None else contextlib.nullcontext()), _ffi.thread_concurrency(plan.loop_hint):
            self._iterate(correlation, st, iters, out, plan, final_only)
            if route is not None:
                # to the frames' own size on the LOOP's stream, in front of `done`: the caller's stream never waits for the loop
                route.flow_back(out, into=res)
            if loop_stream is not None:
                slot.done = torch.cuda.Event()
                slot.done.record(loop_stream)
        pending = None
        if loop_stream is not None:
            for t in (out, res, *correlation.tensors(), *(route.tensors() if route is not None else ())):
                t.record_stream(loop_stream)             # allocated under the caller's stream, in use on the loop stream
            pending = _dev.Pending(slot.done, dev)
        return _dev.wrap(res, pending) if final_only else [_dev.wrap(res[i], pending) for i in range(iters)]   # model.py:109

    def _join_pipeline(self):
        """Make the current stream wait for every loop this model still has in flight: called before anything that frees or
        rewrites buffers a loop reads (weight blobs, training's in-place optimizer updates) -- in the serial schedule stream order
        gave that for free."""
        for slot in self._ring:
            slot.join()

    def _predict_final(self, image1, image2, **how):
        """``flow_predictions[-1]`` of an inference call.  RAFT with overlap and a stored volume computes it with the mask head and
        the convex upsampling in the last iteration only (``raft_iterate_basic_final_f32``: the recurrence itself is unchanged, so
        the result equals ``self(...)[-1]``)."""
        if self.variant == 'raft' and self.overlap and not self.alternate_corr:
            return self._forward([image1, image2], final_only=True, **how)
        return self._forward([image1, image2], **how)[-1]

    def predict_step(self, data, _pipelined=None):
        """reference model.py:160-166: ``flow_predictions[-1]`` of the forward pass (``_predict_final``)."""
        image1, image2, *_ = data
        return self._predict_final(image1, image2, pipelined=_pipelined)

    def predict_step_bidirectional(self, data, alpha=image_ops.CONSISTENCY_ALPHA, beta=image_ops.CONSISTENCY_BETA,
                                   occlusion_test='consistency', range_threshold=image_ops.RANGE_THRESHOLD):
        """The flow in both directions with occlusion masks: ``BidirectionalFlow(forward, backward, occluded_forward,
        occluded_backward)`` of device tensors for ``data = (image1, image2)`` -- ``forward`` what ``predict_step((image1,
        image2))`` predicts, ``backward`` what ``predict_step((image2, image1))`` does, both ``(N, H, W, 2)`` float32 at the
        frames' own size, and per direction the uint8 mask ``(N, H, W)`` of ``image_ops.flow_consistency(forward, backward,
        alpha, beta)``: 1 where the vector's end point leaves the frame or the two directions disagree there (occlusion).

        ONE forward pass over the 2N pairs [(image1, image2) | (image2, image1)], final prediction only, on the serial schedule
        on the caller's stream (a model with pipelined loops in flight joins them first, as a training-mode call does), then one
        consistency launch on the flows that are returned: with a ``target_size`` the call's route takes the 2N predictions back
        to the frames' size first (``fit='tile'``: 2N * K tiles blend to 2N frames).  Cost: the memory and time of ``__call__``
        on 2N pairs (docs/NOTEBOOK.md section 21 has the measurement).

        ``occlusion_test='range'`` takes the masks from the range map instead (``image_ops.range_occlusion(forward, backward,
        range_threshold)``), on the same returned flows; ``alpha`` / ``beta`` are then checked and unused."""
        alpha, beta = self._check_consistency(alpha, beta)
        occlusion_test = image_ops.check_occlusion_test(occlusion_test)
        range_threshold = image_ops.check_range_threshold(range_threshold)
        image1, image2, *_ = data
        flows = self._predict_final(image1, image2, pipelined=False, mirror=True).as_subclass(torch.Tensor)
        N = flows.shape[0] // 2
        if occlusion_test == 'range':
            occ_f, occ_b = image_ops.range_occlusion_launch(flows[:N], flows[N:], range_threshold)
        else:
            occ_f, occ_b = image_ops.flow_consistency_launch(flows[:N], flows[N:], alpha, beta)
        return BidirectionalFlow(_dev.wrap(flows[:N]), _dev.wrap(flows[N:]), _dev.wrap(occ_f), _dev.wrap(occ_b))

    @staticmethod
    def _pair_batches(x, batch_size, steps):
        """The ``(image1, image2)`` batches of ``predict`` / ``predict_bidirectional`` as one generator, and the number of pairs
        they hold where it is known beforehand (else None): ``x`` is ``[image1, image2]`` arrays, split into batches of
        ``batch_size`` (Keras' default 32), or an iterable of ``(image1, image2, ...)`` batches; ``steps`` limits their number."""
        n = None
        if isinstance(x, (list, tuple)) and len(x) == 2 and all(getattr(a, 'ndim', 0) == 4 for a in x):
            n = x[0].shape[0]
            if x[1].shape[0] != n:
                raise ValueError(f'image1 and image2 hold {n} and {x[1].shape[0]} images')
            bs = int(batch_size) if batch_size else 32
            if bs < 1:
                raise ValueError(f'batch_size must be >= 1, got {batch_size}')
            batches = ((x[0][i:i + bs], x[1][i:i + bs]) for i in range(0, n, bs))
        else:
            batches = iter(x)
        if steps is not None:
            batches = itertools.islice(batches, int(steps))
        return ((b[0], b[1]) for b in batches), (n if steps is None else None)

    def predict_bidirectional(self, x, batch_size=None, steps=None, alpha=image_ops.CONSISTENCY_ALPHA, beta=image_ops.CONSISTENCY_BETA,
                              occlusion_test='consistency', range_threshold=image_ops.RANGE_THRESHOLD):
        """``predict_step_bidirectional`` over all pairs of ``x`` (as for ``predict()``: ``[image1, image2]`` arrays split into
        batches of ``batch_size``, Keras' default 32, or an iterable of ``(image1, image2, ...)`` batches; ``steps`` limits the
        number of batches): the same named tuple as host arrays, flows ``(N, H, W, 2)`` float32 and masks ``(N, H, W)`` uint8.
        Host batches are uploaded one batch ahead of the compute stream (``tf_raft_amd.prefetch``); every batch's results are
        copied back synchronously."""
        from .prefetch import prefetch_to_device
        alpha, beta = self._check_consistency(alpha, beta)
        occlusion_test = image_ops.check_occlusion_test(occlusion_test)
        range_threshold = image_ops.check_range_threshold(range_threshold)
        dev = _dev.require_gpu()
        batches, _ = self._pair_batches(x, batch_size, steps)
        parts = [[], [], [], []]
        for image1, image2 in prefetch_to_device(batches, buffer_size=1, device=dev):
            for acc, t in zip(parts, self.predict_step_bidirectional((image1, image2), alpha, beta, occlusion_test, range_threshold)):
                acc.append(t.as_subclass(torch.Tensor).cpu().numpy())
        if not parts[0]:
            raise ValueError('predict_bidirectional() received no batches')
        return BidirectionalFlow(*(np.concatenate(acc, axis=0) for acc in parts))

    def interpolate_step(self, data, t=0.5, skip_occluded=False, **occlusion):
        """The frame at time ``t`` between ``data = (image1, image2)``: one ``predict_step_bidirectional``
        pass (``**occlusion``: its ``alpha``, ``beta``, ``occlusion_test``, ``range_threshold``), then ``image_ops.interpolate_launch``
        on the RETURNED flows and the caller's own frames, at the frames' own size -- so it works with every ``target_size`` /
        ``fit``.  Returns a device tensor ``(N, H, W, 3)``, uint8 for uint8 frames and float32 otherwise; ``t`` in ``[0, 1]`` may be
        a sequence, the result is then ``(T, N, H, W, 3)`` from ONE forward pass.  ``skip_occluded=True`` splats only the pixels
        the occlusion test trusts (``occluded_* == 0`` as ``mask1`` / ``mask2``); the default splats every pixel, which is a
        choice, not a tuned value: random weights and no footage say nothing about which looks better."""
        times, many = image_ops._times(t)
        unknown = set(occlusion) - {'alpha', 'beta', 'occlusion_test', 'range_threshold'}
        if unknown:
            raise TypeError(f'interpolate_step() got unexpected keyword arguments {sorted(unknown)}')
        image1, image2, *_ = data
        shape, in_dtype = image_ops._frames_ahead(image1, 'interpolate_step')
        shape2, in_dtype2 = image_ops._frames_ahead(image2, 'interpolate_step')
        if len(shape) != 4 or shape2 != shape or in_dtype2 != in_dtype:
            raise ValueError(f'expected two frame batches (N, H, W, 3) of one type, got {shape} {in_dtype} / {shape2} {in_dtype2}')
        image_ops._check_frame_sizes(2 * shape[0], shape[1], shape[2], shape[3], 'interpolate_step')
        i1, i2 = image_ops._on_device(image1), image_ops._on_device(image2)
        res = self.predict_step_bidirectional((i1, i2), **occlusion)
        fwd, bwd = res.forward.as_subclass(torch.Tensor), res.backward.as_subclass(torch.Tensor)
        m1 = m2 = None
        if skip_occluded:
            m1 = (res.occluded_forward.as_subclass(torch.Tensor) == 0).view(torch.uint8)
            m2 = (res.occluded_backward.as_subclass(torch.Tensor) == 0).view(torch.uint8)
        out = torch.empty((len(times),) + tuple(i1.shape), device=i1.device, dtype=in_dtype)
        for k, tk in enumerate(times):
            image_ops.interpolate_launch(i1, i2, fwd, bwd, tk, m1, m2, dtype=in_dtype, out=out[k])
        return _dev.wrap(out if many else out[0])

    def predict_interpolated(self, x, t=0.5, batch_size=None, steps=None, skip_occluded=False, **occlusion):
        """``interpolate_step`` over all pairs of ``x`` (as for ``predict_bidirectional()``) as one host array ``(N, H, W, 3)``, or
        ``(T, N, H, W, 3)`` for a sequence of ``t``; uint8 for uint8 frames.  Host batches are uploaded one batch ahead of the
        compute stream (``tf_raft_amd.prefetch``); every batch's frames are copied back synchronously."""
        from .prefetch import prefetch_to_device
        _, many = image_ops._times(t)
        dev = _dev.require_gpu()
        batches, _ = self._pair_batches(x, batch_size, steps)
        parts = []
        for image1, image2 in prefetch_to_device(batches, buffer_size=1, device=dev):
            parts.append(self.interpolate_step((image1, image2), t, skip_occluded, **occlusion).as_subclass(torch.Tensor).cpu().numpy())
        if not parts:
            raise ValueError('predict_interpolated() received no batches')
        return np.concatenate(parts, axis=1 if many else 0)

    def interpolate_video(self, frames, factor=2, batch_size=None):
        """One video ``(T, H, W, 3)``, host or device, at ``factor`` times its frame rate: a host array ``((T - 1) * factor + 1, H,
        W, 3)`` of the frames' type (uint8, else float32) with the original frames verbatim at every ``factor``-th index and
        ``factor - 1`` frames synthesised between neighbours at ``t = k / factor`` (``interpolate_step``, ``batch_size``
        consecutive pairs per call, default 4)."""
        shape = tuple(frames.shape) if hasattr(frames, 'shape') else np.shape(frames)
        if len(shape) != 4 or shape[-1] != 3:
            raise ValueError(f'frames must be one video (T, H, W, 3), got {shape}')
        if shape[0] < 2:
            raise ValueError(f'a video needs at least two frames, got T = {shape[0]}')
        if isinstance(factor, (bool, np.bool_)) or not isinstance(factor, (int, np.integer)) or factor < 1:
            raise ValueError(f'factor must be an integer >= 1, got {factor!r}')
        factor = int(factor)
        host = frames.detach().cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
        if host.dtype != np.uint8:
            host = host.astype(np.float32, copy=False)
        out = np.empty(((shape[0] - 1) * factor + 1,) + shape[1:], host.dtype)
        out[::factor] = host
        if factor > 1:
            mid = self.predict_interpolated([host[:-1], host[1:]], [k / factor for k in range(1, factor)], batch_size or 4)
            for k in range(1, factor):
                out[k::factor] = mid[k - 1]
        return out

    def video(self, warm_start=False):
        """A stream of consecutive frames (``tf_raft_amd.video.FlowVideo``): ``push(frames)`` returns the flow from the previous
        frames to these, with the feature encoder run once per frame; ``warm_start=True`` starts every pair's recurrence from the
        previous pair's flow projected forward (RAFT's video protocol).  Serial schedule, on the caller's stream."""
        from .video import FlowVideo
        return FlowVideo(self, warm_start)

    def predict_video(self, frames, warm_start=False, batch_size=None, steps=None):
        """The flows between the consecutive frames of one video ``(T, H, W, 3)`` as a host array ``(T - 1, H, W, 2)``
        (``tf_raft_amd.video.predict_video``)."""
        from .video import predict_video
        return predict_video(self, frames, warm_start, batch_size, steps)

    def tracker(self, points, start=None, consistency=True, warm_start=False, alpha=image_ops.CONSISTENCY_ALPHA,
                beta=image_ops.CONSISTENCY_BETA, max_points=None, replenish=False, detect=None):
        """Points followed through a stream of frames (``tf_raft_amd.video.FlowTracker``): ``points``
        ``(N, P, 2)`` float32 as ``(x, y)`` in pixels of the frames; ``push(frames)`` returns ``(positions (N, P, 2), lost (N, P))``
        in the pushed frames (None after the first push).  ``consistency=True`` tests every step against the backward flow of a
        bidirectional pass; ``consistency=False`` rides on ``video(warm_start)`` and tests only the frame borders.  ``alpha`` /
        ``beta`` are UnFlow's values, not tuned ones.  ``points=None`` with ``max_points=K`` detects the points in the first
        pushed frames (``image_ops.detect_points`` with the options of ``detect=dict(...)``);
        ``replenish=True`` refills lost slots from a detection on every pushed frame and gives the tracker ``.ids`` and ``.born``."""
        from .video import FlowTracker
        return FlowTracker(self, points, start, consistency, warm_start, alpha, beta, max_points, replenish, detect)

    def track_video(self, frames, points, start=None, consistency=True, batch_size=4, alpha=image_ops.CONSISTENCY_ALPHA,
                    beta=image_ops.CONSISTENCY_BETA, max_points=None, replenish=False, detect=None):
        """``points`` ``(P, 2)`` followed through one video ``(T, H, W, 3)`` as host arrays ``(positions (T, P, 2), lost (T, P))``,
        row 0 the points themselves (``tf_raft_amd.video.track_video``).  ``points=None`` with ``max_points=K`` detects them in
        frame 0; ``replenish=True`` refills lost slots at the chunk boundaries and also returns ``ids (T, P)``."""
        from .video import track_video
        return track_video(self, frames, points, start, consistency, batch_size, alpha, beta, max_points, replenish, detect)

    def camera_motion_step(self, data, model='affine', occlusion_test='consistency', iterations=image_ops.MOTION_ITERATIONS,
                           scale=image_ops.MOTION_SCALE, threshold=1.0, **occlusion):
        """What the camera did between ``data = (image1, image2)`` and what moves on its own:
        ``CameraMotion(motion, stats, residual, moving, forward, occluded_forward)`` of device tensors.  One
        ``predict_step_bidirectional`` pass (``occlusion_test`` and ``**occlusion``: its ``alpha``, ``beta``, ``range_threshold``);
        the RETURNED forward flow, at the frames' own size whatever ``target_size`` / ``fit`` is, is fitted with the pixels of
        ``occluded_forward`` left out (``image_ops.fit_motion_launch``: ``model``, ``iterations``, ``scale``) -> ``motion`` ``(N, 2, 3)``
        and ``stats`` ``(N, 4)``; ``residual`` ``(N, H, W, 2)`` is the flow minus the motion's own and ``moving`` ``(N, H, W)`` uint8
        marks where it is longer than ``threshold`` pixels (``image_ops.residual_flow_launch``).  ``iterations``, ``scale`` and
        ``threshold`` are choices, not tuned values."""
        image_ops.check_motion_args(model, iterations, scale)
        threshold = image_ops.check_motion_threshold(threshold)
        if threshold is None:
            raise ValueError('threshold must be a number, got None')
        unknown = set(occlusion) - {'alpha', 'beta', 'range_threshold'}
        if unknown:
            raise TypeError(f'camera_motion_step() got unexpected keyword arguments {sorted(unknown)}')
        res = self.predict_step_bidirectional(data, occlusion_test=occlusion_test, **occlusion)
        forward, occluded = res.forward.as_subclass(torch.Tensor), res.occluded_forward.as_subclass(torch.Tensor)
        motion, stats = image_ops.fit_motion_launch(forward, occluded, True, model, iterations, scale)
        residual, moving = image_ops.residual_flow_launch(forward, motion, threshold)
        return CameraMotion(_dev.wrap(motion), _dev.wrap(stats), _dev.wrap(residual), _dev.wrap(moving), res.forward, res.occluded_forward)

    def moving_objects_step(self, data, model='affine', threshold=1.0, max_objects=64, min_area=image_ops.OBJECTS_MIN_AREA,
                            connectivity=image_ops.OBJECTS_CONNECTIVITY, occlusion_test='consistency',
                            iterations=image_ops.MOTION_ITERATIONS, scale=image_ops.MOTION_SCALE, **occlusion):
        """Which objects move on their own between ``data = (image1, image2)``: ``MovingObjects`` of device
        tensors.  ONE ``camera_motion_step`` (``model``, ``threshold``, ``occlusion_test``, ``iterations``, ``scale``,
        ``**occlusion``), then ``image_ops.find_objects_launch`` on its ``moving`` mask with the pixels of ``occluded_forward`` left
        out and its ``residual`` as the flow: per pair the up to ``max_objects`` connected components (``connectivity`` 4 or 8) of
        at least ``min_area`` pixels, largest first, with area, inclusive box, centroid and ``mean_flow``, the object's mean motion
        relative to the camera in pixels per frame pair.  All coordinates are those of the frames the caller passed, whatever
        ``target_size`` / ``fit`` is.  Nothing is synchronised or downloaded.  ``threshold``, ``max_objects`` and ``min_area`` are
        choices, not tuned values: random weights and no footage say nothing about what is found."""
        K, min_area, connectivity = image_ops.check_objects_args(max_objects, min_area, connectivity)
        cam = self.camera_motion_step(data, model=model, occlusion_test=occlusion_test, iterations=iterations, scale=scale,
                                      threshold=threshold, **occlusion)
        plain = lambda t: t.as_subclass(torch.Tensor).contiguous()       # noqa: E731
        objects = image_ops.find_objects_launch(plain(cam.moving), K, min_area, connectivity, plain(cam.occluded_forward),
                                                plain(cam.residual), True)
        return MovingObjects(*cam, *(_dev.wrap(t) for t in objects))

    def object_tracker(self, max_objects=64, min_overlap=image_ops.OBJECT_MIN_OVERLAP, **options):
        """Moving objects with identities that last through a stream of frames (``tf_raft_amd.video.ObjectTracker``, DESIGN.md
        section 31): ``push(frames)`` takes one frame ``(N, H, W, 3)`` of each of N videos, runs one ``moving_objects_step((previous,
        frames), max_objects=max_objects, **options)`` and returns ``TrackedObjects`` -- ``MovingObjects``' fields, then ``ids``,
        ``born``, ``match`` and ``origin`` ``(N, K)`` int32 -- for the objects of the PREVIOUS pushed frame (None after the first
        push).  An object keeps its id while at least ``min_overlap`` of its pixels, carried along the flow, land on one object of
        the next pair; ``max_objects`` is at most 128.  ``min_overlap`` is a choice, not a tuned value.  Serial schedule."""
        from .video import ObjectTracker
        return ObjectTracker(self, max_objects, min_overlap, **options)

    def track_objects_video(self, frames, batch_size=4, max_objects=64, min_overlap=image_ops.OBJECT_MIN_OVERLAP, return_labels=False,
                            **options):
        """The moving objects of one video ``(T, H, W, 3)`` with identities that last, as host arrays over its ``T - 1`` pairs:
        ``ObjectTracks(count, ids, born, area, boxes, centroid, mean_flow, labels)`` (``tf_raft_amd.video.track_objects_video``);
        every pair predicted in a call of its own, ``batch_size`` pairs per upload and per identity launch, one download at the end,
        the same result for every ``batch_size``."""
        from .video import track_objects_video
        return track_objects_video(self, frames, batch_size, max_objects, min_overlap, return_labels, **options)

    def stabilize_video(self, frames, model='similarity', radius=15, iterations=image_ops.MOTION_ITERATIONS, scale=image_ops.MOTION_SCALE,
                        batch_size=4, occlusion_test='consistency', return_motion=False):
        """One video ``(T, H, W, 3)`` steadied: the camera's motion fitted pair by pair on the device, its path smoothed on the host
        and every frame resampled under its correction (``tf_raft_amd.video.stabilize_video``); a host array of the frames' shape
        and type."""
        from .video import stabilize_video
        return stabilize_video(self, frames, model, radius, iterations, scale, batch_size, occlusion_test, return_motion)

    def fuse_step(self, data, sigma=image_ops.FUSE_SIGMA, patch_radius=image_ops.FUSE_PATCH_RADIUS,
                  center_weight=image_ops.FUSE_CENTER_WEIGHT, occlusion_test='consistency', **occlusion):
        """Burst fusion: ``data = (center, neighbours)`` with ``center`` ``(N, H, W, 3)`` and ``neighbours``
        ``(K, N, H, W, 3)`` of one type (uint8, or float32 on 0 .. 255; host or device; K in 1 .. 16) -> the centre fused with its
        neighbours, a device tensor ``(N, H, W, 3)`` of the frames' type.  ONE ``predict_step_bidirectional`` call on the ``K * N``
        pairs (centre, neighbour k) (``occlusion_test`` and ``**occlusion``: its ``alpha``, ``beta``, ``range_threshold``): its
        ``forward`` is the flow centre -> neighbour k and its ``occluded_forward`` the ``skip`` of ONE
        ``image_ops.fuse_frames_launch`` (``sigma``, ``patch_radius``, ``center_weight``) on the caller's own frames, at the frames'
        own size -- so it works with every ``target_size`` / ``fit``.  The centre goes through the feature encoder K times (once per
        pair; there is no forward path that shares it).  ``sigma``, ``patch_radius`` and ``center_weight`` are choices, not tuned
        values: random weights and no footage say nothing about how the result looks."""
        image_ops.check_fuse_args(sigma, patch_radius, center_weight)
        image_ops.check_occlusion_test(occlusion_test)
        unknown = set(occlusion) - {'alpha', 'beta', 'range_threshold'}
        if unknown:
            raise TypeError(f'fuse_step() got unexpected keyword arguments {sorted(unknown)}')
        center, neighbours, *_ = data
        neighbours = image_ops._stacked(neighbours)
        shape, in_dtype = image_ops._frames_ahead(center, 'fuse_step')
        nshape, ndtype = image_ops._shape_and_type(neighbours, 'fuse_step')
        if len(shape) != 4 or shape[-1] != 3 or len(nshape) != 5 or nshape[1:] != shape or ndtype != in_dtype:
            raise ValueError(f'expected a centre (N, H, W, 3) and neighbours (K, N, H, W, 3) of one type, got {shape} {in_dtype} / '
                             f'{nshape} {ndtype}')
        K, N, H, W, _ = nshape
        image_ops._check_fuse_sizes(K, N, H, W, 3, 'fuse_step')
        c, stack = image_ops._on_device(center), image_ops._on_device(neighbours)
        first = c.unsqueeze(0).expand(K, N, H, W, 3).reshape(K * N, H, W, 3)
        res = self.predict_step_bidirectional((first, stack.view(K * N, H, W, 3)), occlusion_test=occlusion_test, **occlusion)
        flows = res.forward.as_subclass(torch.Tensor).contiguous().view(K, N, H, W, 2)
        skip = res.occluded_forward.as_subclass(torch.Tensor).contiguous().view(K, N, H, W)
        out, _ = image_ops.fuse_frames_launch(c, stack, flows, None, skip, False, sigma, patch_radius, center_weight)
        return _dev.wrap(out)

    def denoise_video(self, frames, radius=2, sigma=image_ops.FUSE_SIGMA, patch_radius=image_ops.FUSE_PATCH_RADIUS,
                      center_weight=image_ops.FUSE_CENTER_WEIGHT, batch_size=4):
        """One video ``(T, H, W, 3)`` filtered along its motion: every frame fused with up to ``radius`` frames on each side,
        aligned by chained bidirectional flows (``tf_raft_amd.video.denoise_video``); a host array of the frames' shape and type."""
        from .video import denoise_video
        return denoise_video(self, frames, radius, sigma, patch_radius, center_weight, batch_size)

    def predict(self, x, batch_size=None, steps=None, output='flow', clip_flow=None, convert_to_bgr=False, rad_max=None, **kwargs):
        """``keras.Model.predict`` over ``predict_step`` (reference model.py:160-166): the final flow of every image
        pair as one host array ``(N, H, W, 2)``.

        ``x`` is ``[image1, image2]`` (host or device arrays ``(N, H, W, 3)``, split into batches of ``batch_size``,
        Keras' default 32) or an iterable of ``(image1, image2, ...)`` batches (the reference's ``tf.data`` datasets).
        Host batches are uploaded one batch ahead of the compute stream and the predictions come back through pinned
        buffers one batch behind it (``tf_raft_amd.prefetch``), so neither transfer sits on the critical path.

        ``output='image'`` returns the colour-coded flow instead, uint8 ``(N, H, W, 3)``: what the reference's
        ``flow_to_image`` makes of each prediction (``tf_raft_amd.image_ops.flow_to_image``, which takes ``clip_flow``,
        ``convert_to_bgr`` and ``rad_max``), coloured on the download stream in front of the copy, so 3 instead of 8 bytes per
        pixel cross to the host."""
        from .prefetch import prefetch_to_device
        if output not in ('flow', 'image'):
            raise ValueError(f"output must be 'flow' or 'image', got {output!r}")
        viz = image_ops._viz_args(clip_flow, rad_max) if output == 'image' else None
        dev = _dev.require_gpu()
        batches, total = self._pair_batches(x, batch_size, steps)
        down = torch.cuda.Stream(device=dev)
        pins, landing, results = {}, [], []
        whole, filled = None, 0                  # one preallocated host array when the number of pairs is known

        def collect():
            nonlocal whole, filled
            pin, ev = landing.pop(0)
            ev.synchronize()
            got = pin.numpy()
            if total is None:
                results.append(got.copy())
                return
            if whole is None:
                whole = np.empty((total,) + got.shape[1:], got.dtype)
            whole[filled:filled + got.shape[0]] = got
            filled += got.shape[0]

        for i, (image1, image2) in enumerate(prefetch_to_device(batches, buffer_size=1, device=dev)):
            res = self.predict_step((image1, image2), _pipelined=True)   # consumed below on `down`: the compute stream never waits for a loop
            cur = torch.cuda.current_stream(dev)
            shape, dtype = (tuple(res.shape), res.dtype) if viz is None else (tuple(res.shape[:-1]) + (3,), torch.uint8)
            key = (i & 1, shape)
            if key not in pins:
                pins[key] = torch.empty(shape, dtype=dtype).pin_memory()
            down.wait_stream(cur)
            with torch.cuda.stream(down):
                out = res.as_subclass(torch.Tensor)      # pipelined forward: `down`, not the compute stream, waits for the loop
                # the picture (and its workspace) are allocated, written and read under `down` alone
                src = out if viz is None else image_ops.flow_to_image_launch(out, shape[1], shape[2], viz[0], convert_to_bgr, viz[1])
                pins[key].copy_(src, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(down)
            out.record_stream(down)
            landing.append((pins[key], ev))
            if len(landing) > 1:
                collect()
        while landing:
            collect()
        if whole is not None:
            return whole
        if not results:
            raise ValueError('predict() received no batches')
        return np.concatenate(results, axis=0)

    # ---- evaluation plumbing (reference model.py:111-170)
    def compile(self, optimizer=None, clip_norm=None, loss=None, epe=None, trainable='all', tape_dtype='f32', bidirectional=False,
                occlusion=True, alpha=image_ops.CONSISTENCY_ALPHA, beta=image_ops.CONSISTENCY_BETA, occlusion_test='consistency',
                range_threshold=image_ops.RANGE_THRESHOLD, selfsup_crop=None, selfsup_weight=0.3, selfsup_eps=0.001,
                selfsup_mask='teacher', selfsup_transform=None, **kwargs):
        """reference model.py:111-124.  ``loss`` / ``epe`` default to ``tf_raft_amd.losses.sequence_loss`` /
        ``end_point_error``; ``loss=losses.PhotometricSequenceLoss(...)`` makes ``train_step`` take unlabelled pairs
        ``(image1, image2)`` or ``(image1, image2, mask)`` and report ``loss`` / ``photometric`` / ``smoothness`` (DESIGN.md
        section 17; ``test_step`` still wants ground truth), and ``census`` when the loss has ``census_weight > 0`` (section 18);
        ``losses.SSIMSequenceLoss(..., ssim_weight > 0)`` adds ``ssim`` (section 19), and
        ``losses.Smooth2SequenceLoss(..., smooth2_weight > 0)`` ``smoothness2`` directly behind ``smoothness`` (section 24).  ``trainable``: which weights ``train_step`` updates -- ``'all'``
        (the reference's behaviour: encoders, norms and update block) or ``'update_block'`` (encoders frozen, run by the
        inference kernels).

        ``bidirectional=True`` (needs a ``PhotometricSequenceLoss``) makes ``train_step`` train both
        directions of every pair in one step -- ``(image1, image2)`` or ``(image1, image2, (mask1, mask2))``, the loss the mean
        of the two directions -- and, while ``model.occlusion`` is true, leave out of the data terms the pixels that fail the
        forward-backward test of the step's own last predictions (``alpha`` / ``beta`` as in ``image_ops.flow_consistency``;
        the defaults are UnFlow's constants, not tuned here).  ``occlusion`` sets ``model.occlusion``, a plain bool that may be
        flipped between steps; the step also reports ``occluded``, the running mean of the occluded share, whether or not the
        mask is applied, and keeps its ``(2N, H, W)`` uint8 mask in ``model.last_visibility``.  ``occlusion_test='range'``
        (with ``bidirectional=True`` only) takes that mask from the range map of the same predictions instead (DESIGN.md
        section 21; ``range_threshold`` as in ``image_ops.range_occlusion``); everything else about the step stays.

        ``selfsup_crop=(cy, cx)`` (with ``bidirectional=True`` only) adds self-supervision: after the pass
        over the full frames (the teacher) the step runs the network again on the frames with ``cy`` rows and ``cx`` columns
        removed from each side (the student), trains the student's predictions to reproduce the teacher's last flow read through
        that window and held constant (``losses.SelfSupervisionLoss(gamma of the loss, selfsup_weight, selfsup_eps)``), and
        applies the sum of both passes' gradients once.  ``selfsup_mask='teacher'`` uses every pixel the teacher is trusted at
        (``last_visibility``); ``'occluded'`` is UFlow's rule: of those, the pixels that fail the student's own occlusion test
        (its mask is kept in ``model.last_student_visibility``).  ``model.selfsup_weight`` is a plain float that may be changed
        between steps (the recipes ramp it up after a warm-up); at 0 the second pass is skipped.  The step also reports
        ``selfsup`` and ``selfsup_used``.  0.3 and 0.001 are UFlow's constants, not tuned here.

        ``selfsup_transform`` (needs ``selfsup_crop``, which keeps defining the student's size): an
        ``augment.StudentTransform``, or any callable ``(N, (H, W), (Hs, Ws)) -> augment.StudentView``.  The student then sees
        the frames through the step's drawn affine view (flip, zoom, rotation, shift, per-frame gain and bias) instead of the
        centre crop, and is asked for the teacher's flow expressed in its own coordinates; the step's view is kept in
        ``model.last_student_view`` and the ``(2N, Hs, Ws)`` uint8 mask of the student pixels that have a trusted teacher
        vector in ``model.last_target_visibility``.  None: the centre crop, every step, key and bit as before."""
        from . import losses
        if kwargs:
            raise TypeError(f'unexpected keyword arguments {sorted(kwargs)}')
        if trainable not in ('all', 'update_block'):
            raise ValueError(f"trainable must be 'all' or 'update_block', got {trainable!r}")
        if tape_dtype not in ('f32', 'bf16'):     # bf16: the loop's activation tape is STORED as bf16 (BASELINE configs[4]), fp32 arithmetic
            raise ValueError(f"tape_dtype must be 'f32' or 'bf16', got {tape_dtype!r}")
        if not isinstance(bidirectional, (bool, np.bool_)) or not isinstance(occlusion, (bool, np.bool_)):
            raise ValueError(f'bidirectional and occlusion must be True or False, got {bidirectional!r} / {occlusion!r}')
        if bidirectional and not isinstance(loss, losses.PhotometricSequenceLoss):
            raise ValueError(f'bidirectional=True trains on unlabelled pairs: it needs loss=losses.PhotometricSequenceLoss(...) '
                             f'(or a subclass), got {loss!r}')
        self.consistency = self._check_consistency(alpha, beta)
        self.occlusion_test = image_ops.check_occlusion_test(occlusion_test)
        self.range_threshold = image_ops.check_range_threshold(range_threshold)
        if self.occlusion_test == 'range' and not bidirectional:
            raise ValueError("occlusion_test='range' is the mask of a bidirectional step: it needs bidirectional=True")
        if selfsup_crop is not None:
            if not bidirectional:
                raise ValueError('selfsup_crop: the teacher is the bidirectional step\'s pass, it needs bidirectional=True')
            try:
                cy, cx = selfsup_crop
                cy, cx = losses._index('selfsup_crop[0]', cy), losses._index('selfsup_crop[1]', cx)
            except (TypeError, ValueError) as exc:
                raise ValueError(f'selfsup_crop must be None or a pair of ints (cy, cx), got {selfsup_crop!r}') from exc
            if cy < 0 or cx < 0 or (cy == 0 and cx == 0):
                raise ValueError(f'selfsup_crop must be non-negative and not (0, 0), got {selfsup_crop!r}')
            selfsup_crop = (cy, cx)
        if selfsup_mask not in ('teacher', 'occluded'):
            raise ValueError(f"selfsup_mask must be 'teacher' or 'occluded', got {selfsup_mask!r}")
        _, selfsup_weight, selfsup_eps, _ = losses._selfsup_params(0.0, selfsup_weight, selfsup_eps)
        if selfsup_transform is not None:
            if selfsup_crop is None:
                raise ValueError('selfsup_transform draws the view of the student pass: it needs selfsup_crop, which sets the student\'s size')
            draw = getattr(selfsup_transform, 'draw', selfsup_transform)
            if not callable(draw):
                raise ValueError(f'selfsup_transform must be an augment.StudentTransform or a callable (N, (H, W), (Hs, Ws)) -> '
                                 f'StudentView, got {selfsup_transform!r}')
        self.selfsup_crop, self.selfsup_weight, self.selfsup_eps, self.selfsup_mask = selfsup_crop, selfsup_weight, selfsup_eps, selfsup_mask
        self.selfsup_transform = selfsup_transform
        self.last_student_view = self.last_target_visibility = None
        self.bidirectional, self.occlusion = bool(bidirectional), bool(occlusion)
        self.last_visibility = None
        self.last_student_visibility = None
        self.optimizer = optimizer
        self.clip_norm = clip_norm
        self.loss = loss if loss is not None else losses.sequence_loss
        self.epe = epe if epe is not None else losses.end_point_error
        self.trainable = trainable
        self._train_vars = None
        self.tape_dtype = tape_dtype
        self.flow_metrics = OrderedDict((k, losses.Mean(name=k)) for k in ('loss', 'epe', 'u1', 'u3', 'u5'))
        if isinstance(self.loss, losses.PhotometricSequenceLoss):       # (the EPE means stay: test_step feeds them)
            self.flow_metrics.update((k, losses.Mean(name=k)) for k in self._unlabelled_keys()[1:])

    def _unlabelled_keys(self):
        """What ``train_step`` reports under a PhotometricSequenceLoss (``occluded``: in bidirectional mode; ``selfsup`` and
        ``selfsup_used``: with ``selfsup_crop``)."""
        on = [k for k in ('census', 'ssim') if getattr(self.loss, k + '_weight', 0.0) > 0]
        second = ('smoothness2',) if getattr(self.loss, 'smooth2_weight', 0.0) > 0 else ()
        return (('loss', 'photometric', *on, 'smoothness', *second) + (('occluded',) if getattr(self, 'bidirectional', False) else ())
                + (('selfsup', 'selfsup_used') if getattr(self, 'selfsup_crop', None) is not None else ()))

    BN_MOMENTUM = 0.99      # Keras BatchNormalization default (extractor.py:10 passes none)

    def train_step(self, data):
        """reference model.py:126-144: forward with ``iters`` iterations in training mode, ``sequence_loss``, backward,
        ``clip_by_global_norm``, the optimizer's ``apply_gradients``, metrics.  Everything arithmetic is a HIP kernel
        (``tf_raft_amd.grad``: encoders in training form with instance / batch-statistics norms, volume build and its
        backward, the loop and its backward through time; ``tf_raft_amd.training.AdamW``).  With
        ``compile(..., trainable='update_block')`` the encoders stay frozen and run on the inference kernels.
        The step is orchestrated from Python; the updated master weights are re-packed for the kernels ON THE DEVICE, one launch
        per layer and use (``raft_pack_train_conv_f32``).  It is the functional path (parity-tested against autograd on the
        oracle), not yet a tuned one.  RAFT and SmallRAFT.
        After ``compile(..., bidirectional=True)`` the step runs the doubled batch ``[image1 | image2]``
        against ``[image2 | image1]`` with the feature encoder once per frame, and the mask of the loss comes from one
        ``raft_flow_visibility_f32`` launch on its own last prediction (``occlusion_test='range'``:
        ``raft_flow_range_visibility_f32``).
        After ``compile(..., selfsup_crop=(cy, cx))`` a second graded pass follows on the centre crops of the
        frames, its loss ``raft_selfsup_loss_f32`` against the first pass's last prediction; the two passes' gradients are added
        and applied once, and the batch-norm moving statistics are updated with each pass's batch statistics in turn.  The
        forward and backward of one pass is ``_graded_pass``, whatever the loss.
        With ``selfsup_transform`` the student's frames come from one ``raft_view_frames_f32`` launch over
        the 2N distinct frames under the step's drawn view, and the teacher's flow and mask reach the loss through one
        ``raft_view_flow_f32`` launch, already in the student's coordinates."""
        from . import grad, losses
        if not hasattr(self, 'flow_metrics'):
            raise RuntimeError('call compile() before train_step()')
        photometric = isinstance(self.loss, losses.PhotometricSequenceLoss)
        if not photometric and self.loss is not losses.sequence_loss:
            raise NotImplementedError('train_step differentiates tf_raft_amd.losses.sequence_loss and '
                                      'tf_raft_amd.losses.PhotometricSequenceLoss only')
        bidirectional = photometric and self.bidirectional
        if bidirectional:                           # arity and shapes, before anything is enqueued
            pair_masks = losses._check_bidirectional(data)
            crop = self.selfsup_crop
            if crop is not None:
                _, Hf, Wf, _ = losses._shape_of(data[0])
                Hs, Ws = Hf - 2 * crop[0], Wf - 2 * crop[1]
                if Hs % 8 or Ws % 8 or Hs < self.MIN_SIDE or Ws < self.MIN_SIDE:
                    raise ValueError(f'selfsup_crop={crop} leaves a student of {Hs} x {Ws} from frames of {Hf} x {Wf}: both sides must be '
                                     f'multiples of 8 and at least {self.MIN_SIDE}')
                weight2 = losses._selfsup_params(0.0, self.selfsup_weight, self.selfsup_eps)[1]   # (it may have been changed since compile)
        elif photometric and len(data) not in (2, 3):
            raise ValueError(f'train_step with PhotometricSequenceLoss expects (image1, image2) or (image1, image2, mask), '
                             f'got {len(data)} items')
        if not photometric and len(data) != 4:
            raise ValueError(f'train_step with sequence_loss expects (image1, image2, flow, valid), got {len(data)} items')
        self._join_pipeline()                       # inference loops still in flight read the weights this step updates in place
        if self.optimizer is None or not hasattr(self.optimizer, 'apply_gradients'):
            raise RuntimeError('compile() needs an optimizer with apply_gradients(grads, variables, clip_norm) '
                               '(tf_raft_amd.training.AdamW)')
        if photometric:
            image1, image2, flow, valid = data[0], data[1], None, None
            unlabelled = None if bidirectional else losses._check_unlabelled(data, ())[:3]       # shapes, before anything is enqueued
        else:
            image1, image2, flow, valid = data
        image1 = _dev.to_device(image1).as_subclass(torch.Tensor).to(torch.float32)
        image2 = _dev.to_device(image2).as_subclass(torch.Tensor).to(torch.float32)
        # the ground truth goes to the device NOW: an upload from pageable host memory waits for everything already queued on
        # the stream, and in front of the loss that is the whole forward pass (the host would enqueue the backward only after
        # the GPU had drained: 20 ms of a 85 ms step)
        if bidirectional:
            # the doubled batch [image1 | image2] against [image2 | image1]; everything below sees 2N pairs
            pairs = image1.shape[0]
            user_mask = None
            if pair_masks is not None:
                user_mask = torch.cat([losses._mask_to_device(m, image1.device) for m in pair_masks], dim=0).contiguous()
            image1, image2 = torch.cat([image1, image2], dim=0), torch.cat([image2, image1], dim=0)
        elif photometric:                           # (the mask is uploaded now for the same reason)
            y_true = (image1, image2) if unlabelled[2] is None else (image1, image2, losses._mask_to_device(unlabelled[2], image1.device))
        else:
            flow, valid = losses._truth((flow, valid))
        B, H, W, _ = image1.shape
        if H % 8 or W % 8:
            raise ValueError(f'H and W must be multiples of 8 (got {H}x{W})')
        full = self.trainable == 'all'
        # Master copies of EVERY weight (and the batch-norm moving statistics) live on the device from the first step on and
        # are updated in place; grad.* packs them for the convolution kernels on the device too.  Nothing of a step crosses
        # PCIe except the input batch (get_weights_dict / save_weights / the next inference call pull them back lazily).
        if self._dw is None:
            self._dw = {k: _dev.to_device(np.ascontiguousarray(v, dtype=np.float32)).as_subclass(torch.Tensor).clone()
                        for k, v in self._weights.items()}
        wts = self._dw
        grad.clear_pack_cache()                     # packed copies of last step's weights
        view_records = None
        if bidirectional and crop is not None and weight2 > 0.0 and self.selfsup_transform is not None:
            # the step's view is drawn and its records are uploaded NOW, for the reason given above
            from . import augment
            draw = getattr(self.selfsup_transform, 'draw', self.selfsup_transform)
            view = draw(pairs, (H, W), (Hs, Ws))
            if not isinstance(view, augment.StudentView) or len(view) != pairs:
                raise ValueError(f'selfsup_transform must return an augment.StudentView of {pairs} views, got {view!r}')
            view_records = image_ops.view_records(view, 2 * pairs, image1.device)
            self.last_student_view = view
        drop_seed = None
        if full and self.drop_rate:
            # mask seeds: a different stream per data-parallel rank (ranks see different shards), per model seed and per
            # optimizer step.  save_weights / load_weights persist the WEIGHTS only (as the reference's
            # ModelCheckpoint(save_weights_only=True) does, train_sintel.py:104-107): a caller that resumes a run must restore
            # optimizer.iterations itself, otherwise the mask sequence (and the LR schedule) restarts at step 1
            step = int(getattr(getattr(self, 'optimizer', None), 'iterations', 0) or 0)
            self._drop_step = max(getattr(self, '_drop_step', 0) + 1, step + 1)
            drop_seed = _dropout_seed(getattr(self, 'seed', 0), _rank_of_this_process(), self._drop_step)

        def first_loss(preds):
            """The loss of the first (or only) pass and its gradient: ``(d_preds, (terms or loss, last prediction, mask))``."""
            visible = None
            if bidirectional:
                # the mask of the loss from THIS forward pass's last prediction: a constant of the gradient.  Without occlusion
                # and without user masks it is all ones and the loss kernels' "no mask" specialisation runs.
                last = preds[-1].as_subclass(torch.Tensor).contiguous()
                if self.occlusion_test == 'range':
                    visible, occluded = image_ops.range_visibility_launch(last, pairs, user_mask, self.range_threshold, apply=self.occlusion)
                else:
                    visible, occluded = image_ops.flow_visibility_launch(last, pairs, user_mask, *self.consistency, apply=self.occlusion)
                self.last_visibility = _dev.wrap(visible)
                truth = (image1, image2, visible) if (self.occlusion or user_mask is not None) else (image1, image2)
            if photometric:                         # value and gradient share the gathers: one launch per term
                terms, d_preds = self.loss.value_and_grad(truth if bidirectional else y_true, preds)
                if bidirectional:
                    terms = dict(terms, occluded=_dev.wrap(occluded))
                return d_preds, (terms, preds[-1], visible)
            loss = self.loss([flow, valid], preds)
            return grad.sequence_loss_grad((flow, valid), preds), (loss, preds[-1], None)

        def flat(grads):
            return {k: grads[k].as_subclass(torch.Tensor).reshape(wts[k].shape).contiguous() for k in sorted(grads)}

        # the first pass's tape and all but its last prediction die with the call, before a second pass allocates
        grads, stats, (terms, last_pred, visible1) = self._graded_pass(wts, image1, image2, pairs if bidirectional else None, drop_seed,
                                                                       first_loss)
        gt, all_stats = flat(grads), [stats]
        if bidirectional and crop is not None:
            self.last_student_visibility = self.last_target_visibility = None
        if bidirectional and crop is not None and weight2 > 0.0:
            # the student pass on the centre crops [c1 | c2] against [c2 | c1]; the teacher is the first
            # pass's last prediction, read through the window and held constant
            teacher = last_pred.as_subclass(torch.Tensor).contiguous()
            if view_records is None:
                crop1, crop2 = image_ops.window_copy(image1.contiguous(), Hs, Ws), image_ops.window_copy(image2.contiguous(), Hs, Ws)
                origin, teacher_visible = crop, visible1
            else:
                # the 2N distinct frames are the first operand of the doubled batch: ONE gather, then [s1 | s2] against [s2 | s1];
                # the teacher's flow and mask in the student's coordinates by ONE more
                crop1 = image_ops.view_frames_launch(image1.contiguous(), view_records, (Hs, Ws))
                crop2 = torch.cat([crop1[pairs:], crop1[:pairs]], dim=0)
                teacher, teacher_visible = image_ops.view_flow_launch(teacher, view_records, (Hs, Ws), visible1)
                origin = (0, 0)
                self.last_target_visibility = _dev.wrap(teacher_visible)

            def student_loss(preds):
                student_visible = None
                if self.selfsup_mask == 'occluded':     # UFlow's rule: only where the student fails its own occlusion test
                    last = preds[-1].as_subclass(torch.Tensor).contiguous()
                    if self.occlusion_test == 'range':
                        student_visible, _ = image_ops.range_visibility_launch(last, pairs, None, self.range_threshold, apply=True)
                    else:
                        student_visible, _ = image_ops.flow_visibility_launch(last, pairs, None, *self.consistency, apply=True)
                    self.last_student_visibility = _dev.wrap(student_visible)
                selfsup = losses.SelfSupervisionLoss(self.loss.gamma, weight2, self.selfsup_eps)
                terms2, d_preds = selfsup.value_and_grad(teacher, preds, origin, teacher_visible, student_visible,
                                                         _add_to=terms['loss'].as_subclass(torch.Tensor))
                return d_preds, terms2

            grads2, stats2, terms2 = self._graded_pass(wts, crop1, crop2, pairs, None if drop_seed is None else drop_seed + 2, student_loss)
            gt = grad.add_gradients(gt, flat(grads2))               # g1 + g2, one float32 addition per element
            all_stats.append(stats2)
            terms = dict(terms, **terms2)                           # ('loss': the first pass's plus the weighted term)
        names = sorted(gt)
        self._train_vars = {k: wts[k] for k in names}          # views of the device master copies (updated in place)
        from .parallel import all_reduce_gradients, all_reduce_mean_
        all_reduce_gradients(gt)                    # data-parallel training: one bucketed RCCL all-reduce (no-op on one rank)
        self.optimizer.apply_gradients(gt, self._train_vars, clip_norm=self.clip_norm)
        # Keras BatchNormalization moving statistics (momentum 0.99), in place on the device.  TF 2.3's fused kernel feeds the
        # moving variance with the UNBIASED batch variance; that detail cannot be checked here (no TensorFlow) and is stated in
        # DESIGN.md.  Data-parallel: the batch statistics are averaged over the ranks first (one small all-reduce), so that
        # every rank keeps the same moving statistics and a checkpoint does not depend on which rank writes it.
        # A step with a student pass updates them twice, with the first pass's statistics and then the second's: what two
        # training-mode calls inside one Keras train_step do.
        for stats in all_stats:
            if not stats:
                continue
            order = sorted(stats)
            all_reduce_mean_([t for name in order for t in (stats[name][0], stats[name][1])])
            for name in order:
                mean, var, cnt = stats[name]
                mm, mv = wts[f'{name}/moving_mean'], wts[f'{name}/moving_variance']
                mm.copy_(grad._axpby(self.BN_MOMENTUM, mm, 1.0 - self.BN_MOMENTUM, mean.contiguous()))
                mv.copy_(grad._axpby(self.BN_MOMENTUM, mv, (1.0 - self.BN_MOMENTUM) * cnt / max(cnt - 1.0, 1.0), var.contiguous()))
        if any(all_stats):
            grad.bump_pack_version()                     # parameters written outside the optimizer: packed copies are stale
        # the NumPy dictionary and the inference kernels' re-packed (Winograd-transformed, N-fused) copies are refreshed
        # lazily: by get_weights_dict / save_weights, and by the next forward call
        self._host_stale = True
        self._inference_stale = True
        if photometric:
            for k in self._unlabelled_keys():
                if k in terms:                      # ('selfsup' / 'selfsup_used': only by a step that ran the student pass)
                    self.flow_metrics[k].update_state(terms[k])
            return {k: self.flow_metrics[k].result() for k in self._unlabelled_keys()}
        info = self.epe([flow, valid], last_pred)
        self.flow_metrics['loss'].update_state(terms)
        for k in ('epe', 'u1', 'u3', 'u5'):
            self.flow_metrics[k].update_state(info[k])
        return {k: m.result() for k, m in self.flow_metrics.items()}

    def _graded_pass(self, wts, image1, image2, pairs, drop_seed, loss_of):
        """Forward and backward of one pass of ``train_step`` over ``(B, H, W, 3)`` float32 device frames: the encoders, the
        volume, the loop, ``loss_of(preds) -> (d_preds, result)``, and back to the gradient of every trained tensor.  ``pairs``:
        None, or N of a bidirectional pass whose frames are the doubled batch (the feature encoder then runs once per frame).
        ``drop_seed``: the seed of the first of the pass's two dropout masks.  Returns ``(grads, batch-norm statistics, result)``;
        the tape and the predictions ``loss_of`` did not keep are released on return."""
        from . import grad
        bidirectional = pairs is not None
        B, H, W, _ = image1.shape
        h, w = H // 8, W // 8
        full = self.trainable == 'all'
        drop_masks = []
        if full:
            ones = torch.ones_like(image1)
            x1 = grad._axpby(2.0 / 255.0, image1.contiguous(), -1.0, ones)            # model.py:70-71
            if bidirectional:                       # x1 already holds every frame once: both roles of a frame share its features
                frames = x1
            else:
                frames = torch.cat([x1, grad._axpby(2.0 / 255.0, image2.contiguous(), -1.0, ones)], dim=0)
            fout, ftape = grad.encoder_forward(wts, 'fnet', frames, training=True)     # model.py:74
            fout = fout.as_subclass(torch.Tensor)
            cnet, ctape = grad.encoder_forward(wts, 'cnet', x1, training=True)         # model.py:82
            cnet = cnet.as_subclass(torch.Tensor)
            if self.drop_rate:     # extractor.py:109-111, 127-128: Dropout on the encoder outputs while training
                fout, mf = grad.dropout_forward(fout, self.drop_rate, seed=drop_seed)
                cnet, mc = grad.dropout_forward(cnet, self.drop_rate, seed=drop_seed + 1)
                drop_masks = [mf, mc]
            fmap1, fmap2 = grad.mirror_feature_maps(fout, pairs) if bidirectional else (fout[:B].contiguous(), fout[B:].contiguous())
        else:
            if self.drop_rate:
                raise NotImplementedError("drop_rate > 0 with trainable='update_block': dropout sits on the (frozen) encoder "
                                          "outputs; train all weights or use drop_rate=0")
            if bidirectional:
                halves = self.fnet([image1[:pairs], image1[pairs:]], training=False, _raw_images=True)
                fmap1, fmap2 = grad.mirror_feature_maps(torch.cat([t.as_subclass(torch.Tensor) for t in halves], dim=0), pairs)
            else:
                fmap1, fmap2 = self.fnet([image1, image2], training=False, _raw_images=True)
            cnet = self.cnet(image1, training=False, _raw_images=True)
        correlation = CorrBlock(fmap1, fmap2, num_levels=self.corr_levels, radius=self.corr_radius)   # model.py:77
        st = self._get_state(B, h, w, image1.device)
        prep = _dev.lib().raft_prepare_state_f32 if self.variant == 'raft' else _dev.lib().raft_prepare_state_small_f32
        check(prep(_dev.ptr(cnet), st.B, st.h, st.w, C.byref(st.c), _dev.stream_ptr()), 'prepare_state')   # model.py:84-86 / 209-211
        net0 = st.net.clone()
        inp = st.x[..., :self.context_dim].contiguous()
        prefix = 'update_block'
        ub = {k: v for k, v in wts.items() if k.startswith(prefix)}
        preds, tape = grad.loop_forward(ub, correlation, net0, inp, self.iters, prefix, self.variant, tape_dtype=self.tape_dtype)
        d_preds, result = loss_of(preds)
        d_net0, d_inp, d_pyr, grads = grad.loop_backward(ub, correlation, tape, d_preds, prefix)
        stats = {}
        if full:
            d_f1, d_f2 = grad.corr_build_backward(correlation, d_pyr)
            if bidirectional:                       # the sum of a frame's two roles
                d_fout = grad.mirror_feature_maps_backward(d_f1, d_f2, pairs)
            else:
                d_fout = torch.cat([d_f1.as_subclass(torch.Tensor), d_f2.as_subclass(torch.Tensor)], dim=0).contiguous()
            d_cnet = grad.prepare_state_backward(net0, inp, d_net0, d_inp)
            if drop_masks:
                d_fout = grad.dropout_backward(d_fout, drop_masks[0])
                d_cnet = grad.dropout_backward(d_cnet.as_subclass(torch.Tensor).contiguous(), drop_masks[1])
            gf, _ = grad.encoder_backward(wts, 'fnet', ftape, d_fout)
            gc, stats = grad.encoder_backward(wts, 'cnet', ctape, d_cnet)
            grads = dict(grads)
            grads.update(gf)
            grads.update(gc)
        return grads, stats, result

    def test_step(self, data):
        """reference model.py:146-158: forward prediction, then EPE / u1 / u3 / u5 of ``flow_predictions[-1]`` against
        ``(flow, valid)`` into the running means; returns ``{name: mean so far}`` (``loss`` is only fed by train_step).
        Only the last prediction is consumed, so it is computed the ``predict_step`` way."""
        if not hasattr(self, 'flow_metrics'):
            raise RuntimeError('call compile() before test_step()')   # keras raises for an un-compiled model too
        image1, image2, flow, valid = data
        last = self.predict_step((image1, image2))
        info = self.epe([flow, valid], last)
        for k in ('epe', 'u1', 'u3', 'u5'):
            self.flow_metrics[k].update_state(info[k])
        return {k: m.result() for k, m in self.flow_metrics.items()}

    def reset_metrics(self):
        """reference model.py:168-170."""
        for m in getattr(self, 'flow_metrics', {}).values():
            m.reset_states()


class SmallRAFT(RAFT):
    """reference model.py:173-226."""

    variant = 'small'

    def __init__(self, drop_rate=0, iters=12, iters_pred=24, **kwargs):
        super().__init__(drop_rate, iters, iters_pred, **kwargs)
        self.hidden_dim = 96
        self.context_dim = 64
        self.corr_levels = 4
        self.corr_radius = 3

    def _build(self, weights):
        self.fnet = SmallEncoder(output_dim=128, norm_type='instance', drop_rate=self.drop_rate,
                                 weights=weights, prefix='fnet')
        self.cnet = SmallEncoder(output_dim=96 + 64, norm_type=None, drop_rate=self.drop_rate,
                                 weights=weights, prefix='cnet')
        self.update_block = SmallUpdateBlock(filters=96, weights=weights, prefix='update_block')

    def _prepare(self, cnet, st):
        check(_dev.lib().raft_prepare_state_small_f32(_dev.ptr(cnet), st.B, st.h, st.w, C.byref(st.c),
                                                      _dev.stream_ptr()), 'prepare_state_small')

    def _warm_start(self, flow_init, st):
        check(_dev.lib().raft_warm_start_small_f32(_dev.ptr(flow_init), st.B, st.h, st.w, C.byref(st.c), _dev.stream_ptr()), 'warm_start_small')

    def _upsample_into(self, st, out):
        check(_dev.lib().raft_upflow8_f32(_dev.ptr(st.flow), st.B, st.h, st.w, _dev.ptr(out),
                                          _dev.stream_ptr()), 'upflow8')

    def upsample_flow(self, flow, mask=None):
        return upflow8(flow)

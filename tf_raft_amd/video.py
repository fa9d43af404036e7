"""Flow over frame sequences: every frame encoded once, and RAFT's warm start.

In footage frame ``t`` is ``image2`` of one pair and ``image1`` of the next.  A ``FlowVideo`` (``model.video()``) keeps, between
its calls, what the next pair needs of the previous frame: the frame itself at the model's size (the context encoder reads it)
and its feature map (the first operand of the correlation volume), so the feature encoder runs on the new frames alone.  With
``warm_start=True`` it also keeps the low-resolution flow the loop ended on and starts the next pair's recurrence from its forward
projection (``image_ops.forward_interpolate``, the authors' video protocol) instead of from zero.

A call is the final-prediction forward pass of ``predict_step`` on the serial schedule on the caller's stream; the stream object
is the ``video`` argument of ``RAFT._run``, which asks it for the two feature maps and the initial flow and leaves everything from
the correlation volume on as it is.

``FlowTracker`` (``model.tracker(points)``) and ``track_video`` follow points through footage: they chain the
flows the predictor returns with ``image_ops.track_launch``, one launch per call whatever the number of pairs, and with
``consistency=True`` (the default) test every step against the backward flow of ``predict_step_bidirectional``.

``smooth_trajectory`` and ``stabilize_video`` steady footage: the camera's motion of every pair is fitted on the
device (``image_ops.fit_motion_launch``), the path of the camera is smoothed on the host, and every frame is resampled under its
correction (``image_ops.view_frames_launch``).  There is no streaming form: the smoother needs the frames to come.

``denoise_video`` filters footage along its motion: the bidirectional flows of consecutive frames are kept on
the device, every frame's pixel grid is chained through its neighbours both ways in time (``image_ops.track_launch``), and one
``image_ops.fuse_frames_launch`` per frame averages the aligned neighbours robustly, read from the video where they lie.

``ObjectTracker`` (``model.object_tracker()``) and ``track_objects_video`` keep the identity of moving objects through footage
(DESIGN.md section 31): the labels of one ``moving_objects_step`` are carried along its forward flow and counted against the labels
of the next (``image_ops.object_overlap_launch``), slots are matched one to one (``match_objects_launch``) and ids handed on
(``chain_object_ids_launch``), a chunk of pairs per launch.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _dev
from . import image_ops


class FlowVideo:
    """``model.video(warm_start=False)``: ``push(frames)`` takes one frame ``(N, H, W, 3)`` of each of N independent videos (uint8
    or float, host or device) and returns the flow from the previous frames to these, ``(N, H, W, 2)`` at the frames' own size
    (None after the first push).  ``flow_low`` is the model-space 1/8 flow the last loop ended on, ``(N', h, w, 2)`` with
    ``N' = N * tiles`` under ``fit='tile'``; ``reset()`` forgets the stream (and accepts another frame shape)."""

    def __init__(self, model, warm_start=False):
        self.model = model
        self.warm_start = bool(warm_start)
        self.reset()

    def reset(self):
        self._signature = None                  # (N, H, W, dtype) of a time step
        self._frame = self._fmap = None         # the carry: the last time step at the model's size, and its feature map
        self.flow_low = None
        self.route = self.flow_init = None      # of the call in flight (read by RAFT._forward / _run)

    def push(self, frames, flow_init=None):
        """The next frame of every video.  ``flow_init``: an explicit model-space start of the recurrence ``(N', h, w, 2)`` in
        place of the propagated one (also without ``warm_start``)."""
        return self._step(frames, 1, flow_init)

    # ---- what RAFT._run asks
    def feature_maps(self, new):
        """``(fmap1, fmap2)`` of the call from the feature map of its new frames, which holds ``steps`` time steps of ``k`` maps:
        the first operand is the carried map followed by all but the last step, and the last step is carried on."""
        k = self._fmap.shape[0]
        fmap1 = self._fmap if new.shape[0] == k else torch.cat([self._fmap, new[:-k]], dim=0)
        self._fmap = new[-k:]
        return fmap1, new

    # ---- one call: `steps` consecutive time steps of N frames each (push: one; the chunks of predict_video: N = 1)
    def _step(self, frames, steps, flow_init=None):
        m = self.model
        shape = tuple(frames.shape) if hasattr(frames, 'shape') else np.shape(frames)
        dtype = frames.dtype if hasattr(frames, 'dtype') else np.asarray(frames).dtype
        if len(shape) != 4 or shape[-1] != 3 or 0 in shape or shape[0] % steps:
            raise ValueError(f'frames must be (N, H, W, 3), got {shape}')
        signature = (shape[0] // steps,) + shape[1:3] + (str(dtype).replace('torch.', ''),)
        if self._signature is not None and signature != self._signature:
            raise ValueError(f'this stream holds frames (N, H, W, type) = {self._signature}, got {signature}: reset() it first')
        if m.target_size is not None:
            frame, route = m._fit_frames(frames)
        else:
            frame, route = _dev.to_device(frames), None
            if frame.shape[1] % 8 or frame.shape[2] % 8:
                raise ValueError(f'H and W must be multiples of 8 (got {frame.shape[1]}x{frame.shape[2]})')
        k = frame.shape[0] // steps                      # model-space rows of a time step (N, or N * tiles)
        if self._frame is None:
            # the first time step: nothing to pair it with.  Encoded here, as a later call encodes its new frames
            if steps != 1:
                raise ValueError('the first call of a stream takes one time step')
            if flow_init is not None:
                raise ValueError('flow_init belongs to a pair: the first push has none')
            m._sync_inference_weights()
            m._join_pipeline()
            self._signature, self._frame = signature, frame
            self._fmap = m.fnet.forward_device(frame, input_affine=True)
            return None
        if flow_init is not None:
            init = self._check_init(flow_init, frame)
        elif self.warm_start and self.flow_low is not None:
            # into a buffer of its own, in front of the state preparation that overwrites the state
            init = image_ops.forward_interpolate_launch(self.flow_low)
        else:
            init = None
        image1 = self._frame if steps == 1 else torch.cat([self._frame, frame[:-k]], dim=0)
        self.route, self.flow_init = route, init
        try:
            flow = m._predict_final(image1, frame, pipelined=False, video=self)
        finally:
            self.route = self.flow_init = None
        self._frame = frame[-k:]
        # (a copy: the state is the model's, and its next call of any kind overwrites it)
        self.flow_low = m._state.flow.clone()
        return flow

    @staticmethod
    def _check_init(flow_init, frame):
        t = image_ops._on_device(flow_init)
        want = (frame.shape[0], frame.shape[1] // 8, frame.shape[2] // 8, 2)
        if tuple(t.shape) != want or t.dtype != torch.float32 or t.device != frame.device:
            raise ValueError(f'flow_init must be a float32 flow {want} in model space, got {tuple(t.shape)} {t.dtype}')
        return t


def predict_video(model, frames, warm_start=False, batch_size=None, steps=None):
    """``RAFT.predict_video``: the flows between the consecutive frames of ONE video ``(T, H, W, 3)``, host or device, as a host
    array ``(T - 1, H, W, 2)``.  ``warm_start=True`` pushes frame by frame (pair t + 1 starts from pair t's flow: the dependency
    is real); otherwise ``batch_size`` consecutive pairs (default 4) run per call, the feature encoder on the ``batch_size`` new
    frames of the chunk.  ``steps`` limits the number of calls.  Host frames are uploaded one chunk ahead of the compute stream
    (``tf_raft_amd.prefetch``); every call's flows are copied back synchronously."""
    from .prefetch import prefetch_to_device
    shape = tuple(frames.shape) if hasattr(frames, 'shape') else np.shape(frames)
    if len(shape) != 4 or shape[-1] != 3:
        raise ValueError(f'frames must be one video (T, H, W, 3), got {shape}')
    T = shape[0]
    if T < 2:
        raise ValueError(f'a video needs at least two frames, got T = {T}')
    bs = 1 if warm_start else (int(batch_size) if batch_size else 4)
    if bs < 1:
        raise ValueError(f'batch_size must be >= 1, got {batch_size}')
    dev = _dev.require_gpu()
    starts = list(range(1, T, bs))
    if steps is not None:
        starts = starts[:int(steps)]
    # (prefetch_to_device takes batches that are tuples of arrays)
    chunks = ((frames[a:b],) for a, b in [(0, 1)] + [(s, min(s + bs, T)) for s in starts])
    video = FlowVideo(model, warm_start)
    flows = []
    for (chunk,) in prefetch_to_device(chunks, buffer_size=1, device=dev):
        flow = video._step(chunk, chunk.shape[0])
        if flow is not None:
            flows.append(flow.as_subclass(torch.Tensor).cpu().numpy())
    if not flows:
        raise ValueError('predict_video() ran no pair')
    return np.concatenate(flows, axis=0)


def _detect_frames(t):
    """Device frames as the detector takes them: uint8 and float32 as they are, any other type as float32."""
    t = t.detach().as_subclass(torch.Tensor)
    return (t if t.dtype in (torch.uint8, torch.float32) else t.to(torch.float32)).contiguous()


def _check_seeding(points, start, max_points, replenish, detect, lead):
    """The arguments ``points=None`` / ``max_points`` / ``replenish`` / ``detect`` of the tracker and of ``track_video``, checked
    before anything reaches a device: ``(K of the detections or None, detect options without the mask, the mask)``."""
    if not isinstance(replenish, (bool, np.bool_)):
        raise ValueError(f'replenish must be True or False, got {replenish!r}')
    if max_points is not None:
        image_ops.check_detect_args(max_points)
    if points is None:
        if max_points is None:
            raise ValueError('points=None asks the tracker to detect its points: pass max_points=K with it')
        if start is not None:
            raise ValueError('start belongs to given points: detected points begin at the first frame')
        K = int(max_points)
    else:
        K = int(max_points) if max_points is not None else min(lead[-1], image_ops.DETECT_MAX_POINTS)
    if points is not None and not replenish:
        if detect is not None:
            raise ValueError('detect belongs to points=None or replenish=True')
        return None, {}, None
    options = image_ops.check_detect_options(detect, K)
    mask = options.pop('mask', None)
    return K, options, mask


def _check_detect_mask(mask, shape3):
    """The detector's mask against frames of ``shape3 = (N, H, W)``, by shape alone (nothing reaches a device)."""
    if mask is not None:
        mshape, _ = image_ops._shape_and_type(mask, 'detect')
        if tuple(mshape) != tuple(shape3):
            raise ValueError(f'the mask of detect must be {tuple(shape3)} for these frames, got {tuple(mshape)}')


def _detect_mask(mask, shape3):
    """The detector's mask on the device; a wrong shape fails before any launch."""
    _check_detect_mask(mask, shape3)
    return image_ops._mask_on_device(mask, tuple(shape3))


class FlowTracker:
    """``model.tracker(points, start=None, consistency=True, warm_start=False, alpha=..., beta=...)``: ``points`` ``(N, P, 2)``
    float32 are ``(x, y)`` in pixels of the frames' own size, ``P`` query points in each of N videos.  ``push(frames)`` takes one
    frame ``(N, H, W, 3)`` of each video and returns ``(positions (N, P, 2) float32, lost (N, P) uint8)`` as device tensors: where
    every point is in THESE frames (None after the first push, whose frames the points are given in unless ``start`` says
    otherwise).  ``lost``: 0 = tracked, 1 = left the frame, 2 = failed the forward-backward test; a lost point stays lost at the
    position it was last tracked at (``image_ops.track``).  ``start`` (integers ``(N, P)``): the index of the pushed frame a
    point is given in; it waits there, untouched, until that frame has been pushed.

    ``consistency=True`` keeps the previous frames and runs ``predict_step_bidirectional((previous, frames))`` per push, so a
    frame is encoded twice over its life; ``consistency=False`` rides on ``FlowVideo(model, warm_start)`` (every frame encoded
    once) and tests only the frame borders.  It chains the flows the predictor RETURNS, at the frames' own size, so it works
    with every ``target_size`` / ``fit``.  ``reset()`` goes back to the given points and forgets the stream.

    ``points=None`` with ``max_points=K``: the first pushed frames are run through
    ``image_ops.detect_points`` with the options of ``detect=dict(min_distance, quality_level, block_radius, method, harris_k,
    border, mask)``; ``P = K``, N is learned at that push, and the slots the detector could not fill carry the code 3 (empty) at
    ``(-1, -1)``.  ``replenish=True``: after every push's track launch the pushed frames are run through the detector, with the
    tracker's live points as ``avoid`` and the same ``min_distance``, and the new points fill the slots with a nonzero code in
    ascending slot order, strongest point first (``image_ops.refill_points_launch``); the tracker then has ``.ids`` and ``.born``
    ``(N, P)`` int32 device tensors: the identity of the point a slot holds (the given points are 0 .. P - 1, every refill takes
    the next number of its video, an empty slot has -1) and the index of the pushed frame it came in at (``start`` or 0 for the
    given points).  With given ``points`` ``P`` is theirs; ``max_points`` then only limits a push's detections (default
    ``min(P, 4096)``).  Detection runs on the caller's frames at their own size and touches neither the predictor nor its
    schedule."""

    def __init__(self, model, points, start=None, consistency=True, warm_start=False, alpha=image_ops.CONSISTENCY_ALPHA,
                 beta=image_ops.CONSISTENCY_BETA, max_points=None, replenish=False, detect=None):
        self.alpha, self.beta = image_ops.check_consistency_args(alpha, beta)
        self.consistency = bool(consistency)
        if self.consistency and warm_start:
            raise ValueError('warm_start belongs to the one-directional stream: pass consistency=False with it')
        self._lead = None if points is None else image_ops._points_ahead(points, None, start, 'tracker')
        self._K, self._detect, self._mask = _check_seeding(points, start, max_points, replenish, detect, self._lead)
        self.replenish = bool(replenish)
        self.model = model
        self._video = None if self.consistency else FlowVideo(model, warm_start)
        self._given, self._given_start = points, start
        self._points = self._start = None         # on the device from the first push on
        self.reset()

    def reset(self):
        self._signature = None
        self._previous = None                    # consistency: the last frames, as they came
        self._pos = self._lost = None
        self.ids = self.born = self._next_id = self._mask_dev = None
        self._t = 0                              # frames pushed so far
        if self._video is not None:
            self._video.reset()

    def _seed(self, frames):
        """The first push of a tracker that detects or replenishes: the state, and who is in it."""
        if self._given is None:
            self._pos, _, _, self._lost = image_ops.detect_points_launch(frames, self._K, mask=self._mask_dev, want_lost=True,
                                                                         **self._detect)
        if self.replenish:
            if self._lost is None:
                self._lost = torch.zeros(self._points.shape[:2], device=self._points.device, dtype=torch.uint8)
            self.born, self.ids, self._next_id = image_ops.tracker_ids(self._lost, self._start)

    def push(self, frames):
        shape = tuple(frames.shape) if hasattr(frames, 'shape') else np.shape(frames)
        dtype = frames.dtype if hasattr(frames, 'dtype') else np.asarray(frames).dtype
        if self._lead is None:
            if len(shape) != 4 or shape[-1] != 3 or 0 in shape:
                raise ValueError(f'frames must be (N, H, W, 3), one frame per video, got {shape}')
        elif len(shape) != 4 or shape[-1] != 3 or 0 in shape or shape[0] != self._lead[0]:
            raise ValueError(f'frames must be (N, H, W, 3) with N = {self._lead[0]}, one frame per video of the points, got {shape}')
        signature = shape[:3] + (str(dtype).replace('torch.', ''),)
        if self._signature is not None and signature != self._signature:
            raise ValueError(f'this tracker holds frames (N, H, W, type) = {self._signature}, got {signature}: reset() it first')
        seeding = self._K is not None
        if seeding and self._signature is None:
            self._mask_dev = _detect_mask(self._mask, shape[:3])
        if self._points is None and self._given is not None:
            self._points = image_ops._on_device(self._given)
            self._start = image_ops._start_on_device(self._given_start, self._lead)
        forward = backward = None
        if self.consistency or seeding:
            frames = image_ops._on_device(frames)
        if self.consistency:
            if self._previous is not None:
                res = self.model.predict_step_bidirectional((self._previous, frames), self.alpha, self.beta)
                forward, backward = res.forward.as_subclass(torch.Tensor), res.backward.as_subclass(torch.Tensor)
            self._previous = frames
        else:
            flow = self._video.push(frames)
            forward = None if flow is None else flow.as_subclass(torch.Tensor)
        first = self._signature is None
        self._signature = signature
        self._t += 1
        if seeding and first:
            self._seed(_detect_frames(frames))
        if forward is None:
            return None
        pos, lost = image_ops.track_launch(self._points if self._pos is None else self._pos, forward[None],
                                           None if backward is None else backward[None], self._lost,
                                           self.born if self.replenish else self._start, self._t - 2, self.alpha, self.beta)
        self._pos, self._lost = pos[0], lost[0]
        if self.replenish:
            new, _, count, _ = image_ops.detect_points_launch(_detect_frames(frames), self._K, mask=self._mask_dev,
                                                              avoid=(self._pos, self._lost), **self._detect)
            image_ops.refill_points_launch(self._pos, self._lost, new, count, self._t - 1, self.born, self.ids, self._next_id,
                                           out=(self._pos, self._lost))
        return _dev.wrap(self._pos), _dev.wrap(self._lost)


def _as_3x3(m):
    g = np.zeros(m.shape[:-2] + (3, 3), np.float64)
    g[..., :2, :] = m
    g[..., 2, 2] = 1.0
    return g


def smooth_trajectory(motions, radius=15, sigma=None):
    """The corrections that steady a camera path (host only, float64 NumPy): ``motions`` ``(T - 1, 2, 3)`` are
    the maps of consecutive frame pairs, frame ``t`` to frame ``t + 1`` in pixels (``image_ops.fit_motion``) -> ``(T, 2, 3)``, one
    correction per frame.  With the path ``G_0 = I``, ``G_t = M_{t-1} G_{t-1}`` (3 x 3 products: where a pixel of frame 0 is in
    frame ``t``), the steadied path ``S_t`` is the mean of ``G_s`` over ``|s - t| <= radius`` with the weights ``exp(-(s - t)^2 /
    (2 sigma^2))``, renormalised where the window leaves the video (``sigma`` defaults to ``radius / 2``), and correction ``t`` is
    ``G_t S_t^-1``: the map from a pixel of the steadied frame to the position in frame ``t`` that it shows, the ``p = M q + o`` of
    ``image_ops.view_frames``.  The mean is taken entry by entry, which is a choice (it is exact for translations and a first-order
    one for rotations and zooms that vary little within a window), not a derived optimum.  Where ``S_t`` equals ``G_t`` entry for
    entry -- always with ``radius=0`` -- the correction is the identity exactly."""
    m = np.asarray(motions, dtype=np.float64)
    if m.ndim != 3 or m.shape[1:] != (2, 3):
        raise ValueError(f'motions must be (T - 1, 2, 3), got {m.shape}')
    if not np.isfinite(m).all():
        raise ValueError('motions must be finite')
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or radius < 0:
        raise ValueError(f'radius must be an integer >= 0, got {radius!r}')
    radius = int(radius)
    if sigma is None:
        sigma = radius / 2.0
    elif isinstance(sigma, (bool, np.bool_)) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not (
            float(sigma) > 0.0 and np.isfinite(float(sigma))):
        raise ValueError(f'sigma must be positive and finite, got {sigma!r}')
    sigma = float(sigma)
    T = m.shape[0] + 1
    step = _as_3x3(m)
    path = np.empty((T, 3, 3), np.float64)
    path[0] = np.eye(3)
    for t in range(1, T):
        path[t] = step[t - 1] @ path[t - 1]
    out = np.empty((T, 2, 3), np.float64)
    for t in range(T):
        lo, hi = max(t - radius, 0), min(t + radius, T - 1)
        k = np.arange(lo, hi + 1, dtype=np.float64) - t
        w = np.exp(-(k * k) / (2.0 * sigma * sigma)) if radius > 0 else np.ones(1)
        # (the mean as G_t plus the mean deviation from it: a path that stands still is its own mean to the last bit)
        steady = path[t] + np.tensordot(w, path[lo:hi + 1] - path[t], axes=1) / w.sum()
        if np.array_equal(steady, path[t]):
            out[t] = np.eye(3)[:2]
        else:
            out[t] = (path[t] @ np.linalg.inv(steady))[:2]
    return out


def stabilize_video(model, frames, motion_model='similarity', radius=15, iterations=image_ops.MOTION_ITERATIONS,
                    scale=image_ops.MOTION_SCALE, batch_size=4, occlusion_test='consistency', return_motion=False):
    """``RAFT.stabilize_video``: ONE video ``(T, H, W, 3)``, host or device, uint8 or float32 on 0 .. 255 -> the steadied video as a
    host array of the same shape and type (and with ``return_motion=True`` the fitted motions ``(T - 1, 2, 3)`` float32 and the
    corrections ``(T, 2, 3)`` float64).  ``batch_size`` consecutive pairs run per call (``predict_step_bidirectional`` with
    ``occlusion_test``), each forward flow is fitted on the device with its ``occluded_forward`` mask left out
    (``image_ops.fit_motion_launch``: ``motion_model``, ``iterations``, ``scale``), the motions come to the host in ONE copy,
    ``smooth_trajectory(motions, radius)`` steadies the path there, and every frame is resampled bilinearly under its correction
    (``image_ops.view_frames_launch``), pixels from outside the frame 0.  uint8 frames are rounded (half to even) and clipped back
    to uint8.  The frames stay on the device between the two passes.  Nothing is claimed about how the result looks."""
    from .prefetch import prefetch_to_device
    image_ops.check_motion_args(motion_model, iterations, scale)
    occlusion_test = image_ops.check_occlusion_test(occlusion_test)
    shape, dtype = image_ops._frames_ahead(frames, 'stabilize_video')
    if len(shape) != 4 or shape[-1] != 3:
        raise ValueError(f'frames must be one video (T, H, W, 3), got {shape}')
    T, H, W, _ = shape
    if T < 2:
        raise ValueError(f'a video needs at least two frames, got T = {T}')
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or radius < 0:
        raise ValueError(f'radius must be an integer >= 0, got {radius!r}')
    if isinstance(batch_size, (bool, np.bool_)) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError(f'batch_size must be an integer >= 1, got {batch_size!r}')
    bs = int(batch_size)
    dev = _dev.require_gpu()
    motions = torch.empty((T - 1, 2, 3), device=dev, dtype=torch.float32)
    chunks = ((frames[a:b],) for a, b in [(0, 1)] + [(s, min(s + bs, T)) for s in range(1, T, bs)])
    kept, t = [], 0
    for (chunk,) in prefetch_to_device(chunks, buffer_size=1, device=dev):
        chunk = image_ops._on_device(chunk)
        if kept:
            both = torch.cat([kept[-1][-1:], chunk], dim=0)
            res = model.predict_step_bidirectional((both[:-1], both[1:]), occlusion_test=occlusion_test)
            fit, _ = image_ops.fit_motion_launch(res.forward.as_subclass(torch.Tensor), res.occluded_forward.as_subclass(torch.Tensor),
                                                 True, motion_model, iterations, scale)
            motions[t:t + chunk.shape[0]] = fit
            t += chunk.shape[0]
        kept.append(chunk)
    host_motions = motions.cpu().numpy()                        # the one download
    corrections = smooth_trajectory(host_motions, radius)
    out = np.empty(shape, np.uint8 if dtype == torch.uint8 else np.float32)
    t = 0
    for chunk in kept:
        k = chunk.shape[0]
        records = image_ops.view_records(image_ops.MotionViews(corrections[t:t + k]), k, dev)
        seen = image_ops.view_frames_launch(chunk.to(torch.float32), records, (H, W))
        if dtype == torch.uint8:
            seen = seen.round_().clamp_(0, 255).to(torch.uint8)
        out[t:t + k] = seen.cpu().numpy()
        t += k
    return (out, host_motions, corrections) if return_motion else out


def track_video(model, frames, points, start=None, consistency=True, batch_size=4, alpha=image_ops.CONSISTENCY_ALPHA,
                beta=image_ops.CONSISTENCY_BETA, max_points=None, replenish=False, detect=None):
    """``RAFT.track_video``: ``points`` ``(P, 2)`` float32, ``(x, y)`` in pixels, followed through ONE video ``(T, H, W, 3)``,
    host or device -> host arrays ``(positions (T, P, 2) float32, lost (T, P) uint8)``: row ``t`` says where every point is in
    frame ``t`` (row 0: the points themselves; a point with ``start[p] = k`` holds its given position in rows ``0 .. k``).
    ``batch_size`` consecutive pairs run per call (``predict_step_bidirectional``; with ``consistency=False`` a ``FlowVideo``
    call, every frame encoded once, only the frame borders tested) and ONE ``image_ops.track_launch`` chains the call's pairs,
    positions and codes carried from call to call.  Host frames are uploaded one chunk ahead of the compute stream.

    ``points=None`` with ``max_points=K``: frame 0 is run through ``image_ops.detect_points`` with the
    options of ``detect=dict(...)`` (its ``mask`` is ``(1, H, W)``); ``P = K`` and the slots the detector could not fill hold the
    code 3 and ``(-1, -1)`` in every row.  ``replenish=True`` also returns ``ids (T, P)`` int32, the identity of the point a slot
    holds in every row (``FlowTracker``): lost slots are refilled from a detection on the LAST frame of every call, so a slot is
    refilled only at a chunk boundary, every ``batch_size`` frames, and stays lost within a chunk -- one track launch still
    chains a chunk."""
    from .prefetch import prefetch_to_device
    alpha, beta = image_ops.check_consistency_args(alpha, beta)
    shape = tuple(frames.shape) if hasattr(frames, 'shape') else np.shape(frames)
    if len(shape) != 4 or shape[-1] != 3:
        raise ValueError(f'frames must be one video (T, H, W, 3), got {shape}')
    T = shape[0]
    if T < 2:
        raise ValueError(f'a video needs at least two frames, got T = {T}')
    lead = None if points is None else image_ops._points_ahead(points, None, start, 'track_video', lead=1)
    K, options, mask = _check_seeding(points, start, max_points, replenish, detect, lead)
    P = K if points is None else lead[0]
    if isinstance(batch_size, (bool, np.bool_)) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError(f'batch_size must be an integer >= 1, got {batch_size!r}')
    bs = int(batch_size)
    _check_detect_mask(mask, (1,) + shape[1:3])
    dev = _dev.require_gpu()
    mask = image_ops._mask_on_device(mask, (1,) + shape[1:3])
    begin = image_ops._start_on_device(start, (1, P))
    pos = torch.empty((T, 1, P, 2), device=dev, dtype=torch.float32)
    lost = torch.zeros((T, 1, P), device=dev, dtype=torch.uint8)
    if points is not None:
        pos[0] = image_ops._on_device(points).reshape(1, P, 2)
    ids = ids_now = next_id = None
    video = None if consistency else FlowVideo(model, False)
    # a chunk holds the new frames of a call; the call's first frame is the one before them
    chunks = ((frames[a:b],) for a, b in [(0, 1)] + [(s, min(s + bs, T)) for s in range(1, T, bs)])
    previous, t = None, 0                        # the last frame of the chunk before, and its index
    for (chunk,) in prefetch_to_device(chunks, buffer_size=1, device=dev):
        k = chunk.shape[0]
        if previous is None:                                                      # frame 0
            if points is None:
                image_ops.detect_points_launch(_detect_frames(chunk), K, mask=mask, want_lost=True, out=(pos[0], None, None, lost[0]),
                                               **options)
            if replenish:
                begin, ids_now, next_id = image_ops.tracker_ids(lost[0], begin)
                ids = torch.empty((T, 1, P), device=dev, dtype=torch.int32)
                ids[0] = ids_now
        if video is not None:
            forward, backward = video._step(chunk, k), None
        elif previous is None:
            forward = backward = None
        else:
            both = torch.cat([previous, chunk], dim=0)
            res = model.predict_step_bidirectional((both[:-1], both[1:]), alpha, beta)
            forward, backward = res.forward, res.backward
        previous = chunk[-1:]
        if forward is None:
            continue
        forward = forward.as_subclass(torch.Tensor)[:, None]
        backward = None if backward is None else backward.as_subclass(torch.Tensor)[:, None]
        image_ops.track_launch(pos[t], forward, backward, lost[t], begin, t, alpha, beta, out=(pos[t + 1:t + 1 + k], lost[t + 1:t + 1 + k]))
        t += k
        if replenish:
            ids[t - k + 1:t] = ids_now                   # within the chunk nobody came in
            new, _, count, _ = image_ops.detect_points_launch(_detect_frames(chunk[-1:]), K, mask=mask, avoid=(pos[t], lost[t]), **options)
            image_ops.refill_points_launch(pos[t], lost[t], new, count, t, begin, ids_now, next_id, out=(pos[t], lost[t]))
            ids[t] = ids_now
    if replenish:
        return pos[:, 0].cpu().numpy(), lost[:, 0].cpu().numpy(), ids[:, 0].cpu().numpy()
    return pos[:, 0].cpu().numpy(), lost[:, 0].cpu().numpy()


def check_denoise_args(frames, radius=2, batch_size=4):
    """What ``denoise_video`` asks of its video, ``radius`` and ``batch_size`` before anything reaches a device: ``(shape, torch
    type of the frames, radius, batch_size)``.  ``radius`` is an integer in 1 .. 8 (``2 * radius`` neighbours, at most the 16 of
    one fuse launch)."""
    shape, _ = image_ops._shape_and_type(frames, 'denoise_video')
    if len(shape) != 4 or shape[-1] != 3:
        raise ValueError(f'frames must be one video (T, H, W, 3), got {shape}')
    shape, dtype = image_ops._frames_ahead(frames, 'denoise_video')
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or \
            not 1 <= radius <= image_ops.FUSE_MAX_NEIGHBOURS // 2:
        raise ValueError(f'radius must be an integer in 1 .. {image_ops.FUSE_MAX_NEIGHBOURS // 2}, got {radius!r}')
    if isinstance(batch_size, (bool, np.bool_)) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError(f'batch_size must be an integer >= 1, got {batch_size!r}')
    return shape, dtype, int(radius), int(batch_size)


def denoise_neighbours(t, T, radius):
    """The frames that frame ``t`` of a ``T``-frame video is fused with, in the order of the launch: ``t - 1, t - 2, ...`` down to
    ``max(t - radius, 0)``, then ``t + 1, t + 2, ...`` up to ``min(t + radius, T - 1)``; fewer at the ends of the video."""
    return list(range(t - 1, max(t - radius, 0) - 1, -1)) + list(range(t + 1, min(t + radius, T - 1) + 1))


def denoise_video(model, frames, radius=2, sigma=image_ops.FUSE_SIGMA, patch_radius=image_ops.FUSE_PATCH_RADIUS,
                  center_weight=image_ops.FUSE_CENTER_WEIGHT, batch_size=4):
    """``RAFT.denoise_video``: ONE video ``(T, H, W, 3)``, host or device, uint8 or float32 on 0 .. 255 -> the video filtered along
    its motion, a host array of the same shape and type.  ``T - 1`` bidirectional passes, ``batch_size``
    consecutive pairs per ``predict_step_bidirectional`` call, give the flows ``t -> t + 1`` and ``t + 1 -> t``; host frames are
    uploaded one chunk ahead of the compute stream.  The frames, both flows and the result stay on the device until the one
    download at the end: ``T * H * W * 3`` elements of the frames' type twice and ``2 * (T - 1) * H * W * 8`` bytes of flows (a
    100-frame 448 x 512 uint8 video: 138 MB of frames and results, 363 MB of flows).  For frame ``t`` the dense ``point_grid(H, W)``
    is chained through the frames ``t - 1 .. t - radius`` (``image_ops.track_launch`` with the backward flows, tested against the
    forward flows) and through ``t + 1 .. t + radius`` (the roles swapped), one launch each way; the positions go into ONE
    ``image_ops.fuse_frames_launch`` as they are (``absolute``), ``track``'s lost codes as its ``skip``, and the neighbours are
    read from the video where they lie (``denoise_neighbours``: fewer at the ends of the video).  ``T == 1`` returns the frame.
    ``radius``, ``sigma``, ``patch_radius`` and ``center_weight`` are choices, not tuned values, and nothing is claimed about
    picture quality on real footage."""
    from .prefetch import prefetch_to_device
    image_ops.check_fuse_args(sigma, patch_radius, center_weight)
    shape, dtype, radius, bs = check_denoise_args(frames, radius, batch_size)
    T, H, W, _ = shape
    image_ops._check_fuse_sizes(2 * radius, 1, H, W, 3, 'denoise_video')
    if T == 1:
        host = frames.detach().cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
        return np.array(host, dtype=np.uint8 if dtype == torch.uint8 else np.float32)
    dev = _dev.require_gpu()
    video = torch.empty(shape, device=dev, dtype=dtype)
    forward = torch.empty((T - 1, 1, H, W, 2), device=dev, dtype=torch.float32)       # t -> t + 1
    backward = torch.empty((T - 1, 1, H, W, 2), device=dev, dtype=torch.float32)      # t + 1 -> t
    chunks = ((frames[a:b],) for a, b in [(0, 1)] + [(s, min(s + bs, T)) for s in range(1, T, bs)])
    t = 0
    for (chunk,) in prefetch_to_device(chunks, buffer_size=1, device=dev):
        k = chunk.shape[0]
        video[t:t + k] = image_ops._on_device(chunk)
        if t:
            res = model.predict_step_bidirectional((video[t - 1:t + k - 1], video[t:t + k]))
            forward[t - 1:t + k - 1, 0] = res.forward.as_subclass(torch.Tensor)
            backward[t - 1:t + k - 1, 0] = res.backward.as_subclass(torch.Tensor)
        t += k
    grid = torch.from_numpy(image_ops.point_grid(H, W).copy()).to(dev)
    stack = video.view(T, 1, H, W, 3)
    positions = torch.empty((2 * radius, 1, H * W, 2), device=dev, dtype=torch.float32)
    lost = torch.empty((2 * radius, 1, H * W), device=dev, dtype=torch.uint8)
    out = torch.empty(shape, device=dev, dtype=dtype)
    for t in range(T):
        back, ahead = min(radius, t), min(radius, T - 1 - t)
        if back:            # step s goes from frame t - s to t - s - 1 along backward[t - s - 1]
            image_ops.track_launch(grid, backward[t - back:t].flip(0), forward[t - back:t].flip(0), out=(positions[:back], lost[:back]))
        if ahead:
            image_ops.track_launch(grid, forward[t:t + ahead], backward[t:t + ahead],
                                   out=(positions[back:back + ahead], lost[back:back + ahead]))
        K = back + ahead
        image_ops.fuse_frames_launch(stack[t], stack, positions[:K].view(K, 1, H, W, 2), denoise_neighbours(t, T, radius),
                                     lost[:K].view(K, 1, H, W), True, sigma, patch_radius, center_weight, out=out[t:t + 1])
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------ object identity
_OBJECT_STEP_OPTIONS = ('model', 'threshold', 'min_area', 'connectivity', 'occlusion_test', 'iterations', 'scale', 'alpha', 'beta',
                        'range_threshold')


class TrackedObjects(NamedTuple):
    """What ``ObjectTracker.push`` returns: the twelve fields of ``MovingObjects`` for the pair (previous frames, pushed frames),
    then per slot ``(N, K)`` int32: ``ids`` the identity of the object the slot holds (-1: empty), ``born`` the index of the pushed
    frame its identity first appeared in, ``match`` the slot it held in the pair before (-1: a new object) and ``origin`` the slot
    of the pair before most of whose pixels landed on it (-1: none; after a split, the object that was divided)."""
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
    ids: object
    born: object
    match: object
    origin: object


class ObjectTracks(NamedTuple):
    """What ``track_objects_video`` returns, host arrays over the ``T - 1`` pairs of a video: ``count`` ``(T - 1,)``, ``ids``,
    ``born``, ``area`` ``(T - 1, K)`` int32, ``boxes`` ``(T - 1, K, 4)`` int32, ``centroid`` and ``mean_flow`` ``(T - 1, K, 2)``
    float32, and ``labels`` ``(T - 1, H, W)`` int32 (None without ``return_labels``).  Row ``t`` holds the objects of frame ``t``."""
    count: object
    ids: object
    born: object
    area: object
    boxes: object
    centroid: object
    mean_flow: object
    labels: object


def check_object_tracker_args(max_objects=64, min_overlap=image_ops.OBJECT_MIN_OVERLAP, options=None):
    """What ``ObjectTracker`` and ``track_objects_video`` ask of their arguments before anything reaches a device: ``(K,
    min_overlap, options)`` with ``options`` the keyword arguments of ``RAFT.moving_objects_step`` other than ``max_objects``."""
    K, share = image_ops.check_object_track_args(max_objects, min_overlap)
    options = dict(options or {})
    unknown = set(options) - set(_OBJECT_STEP_OPTIONS)
    if unknown:
        raise TypeError(f'unexpected keyword arguments {sorted(unknown)}: the options of moving_objects_step are {_OBJECT_STEP_OPTIONS}')
    image_ops.check_objects_args(K, options.get('min_area', image_ops.OBJECTS_MIN_AREA),
                                 options.get('connectivity', image_ops.OBJECTS_CONNECTIVITY))
    image_ops.check_motion_args(options.get('model', 'affine'), options.get('iterations', image_ops.MOTION_ITERATIONS),
                                options.get('scale', image_ops.MOTION_SCALE))
    if image_ops.check_motion_threshold(options.get('threshold', 1.0)) is None:
        raise ValueError('threshold must be a number, got None')
    image_ops.check_occlusion_test(options.get('occlusion_test', 'consistency'))
    return K, share, options


def _plain(t):
    return t.as_subclass(torch.Tensor).contiguous()


class ObjectTracker:
    """``model.object_tracker(max_objects=64, min_overlap=0.25, **moving_objects_step options)``: the moving objects of a stream
    of frames with identities that last.  ``push(frames)`` takes one frame ``(N, H, W, 3)`` of each of N
    independent videos (uint8 or float32, host or device), keeps the previous frames as ``FlowTracker(consistency=True)`` does and
    runs ONE ``moving_objects_step((previous, frames))`` per push.  It returns None after the first push, then ``TrackedObjects``:
    the fields of ``MovingObjects``, then ``ids``, ``born``, ``match`` and ``origin`` ``(N, K)`` int32, all device tensors, nothing
    synchronised.  As with ``moving_objects_step`` the objects are those of the PREVIOUS pushed frame, in its coordinates: the
    pair's flow says what moves in its first frame.

    The second push numbers its objects ``0 .. count - 1``.  From the third push on the labels and the forward flow kept from the
    pair before are matched against the new labels (``image_ops.object_overlap_launch`` / ``match_objects_launch``): a matched
    object keeps its id and ``born``, an unmatched one takes the next id of its video (``image_ops.chain_object_ids_launch``);
    ids never repeat within a video.  There is no memory beyond one pair: an object that is missed in one pair comes back under a
    new id.  ``reset()`` forgets the stream; a change of shape or type without it raises.  ``min_overlap``, the nearest-pixel
    landing and the greedy one-to-one rule are choices, not tuned values."""

    def __init__(self, predictor, max_objects=64, min_overlap=image_ops.OBJECT_MIN_OVERLAP, **options):       # (`model` is an option)
        self.max_objects, self.min_overlap, self._options = check_object_tracker_args(max_objects, min_overlap, options)
        self.model = predictor
        self.reset()

    def reset(self):
        self._signature = None
        self._previous = None                    # the last frames, as they came
        self._labels = self._forward = None      # of the pair before: labels in its first frame, the flow into its second
        self.ids = self.born = self._next_id = None
        self._t = 0                              # frames pushed so far

    def push(self, frames):
        shape = tuple(frames.shape) if hasattr(frames, 'shape') else np.shape(frames)
        dtype = frames.dtype if hasattr(frames, 'dtype') else np.asarray(frames).dtype
        if len(shape) != 4 or shape[-1] != 3 or 0 in shape:
            raise ValueError(f'frames must be (N, H, W, 3), one frame per video, got {shape}')
        signature = shape[:3] + (str(dtype).replace('torch.', ''),)
        if self._signature is not None and signature != self._signature:
            raise ValueError(f'this tracker holds frames (N, H, W, type) = {self._signature}, got {signature}: reset() it first')
        frames = image_ops._on_device(frames)
        previous, self._previous = self._previous, frames
        self._signature = signature
        self._t += 1
        if previous is None:
            return None
        K, N, dev = self.max_objects, shape[0], frames.device
        res = self.model.moving_objects_step((previous, frames), max_objects=K, **self._options)
        labels, count, area, forward = _plain(res.labels), _plain(res.count), _plain(res.area), _plain(res.forward)
        if self._labels is None:                 # the first pair: everybody is new
            match = torch.full((N, K), -1, device=dev, dtype=torch.int32)
            origin = match.clone()
            self.ids, self.born = match.clone(), match.clone()
            self._next_id = torch.zeros((N,), device=dev, dtype=torch.int32)
        else:
            overlap, landed = image_ops.object_overlap_launch(self._labels, self._forward, labels, K)
            match, _, origin = image_ops.match_objects_launch(overlap, landed, area, self.min_overlap, want_overlap=False)
        ids, born = image_ops.chain_object_ids_launch(match[None], count[None], self._t - 2, self.ids, self.born, self._next_id)
        self.ids, self.born = ids[0], born[0]    # (new tensors every push: what an earlier push returned stays as it was)
        self._labels, self._forward = labels, forward
        return TrackedObjects(*res, _dev.wrap(self.ids), _dev.wrap(self.born), _dev.wrap(match), _dev.wrap(origin))


def track_objects_video(predictor, frames, batch_size=4, max_objects=64, min_overlap=image_ops.OBJECT_MIN_OVERLAP, return_labels=False,
                        **options):
    """``RAFT.track_objects_video``: the moving objects of ONE video ``(T, H, W, 3)``, host or device, with identities that last
    -> ``ObjectTracks`` of host arrays over its ``T - 1`` pairs (row ``t``: the objects of frame ``t``, from the pair ``t, t + 1``).
    Every pair goes through a ``moving_objects_step`` call OF ITS OWN (its options go in as keywords): the predictor's launch plans
    choose kernel shapes by batch, so the flow of a pair differs in its last bits with the batch it runs in, and a result that
    must not depend on how the video is cut cannot batch the predictor.  ``batch_size`` is the number of
    consecutive pairs per CHUNK: a chunk's frames are uploaded together, one chunk ahead of the compute stream, and its overlaps
    come from ONE ``image_ops.object_overlap_launch`` -- pair i against pair i + 1 as batch slices, in front of them the pair
    kept from the chunk before -- then one ``match_objects_launch`` and one ``chain_object_ids_launch`` over the chunk's steps.
    Everything is downloaded once, at the end.  The result does not depend on ``batch_size`` and equals an ``ObjectTracker`` fed
    the frames one by one.  Ids are ``ObjectTracker``'s: 0, 1, ... in order of appearance, never reused."""
    from .prefetch import prefetch_to_device
    K, share, options = check_object_tracker_args(max_objects, min_overlap, options)
    shape, _ = image_ops._frames_ahead(frames, 'track_objects_video')
    if len(shape) != 4 or shape[-1] != 3:
        raise ValueError(f'frames must be one video (T, H, W, 3), got {shape}')
    T, H, W, _ = shape
    if T < 2:
        raise ValueError(f'a video needs at least two frames, got T = {T}')
    if isinstance(batch_size, (bool, np.bool_)) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError(f'batch_size must be an integer >= 1, got {batch_size!r}')
    bs, P = int(batch_size), T - 1
    dev = _dev.require_gpu()
    i32 = dict(device=dev, dtype=torch.int32)
    count = torch.empty((P, 1), **i32)
    ids, born = torch.empty((P, 1, K), **i32), torch.empty((P, 1, K), **i32)
    area, boxes = torch.empty((P, K), **i32), torch.empty((P, K, 4), **i32)
    centroid = torch.empty((P, K, 2), device=dev, dtype=torch.float32)
    mean_flow = torch.empty((P, K, 2), device=dev, dtype=torch.float32)
    all_labels = torch.empty((P, H, W), **i32) if return_labels else None
    # slice 0: the last pair of the chunk before; slices 1 .. k: this chunk's pairs
    labels = torch.empty((bs + 1, H, W), **i32)
    flows = torch.empty((bs + 1, H, W, 2), device=dev, dtype=torch.float32)
    state = (torch.full((1, K), -1, **i32), torch.full((1, K), -1, **i32))
    next_id = torch.zeros((1,), **i32)
    chunks = ((frames[a:b],) for a, b in [(0, 1)] + [(s, min(s + bs, T)) for s in range(1, T, bs)])
    previous, p = None, 0                        # the last frame of the chunk before; pairs done so far
    for (chunk,) in prefetch_to_device(chunks, buffer_size=1, device=dev):
        chunk = image_ops._on_device(chunk)
        if previous is None:
            previous = chunk[-1:]
            continue
        k = chunk.shape[0]
        both = torch.cat([previous, chunk], dim=0)
        previous = chunk[-1:]
        for i in range(k):                       # one pair per call: what a pair gives must not depend on its neighbours
            res = predictor.moving_objects_step((both[i:i + 1], both[i + 1:i + 2]), max_objects=K, **options)
            labels[1 + i], flows[1 + i] = _plain(res.labels)[0], _plain(res.forward)[0]
            count[p + i, 0], area[p + i], boxes[p + i] = _plain(res.count)[0], _plain(res.area)[0], _plain(res.boxes)[0]
            centroid[p + i], mean_flow[p + i] = _plain(res.centroid)[0], _plain(res.mean_flow)[0]
        if return_labels:
            all_labels[p:p + k] = labels[1:k + 1]
        first = 1 if p == 0 else 0               # the video's first pair has nothing in front of it
        match = torch.full((k, 1, K), -1, **i32)
        if k - first > 0:
            overlap, landed = image_ops.object_overlap_launch(labels[first:k], flows[first:k], labels[first + 1:k + 1], K)
            match[first:, 0] = image_ops.match_objects_launch(overlap, landed, area[p + first:p + k], share, False, False).match
        image_ops.chain_object_ids_launch(match, count[p:p + k], p, state[0], state[1], next_id, out=(ids[p:p + k], born[p:p + k]))
        state = (ids[p + k - 1], born[p + k - 1])
        labels[0], flows[0] = labels[k], flows[k]
        p += k
    host = lambda t: t.cpu().numpy()             # noqa: E731
    return ObjectTracks(host(count[:, 0]), host(ids[:, 0]), host(born[:, 0]), host(area), host(boxes), host(centroid), host(mean_flow),
                        host(all_labels) if return_labels else None)

"""``FlowAugmentor`` and ``SparseFlowAugmentor`` of reference ``tf_raft/datasets/augmentor.py`` on the device: the augmentation every
training sample of the reference passes through (``dataset.py:87-91``; the sparse one for KITTI and HD1K), without ``cv2`` and
``albumentations``.

The work is split in two.  ``draw`` makes one sample's random decisions on the host, in the reference's order and with the
reference's ``np.random`` calls (so the generator ends in the state the reference leaves it in), and returns them as a record.
``apply`` uploads the records of a batch once and runs two kernels (``tf_raft_amd/csrc/augment.hip``): the channel sums of
colour-mapped frame 2 for the samples whose eraser fired, and the gather that writes both crops, the flow and ``valid``.
Composed, the reference's chain -- colour map, erase, resize, flip, crop, flow factors -- is a gather: every pixel of the crop is a
bilinear blend of four source pixels.  DESIGN.md section 10 states the semantics and says which are executed and which recalled.
The sparse augmentor shares the host code and the frame path; its flow resize, a scatter in the reference, is a gather as well
(DESIGN.md section 11).

The colour-jitter parameters are ``albumentations``' own draws in the reference and do not come from ``np.random``; here they
come from a second generator, ``photo_rng``, by the protocol of ``draw_photo`` -- the first sequence stays aligned.

``StudentView`` / ``StudentTransform`` are not the reference's: they describe and draw the affine view the student pass of a
self-supervised step sees (the gathers are ``image_ops.view_frames`` / ``view_flow``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _dev
from ._ffi import AUGMENT_SUM_BLOCKS, AugmentParams, ViewParams, check
from .image_ops import _on_device

__all__ = ['FlowAugmentor', 'SparseFlowAugmentor', 'PhotoAug', 'draw_photo', 'StudentView', 'StudentTransform']


class PhotoAug:
    """The limits of the reference's ``A.Compose([RandomBrightnessContrast, HueSaturationValue])`` (augmentor.py:27-37); each
    transform fires with its own ``p``."""

    def __init__(self, brightness_limit, contrast_limit, hue_shift_limit, sat_shift_limit, val_shift_limit, p=0.5):
        self.brightness_limit, self.contrast_limit = float(brightness_limit), float(contrast_limit)
        self.hue_shift_limit, self.sat_shift_limit, self.val_shift_limit = hue_shift_limit, sat_shift_limit, val_shift_limit
        self.p = p


def draw_photo(photo_rng, photo_aug):
    """One application of the colour jitter: ``{'bc': None | (alpha, beta), 'hsv': None | (hue, sat, val)}``.

    The protocol (tests/augstub/albumentations follows the same one): ``rand() < p`` decides brightness / contrast, and if it
    fires ``alpha = 1 + uniform(-contrast_limit, contrast_limit)`` then ``beta = uniform(-brightness_limit, brightness_limit)``;
    ``rand() < p`` decides hue / saturation / value, and if it fires the three shifts are ``uniform(-limit, limit)`` in that order."""
    out = {'bc': None, 'hsv': None}
    if photo_rng.rand() < photo_aug.p:
        alpha = 1.0 + photo_rng.uniform(-photo_aug.contrast_limit, photo_aug.contrast_limit)
        beta = 0.0 + photo_rng.uniform(-photo_aug.brightness_limit, photo_aug.brightness_limit)
        out['bc'] = (alpha, beta)
    if photo_rng.rand() < photo_aug.p:
        out['hsv'] = tuple(photo_rng.uniform(-lim, lim) for lim in
                           (photo_aug.hue_shift_limit, photo_aug.sat_shift_limit, photo_aug.val_shift_limit))
    return out


def cv_round(x) -> int:
    """OpenCV's ``cvRound`` of a double: to the nearest integer, halves to even."""
    return int(np.rint(x))


class _Staging:
    """Pinned host buffers for the records of a call.  A buffer is reused only once the copy that read it has completed, which is
    asked of its event without waiting; while every buffer is still in flight a new one is made."""

    def __init__(self):
        self.free = []

    def upload(self, raw: bytes, device) -> torch.Tensor:
        for k, (buf, ev) in enumerate(self.free):
            if buf.numel() >= len(raw) and ev.query():
                del self.free[k]
                break
        else:
            buf, ev = torch.empty(max(len(raw), 4096), dtype=torch.uint8).pin_memory(), torch.cuda.Event()
        C.memmove(buf.data_ptr(), raw, len(raw))
        dev = buf[:len(raw)].to(device, non_blocking=True)
        ev.record(torch.cuda.current_stream(device))
        self.free.append((buf, ev))
        return dev


class _Augmentor:
    """What the two augmentors share on the host: the constructor's common part, the eraser's draws, the record of a sample, the
    argument checks, the staging and the launches.  A subclass draws (``_check_size``, ``_draw_one``) and names its gather."""

    _name = ''
    _gather = ''                # the entry point of the gather
    _label = ''                 # what an error of that entry is reported under

    def _setup(self, crop_size, min_scale, max_scale, do_flip, rng, photo_rng):
        self.crop_size = tuple(int(v) for v in crop_size)
        if len(self.crop_size) != 2 or min(self.crop_size) < 1:
            raise ValueError(f'crop_size must be (height, width) >= 1, got {crop_size!r}')
        self.min_scale = min_scale
        self.max_scale = max_scale
        self.do_flip = do_flip
        self.eraser_bounds = (50, 100)
        self.rng = rng
        self.photo_rng = photo_rng if photo_rng is not None else np.random.RandomState()
        self._staging = _Staging()

    # ------------------------------------------------------------------ host: the draws
    def _draw_rects(self, rng, H, W):
        """eraser_transform (augmentor.py:61-74, 170-181)."""
        rects = []
        if rng.rand() < self.eraser_aug_prob:
            for _ in range(rng.randint(1, 3)):
                x0 = rng.randint(0, W)
                y0 = rng.randint(0, H)
                dx = rng.randint(self.eraser_bounds[0], self.eraser_bounds[1])
                dy = rng.randint(self.eraser_bounds[0], self.eraser_bounds[1])
                rects.append((int(x0), int(y0), int(dx), int(dy)))
        return rects

    def draw(self, H, W, n=1):
        """The parameter records of ``n`` samples of ``H x W`` frames, drawn one sample after the other; touches no device."""
        H, W, n = int(H), int(W), int(n)
        if n < 1:
            raise ValueError(f'n must be >= 1, got {n}')
        self._check_size(H, W)
        return [self._draw_one(H, W) for _ in range(n)]

    # ------------------------------------------------------------------ device: the kernels
    def _check_record(self, p):
        pass

    def _records(self, params, H, W) -> bytes:
        ch, cw = self.crop_size
        recs = (AugmentParams * len(params))()
        for r, p in zip(recs, params):
            if tuple(p['source']) != (H, W):
                raise ValueError(f"a record drawn for {tuple(p['source'])} frames cannot be applied to {H}x{W} frames")
            H1, W1 = p['size']
            if not (0 <= p['y0'] <= H1 - ch and 0 <= p['x0'] <= W1 - cw):
                raise ValueError(f"crop origin ({p['y0']}, {p['x0']}) of a {ch}x{cw} crop lies outside the {H1}x{W1} frame")
            if len(p['rects']) > 2:
                raise ValueError('at most two eraser rectangles per sample')
            self._check_record(p)
            r.resize = int(p['resize'])
            r.fx, r.fy = (p['scale_x'], p['scale_y']) if p['resize'] else (1.0, 1.0)
            r.inv_fx, r.inv_fy = 1.0 / r.fx, 1.0 / r.fy
            r.W1, r.H1, r.x0, r.y0 = W1, H1, p['x0'], p['y0']
            r.flip_h, r.flip_v = int(p['flip_h']), int(p['flip_v'])
            for k, ph in enumerate(p['photo']):
                r.alpha[k], r.beta[k] = 1.0, 0.0
                if ph['bc'] is not None:
                    r.color[k] |= 1
                    r.alpha[k] = np.float32(ph['bc'][0])
                    r.beta[k] = np.float32(ph['bc'][1] * 255)
                if ph['hsv'] is not None:
                    r.color[k] |= 2
                    r.hue[k], r.sat[k], r.val[k] = ph['hsv']
            r.n_rect = len(p['rects'])
            for k, (x0, y0, dx, dy) in enumerate(p['rects']):
                r.rect[k][:] = [x0, y0, min(x0 + dx, W), min(y0 + dy, H)]
        return bytes(recs)

    @classmethod
    def _inputs(cls, img1, img2, flow, *valid):
        """Shape of the frames after the argument checks (``ValueError``); converts nothing."""
        def describe(x):
            if isinstance(x, torch.Tensor):
                return {torch.uint8: 'uint8', torch.float32: 'float32'}.get(x.dtype, str(x.dtype)), tuple(x.shape)
            x = np.asarray(x)
            return x.dtype.name, tuple(x.shape)
        (d1, s1), (d2, s2), (df, sf) = describe(img1), describe(img2), describe(flow)
        if (d1, d2, df) != ('uint8', 'uint8', 'float32'):
            raise ValueError(f'{cls._name} takes uint8 frames and a float32 flow, got {d1}, {d2}, {df}')
        if len(s1) not in (3, 4) or s1[-1] != 3 or sf[-1:] != (2,) or 0 in s1:
            raise ValueError(f'expected (H, W, 3) / (H, W, 2) or (N, H, W, 3) / (N, H, W, 2), got {s1}, {s2}, {sf}')
        if s2 != s1 or sf != s1[:-1] + (2,):
            raise ValueError(f'the frames and the flow of a call share one size, got {s1}, {s2}, {sf}')
        for v in valid:
            dv, sv = describe(v)
            if dv != 'float32':
                raise ValueError(f'{cls._name} takes a float32 validity map, got {dv}')
            if sv != s1[:-1]:
                raise ValueError(f'the validity map has the size of the frames, {s1[:-1]}, got {sv}')
        return s1

    def _run(self, params, img1, img2, flow, *valid):
        shape = self._inputs(img1, img2, flow, *valid)
        single = len(shape) == 3
        N, (H, W) = (1 if single else shape[0]), shape[-3:-1]
        if len(params) != N:
            raise ValueError(f'{len(params)} records for {N} samples')
        raw = self._records(params, H, W)
        ch, cw = self.crop_size
        img1, img2, flow = _on_device(img1), _on_device(img2), _on_device(flow)
        valid = tuple(_on_device(v) for v in valid)
        dev = img1.device
        if any(t.device != dev for t in (img2, flow, *valid)):
            raise ValueError('the frames, the flow and the validity map must be on one device' if valid else
                             'the frames and the flow must be on one device')
        lib = _dev.lib()
        with torch.cuda.device(dev):
            recs = self._staging.upload(raw, dev)
            partial = torch.empty((N, AUGMENT_SUM_BLOCKS, 4), dtype=torch.int32, device=dev)
            out1 = torch.empty((N, ch, cw, 3), dtype=torch.uint8, device=dev)
            out2 = torch.empty((N, ch, cw, 3), dtype=torch.uint8, device=dev)
            oflow = torch.empty((N, ch, cw, 2), dtype=torch.float32, device=dev)
            ovalid = torch.empty((N, ch, cw), dtype=torch.float32, device=dev)
            stream = _dev.stream_ptr()
            if any(p['rects'] for p in params):
                check(lib.raft_augment_sums_u8(_dev.ptr(img2), _dev.ptr(recs), _dev.ptr(partial), N, H, W, stream), 'augment_sums')
            check(getattr(lib, self._gather)(_dev.ptr(img1), _dev.ptr(img2), _dev.ptr(flow), *(_dev.ptr(v) for v in valid), _dev.ptr(recs),
                                             _dev.ptr(partial), _dev.ptr(out1), _dev.ptr(out2), _dev.ptr(oflow), _dev.ptr(ovalid),
                                             N, H, W, ch, cw, stream), self._label)
        outs = (out1, out2, oflow, ovalid)
        return tuple(_dev.wrap(o[0] if single else o) for o in outs)


class FlowAugmentor(_Augmentor):
    """``FlowAugmentor(crop_size, min_scale=-0.2, max_scale=0.5, do_flip=True)``: the reference's constructor, attribute names and
    probabilities (augmentor.py:10-40).

    ``aug(img1, img2, flow)`` -> ``(image1 uint8, image2 uint8, flow float32)`` device tensors at ``crop_size``;
    ``aug.batch(img1, img2, flow)`` -> ``(image1, image2, flow, valid)`` with ``valid`` float32 ``(N, h, w)`` by dataset.py:102 --
    the tuple ``RAFT.train_step`` takes.  Inputs: uint8 ``(H, W, 3)`` and float32 ``(H, W, 2)``, or ``(N, H, W, 3)`` and
    ``(N, H, W, 2)``, NumPy or torch, host or device; the samples of a call share one source size.

    ``rng``: a ``np.random.RandomState``, or None for the global ``np.random`` (what the reference draws from).  A batch is drawn
    sample by sample, so a batch of N equals N reference calls.  ``photo_rng``: the generator of the colour parameters (None: one
    of its own, seeded by the system)."""

    _name = 'FlowAugmentor'
    _gather = 'raft_augment_gather_u8'
    _label = 'augment_gather'

    def __init__(self, crop_size, min_scale=-0.2, max_scale=0.5, do_flip=True, *, rng=None, photo_rng=None):
        self._setup(crop_size, min_scale, max_scale, do_flip, rng, photo_rng)
        # spatial augmentation params
        self.spatial_aug_prob = 0.8
        self.stretch_prob = 0.8
        self.max_stretch = 0.2
        # flip augmentation params
        self.h_flip_prob = 0.5
        self.v_flip_prob = 0.1
        # photometric augmentation params
        self.photo_aug = PhotoAug(brightness_limit=0.4, contrast_limit=0.4, hue_shift_limit=int(0.5 / 3.14 * 180),
                                  sat_shift_limit=int(0.4 * 255), val_shift_limit=int(0.))
        self.asymmetric_color_aug_prob = 0.2
        self.eraser_aug_prob = 0.5

    def _check_size(self, H, W):
        """The crop has to fit the source after the minimum scale.  The resize never goes below ``(crop + 8) / source``, but one
        sample in five is not resized at all and its crop origin is ``randint(0, source - crop)``: the source must be larger than
        the crop on both axes."""
        ch, cw = self.crop_size
        if H <= ch or W <= cw:
            raise ValueError(f'a {ch}x{cw} crop does not fit a {H}x{W} source: the source must be larger on both axes')

    def _draw_one(self, H, W):
        rng = self.rng if self.rng is not None else np.random
        ch, cw = self.crop_size
        # color_transform (augmentor.py:42-59)
        asymmetric = bool(rng.rand() < self.asymmetric_color_aug_prob)
        photo1 = draw_photo(self.photo_rng, self.photo_aug)
        photo2 = draw_photo(self.photo_rng, self.photo_aug) if asymmetric else photo1
        rects = self._draw_rects(rng, H, W)
        # spatial_transform (augmentor.py:76-118)
        min_scale = np.maximum((ch + 8) / float(H), (cw + 8) / float(W))
        scale = 2 ** rng.uniform(self.min_scale, self.max_scale)
        scale_x = scale
        scale_y = scale
        stretch = bool(rng.rand() < self.stretch_prob)
        if stretch:
            scale_x *= 2 ** rng.uniform(-self.max_stretch, self.max_stretch)
            scale_y *= 2 ** rng.uniform(-self.max_stretch, self.max_stretch)
        clipped = bool(scale_x < min_scale or scale_y < min_scale)
        scale_x = np.clip(scale_x, min_scale, None)
        scale_y = np.clip(scale_y, min_scale, None)
        resize = bool(rng.rand() < self.spatial_aug_prob)
        H1, W1 = (cv_round(H * scale_y), cv_round(W * scale_x)) if resize else (H, W)
        flip_h = flip_v = False
        if self.do_flip:
            flip_h = bool(rng.rand() < self.h_flip_prob)
            flip_v = bool(rng.rand() < self.v_flip_prob)
        y0 = int(rng.randint(0, H1 - ch))
        x0 = int(rng.randint(0, W1 - cw))
        return {'asymmetric': asymmetric, 'photo': (photo1, photo2), 'rects': rects, 'scale_x': float(scale_x), 'scale_y': float(scale_y),
                'stretch': stretch, 'clipped': clipped, 'resize': resize, 'size': (H1, W1), 'flip_h': flip_h, 'flip_v': flip_v,
                'y0': y0, 'x0': x0, 'source': (int(H), int(W))}

    def apply(self, params, img1, img2, flow):
        """Run the kernels with given records (one per sample) -> ``(image1, image2, flow, valid)`` on the device, with a leading
        batch axis exactly when the inputs have one.  Current stream; no synchronisation, nothing returns to the host."""
        return self._run(params, img1, img2, flow)

    def batch(self, img1, img2, flow):
        """``(image1, image2, flow, valid)``: what ``RAFT.train_step`` takes."""
        shape = self._inputs(img1, img2, flow)
        H, W = shape[-3:-1]
        return self.apply(self.draw(H, W, 1 if len(shape) == 3 else shape[0]), img1, img2, flow)

    def __call__(self, img1, img2, flow):
        return self.batch(img1, img2, flow)[:3]


MIN_SPARSE_FACTOR = 1.0 / 8     # the sparse gather looks ceil(0.5 / f) + 1 <= 5 sources beyond X / f (csrc/augment.hip)
SPARSE_MARGIN = (20, 50)        # margin_y, margin_x of the sparse crop origin's draw (augmentor.py:242-243)


class SparseFlowAugmentor(_Augmentor):
    """``SparseFlowAugmentor(crop_size, min_scale=-0.2, max_scale=0.5, do_flip=False)``: the reference's constructor, attribute names
    and values (augmentor.py:132-161), for sparse ground truth (KITTI, HD1K: dataset.py:36-37, 88-89).

    ``aug(img1, img2, flow, valid)`` and ``aug.batch(...)`` -> ``(image1 uint8, image2 uint8, flow float32, valid float32)`` device
    tensors at ``crop_size``, as the reference's call returns all four.  ``valid``: float32 ``(H, W)`` or ``(N, H, W)``; the other
    inputs, ``rng`` and ``photo_rng`` as for ``FlowAugmentor``.

    One colour application serves both frames, one factor both axes, there is no vertical flip, and the crop origin is drawn beyond
    the frame and clipped into it.  A resized sample takes flow and validity through ``resize_sparse_flow_map`` (augmentor.py:183-215):
    every source with ``valid >= 1`` lands on ``(rint(x f), rint(y f))``, targets in row or column 0 are dropped, and of several
    sources on one target the last in row-major order stays -- computed per output pixel as a gather."""

    _name = 'SparseFlowAugmentor'
    _gather = 'raft_augment_gather_sparse_u8'
    _label = 'augment_gather_sparse'

    def __init__(self, crop_size, min_scale=-0.2, max_scale=0.5, do_flip=False, *, rng=None, photo_rng=None):
        self._setup(crop_size, min_scale, max_scale, do_flip, rng, photo_rng)
        # spatial augmentation params
        self.spatial_aug_prob = 0.8
        self.stretch_prob = 0.8             # the reference keeps these two and never reads them
        self.max_stretch = 0.2
        # flip augmentation params
        self.h_flip_prob = 0.5
        self.v_flip_prob = 0.1              # never read by the reference either: there is no vertical flip
        # photometric augmentation params
        self.photo_aug = PhotoAug(brightness_limit=0.3, contrast_limit=0.3, hue_shift_limit=int(0.3 / 3.14 * 180),
                                  sat_shift_limit=int(0.3 * 255), val_shift_limit=int(0.))
        self.asymmetric_color_aug_prob = 0.2
        self.eraser_aug_prob = 0.5

    def _min_clip(self, H, W):
        ch, cw = self.crop_size
        return np.maximum((ch + 1) / float(H), (cw + 1) / float(W))

    def _check_size(self, H, W):
        """The crop origin is clipped into the frame, so a source of the crop's own size is legal (every resize then enlarges it);
        a smaller one is not.  The smallest factor the draws can give is known beforehand and has to stay in the gather's reach."""
        ch, cw = self.crop_size
        if H < ch or W < cw:
            raise ValueError(f'a {ch}x{cw} crop does not fit a {H}x{W} source')
        lowest = max(2.0 ** min(self.min_scale, self.max_scale), float(self._min_clip(H, W)))
        if not lowest >= MIN_SPARSE_FACTOR:
            raise ValueError(f'scale exponents ({self.min_scale}, {self.max_scale}) allow a factor of {lowest:g}, below 1/8')

    def _check_record(self, p):
        if p['scale_x'] != p['scale_y'] or p['flip_v']:
            raise ValueError('a sparse record has one factor for both axes and no vertical flip')
        if p['resize'] and not p['scale_x'] >= MIN_SPARSE_FACTOR:
            raise ValueError(f"factor {p['scale_x']:g} is below 1/8")
        if p['photo'][0] != p['photo'][1]:
            raise ValueError('a sparse record has one colour application for both frames')

    def _draw_one(self, H, W):
        rng = self.rng if self.rng is not None else np.random
        ch, cw = self.crop_size
        # color_transform (augmentor.py:163-168): always symmetric
        photo = draw_photo(self.photo_rng, self.photo_aug)
        rects = self._draw_rects(rng, H, W)
        # spatial_transform (augmentor.py:217-255)
        min_scale = self._min_clip(H, W)
        scale = 2 ** rng.uniform(self.min_scale, self.max_scale)
        clipped = bool(scale < min_scale)
        scale = np.clip(scale, min_scale, None)
        resize = bool(rng.rand() < self.spatial_aug_prob)
        H1, W1 = (cv_round(H * scale), cv_round(W * scale)) if resize else (H, W)
        flip_h = bool(rng.rand() < 0.5) if self.do_flip else False
        y0 = int(rng.randint(0, H1 - ch + SPARSE_MARGIN[0]))
        x0 = int(rng.randint(-SPARSE_MARGIN[1], W1 - cw + SPARSE_MARGIN[1]))
        return {'photo': (photo, photo), 'rects': rects, 'scale_x': float(scale), 'scale_y': float(scale), 'clipped': clipped,
                'resize': resize, 'size': (H1, W1), 'flip_h': flip_h, 'flip_v': False,
                'y0': int(np.clip(y0, 0, H1 - ch)), 'x0': int(np.clip(x0, 0, W1 - cw)), 'y0_drawn': y0, 'x0_drawn': x0,
                'source': (int(H), int(W))}

    def apply(self, params, img1, img2, flow, valid):
        """Run the kernels with given records (one per sample) -> ``(image1, image2, flow, valid)`` on the device, with a leading
        batch axis exactly when the inputs have one.  Current stream; no synchronisation, nothing returns to the host."""
        return self._run(params, img1, img2, flow, valid)

    def batch(self, img1, img2, flow, valid):
        """``(image1, image2, flow, valid)``: what ``RAFT.train_step`` takes."""
        shape = self._inputs(img1, img2, flow, valid)
        H, W = shape[-3:-1]
        return self.apply(self.draw(H, W, 1 if len(shape) == 3 else shape[0]), img1, img2, flow, valid)

    def __call__(self, img1, img2, flow, valid):
        return self.batch(img1, img2, flow, valid)


# ---------------------------------------------------------------- the student's view of a self-supervised step
class StudentView:
    """N affine views, one per pair: ``theta`` ``(N, 2, 3)`` float64 holds ``[M | o]``, the map from the student's pixel indices
    ``q = (x, y)`` to the teacher's, ``p = M q + o``.  ``gain`` / ``bias``: None (the frames are stored as sampled), or ``(N, 2,
    3)`` float64 -- index 0 is frame 1, index 1 frame 2, then the channel -- for ``clip(v * gain + bias, 0, 255)``.  Everything
    is held in float64; ``records`` inverts ``M`` in float64 and rounds each number once to float32 for the device."""

    def __init__(self, theta, gain=None, bias=None):
        theta = np.array(theta, dtype=np.float64)
        if theta.ndim != 3 or theta.shape[1:] != (2, 3) or theta.shape[0] < 1:
            raise ValueError(f'theta must be (N, 2, 3), got {theta.shape}')
        if not np.isfinite(theta).all():
            raise ValueError('theta must be finite')
        det = theta[:, 0, 0] * theta[:, 1, 1] - theta[:, 0, 1] * theta[:, 1, 0]
        if not (np.abs(det) > 0).all():
            raise ValueError(f'every view needs an invertible M, got determinants {det}')
        if (gain is None) != (bias is None):
            raise ValueError('gain and bias come together')
        if gain is not None:
            gain, bias = np.array(gain, dtype=np.float64), np.array(bias, dtype=np.float64)
            want = (theta.shape[0], 2, 3)
            if gain.shape != want or bias.shape != want or not (np.isfinite(gain).all() and np.isfinite(bias).all()):
                raise ValueError(f'gain and bias must be finite arrays {want}, got {gain.shape} / {bias.shape}')
        self.theta, self.gain, self.bias = theta, gain, bias

    def __len__(self):
        return self.theta.shape[0]

    def __repr__(self):
        return f'StudentView(N={len(self)}, colour={self.gain is not None})'

    @classmethod
    def identity(cls, N, crop):
        """The view of section 22's centre crop: ``M = I``, ``o = (cx, cy)`` for ``crop = (cy, cx)``, no colour change.  Both
        gathers are then exact copies through the window."""
        cy, cx = crop
        theta = np.tile(np.array([[1.0, 0.0, float(cx)], [0.0, 1.0, float(cy)]]), (int(N), 1, 1))
        return cls(theta)

    def matrix(self):
        """``M``, ``(N, 2, 2)`` float64."""
        return self.theta[:, :, :2].copy()

    def inverse(self):
        """``M^-1`` in float64, ``(N, 2, 2)``: a teacher vector ``f`` is seen by the student as ``M^-1 f``."""
        return np.linalg.inv(self.theta[:, :, :2])

    def records(self, doubled=False):
        """The ``RaftViewParams`` records (a ctypes array on the host), each number rounded once to float32: ``N`` records with frame
        1's colour, or (``doubled``) the ``2N`` of a training step's doubled batch -- record ``n`` is view ``n`` with frame 1's
        colour, record ``n + N`` the same view with frame 2's."""
        N = len(self)
        with np.errstate(over='ignore'):            # (a number float32 cannot hold becomes infinite: image_ops refuses the record)
            m, o, inv = (a.astype(np.float32) for a in (self.theta[:, :, :2].reshape(N, 4), self.theta[:, :, 2], self.inverse().reshape(N, 4)))
            gain, bias = (None, None) if self.gain is None else (self.gain.astype(np.float32), self.bias.astype(np.float32))
        recs = (ViewParams * (2 * N if doubled else N))()
        for k, r in enumerate(recs):
            n, frame = k % N, k // N
            r.m[:], r.o[:], r.inv[:] = m[n].tolist(), o[n].tolist(), inv[n].tolist()
            if gain is not None:
                r.gain[:], r.bias[:] = gain[n, frame].tolist(), bias[n, frame].tolist()
                r.colour = 1
            else:
                r.gain[:], r.bias[:], r.colour = [1.0] * 3, [0.0] * 3, 0
        return recs


def _range(name, v, lowest=None):
    try:
        lo, hi = (float(x) for x in v)
    except (TypeError, ValueError) as exc:
        raise ValueError(f'{name} must be a pair (low, high), got {v!r}') from exc
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi) or (lowest is not None and not lo > lowest):
        raise ValueError(f'{name} must be a finite pair low <= high{"" if lowest is None else f" above {lowest:g}"}, got {v!r}')
    return lo, hi


class StudentTransform:
    """Draws the ``StudentView`` of a step: ``M = (1 / s) R(angle) diag(+-1, +-1)`` about the frames' centres,
    ``p - c_t - shift = M (q - c_s)`` with ``c = ((W - 1) / 2, (H - 1) / 2)`` and ``R(t) = [[cos t, -sin t], [sin t, cos t]]``.

    ``flip_x`` / ``flip_y``: the probabilities of the two mirrors; ``zoom = (low, high)``: ``s`` uniform in it (``s > 1`` shows the
    student a magnified, smaller part of the scene); ``rotate``: the angle uniform in ``[-rotate, rotate]`` degrees; ``translate``:
    a transformed view is shifted uniformly within the slack that keeps the student's four corners inside the teacher, per axis
    (an axis without slack stays centred; what then falls outside is zero-filled and unused).  ``gain`` / ``bias``: ranges of one
    gain and one bias per frame for ``clip(v * gain + bias, 0, 255)``, the same for the three channels; with probability
    ``asymmetric`` frame 2 draws its own pair, else it shares frame 1's.

    The draws of one sample, in this order, from ``rng`` (a ``np.random.RandomState``; None: the global ``np.random``, as
    ``FlowAugmentor``): ``rand()`` flip_x, ``rand()`` flip_y, ``uniform(*zoom)``, ``uniform(-rotate, rotate)``; if ``translate`` and
    the transform can change the geometry at all (a flip probability, a zoom range other than (1, 1) or ``rotate`` is set):
    ``rand()`` for the shift along x and ``rand()`` along y; if the ranges can change a colour at all (``gain != (1, 1)`` or
    ``bias != (0, 0)``): ``uniform(*gain)``, ``uniform(*bias)``, ``rand()`` asymmetric, and if that fires ``uniform(*gain)``,
    ``uniform(*bias)`` for frame 2.  A batch is drawn sample after sample.

    The defaults change nothing: the default object draws ``StudentView.identity`` -- the centre crop of DESIGN.md section 22 --
    which is why a transform that cannot change the geometry draws no shift either.  Every default and range is a choice, not a
    tuned value; nothing here was trained on real footage."""

    def __init__(self, flip_x=0.0, flip_y=0.0, zoom=(1.0, 1.0), rotate=0.0, translate=True, gain=(1.0, 1.0), bias=(0.0, 0.0),
                 asymmetric=0.0, rng=None):
        for name, v in (('flip_x', flip_x), ('flip_y', flip_y), ('asymmetric', asymmetric)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
                raise ValueError(f'{name} must be a probability in [0, 1], got {v!r}')
        if isinstance(rotate, (bool, np.bool_)) or not isinstance(rotate, (int, float, np.integer, np.floating)) \
                or not 0.0 <= float(rotate) <= 180.0:
            raise ValueError(f'rotate must be an angle in [0, 180] degrees, got {rotate!r}')
        if not isinstance(translate, (bool, np.bool_)):
            raise ValueError(f'translate must be True or False, got {translate!r}')
        self.flip_x, self.flip_y, self.asymmetric, self.rotate = float(flip_x), float(flip_y), float(asymmetric), float(rotate)
        self.zoom, self.gain, self.bias = _range('zoom', zoom, lowest=0.0), _range('gain', gain), _range('bias', bias)
        self.translate, self.rng = bool(translate), rng

    @property
    def spatial(self):
        """Whether a draw can differ from the centre crop's geometry."""
        return self.flip_x > 0 or self.flip_y > 0 or self.zoom != (1.0, 1.0) or self.rotate > 0

    @property
    def colour(self):
        return self.gain != (1.0, 1.0) or self.bias != (0.0, 0.0)

    def draw(self, N, frame_size, student_size):
        """The views of ``N`` pairs of ``frame_size = (H, W)`` frames for a student of ``student_size = (Hs, Ws)``; touches no
        device."""
        (H, W), (Hs, Ws), N = (int(v) for v in frame_size), (int(v) for v in student_size), int(N)
        if N < 1 or min(H, W, Hs, Ws) < 1:
            raise ValueError(f'N and the sizes must be >= 1, got {N}, {frame_size}, {student_size}')
        rng = self.rng if self.rng is not None else np.random
        ct, cs = np.array([(W - 1) / 2.0, (H - 1) / 2.0]), np.array([(Ws - 1) / 2.0, (Hs - 1) / 2.0])
        theta = np.zeros((N, 2, 3))
        gain, bias = (np.ones((N, 2, 3)), np.zeros((N, 2, 3))) if self.colour else (None, None)
        for n in range(N):
            fx = -1.0 if rng.rand() < self.flip_x else 1.0
            fy = -1.0 if rng.rand() < self.flip_y else 1.0
            s = rng.uniform(*self.zoom)
            angle = np.deg2rad(rng.uniform(-self.rotate, self.rotate))
            c, sn = (1.0, 0.0) if angle == 0.0 else (np.cos(angle), np.sin(angle))
            M = np.array([[c * fx, -sn * fy], [sn * fx, c * fy]]) / s + 0.0       # (+ 0.0: no negative zeros)
            shift = np.zeros(2)
            if self.translate and self.spatial:
                reach = np.abs(M) @ cs                                    # how far from its centre the student's corners land
                slack = np.maximum(ct - reach, 0.0)
                shift = (2.0 * np.array([rng.rand(), rng.rand()]) - 1.0) * slack
            theta[n, :, :2] = M
            theta[n, :, 2] = ct + shift - M @ cs
            if self.colour:
                g1, b1 = rng.uniform(*self.gain), rng.uniform(*self.bias)
                g2, b2 = (rng.uniform(*self.gain), rng.uniform(*self.bias)) if rng.rand() < self.asymmetric else (g1, b1)
                gain[n, 0], bias[n, 0], gain[n, 1], bias[n, 1] = g1, b1, g2, b2
        return StudentView(theta, gain, bias)

"""Stand-in ``cv2`` for the tests: the calls reference tf_raft/datasets/augmentor.py and the stand-in albumentations make, in NumPy.
DESIGN.md section 10 is the specification; tests/augstub/README.md says what this is and is not."""
import types

import numpy as np

INTER_LINEAR = 1
COLOR_RGB2HSV = 41
COLOR_HSV2RGB = 55

resized = []        # (fx, fy, output shape) of every resize call, for the fixture generator


def setNumThreads(n):
    pass


ocl = types.SimpleNamespace(setUseOpenCL=lambda flag: None)


def cvRound(x):
    return int(np.rint(x))


def _axis(dsize, f, ssize):
    """Source indices and weights of one axis: coordinate (d + 0.5) * (1 / f) - 0.5 in double, narrowed to float, floored,
    clamped at both ends with weight 0."""
    inv = 1.0 / float(f)
    c = ((np.arange(dsize, dtype=np.float64) + 0.5) * inv - 0.5).astype(np.float32)
    s = np.floor(c).astype(np.int64)
    w = c - s.astype(np.float32)
    assert w.dtype == np.float32
    lo, hi = s < 0, s >= ssize - 1
    s[lo], w[lo] = 0, 0
    s[hi], w[hi] = ssize - 1, 0
    return s, np.minimum(s + 1, ssize - 1), np.float32(1) - w, w


def resize(src, dsize, fx=0, fy=0, interpolation=INTER_LINEAR):
    assert dsize is None and interpolation == INTER_LINEAR and src.ndim == 3
    H, W = src.shape[:2]
    Wd, Hd = cvRound(W * fx), cvRound(H * fy)
    x0, x1, a0, a1 = _axis(Wd, fx, W)
    y0, y1, b0, b1 = _axis(Hd, fy, H)
    if src.dtype == np.float32:
        rows = src[:, x0] * a0[None, :, None] + src[:, x1] * a1[None, :, None]               # horizontal first
        out = rows[y0] * b0[:, None, None] + rows[y1] * b1[:, None, None]
        assert out.dtype == np.float32
    elif src.dtype == np.uint8:
        fixed = lambda w: np.rint(w * np.float32(2048)).astype(np.int32)                    # noqa: E731  (saturate_cast<short>)
        ia0, ia1, ib0, ib1 = fixed(a0), fixed(a1), fixed(b0), fixed(b1)
        s = src.astype(np.int32)
        rows = s[:, x0] * ia0[None, :, None] + s[:, x1] * ia1[None, :, None]
        out = (((ib0[:, None, None] * (rows[y0] >> 4)) >> 16) + ((ib1[:, None, None] * (rows[y1] >> 4)) >> 16) + 2) >> 2
        out = np.clip(out, 0, 255).astype(np.uint8)
    else:
        raise TypeError(src.dtype)
    resized.append((float(fx), float(fy), out.shape))
    return out


_I = np.arange(1, 256, dtype=np.float64)
SDIV = np.concatenate([[0], np.rint((255 << 12) / (1.0 * _I))]).astype(np.int32)
HDIV = np.concatenate([[0], np.rint((180 << 12) / (6.0 * _I))]).astype(np.int32)


def _rgb2hsv(img):
    r, g, b = (img[..., k].astype(np.int32) for k in range(3))
    v = np.maximum(r, np.maximum(g, b))
    diff = v - np.minimum(r, np.minimum(g, b))
    s = (diff * SDIV[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV[diff] + (1 << 11)) >> 12
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


def _hsv2rgb(img):
    f32 = np.float32
    h, s, v = (img[..., k].astype(f32) for k in range(3))
    hf = h * f32(1.0 / 30.0)
    sector = np.floor(hf)
    f = hf - sector
    sector = sector.astype(np.int32)
    sector = np.where(sector >= 6, sector - 6, sector)
    sf, vf = s * f32(1.0 / 255.0), v * f32(1.0 / 255.0)
    p = vf * (f32(1) - sf)
    q = vf * (f32(1) - sf * f)
    t = vf * (f32(1) - sf * (f32(1) - f))
    pick = lambda options: np.choose(sector, options)      # noqa: E731
    rgb = np.stack([pick([vf, q, p, p, t, vf]), pick([t, vf, vf, q, p, p]), pick([p, p, t, vf, vf, q])], axis=-1)
    assert rgb.dtype == np.float32
    return np.clip(np.rint(rgb * f32(255)), 0, 255).astype(np.uint8)


def cvtColor(img, code):
    assert img.dtype == np.uint8 and img.shape[-1] == 3
    return {COLOR_RGB2HSV: _rgb2hsv, COLOR_HSV2RGB: _hsv2rgb}[code](img)


def split(img):
    return [np.ascontiguousarray(img[..., k]) for k in range(img.shape[-1])]


def merge(channels):
    return np.stack(channels, axis=-1)


def LUT(src, lut):
    return lut[src]

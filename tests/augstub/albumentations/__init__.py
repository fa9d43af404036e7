"""Stand-in ``albumentations`` for the tests: ``Compose``, ``RandomBrightnessContrast`` and ``HueSaturationValue`` on uint8 images,
as reference tf_raft/datasets/augmentor.py:27-37 builds them.  The parameters come from ``photo_rng`` by the protocol of
``tf_raft_amd.augment.draw_photo``; DESIGN.md section 10 is the specification of the pixel maps."""
import cv2
import numpy as np

photo_rng = np.random.RandomState(0)
applied = []        # one dict per Compose call: {'bc': None | (alpha, beta), 'hsv': None | (hue, sat, val)}


def set_photo_rng(rs):
    global photo_rng
    photo_rng = rs


def _limit(v):
    return (-v, v) if np.isscalar(v) else tuple(v)


class RandomBrightnessContrast:
    key = 'bc'

    def __init__(self, brightness_limit=0.2, contrast_limit=0.2, brightness_by_max=True, p=0.5):
        assert brightness_by_max
        self.brightness_limit, self.contrast_limit, self.p = _limit(brightness_limit), _limit(contrast_limit), p

    def get_params(self):
        alpha = 1.0 + photo_rng.uniform(self.contrast_limit[0], self.contrast_limit[1])
        beta = 0.0 + photo_rng.uniform(self.brightness_limit[0], self.brightness_limit[1])
        return alpha, beta

    def apply(self, img, alpha, beta):
        assert img.dtype == np.uint8
        lut = np.arange(0, 256).astype('float32')
        lut *= np.float32(alpha)
        lut += np.float32(beta * 255)
        return cv2.LUT(img, np.clip(lut, 0, 255).astype(np.uint8))


class HueSaturationValue:
    key = 'hsv'

    def __init__(self, hue_shift_limit=20, sat_shift_limit=30, val_shift_limit=20, p=0.5):
        self.limits, self.p = [_limit(v) for v in (hue_shift_limit, sat_shift_limit, val_shift_limit)], p

    def get_params(self):
        return tuple(photo_rng.uniform(lo, hi) for lo, hi in self.limits)

    def apply(self, img, hue_shift, sat_shift, val_shift):
        assert img.dtype == np.uint8
        hue, sat, val = cv2.split(cv2.cvtColor(img, cv2.COLOR_RGB2HSV))
        ramp = np.arange(0, 256, dtype=np.int16)
        hue = cv2.LUT(hue, np.mod(ramp + hue_shift, 180).astype(np.uint8))
        sat = cv2.LUT(sat, np.clip(ramp + sat_shift, 0, 255).astype(np.uint8))
        val = cv2.LUT(val, np.clip(ramp + val_shift, 0, 255).astype(np.uint8))
        return cv2.cvtColor(cv2.merge((hue, sat, val)), cv2.COLOR_HSV2RGB)


class Compose:
    def __init__(self, transforms, p=1.0):
        assert p == 1.0
        self.transforms = list(transforms)

    def __call__(self, image):
        record = {t.key: None for t in self.transforms}
        for t in self.transforms:
            if photo_rng.rand() < t.p:
                record[t.key] = params = t.get_params()
                image = t.apply(image, *params)
        applied.append(record)
        return {'image': image}

"""Generates tests/golden/flow_viz_device_golden.npz: the fixtures of the device-side flow colour coding
(tf_raft_amd/csrc/flow_viz.hip), made by running the REFERENCE's own flow_viz.py (pure NumPy, importable without TensorFlow,
unmodified) on small flows chosen for what the kernels can get wrong.  Run in the build container only (the reference tree does
not exist on the GPU box), with NumPy 2 (the types of the reference's expressions are NumPy 2's):
    python tests/golden/make_flow_viz_device_golden.py

The file holds a JSON `manifest` -- one entry per check: the flow it reads, the window, clip, channel order and fixed radius --
and per check `img/<name>` (N, h, w, 3) uint8 and, where the images are normalised by their own maximum, `rad/<name>` (N,) float32.
Windowed checks are NumPy crop-or-pad followed by the reference.

Every fixture is also run through a NumPy restatement whose ONLY difference from the reference is atan2 in double, rounded once
(what the kernel does): the number of differing channel values is printed, and a fixture on which the restatement alone exceeds
the parity cap max(2, 1e-5 * values) or differs by more than one level stops the script.
"""
import importlib.util
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location('ref_flow_viz', '/root/reference/tf_raft/datasets/flow_viz.py')
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)
assert int(np.__version__.split('.')[0]) >= 2, np.__version__

EPS = np.float32(1e-5)


def crop_or_pad(x, th, tw):
    """tf.image.resize_with_crop_or_pad of (H, W, C): per axis, d = target - source, crop at max(-d // 2, 0), pad max(d // 2, 0)."""
    H, W = x.shape[:2]
    out = np.zeros((th, tw) + x.shape[2:], x.dtype)
    cy, py, ey = max(-(th - H) // 2, 0), max((th - H) // 2, 0), min(H, th)
    cx, px, ex = max(-(tw - W) // 2, 0), max((tw - W) // 2, 0), min(W, tw)
    out[py:py + ey, px:px + ex] = x[cy:cy + ey, cx:cx + ex]
    return out


def restated(flow, clip=None, bgr=False, rad_max=None):
    """flow_viz.py:109-132 and 85-105 with atan2 in double, rounded once to float32; everything else as NumPy types it."""
    if clip is not None:
        flow = np.clip(flow, 0, clip)
    u, v = flow[:, :, 0], flow[:, :, 1]
    d = (np.max(np.sqrt(np.square(u) + np.square(v))) if rad_max is None else np.float32(rad_max)) + EPS
    u, v = u / d, v / d
    wheel = ref.make_colorwheel()
    rad = np.sqrt(np.square(u) + np.square(v))
    a = np.arctan2(-v.astype(np.float64), -u.astype(np.float64)).astype(np.float32) / np.float32(np.pi)
    fk = (a + 1) / 2 * 54
    assert fk.dtype == np.float32
    k0 = np.floor(fk).astype(np.int32)
    k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
    f = fk - k0
    assert f.dtype == np.float64
    img = np.zeros(u.shape + (3,), np.uint8)
    for i in range(3):
        col = (1 - f) * (wheel[k0, i] / 255.0) + f * (wheel[k1, i] / 255.0)
        col = np.where(rad <= 1, 1 - rad * (1 - col), col * 0.75)
        img[:, :, 2 - i if bgr else i] = np.floor(255 * col)
    return img


rng = np.random.default_rng(7)


def gauss(shape, scale):
    return rng.normal(scale=scale, size=shape + (2,)).astype(np.float32)


def scaled_to(shape, peak):
    f = gauss(shape, 1.0)
    return (f * (np.float32(peak) / np.sqrt((f.astype(np.float64) ** 2).sum(-1)).max())).astype(np.float32)


flows = {}
flows['odd'] = gauss((37, 53), 3.0)[None]                      # width no multiple of 4, rows unaligned for dword stores, two blocks
flows['batch3'] = np.stack([scaled_to((29, 41), p) for p in (0.5, 3.0, 40.0)])      # a maximum leaking across images shows
last = gauss((19, 23), 0.3)
last[-1, -1] = (30.0, -40.0)                                    # the only large vector is the last pixel: the reduction's tail
flows['lastpix'] = last[None]
flows['zeros'] = np.zeros((1, 9, 11, 2), np.float32)            # divides by 1e-5, comes out white
flows['one'] = np.array([3.0, -4.0], np.float32).reshape(1, 1, 1, 2)
# axis-aligned and signed-zero vectors, the diagonals, and one vector at (the float32 neighbourhood of) each of the 55 bin borders
special = [(1, 0.0), (1, -0.0), (-1, 0.0), (-1, -0.0), (0.0, 1), (-0.0, 1), (0.0, -1), (-0.0, -1), (0.0, 0.0), (-0.0, -0.0), (0.0, -0.0),
           (-0.0, 0.0), (1, 1), (1, -1), (-1, 1), (-1, -1), (2, 0.0), (0.0, -2), (0.5, 0.5), (-2, -2)]
angles = np.pi * (2 * np.arange(55) / 54 - 1)                   # atan2(-v, -u) of border k
radii = 0.25 + 1.75 * ((np.arange(55) * 7) % 11) / 10
border = [(-r * np.cos(t), -r * np.sin(t)) for t, r in zip(angles, radii)]
vectors = np.array(special + border + [(0.0, 0.0)] * 3, np.float32)
assert vectors.shape == (78, 2)
flows['axes'] = vectors.reshape(1, 6, 13, 2)
win = np.stack([gauss((64, 72), 2.0), gauss((64, 72), 0.7)])
win[:, 0, 71] = (-30.0, 40.0)                                   # 50 px in the margin that both crops below cut away
flows['window'] = win

checks = []


def check(name, flow, size=None, clip=None, bgr=False, rad_max=None):
    checks.append(dict(name=name, flow=flow, size=size, clip=clip, bgr=bgr, rad_max=rad_max))


for name in flows:
    check(name, name)
check('odd_bgr', 'odd', bgr=True)
check('odd_clip', 'odd', clip=2.0)
check('odd_clip_bgr', 'odd', clip=2.0, bgr=True)
check('batch3_clip', 'batch3', clip=2.0)
check('odd_fixed', 'odd', rad_max=2.0)                          # smaller than the image's own maximum: the rad > 1 branch runs
check('batch3_fixed', 'batch3', rad_max=3.0)
check('axes_fixed', 'axes', rad_max=1.0)
check('window_crop', 'window', size=(61, 67))                   # crop with an odd surplus
check('window_pad', 'window', size=(70, 80))                    # pad: nothing is cut away, the 50 px vector sets the scale
check('window_mixed', 'window', size=(70, 60))                  # pad in y, crop in x
check('window_mixed_clip', 'window', size=(70, 60), clip=2.0)

out = {f'flow/{k}': v for k, v in flows.items()}
for c in checks:
    imgs, rads, differing, values = [], [], 0, 0
    for f in flows[c['flow']]:
        if c['size'] is not None:
            f = crop_or_pad(f, *c['size'])
        if c['rad_max'] is None:
            img = ref.flow_to_image(f, clip_flow=c['clip'], convert_to_bgr=c['bgr'])
            g = f if c['clip'] is None else np.clip(f, 0, c['clip'])
            rads.append(np.max(np.sqrt(np.square(g[:, :, 0]) + np.square(g[:, :, 1]))))
            assert rads[-1].dtype == np.float32
        else:
            d = np.float32(c['rad_max']) + EPS
            assert c['clip'] is None and d.dtype == np.float32
            img = ref.flow_uv_to_colors(f[:, :, 0] / d, f[:, :, 1] / d, c['bgr'])
        mine = restated(f, c['clip'], c['bgr'], c['rad_max'])
        diff = np.abs(mine.astype(np.int32) - img.astype(np.int32))
        assert diff.max() <= 1, (c['name'], diff.max())
        differing += int((diff != 0).sum())
        values += img.size
        imgs.append(img)
    assert differing <= max(2, 1e-5 * values), (c['name'], differing, values)
    print(f"{c['name']}: {values} values, restatement with double atan2 differs in {differing}")
    out[f"img/{c['name']}"] = np.stack(imgs)
    if rads:
        out[f"rad/{c['name']}"] = np.array(rads, np.float32)
for k in ('zeros', 'window_pad'):
    print(k, 'white fraction', float((out[f'img/{k}'] == 255).mean()))
out['manifest'] = np.array(json.dumps(checks))
np.savez_compressed(os.path.join(HERE, 'flow_viz_device_golden.npz'), **out)
print('wrote', len(checks), 'checks,', os.path.getsize(os.path.join(HERE, 'flow_viz_device_golden.npz')), 'bytes')

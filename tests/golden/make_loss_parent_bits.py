"""Generates tests/golden/loss_parent_bits.json: what the loss and metric kernels gave on the commit BEFORE their reductions
moved into csrc/loss_common.h, as the uint32 bits of every float32 scalar and the sha256 of every gradient's bytes.  It uses the
public Python entry points only, so it runs unchanged on that commit and on every later one; run it on a GPU:
    python tests/golden/make_loss_parent_bits.py
tests/test_gpu_loss_parent_bits.py imports ``CASES`` and ``compute`` from here and requires equality with the file.

The cases are the smallest that reach each branch of the reduction (csrc/loss_common.h):
    supervised (two predictions)   npix 1, 63 (less than a wave), 257 (two workgroups), 1024*256+3 (the grid-stride loop wraps
                                   past METRIC_WGS records)
    photometric (B, H, W, n)       1x3x5x1, 2x37x53x3, 1025x1x2x1 (B > kMaxRecords: the blockIdx.y loop wraps), 1x513x512x1
                                   (H*W > 1024*256: the x loop wraps)
    census, census_weight 0.5      1x7x7x1 (one interior pixel), 2x37x53x2, 769x7x7x1 (B > 768), 1x444x444x1 (H*W > 768*256)
and, from the commit BEFORE the census and SSIM kernels came to share csrc/warped_gray.h, of the SSIM entry's sweep
(csrc/ssim_loss.hip) and of the value-only kernels, which run only when no gradient is asked for:
    ssim, ssim_weight 0.5          1x3x3x1 (one interior window; every pixel takes the edge path), 1x5x5x1 (one pixel takes
    (census off)                   ssim_pixel_whole), 2x37x53x3, 769x3x3x1 (B > 768), 1x444x444x1 (H*W > 768*256); frames of
                                   five pixels or less a side take vectors of less than a pixel, so that their windows are in frame
    census+ssim, both 0.5          2x37x53x2: the chaining of add_to and accumulate
    value-only, both 0.5           1x7x7x1, 2x37x53x2 through SSIMSequenceLoss.terms: scalars only
The unlabelled cases run with and without a mask, from a list of host arrays and from views of one device buffer.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

SUPERVISED = [1, 63, 257, 1024 * 256 + 3]
PHOTOMETRIC = [(1, 3, 5, 1), (2, 37, 53, 3), (1025, 1, 2, 1), (1, 513, 512, 1)]
CENSUS = [(1, 7, 7, 1), (2, 37, 53, 2), (769, 7, 7, 1), (1, 444, 444, 1)]
SSIM = [(1, 3, 3, 1), (1, 5, 5, 1), (2, 37, 53, 3), (769, 3, 3, 1), (1, 444, 444, 1)]
BOTH = [(2, 37, 53, 2)]
VALUE_ONLY = [(1, 7, 7, 1), (2, 37, 53, 2)]
CASES = ([('supervised', npix) for npix in SUPERVISED] + [('photometric', s) for s in PHOTOMETRIC] + [('census', s) for s in CENSUS]
         + [('ssim', s) for s in SSIM] + [('census+ssim', s) for s in BOTH] + [('value-only', s) for s in VALUE_ONLY])
# kind -> (census_weight, ssim_weight or None: the entries without the SSIM term, with the gradient)
WEIGHTS = {'photometric': (0.0, None, True), 'census': (0.5, None, True), 'ssim': (0.0, 0.5, True), 'census+ssim': (0.5, 0.5, True),
           'value-only': (0.5, 0.5, False)}
PATH = os.path.join(HERE, 'loss_parent_bits.json')


def case_id(case):
    kind, what = case
    return f'{kind}-{what}' if kind == 'supervised' else f"{kind}-{'x'.join(map(str, what))}"


def _bits(t):
    return '0x%08x' % int(t.detach().cpu().numpy().reshape(()).astype(np.float32).view(np.uint32))


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def _views(preds):
    import torch
    buf = torch.as_tensor(np.stack(preds)).cuda().contiguous()
    return [buf[i] for i in range(buf.shape[0])]


def supervised(npix):
    from tf_raft_amd import grad, losses
    rng = np.random.default_rng(npix)
    shape = (1, 1, npix)
    flow_gt = (rng.normal(size=shape + (2,)) * 4).astype(np.float32)
    flow_gt.reshape(-1, 2)[::53] *= 200.0                      # beyond max_flow: masked
    valid = rng.uniform(size=shape) < 0.8
    preds = [(flow_gt + rng.normal(size=shape + (2,)) * (3.0 / (i + 1))).astype(np.float32) for i in range(2)]
    out = {}
    for name, ps in (('list', preds), ('views', _views(preds))):
        out[f'{name}/sequence_loss'] = _bits(losses.sequence_loss((flow_gt, valid), ps, gamma=0.8, max_flow=400))
        for i, g in enumerate(grad.sequence_loss_grad((flow_gt, valid), ps, gamma=0.8, max_flow=400, upstream=0.75)):
            out[f'{name}/sequence_loss_grad/{i}'] = _sha(g)
    for k, v in losses.end_point_error((flow_gt, valid), preds[-1], max_flow=400).items():
        out[k] = _bits(v)
    return out


def unlabelled_case(shape, with_mask, ssim=False):
    """``make_case``; for the kinds with the SSIM term a frame of five pixels or less a side takes vectors of less than a pixel
    (test_ssim_loss.ssim_case's rule for its one-window shape)."""
    from test_photometric_loss import make_case
    return make_case(*shape, with_mask=with_mask, **({'amp': 0} if ssim and min(shape[1:3]) <= 5 else {}))


def unlabelled(shape, census_weight, ssim_weight, with_grad):
    from test_photometric_loss import DEFAULTS
    from tf_raft_amd import grad, losses
    out = {}
    for with_mask in (True, False):
        image1, image2, mask, preds = unlabelled_case(shape, with_mask, ssim_weight is not None)
        y_true = (image1, image2) if mask is None else (image1, image2, mask)
        for name, ps in (('list', preds), ('views', _views(preds))):
            if not with_grad:
                terms, grads = losses.SSIMSequenceLoss(census_weight=census_weight, ssim_weight=ssim_weight, **DEFAULTS).terms(y_true, ps), []
            elif ssim_weight is None:
                terms, grads = grad.photometric_sequence_loss_value_and_grad(y_true, ps, census_weight=census_weight, **DEFAULTS)
            else:
                terms, grads = grad.ssim_sequence_loss_value_and_grad(y_true, ps, census_weight=census_weight, ssim_weight=ssim_weight,
                                                                      **DEFAULTS)
            key = f"{'mask' if with_mask else 'nomask'}/{name}"
            for k, v in terms.items():
                out[f'{key}/{k}'] = _bits(v)
            for i, g in enumerate(grads):
                out[f'{key}/grad/{i}'] = _sha(g)
    return out


def compute(case):
    kind, what = case
    return supervised(what) if kind == 'supervised' else unlabelled(what, *WEIGHTS[kind])


if __name__ == '__main__':
    import torch
    res = {case_id(c): compute(c) for c in CASES}
    torch.cuda.synchronize()
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', sum(len(v) for v in res.values()), 'pins of', len(res), 'cases')

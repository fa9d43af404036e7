"""What the update-block launch-plan tests share (test_gpu_update_plans.py on the GPU, test_update_plan_bounds.py on the CPU):
the inputs, the float64 / float32 oracle outputs of one update-block call (computed once per (variant, shape), returned
read-only) and the bound rule.

Bounds come from the reference, never from the kernels: ``err_o`` is the distance of the fp32 oracle (torch's fp32 convolutions
on the CPU) to the float64 oracle on the same inputs, i.e. what a correct fp32 evaluation of the block loses.  A plan without
an F(4x4, 3x3) layer must stay within ``FACTOR * err_o``; a plan with one gets ``FACTOR_WINO4 * err_o``: the factor 3 is the
ratio of that algorithm's fp32 deviation to the other kernels' (include/raft_hip.h, test_conv2d_winograd4_matches_oracle).
The absolute bounds of test_basic_update_block_matches_oracle stay as an outer limit (``OUTER``).
test_update_plan_bounds.py proves on the CPU that a one-tap error of 2^-10 in any layer crosses these bounds.
"""
import functools

import numpy as np
import torch

from conftest import report

SEED = 1234                        # inputs: the seed of the suite's rng fixture
WEIGHT_SEED = {'raft': 3, 'small': 4}
RAGGED = [(2, 9, 13),              # one ragged tile of every kernel, two images
          (1, 9, 70)]              # two row blocks with a tail, two 64-pixel x-tiles with a 6-pixel tail, a cut 4 x 4 tile
PLANNER = (1, 56, 64)              # 3584 pixels: times the hint it crosses every threshold of launch_plan.h
FACTOR, FACTOR_WINO4 = 4.0, 12.0
OUTER = {'net': 2e-5, 'mask': 5e-5, 'delta': 5e-5}
TAP_SCALE = 1.0 + 2.0 ** -10


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def weights(variant):
    from tf_raft_amd import weights as wm
    wts = wm.init_weights(variant, seed=WEIGHT_SEED[variant], perturb=True)
    return {k: v for k, v in wts.items() if k.startswith('update_block/')}   # shared: scaled_tap copies what it changes


def conv_layers(variant):
    """Names of the block's convolutions ('update_block/encoder/convc1', ...)."""
    return [k[:-len('/kernel')] for k in weights(variant) if k.endswith('/kernel')]


@functools.lru_cache(maxsize=None)
def inputs(variant, shape):
    """(net, inp, corr, flow) as float32: the recipe of test_gpu_kernels._update_inputs with a seed of its own."""
    from tf_raft_amd.layers.update import _GEOM
    g, (B, h, w) = _GEOM[variant], shape
    rng = np.random.default_rng(SEED)
    net = np.tanh(rng.normal(size=(B, h, w, g['hdim']))).astype(np.float32)
    inp = np.maximum(rng.normal(size=(B, h, w, g['cdim'])), 0).astype(np.float32)
    corr = rng.normal(size=(B, h, w, g['corr_used'])).astype(np.float32)
    flow = rng.normal(scale=3.0, size=(B, h, w, 2)).astype(np.float32)
    return tuple(_frozen(a) for a in (net, inp, corr, flow))


def run_oracle(variant, shape, dtype, wts=None):
    """{'net', 'delta'[, 'mask']} of oracle.layers.*_update_block in ``dtype`` as NumPy."""
    from oracle.layers import W, basic_update_block, small_update_block
    fn = basic_update_block if variant == 'raft' else small_update_block
    args = [torch.tensor(a).to(dtype) for a in inputs(variant, shape)]
    net, mask, delta = fn(W(weights(variant) if wts is None else wts, dtype), 'update_block', *args)
    out = {'net': net.numpy(), 'delta': delta.numpy()}
    if mask is not None:
        out['mask'] = mask.numpy()
    return out


@functools.lru_cache(maxsize=None)
def oracle(variant, shape):
    """(float64 oracle outputs, err_o per output): computed once, shared, read-only."""
    want = {k: _frozen(v) for k, v in run_oracle(variant, shape, torch.float64).items()}
    o32 = run_oracle(variant, shape, torch.float32)
    err_o = {k: float(np.abs(o32[k] - want[k]).max()) for k in want}
    return want, err_o


def bounds(variant, shape, wino4):
    """{output: bound} of a plan with (wino4) / without an F(4x4, 3x3) layer."""
    _, err_o = oracle(variant, shape)
    return {k: (FACTOR_WINO4 if wino4 else FACTOR) * e for k, e in err_o.items()}


def scaled_tap(variant, layer):
    """The block's weights with tap [kh // 2, kw - 1] of ``layer`` scaled by 1 + 2^-10 across all channels."""
    wts = dict(weights(variant))
    k = wts[f'{layer}/kernel'].copy()
    k[k.shape[0] // 2, k.shape[1] - 1] *= np.float32(TAP_SCALE)
    wts[f'{layer}/kernel'] = k
    return wts


def diagnose(tag, got, want):
    """Locate a structural fault from one run: the worst pixel / channel and the error pattern over the positions inside the
    4 x 4 Winograd tile and the 8 x 64-pixel workgroup tile, by row, by column and by channel block.  Returns the 4 x 4 table."""
    e = np.abs(got - want)
    b, y, x, n = np.unravel_index(int(e.argmax()), e.shape)
    H, W, N = e.shape[1:]
    print(f'[plans] {tag}: worst at b {b} y {y} x {x} n {n}: got {got[b, y, x, n]} want {want[b, y, x, n]}')
    pos = np.array([[e[:, i::4, j::4].max() if i < H and j < W else 0.0 for j in range(4)] for i in range(4)])
    print(f'[plans] {tag}: max error by position inside the 4x4 tile:\n', pos)
    print(f'[plans] {tag}: max error by row inside the 8-row workgroup tile:',
          [float(e[:, i::8].max()) for i in range(min(8, H))])
    print(f'[plans] {tag}: max error by column inside the 64-pixel workgroup tile:',
          [round(float(e[:, :, j::64].max()), 8) for j in range(min(64, W))])
    print(f'[plans] {tag}: max error by row:', [float(e[:, i].max()) for i in range(H)])
    print(f'[plans] {tag}: max error by column:', [round(float(e[:, :, j].max()), 8) for j in range(W)])
    print(f'[plans] {tag}: max error by channel block of 16:', [float(e[..., k:k + 16].max()) for k in range(0, N, 16)])
    return pos


def check(tag, variant, shape, got, wino4, outer_only=()):
    """Report err / err_o of every output of ``got`` ({output: float32 NumPy}) and assert the bound of its plan and the outer
    absolute bound; on a miss the diagnostics come first.  Outputs in ``outer_only`` are held to the outer bound alone (open
    findings, docs/NOTEBOOK.md).  Returns {output: err / err_o}."""
    want, err_o = oracle(variant, shape)
    bound = bounds(variant, shape, wino4)
    errs, ratios = {}, {}
    for k in want:
        assert got[k].shape == want[k].shape and not np.isnan(got[k]).any(), (tag, k)
        errs[k] = float(np.abs(got[k] - want[k]).max())
        ratios[k] = errs[k] / err_o[k]
    report(f'update plan {variant} {shape} {tag}', **{f'{k}_over_err_o': round(r, 3) for k, r in ratios.items()},
           **{f'{k}_err': e for k, e in errs.items()}, **{f'{k}_err_o': e for k, e in err_o.items()})
    for k in want:
        if errs[k] > bound[k] or errs[k] >= OUTER[k]:
            diagnose(f'{tag} {k}', got[k], want[k])
    for k in want:
        if k not in outer_only:
            assert errs[k] <= bound[k], f'{tag}: {k} {errs[k]:.3e} > {bound[k]:.3e} = {FACTOR_WINO4 if wino4 else FACTOR} x err_o'
        assert errs[k] < OUTER[k], f'{tag}: {k} {errs[k]:.3e} >= {OUTER[k]:.0e}'
    return ratios

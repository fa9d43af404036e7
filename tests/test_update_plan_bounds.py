"""The condition that makes the bounds of test_gpu_update_plans.py meaningful, on the CPU: a one-tap error of 2^-10 in any
convolution of the update blocks moves the float64 oracle by more than twice the widest bound those tests apply
(update_plan_cases.FACTOR_WINO4 x err_o), so no such error can hide inside it."""
import numpy as np
import pytest
import torch

import update_plan_cases as upc
from conftest import report

MARGIN = 2.0
# Layers that meet the condition at one of the two ragged shapes only (the reference alone decides: no kernel runs here).
# convf1 of the basic block, 7 x 7 on the two flow channels: at (2, 9, 13) a tap moves net by 1.4 - 2.1 x the F(4x4) bound (1.6
# at the tap used here; all 49 taps scanned), above the bound but short of the margin; at (1, 9, 70) every tap moves it by 2.0 -
# 3.3 x (2.55 here).  It is held to the condition at (1, 9, 70) and to the bare bound at (2, 9, 13).
ONE_SHAPE = {('raft', 'update_block/encoder/convf1'): (1, 9, 70)}
LAYERS = [(v, layer) for v in ('raft', 'small') for layer in upc.conv_layers(v)]


def test_the_layer_list_is_complete():
    assert [v for v, _ in LAYERS].count('raft') == 15 and [v for v, _ in LAYERS].count('small') == 9


@pytest.mark.parametrize('variant,layer', LAYERS, ids=[f'{v}-{layer.split("/", 1)[1]}' for v, layer in LAYERS])
def test_one_tap_error_crosses_the_bound(variant, layer):
    """Tap [kh // 2, kw - 1] of one layer scaled by 1 + 2^-10 across all channels: at (2, 9, 13) and at (1, 9, 70) at least one
    output of the float64 oracle moves by more than 2 x (12 x err_o) of that output."""
    wts = upc.scaled_tap(variant, layer)
    for shape in upc.RAGGED:
        want, _ = upc.oracle(variant, shape)
        bound = upc.bounds(variant, shape, wino4=True)
        moved = upc.run_oracle(variant, shape, torch.float64, wts)
        margin = {k: float(np.abs(moved[k] - want[k]).max()) / bound[k] for k in want}
        report(f'one tap of {layer} {variant} {shape}', **{f'{k}_move_over_bound': round(m, 2) for k, m in margin.items()})
        need = MARGIN if ONE_SHAPE.get((variant, layer), shape) == shape else 1.0
        assert max(margin.values()) > need, (layer, shape, margin)


def test_bound_rule_and_shared_reference():
    """The rule itself: 4 x err_o without and 12 x err_o with an F(4x4) layer, the former inside the old absolute bounds at
    every shape the GPU tests use; the shared reference is read-only and computed once."""
    for variant, shape in [('raft', s) for s in upc.RAGGED + [upc.PLANNER]] + [('small', upc.PLANNER)]:
        want, err_o = upc.oracle(variant, shape)
        assert upc.oracle(variant, shape)[0] is want
        assert set(want) == ({'net', 'mask', 'delta'} if variant == 'raft' else {'net', 'delta'})
        for k, e in err_o.items():
            assert upc.bounds(variant, shape, False)[k] == 4 * e and upc.bounds(variant, shape, True)[k] == 12 * e
            assert 0 < 4 * e < upc.OUTER[k], (variant, shape, k, e)
            with pytest.raises(ValueError):
                want[k][0, 0, 0, 0] = 0.0


def test_check_accepts_the_fp32_oracle_and_locates_a_planted_tile_fault(capsys):
    """upc.check, the one comparison of the GPU tests, on the CPU: the fp32 oracle itself passes the plain bound (ratio 1); the
    same output with 13 x err_o added at position (3, 1) of every 4 x 4 tile fails the F(4x4) bound though it is far inside
    the old absolute one, after printing diagnostics that show the tile structure."""
    variant, shape = 'raft', (1, 9, 70)
    got = upc.run_oracle(variant, shape, torch.float32)
    ratios = upc.check('fp32 oracle', variant, shape, got, wino4=False)
    assert all(abs(r - 1.0) < 1e-12 for r in ratios.values())
    want, err_o = upc.oracle(variant, shape)
    bad = dict(got, mask=want['mask'].astype(np.float32))
    bad['mask'][:, 3::4, 1::4] += np.float32(13 * err_o['mask'])
    assert 13 * err_o['mask'] < 0.1 * upc.OUTER['mask']
    with pytest.raises(AssertionError, match='mask'):
        upc.check('planted', variant, shape, bad, wino4=True)
    out = capsys.readouterr().out
    assert 'planted mask: worst at' in out and 'by position inside the 4x4 tile' in out and 'workgroup tile' in out
    pos = upc.diagnose('planted mask', bad['mask'], want['mask'])
    assert pos.argmax() == 3 * 4 + 1 and pos[3, 1] > 6 * np.delete(pos.ravel(), 13).max()
    upc.check('planted, outer bound only', variant, shape, bad, wino4=True, outer_only=('mask',))

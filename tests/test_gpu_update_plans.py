"""Update-block parity against the float64 oracle under the launch plan of every batch regime (csrc/launch_plan.h): the plans
the planner itself chooses as pixels x hint grows, and every F(4x4, 3x3) / F(4, 5) layer forced one at a time at ragged shapes.
Inputs, references and the bound rule: update_plan_cases.py; what the bounds can see: test_update_plan_bounds.py."""
import functools
import itertools

import numpy as np
import pytest

import update_plan_cases as upc

pytestmark = pytest.mark.gpu

BASIC_HINTS = [1, 2, 3, 4, 6, 8, 16]    # x 3584 pixels: every threshold of raft_wino4_default_mask, GRU F(4, 5), TNW / KS rules
SMALL_HINTS = [1, 3, 8, 16]
CONV_BITS = {1: 'convc2', 2: 'convf2', 4: 'conv', 8: 'fh1_mask0', 15: 'all'}     # RAFT_CONV_WINO4
GRU_BITS = {1: 'gru_zr1', 2: 'gru_q1', 4: 'gru_zr2', 8: 'gru_q2', 15: 'all'}     # RAFT_GRU_WINO4


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _block(variant):
    from tf_raft_amd.layers.update import BasicUpdateBlock, SmallUpdateBlock
    return BasicUpdateBlock(filters=128, weights=upc.weights(variant)) if variant == 'raft' \
        else SmallUpdateBlock(filters=96, weights=upc.weights(variant))


def _run(variant, shape):
    import torch
    net, mask, delta = _block(variant)([a.copy() for a in upc.inputs(variant, shape)])   # the shared inputs are read-only
    torch.cuda.synchronize()
    out = {'net': _np(net), 'delta': _np(delta)}
    if mask is not None:
        out['mask'] = _np(mask)
    return out


@functools.lru_cache(maxsize=None)
def _planned(variant, hint):
    """One block call at (1, 56, 64) under the planner's own choices for ``hint`` loops sharing the chip (no switch forced)."""
    from tf_raft_amd import _ffi
    with _ffi.thread_concurrency(hint):
        return _run(variant, upc.PLANNER)


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ a. the planner's own choices
@pytest.mark.parametrize('hint', BASIC_HINTS)
def test_basic_block_under_the_planners_choice(hint):
    """Pixels x hint = hint x 3584.  By launch_plan.h: hint 1 direct / F(2x2) / F(2, 5); from 2 fh1_mask0 on F(4x4) and the GRU on
    F(4, 5); from 3 convc2 and convf2 on F(4x4); from 8 conv; workgroup shapes (TNW, KS, convf2's layer_ks) by the grid rules."""
    upc.check(f'planner hint {hint}', 'raft', upc.PLANNER, _planned('raft', hint), wino4=hint >= 2)


def test_basic_block_plans_really_change_with_the_hint():
    """Hints 1, 2, 3 and 8 add, in turn, fh1_mask0 F(4x4) + GRU F(4, 5), then convc2 + convf2, then conv: each step moves a
    layer that feeds net, the first one also the layer that feeds mask and delta."""
    for a, b in itertools.combinations((1, 2, 3, 8), 2):
        assert not _same_bits(_planned('raft', a)['net'], _planned('raft', b)['net']), (a, b)
    for k in ('mask', 'delta'):
        assert not _same_bits(_planned('raft', 1)[k], _planned('raft', 2)[k]), k


@pytest.mark.parametrize('hint', SMALL_HINTS)
def test_small_block_under_the_planners_choice(hint):
    """SmallRAFT has no F(4x4) / F(4, 5) layer: the hint moves workgroup shapes only (the bits may or may not move)."""
    upc.check(f'planner hint {hint}', 'small', upc.PLANNER, _planned('small', hint), wino4=False)


# ------------------------------------------------------------------------------------------------ b. forced, one layer at a time
@pytest.mark.parametrize('ks', [1, 2])
@pytest.mark.parametrize('bits', list(CONV_BITS), ids=list(CONV_BITS.values()))
@pytest.mark.parametrize('shape', upc.RAGGED, ids=str)
def test_basic_block_with_a_3x3_layer_forced_to_f4x4(shape, bits, ks, raft_opt):
    """RAFT_CONV_WINO4 = one layer (or all four) on F(4x4, 3x3), eight-row (RAFT_WINO4_KS = 1) or K-split workgroups (2); the
    other 3x3 layers on F(2x2) (RAFT_CONV_WINO = 15).  A single layer must move the bits of the output it feeds."""
    raft_opt.set('RAFT_CONV_WINO', '15')
    raft_opt.set('RAFT_WINO4_KS', str(ks))
    raft_opt.set('RAFT_CONV_WINO4', str(bits))
    got = _run('raft', shape)
    upc.check(f'F(4x4) {CONV_BITS[bits]} ks {ks}', 'raft', shape, got, wino4=True)
    if bits != 15:
        raft_opt.set('RAFT_CONV_WINO4', '0')
        base = _run('raft', shape)
        for k in (('mask', 'delta') if bits == 8 else ('net',)):
            assert not _same_bits(got[k], base[k]), f'{CONV_BITS[bits]} on F(4x4) left {k} unchanged'


@pytest.mark.parametrize('tnw', [1, 2])
@pytest.mark.parametrize('bits', list(GRU_BITS), ids=list(GRU_BITS.values()))
@pytest.mark.parametrize('shape', upc.RAGGED, ids=str)
def test_basic_block_with_a_gru_layer_forced_to_f45(shape, bits, tnw, raft_opt):
    """RAFT_GRU_WINO4 = one SepConvGRU convolution (or all four) on F(4, 5) with 32- (RAFT_WINO_TNW = 1) or 64-channel workgroups
    (2), the others on F(2, 5); bits 1 and 4 also move the context passes of raft_gru_context_f32.  No F(4x4) layer at these
    sizes (the planner's mask is 0 below 2 x 3584 pixels).  A single layer must move the bits of net."""
    raft_opt.set('RAFT_WINO_TNW', str(tnw))
    raft_opt.set('RAFT_GRU_WINO4', str(bits))
    got = _run('raft', shape)
    upc.check(f'F(4,5) {GRU_BITS[bits]} tnw {tnw}', 'raft', shape, got, wino4=False)
    if bits != 15:
        raft_opt.set('RAFT_GRU_WINO4', '0')
        assert not _same_bits(got['net'], _run('raft', shape)['net']), f'{GRU_BITS[bits]} on F(4, 5) left net unchanged'

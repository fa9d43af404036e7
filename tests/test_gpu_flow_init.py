"""The forward projection of a flow and the warm start on the GPU: ``raft_forward_interpolate_f32`` bit for bit against the float32
NumPy restatement of its rule (tests/golden/make_flow_init_golden.py, itself equal to SciPy on the golden cases:
tests/test_flow_init.py), the public op, and ``raft_warm_start_f32`` / ``raft_warm_start_small_f32`` through ctypes on the state a
preparation leaves.

The kernel stages a frame's end points in LDS chunks of 1024 and runs 256 targets per workgroup: (1, 7) is one partial
workgroup, (32, 32) exactly one chunk, (25, 41) one chunk and a single source, (56, 64) four chunks and fourteen workgroups.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_flow_init import shifted_flow, tied_flow

sys.path.insert(0, GOLDEN)
from make_flow_init_golden import CASES, case_flow, np_forward_interpolate      # noqa: E402

pytestmark = pytest.mark.gpu

EXTRA = [(11, 32, 32, 3), (12, 25, 41, 3)]


def _np(t):
    return t.detach().cpu().numpy()


def _guarded(numel):
    """A float32 destination of ``numel`` elements between two guard bands, and the check that only it was written
    (tests/test_gpu_consistency.py)."""
    slab = torch.full((numel + 64,), float('nan'), dtype=torch.float32, device='cuda')

    def untouched():
        return bool(torch.isnan(torch.cat([slab[:32], slab[32 + numel:]])).all())
    return slab[32:32 + numel], untouched


def _launch_guarded(flow):
    """``flow`` (B, h, w, 2) through the launch form into a guarded destination."""
    from tf_raft_amd import image_ops
    out, untouched = _guarded(flow.size)
    got = image_ops.forward_interpolate_launch(torch.as_tensor(flow).cuda(), out=out.view(flow.shape))
    assert got.data_ptr() == out.data_ptr()
    res = _np(got)
    assert untouched(), 'the kernel wrote outside its destination'
    assert not np.isnan(res).any(), 'an element of the destination was left unwritten'
    return res


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'flow_init_golden.npz')) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize('case', CASES + EXTRA, ids=[f'seed{c[0]}_{c[1]}x{c[2]}' for c in CASES + EXTRA])
def test_the_device_is_bitwise_the_float32_rule(golden, case):
    from tf_raft_amd import image_ops
    seed, h, w, scale = case
    flow = golden[f'flow_{seed}'] if f'flow_{seed}' in golden else case_flow(seed, h, w, scale)
    want = np_forward_interpolate(flow)
    np.testing.assert_array_equal(_launch_guarded(flow[None])[0], want)
    if f'scipy_{seed}' in golden:
        np.testing.assert_array_equal(want, golden[f'scipy_{seed}'])
    res = image_ops.forward_interpolate(flow)                                             # the public op from the host, (h, w, 2)
    assert tuple(res.shape) == (h, w, 2) and res.dtype == torch.float32 and res.is_cuda
    np.testing.assert_array_equal(_np(res), want)
    assert want.any()


def test_a_batch_is_its_images_and_an_image_without_a_valid_source_is_zero():
    from tf_raft_amd import image_ops
    h, w = 23, 37
    flow = np.stack([case_flow(3, h, w, 10), np.full((h, w, 2), 1000, np.float32), case_flow(7, h, w, 2)])
    want = np_forward_interpolate(flow)
    assert not want[1].any() and want[0].any() and want[2].any() and (want[0] != want[2]).any()
    np.testing.assert_array_equal(_launch_guarded(flow), want)
    lead = image_ops.forward_interpolate(flow.reshape(3, 1, h, w, 2))                     # any leading axes
    assert tuple(lead.shape) == (3, 1, h, w, 2)
    np.testing.assert_array_equal(_np(lead).reshape(flow.shape), want)
    for zero in (np.zeros((2, h, w, 2), np.float32), np.full((1, 1, 7, 2), -50, np.float32)):
        assert not _launch_guarded(zero).any()
    assert image_ops.forward_interpolate(np.zeros((4, 5, 2), np.float64)).dtype == torch.float32      # float64 narrows


@pytest.mark.parametrize('h,w', [(6, 9), (20, 30), (33, 40)])
def test_ties_go_to_the_lowest_index_and_an_integer_shift_moves_the_field(h, w):
    """u = +0.5, v = 0: every target with a column to its left is an exact tie of two sources; the tagged variant shows that the
    lower index won.  u = 1 with a v that names its source: the field moves one cell to the right."""
    for flow in (tied_flow(h, w, False), tied_flow(h, w, True), shifted_flow(h, w)):
        want, ties = np_forward_interpolate(flow, return_ties=True)
        got = _launch_guarded(flow[None])[0]
        np.testing.assert_array_equal(got, want)
    tagged = tied_flow(h, w, True)
    np.testing.assert_array_equal(_launch_guarded(tagged[None])[0][1:-1, 1:], tagged[1:-1, :-1])
    assert np_forward_interpolate(tied_flow(h, w, False), return_ties=True)[1] >= (h - 1) * (w - 1)
    shift = shifted_flow(h, w)
    got = _launch_guarded(shift[None])[0]
    np.testing.assert_array_equal(got[:, 1:], shift[:, :-1])
    np.testing.assert_array_equal(got[:, 0], shift[:, 0])


def test_the_op_follows_the_current_stream_and_takes_or_rejects_views_as_the_tile_ops_do():
    from tf_raft_amd import _dev, image_ops
    h, w = 23, 37
    flow_h = np.stack([case_flow(3, h, w, 2), case_flow(4, h, w, 3)])
    flow = torch.as_tensor(flow_h).cuda()
    # a side stream the package owns already, not a new one: torch hands streams out of a pool of 32 per device in turn, so a test
    # that opens its own moves every stream made after it to another place in the pool
    side = _dev.side_stream(flow.device, 'encoder')
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        doubled = flow * 2                                                   # produced on `side`: only stream order makes the op see it
        got = image_ops.forward_interpolate(doubled)
    side.synchronize()
    np.testing.assert_array_equal(_np(got), np_forward_interpolate(flow_h * 2))
    base = np_forward_interpolate(flow_h)
    # views: a non-contiguous or offset input is made contiguous (as by every op here), with the same result
    wide = torch.zeros((2, h, w, 3), device='cuda')
    wide[..., 1:] = flow
    np.testing.assert_array_equal(_np(image_ops.forward_interpolate(wide[..., 1:])), base)
    np.testing.assert_array_equal(_np(image_ops.forward_interpolate(flow[1])), base[1])
    # the launch form reads whole vectors from a contiguous tensor and never works in place
    out = torch.full((2, h, w, 2), float('nan'), device='cuda')
    with pytest.raises(ValueError, match='contiguous'):
        image_ops.forward_interpolate_launch(wide[..., 1:], out=out)
    slab = torch.zeros((2 * h * w * 2 + 2,), device='cuda')
    with pytest.raises(ValueError, match='aligned'):
        image_ops.forward_interpolate_launch(slab[1:1 + 2 * h * w * 2].view(2, h, w, 2), out=out)
    with pytest.raises(ValueError, match='out'):
        image_ops.forward_interpolate_launch(flow, out=out[:1])
    assert torch.isnan(out).all()
    keep = flow.clone()
    with pytest.raises(ValueError):
        image_ops.forward_interpolate_launch(flow, out=flow)
    assert torch.equal(flow, keep)
    with pytest.raises(TypeError):
        image_ops.forward_interpolate(flow.to(torch.float16))
    with pytest.raises(ValueError):
        image_ops.forward_interpolate(flow[..., :1])


@pytest.mark.parametrize('variant', ['raft', 'small'])
def test_warm_start_writes_the_three_copies_of_the_flow_and_nothing_else(variant):
    """After a state preparation: ``coords1`` is bitwise ``grid + init``, ``flow`` and the flow channels of the GRU input ``x``
    are bitwise ``init`` (the loop's first iteration reads the flow from all three: lookup, flow convolution, GRU), and every
    other element of every state field is bitwise what the preparation alone leaves."""
    from tf_raft_amd import _dev
    from tf_raft_amd.layers.update import UpdateState, _GEOM
    B, h, w = 2, 8, 12
    g = _GEOM[variant]
    lib = _dev.lib()
    prepare, warm = ((lib.raft_prepare_state_f32, lib.raft_warm_start_f32) if variant == 'raft'
                     else (lib.raft_prepare_state_small_f32, lib.raft_warm_start_small_f32))
    fields = ('net', 'x', 'corr', 'coords1', 'flow', 'delta', 'mask', 'ws', 'ctx')
    gen = torch.Generator().manual_seed(5)
    cnet = torch.randn((B, h, w, g['hdim'] + g['cdim']), generator=gen).cuda()
    init = (torch.randn((B, h, w, 2), generator=gen) * 3).cuda()
    states = []
    for warmed in (False, True):
        st = UpdateState(variant, B, h, w, torch.device('cuda'))
        fill = torch.Generator().manual_seed(6)
        for name in fields:
            t = getattr(st, name)
            t.copy_(torch.randn(tuple(t.shape), generator=fill))
        assert prepare(_dev.ptr(cnet), B, h, w, C.byref(st.c), _dev.stream_ptr()) == 0
        if warmed:
            assert warm(_dev.ptr(init), B, h, w, C.byref(st.c), _dev.stream_ptr()) == 0
        torch.cuda.synchronize()
        states.append({name: _np(getattr(st, name)).copy() for name in fields})
    cold, hot = states
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    grid = np.broadcast_to(np.stack([xs, ys], axis=-1), (B, h, w, 2))
    init_h = _np(init)
    np.testing.assert_array_equal(cold['coords1'], grid)
    assert not cold['flow'].any()
    np.testing.assert_array_equal(hot['coords1'], grid + init_h)                           # float32 + float32, one rounding
    np.testing.assert_array_equal(hot['flow'], init_h)
    slot = g['flow_slot']
    np.testing.assert_array_equal(hot['x'][..., slot:slot + 2], init_h)
    assert not cold['x'][..., slot:slot + 2].any()
    rest = np.ones(g['x_ld'], bool)
    rest[slot:slot + 2] = False
    assert np.array_equal(cold['x'][..., rest].view(np.uint32), hot['x'][..., rest].view(np.uint32))
    for name in fields:
        if name not in ('coords1', 'flow', 'x'):
            assert np.array_equal(cold[name].view(np.uint32), hot[name].view(np.uint32)), name

"""The loss and metric kernels give the bits they gave before their reductions moved into csrc/loss_common.h:
tests/golden/loss_parent_bits.json holds, from the commit before that move, the uint32 bits of every scalar and the sha256 of every
gradient that tests/golden/make_loss_parent_bits.py computes through the public Python entry points (its docstring lists the cases:
the smallest that reach each branch of the reduction, the wrapping grid-stride loops included).  The test recomputes them and
requires equality.

The wrap cases are outside the shapes of test_gpu_photometric_loss.py and test_gpu_census_loss.py, so before they were pinned they
were measured on that commit against the float64 yardsticks at those files' tolerances (MI355X; the larger of with and without mask;
list and views alike; the kernel's distances equal the float32 restatement's to the printed digits, so every case is inside):
    photometric 1025x1x2x1                      loss rel 4.5e-08, gradient / max|g| 1.5e-06
    photometric 1x513x512x1                     loss rel 8.2e-08, gradient / max|g| 6.6e-04
    census 769x7x7x1, census_weight 0.5         loss rel 5.9e-08, gradient / max|g| 5.2e-05
    census 1x444x444x1, census_weight 0.5       loss rel 7.2e-08, gradient / max|g| 8.3e-03

The SSIM, census+ssim and value-only cases were added from the commit before the census and SSIM kernels came to share
csrc/warped_gray.h (the SSIM sweep and the value-only kernels were pinned nowhere until then).  The two SSIM wrap cases are outside
the shapes of test_gpu_ssim_loss.py and were measured on that commit in the same way, by that file's rule (4 x the float32
restatement's own distance, floors 8 * 2^-24 and 16 * 2^-24 * max|g|), photometric + smoothness + 0.5 * SSIM, census off; with
mask / without; list and views alike; the kernel's distances equal the restatement's to the printed digits, so both are inside:
    ssim 769x3x3x1, ssim_weight 0.5             loss rel 9.8e-08 / 4.4e-08, gradient / max|g| 1.3e-06 / 1.2e-06
    ssim 1x444x444x1, ssim_weight 0.5           loss rel 1.8e-08 / 2.7e-09, gradient / max|g| 1.2e-04 / 1.1e-04

Two streams: losses on two streams of one device keep their partial records apart (losses._workspace is keyed by the stream).
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location('make_loss_parent_bits', os.path.join(GOLDEN, 'make_loss_parent_bits.py'))
pins = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pins)


@pytest.fixture(scope='module')
def parent():
    with open(pins.PATH) as f:
        return json.load(f)


@pytest.mark.parametrize('case', pins.CASES, ids=pins.case_id)
def test_the_bits_are_the_parent_commits(parent, case):
    want = parent[pins.case_id(case)]
    got = pins.compute(case)
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if v != want[k]} == {}


def test_two_streams_keep_their_records_apart():
    from test_photometric_loss import DEFAULTS, make_case
    from tf_raft_amd import _dev, losses
    image1, image2, mask, preds = make_case(2, 37, 53, 3)
    rng = np.random.default_rng(5)
    flow_gt = (rng.normal(size=(2, 37, 53, 2)) * 4).astype(np.float32)
    valid = rng.uniform(size=(2, 37, 53)) < 0.8
    bits = lambda t: t.detach().cpu().numpy().tobytes()
    # each call alone
    alone_seq = bits(losses.sequence_loss((flow_gt, valid), preds))
    alone_ph = bits(losses.photometric_sequence_loss((image1, image2, mask), preds, **DEFAULTS))
    torch.cuda.synchronize()
    losses._WORKSPACES.clear()
    # one of the package's own side streams, not a new torch.cuda.Stream(): torch hands streams out of a pool of 32 per device
    # in turn, and the models' lazily created lane streams must not find the pool wrapped round onto each other
    _dev.reserve_streams(torch.device('cuda', torch.cuda.current_device()))
    other = _dev.side_stream(torch.device('cuda', torch.cuda.current_device()), 'encoder')
    seq = losses.sequence_loss((flow_gt, valid), preds)
    with torch.cuda.stream(other):
        ph = losses.photometric_sequence_loss((image1, image2, mask), preds, **DEFAULTS)
    torch.cuda.synchronize()
    assert bits(seq) == alone_seq and bits(ph) == alone_ph
    held = list(losses._WORKSPACES.values())
    assert len(held) == 2 and held[0].data_ptr() != held[1].data_ptr()

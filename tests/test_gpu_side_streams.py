"""The package's side streams are distinct streams, however many streams the process has made in between.

torch hands out the 32 streams of its pool round robin.  A role whose stream is made lazily (lane 1's ``flow1`` / ``mask1``, at that
lane's first three-stream loop) could therefore receive the very stream an earlier role holds, once a multiple of 32 streams had
been made in between -- every ``prefetch_to_device`` call makes one -- and ``raft_iterate_basic_overlap_f32`` refuses a loop whose
three streams are not distinct (RAFT_E_UNSUPPORTED).  Whether that happened depended on how many tests ran before."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_two_roles_never_share_a_stream():
    from tf_raft_amd import _dev
    dev = _dev.require_gpu()
    first = _dev.side_stream(dev, 'test_role_a')
    kept = [torch.cuda.Stream(device=dev) for _ in range(31)]          # the pool's round robin is back at `first`'s stream
    second = _dev.side_stream(dev, 'test_role_b')
    assert first.cuda_stream != second.cuda_stream
    assert _dev.side_stream(dev, 'test_role_a') is first and _dev.side_stream(dev, 'test_role_b') is second
    held = [s.cuda_stream for (d, _), s in _dev._SIDE_STREAMS.items() if d == (dev.index or 0)]
    assert len(held) == len(set(held)) and len(kept) == 31

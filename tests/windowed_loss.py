"""What the tests of the two windowed data terms share (census: DESIGN.md section 18, SSIM: section 19; csrc/warped_gray.h): the
direct call of an entry on the GPU and the argument errors every such entry returns.  ``name`` is 'census' or 'ssim'."""
import ctypes as C

import torch

from test_photometric_loss import DEFAULTS


def entry(name, case, weight=1.0, upstream=1.0, add_to=None, prefill=None, want_grad=True, gap=0, guard=0):
    """raft_<name>_loss_f32 called directly: ``(out2 as float32 NumPy, d_preds (n, B, H, W, 2) or None, the whole slab)``.
    ``prefill`` (a float or a tensor, with accumulate = 1) fills d_preds before the call; ``gap`` floats lie behind every
    prediction and ``guard`` floats of NaN around d_preds."""
    from tf_raft_amd import _dev, losses
    from tf_raft_amd._ffi import check
    image1, image2, mask, preds = case
    B, H, W, _ = image1.shape
    n, npix = len(preds), B * H * W
    stride = 2 * npix + gap
    i1, i2 = torch.as_tensor(image1).cuda(), torch.as_tensor(image2).cuda()
    m = None if mask is None else torch.as_tensor(mask).cuda()
    src = torch.zeros((n * stride,), dtype=torch.float32, device='cuda')
    for i, p in enumerate(preds):
        src[i * stride:i * stride + 2 * npix] = torch.as_tensor(p).cuda().reshape(-1)
    slab = torch.full((n * stride + 2 * guard,), float('nan'), dtype=torch.float32, device='cuda')
    dst = slab[guard:guard + n * stride]
    if prefill is not None:
        dst.reshape(n, stride)[:, :2 * npix] = prefill
    add = None if add_to is None else torch.tensor([add_to], dtype=torch.float32, device='cuda')
    out = torch.full((2,), float('nan'), dtype=torch.float32, device='cuda')
    lib = _dev.lib()
    ws = losses._workspace(out.device, int(getattr(lib, f'raft_{name}_loss_workspace_bytes')(n, B, H, W)))
    check(getattr(lib, f'raft_{name}_loss_f32')(_dev.ptr(i1), _dev.ptr(i2), None if m is None else _dev.ptr(m), _dev.ptr(src), stride,
                                                n, B, H, W, DEFAULTS['gamma'], weight, upstream,
                                                None if add is None else _dev.ptr(add), _dev.ptr(out),
                                                _dev.ptr(dst) if want_grad else None, 0 if prefill is None else 1, _dev.ptr(ws),
                                                _dev.stream_ptr()), f'{name}_loss')
    torch.cuda.synchronize()
    to_np = lambda t: t.detach().cpu().numpy()
    d = to_np(dst.reshape(n, stride)[:, :2 * npix]).reshape(n, B, H, W, 2) if want_grad else None
    return to_np(out), d, slab


def check_argument_errors(fn):
    """``fn`` = raft_<name>_loss_f32.  No GPU here: a call that got past its checks would fail in the launch (a positive
    hipError_t) or crash."""
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off = C.c_void_p(p.value + 4)
    #       image1 image2 mask preds stride n  B  H  W  gamma weight upstream add_to out2 d_preds accumulate ws stream
    good = [p, p, p, p, 2 * 20, 3, 1, 4, 5, 0.8, 1.0, 1.0, p, p, p, 0, p, None]
    for k in (0, 1, 3, 13, 16):                                             # (mask, add_to and d_preds may be NULL)
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    for k in (5, 6, 7, 8):
        for v in (0, -3):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for bad in ((1, 1 << 15, 1 << 15), (1 << 10, 1 << 10, 1 << 10), (1, 1, 1 << 30), (1, 26755, 26755)):   # B*H*W*3 reaches 2^31
        args = list(good)
        args[6:9] = bad
        args[4] = 1 << 40
        assert fn(*args) == -2, bad
    args = list(good)
    args[4] = 2 * 20 - 2                                                    # predictions would overlap
    assert fn(*args) == -2
    args[4] = 2 * 20 + 1                                                    # read as float2
    assert fn(*args) == -3
    args = list(good)
    args[5] = 65
    assert fn(*args) == -3
    for k in (9, 10):
        for v in (-1e-3, float('nan'), float('inf'), -float('inf')):
            args = list(good)
            args[k] = v
            assert fn(*args) == -2, (k, v)
    for v in (float('nan'), float('inf')):
        args = list(good)
        args[11] = v
        assert fn(*args) == -2, v
    for v in (-1, 2):
        args = list(good)
        args[15] = v
        assert fn(*args) == -2, v
    for k in (3, 14, 16):
        args = list(good)
        args[k] = off
        assert fn(*args) == -4, k
    for m, a, d in ((None, None, None), (p, None, None), (None, p, None), (None, None, p)):      # no error of their own when NULL
        args = list(good)
        args[2], args[12], args[14], args[5] = m, a, d, 65
        assert fn(*args) == -3, (m, a, d)

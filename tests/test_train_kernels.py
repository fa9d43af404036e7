"""The references and bounds of tests/train_kernels_ref.py, checked without a GPU.

Anchors: ``adamw_steps`` against torch.optim.Adam, the normalisation references against torch's instance_norm / batch_norm under
autograd, the gates against autograd through torch.sigmoid / torch.tanh, all in float64 -- code this project did not write.

Sensitivity: a statement-by-statement float32 NumPy emulation of each kernel of csrc/backward.hip passes the comparison function
the GPU tests use (tests/test_gpu_train_kernels.py), and each of a list of subtle mutations of that emulation makes the same
function raise.  A bound that let one of them through could not see that error on the device either.
"""
import math

import numpy as np
import pytest
import torch

import train_kernels_ref as ref
from conftest import report

f32 = np.float32
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-7)
NORM_SLICES = 256
SCALES = (1e-8, 1.0, 1e4)


# ------------------------------------------------------------------------------------------------ float32 emulations

def emu_adamw(var, grad, m, v, lr_t, wd, gnsq=None, clip=0.0, mutation=None):
    """adamw_kernel of csrc/backward.hip, one float32 statement at a time (no contraction)."""
    one = f32(1)
    lr_t, wd, clip = f32(lr_t), f32(wd), f32(clip)
    with np.errstate(all='ignore'):
        scale = one
        if gnsq is not None:
            gn = f32(np.sqrt(np.float64(gnsq)))
            scale = clip / np.maximum(gn, clip) if not np.isnan(gn) else one      # fmaxf(NaN, clip) = clip
            scale = f32(scale + (gn - gn))
            if mutation == 'clip scale off by 1e-3':
                scale = f32(scale * f32(1.001))
        g = grad * scale
        w = var - (f32(wd * lr_t) if mutation == 'decay multiplied by lr' else wd) * var
        b1 = B2 if mutation == 'beta2 where beta1 belongs' else B1
        mi = b1 * m + (one - b1) * g
        vi = B2 * v + (one - B2) * g * g
        den = np.sqrt(vi + EPS) if mutation == 'eps inside the square root' else np.sqrt(vi) + EPS
        out = w - lr_t * mi / den
    assert out.dtype == mi.dtype == vi.dtype == np.float32
    return out, mi, vi


def _slices(P):
    return [(P * s // NORM_SLICES, P * (s + 1) // NORM_SLICES) for s in range(NORM_SLICES)]


def emu_norm_forward(x, G, P, C, gamma, beta, relu, mutation=None):
    """norm_partial_kernel (mode 0) + norm_stats_final_kernel + norm_apply_kernel."""
    x = x.reshape(G, P, C)
    x0 = x[:, 0].astype(np.float64)                                      # the shift: the group's first pixel
    xd = x.astype(np.float64) - x0[:, None]
    a, b = np.zeros((G, C)), np.zeros((G, C))
    for s, (lo, hi) in enumerate(_slices(P)):
        if mutation == 'one pixel dropped from one slice' and s == 100:
            assert hi > lo
            hi -= 1
        a += xd[:, lo:hi].sum(axis=1)
        b += (xd[:, lo:hi] ** 2).sum(axis=1)
    inv = 1.0 / P
    mu = a * inv
    var = np.maximum(b * inv - mu * mu, 0.0)
    if mutation == 'unbiased variance':
        var = var * P / (P - 1)
    eps = np.float64(f32(1e-5) if mutation == 'eps = 1e-5' else f32(1e-3))
    mean, rstd, var = (x0 + mu).astype(f32), (1.0 / np.sqrt(var + eps)).astype(f32), var.astype(f32)
    y = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    if relu:
        y = np.maximum(y, f32(0))
    assert y.dtype == np.float32
    return y, mean, rstd, var


def emu_norm_backward(x, dy, mean, rstd, gamma, G, P, C, mutation=None):
    """norm_partial_kernel (mode 1) + norm_bwd_final_kernel + norm_bwd_dx_kernel."""
    x, dy = x.reshape(G, P, C), dy.reshape(G, P, C)
    mean, rstd = mean.reshape(G, 1, C), rstd.reshape(G, 1, C)
    xh = (x - mean) * rstd
    prod = dy.astype(np.float64) * ((x.astype(np.float64) - mean) * rstd.astype(np.float64))      # the sums' products are float64
    a, b = np.zeros((G, C)), np.zeros((G, C))
    for s, (lo, hi) in enumerate(_slices(P)):
        if mutation == 'one pixel dropped from one slice' and s == 100:
            assert hi > lo
            hi -= 1
        a += dy[:, lo:hi].astype(np.float64).sum(axis=1)
        b += prod[:, lo:hi].sum(axis=1)
    dgamma, dbeta = b.sum(axis=0).astype(f32), a.sum(axis=0).astype(f32)
    if mutation == 'dgamma and dbeta swapped':
        dgamma, dbeta = dbeta, dgamma
    inv = 1.0 / P
    m1, m2 = (a * inv).astype(f32)[:, None], (b * inv).astype(f32)[:, None]
    if mutation == 'mean dy dropped from dx':
        m1 = np.zeros_like(m1)
    dx = gamma * rstd * (dy - m1 - xh * m2)
    assert dx.dtype == np.float32
    return dx, dgamma, dbeta


def _sigmoid32(v):
    with np.errstate(over='ignore'):
        return f32(1) / (f32(1) + np.exp(-v))


def emu_gate_zr(a, h, C, mutation=None):
    a = a.reshape(-1, 2 * C)
    lo, hi = (a[:, C:], a[:, :C]) if mutation == 'z and r halves swapped' else (a[:, :C], a[:, C:])
    z, r = _sigmoid32(lo), _sigmoid32(hi)
    return z, r, r * h.reshape(-1, C)


def emu_gate_q(a, z, h):
    q = np.tanh(a)
    return q, (f32(1) - z) * h + z * q


def _fma(a, b, c):
    """One rounding of a * b + c (the float64 product of two float32 is exact; the second rounding is far below)."""
    return (a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def emu_gate_q_backward(g, z, q, h):
    one = f32(1)
    return g * (q - h) * z * (one - z), g * z * _fma(-q, q, one), g * (one - z)


def emu_gate_r_backward(g, r, h, dh, mutation=None):
    dr = g * h * r * (f32(1) - r)
    return dr, (g * r if mutation == 'dh overwritten' else _fma(g, r, dh))


# ------------------------------------------------------------------------------------------------ shared cases

def adamw_case(rng, n, scale, zero_every=7):
    """Weights of magnitude in [0.05, 1] (see assert_adamw_close), non-zero slots at the gradient's scale, one gradient in seven 0."""
    var = (rng.uniform(0.05, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(f32)
    m = (0.3 * scale * rng.normal(size=n)).astype(f32)
    v = (scale * scale * rng.uniform(0.2, 2.0, n)).astype(f32)
    grads = []
    for _ in range(3):
        g = (scale * rng.normal(size=n)).astype(f32)
        g[::zero_every] = 0
        grads.append(g)
    return var, m, v, grads


def lr_t_of(lr, t):
    return f32(lr * math.sqrt(1.0 - float(B2) ** t) / (1.0 - float(B1) ** t))


def norm_case(rng, G, P, C):
    """x with one channel of mean 100 and spread 0.01 and one constant channel; gamma, beta, dy."""
    x = rng.normal(size=(G, P, C)).astype(f32)
    x[..., 3] = (100.0 + 0.01 * rng.normal(size=(G, P))).astype(f32)
    x[..., 5] = f32(2.5)
    gamma = rng.uniform(0.5, 1.5, C).astype(f32)
    beta = rng.uniform(-0.2, 0.2, C).astype(f32)
    dy = rng.normal(size=(G, P, C)).astype(f32)
    return x, gamma, beta, dy


NORM_CASES = [('instance', 2, 35, 96), ('instance', 3, 300, 64), ('instance', 2, 1, 32), ('batch', 1, 1536, 128),
              ('batch', 1, 1031, 160)]


def gate_case(rng, M, C):
    """Pre-activations N(0, 3) with planted +-20 and +-90, h = tanh(N(0, 1)), upstreams N(0, 1)."""
    a_zr = (3.0 * rng.normal(size=(M, 2 * C))).astype(f32)
    a_q = (3.0 * rng.normal(size=(M, C))).astype(f32)
    planted = np.array([20.0, -20.0, 90.0, -90.0], dtype=f32)
    a_zr[0, :4] = a_zr[1, C:C + 4] = a_zr[M - 1, 2 * C - 4:] = planted
    a_q[0, :4] = a_q[M - 1, C - 4:] = planted
    h = np.tanh(rng.normal(size=(M, C))).astype(f32)
    ups = [rng.normal(size=(M, C)).astype(f32) for _ in range(3)]
    return a_zr, a_q, h, ups


# ------------------------------------------------------------------------------------------------ anchors

@pytest.mark.parametrize('scale', SCALES)
def test_adamw_reference_matches_torch_adam(rng, scale):
    """Keras' update is torch's with eps / sqrt(1 - beta2^t) and the decoupled decay p *= 1 - wd applied by hand."""
    n, lr, wd, b1, b2, eps = 257, 4e-4, 1e-4, 0.9, 0.999, 1e-7
    var0 = rng.normal(size=n)
    grads = [scale * rng.normal(size=n) for _ in range(3)]
    p = torch.tensor(var0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    steps = ref.adamw_steps(var0, np.zeros(n), np.zeros(n), grads, lr, b1, b2, eps, wd)
    worst = 0.0
    for t, g in enumerate(grads, start=1):
        opt.param_groups[0]['eps'] = eps / math.sqrt(1.0 - b2 ** t)
        with torch.no_grad():
            p.mul_(1.0 - wd)
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        st = opt.state[p]
        for got, want in ((steps[t - 1]['var'], p.detach().numpy()), (steps[t - 1]['m'], st['exp_avg'].numpy()),
                          (steps[t - 1]['v'], st['exp_avg_sq'].numpy())):
            worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    report(f'adamw_steps vs torch.optim.Adam scale {scale:g}', worst_rel=worst)
    assert worst <= 1e-14


def _torch_norm(kind, x, gamma, beta, dy, G, P, C):
    xt = torch.tensor(x, dtype=torch.float64).reshape(G, P, C).requires_grad_(True)
    gt, bt = (torch.tensor(t, dtype=torch.float64).requires_grad_(True) for t in (gamma, beta))
    if P == 1:                                         # torch refuses instance_norm over one element: the definition itself
        mu = xt.mean(dim=1, keepdim=True)
        y = (xt - mu) / torch.sqrt(xt.var(dim=1, unbiased=False, keepdim=True) + 1e-3) * gt + bt
    elif kind == 'instance':
        y = torch.nn.functional.instance_norm(xt.permute(0, 2, 1), weight=gt, bias=bt, eps=1e-3).permute(0, 2, 1)
    else:
        y = torch.nn.functional.batch_norm(xt.reshape(P, C), None, None, weight=gt, bias=bt, training=True, eps=1e-3).reshape(G, P, C)
    y.backward(torch.tensor(dy, dtype=torch.float64).reshape(G, P, C))
    return y.detach().numpy(), xt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize('kind,G,P,C', [('instance', 2, 35, 96), ('batch', 1, 1031, 160), ('instance', 2, 1, 32)])
def test_norm_references_match_torch_autograd(rng, kind, G, P, C):
    x, gamma, beta, dy = norm_case(rng, G, P, C)
    y, mean, rstd, var = ref.norm_forward(x, G, P, C, gamma, beta, 1e-3, False)
    dx, dgamma, dbeta = ref.norm_backward(x, dy, mean, rstd, gamma, G, P, C)
    ty, tdx, tdg, tdb = _torch_norm(kind, x, gamma, beta, dy, G, P, C)
    errs = {}
    for name, got, want in (('y', y, ty), ('dx', dx, tdx), ('dgamma', dgamma, tdg), ('dbeta', dbeta, tdb)):
        errs[name] = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
    report(f'norm references vs torch {kind} ({G}, {P}, {C})', **errs)
    # the channel of mean 100 / spread 0.01 loses 1e4 / 1e-2 of float64's 1e-16 in torch's own single-pass statistics
    assert max(errs.values()) <= 1e-9
    ok = np.ones(C, bool)
    ok[3] = False
    assert np.abs(y[..., ok] - ty[..., ok]).max() <= 1e-12 and np.abs(dx[..., ok] - tdx[..., ok]).max() <= 1e-12
    if P == 1:
        assert np.array_equal(dx, np.zeros_like(dx)) and np.allclose(rstd, 1.0 / math.sqrt(1e-3), rtol=1e-15)


def test_gate_references_match_torch_autograd(rng):
    M, C = 15, 96
    a_zr, a_q, h, (d_hn, d_rh, dh0) = gate_case(rng, M, C)
    t = lambda v: torch.tensor(v, dtype=torch.float64).requires_grad_(True)      # noqa: E731
    az, ar, aq, ht, ht2 = t(a_zr[:, :C]), t(a_zr[:, C:]), t(a_q), t(h), t(h)
    zt, rt, qt = torch.sigmoid(az), torch.sigmoid(ar), torch.tanh(aq)
    hn = (1 - zt) * ht + zt * qt
    hn.backward(torch.tensor(d_hn, dtype=torch.float64))
    rh = rt * ht2
    rh.backward(torch.tensor(d_rh, dtype=torch.float64))
    z, r, rh_ref = ref.gate_zr(a_zr, h, C)
    q, hn_ref = ref.gate_q(a_q, z, h)
    dz, dq, dh = ref.gate_q_backward(d_hn, z, q, h)
    dr, dh_acc = ref.gate_r_backward(d_rh, r, h, dh0)
    worst = 0.0
    for got, want in ((z, zt), (r, rt), (rh_ref, rh), (q, qt), (hn_ref, hn), (dz, az.grad), (dq, aq.grad), (dh, ht.grad),
                      (dr, ar.grad), (dh_acc - dh0, ht2.grad)):
        worst = max(worst, float(np.abs(got - want.detach().numpy()).max()))
    report('gate references vs torch autograd', max_abs=worst)
    assert worst <= 1e-14


def test_clip_scale_follows_tensorflow():
    assert math.isnan(ref.clip_scale(float('inf'), 1.0)) and math.isnan(ref.clip_scale(float('nan'), 1.0))
    assert ref.clip_scale(1.0, 1.0) == 1.0 and ref.clip_scale(0.25, 1.0) == 1.0 and ref.clip_scale(0.0, 1.0) == 1.0
    assert ref.clip_scale(9.0, 1.0) == 1.0 / 9.0
    assert ref.sumsq([np.array([1e20, 1e-30], f32), np.array([3.0], f32)]) == float(f32(1e20)) ** 2 + 9.0


def test_oracle_stub_clip_by_global_norm_sets_nan_for_a_non_finite_norm():
    """oracle/tfstub stands in for TensorFlow under the reference's source: the same rule there."""
    import importlib
    from oracle import reference_runner
    with reference_runner._stub_on_path():             # the stub alone: it needs no reference tree
        tf = importlib.import_module('tensorflow')
    a, b = torch.tensor([3.0, 4.0]), torch.tensor([12.0])
    out, norm = tf.clip_by_global_norm([a, b], 1.0)
    assert float(norm) == 13.0 and torch.allclose(out[0], a / 13.0) and torch.allclose(out[1], b / 13.0)
    out, norm = tf.clip_by_global_norm([a, b], 13.0)
    assert torch.equal(out[0], a) and torch.equal(out[1], b)
    for bad in (float('inf'), float('nan')):
        out, norm = tf.clip_by_global_norm([a, torch.tensor([bad])], 1.0)
        assert not math.isfinite(float(norm))
        assert all(bool(torch.isnan(t).all()) for t in out)


# ------------------------------------------------------------------------------------------------ sensitivity

def _adamw_run(rng, scale, wd, mutation, clip_factor):
    """Three steps of the emulation, each compared with the float64 step from the emulation's own float32 state.
    ``clip_factor``: None = no clipping, else clip_norm = clip_factor * the gradient's norm."""
    n = 1000
    var, m, v, grads = adamw_case(rng, n, scale)
    worst = 0.0
    for t, g in enumerate(grads, start=1):
        lr_t = lr_t_of(4e-4, t)
        gnsq = clip = None
        scales = None
        if clip_factor is not None:
            gnsq = ref.sumsq([g])
            clip = f32(clip_factor * math.sqrt(gnsq))
            scales = [ref.clip_scale(math.sqrt(gnsq), float(clip))]
        want = ref.adamw_steps(var, m, v, [g], None, float(B1), float(B2), float(EPS), float(f32(wd)), scales=scales,
                               lr_t=[float(lr_t)])[0]
        var, m, v = emu_adamw(var, g, m, v, lr_t, wd, gnsq, clip if clip is not None else 0.0, mutation)
        worst = max(worst, ref.assert_adamw_close((var, m, v), want, f'emulation step {t}'))
    return worst


@pytest.mark.parametrize('scale', SCALES)
def test_adamw_emulation_is_inside_the_bound(rng, scale):
    for wd in (0.0, 1e-4):
        for clip_factor in (None, 2.0, 1.0, 1.0 / 9.0):
            worst = _adamw_run(rng, scale, wd, None, clip_factor)
            report(f'adamw emulation scale {scale:g} wd {wd:g} clip factor {clip_factor}', worst_in_units_of_bound=worst)


@pytest.mark.parametrize('mutation,scale,clip_factor', [('clip scale off by 1e-3', 1.0, 1.0 / 9.0), ('clip scale off by 1e-3', 1e4, 1.0 / 9.0),
                                                        ('decay multiplied by lr', 1.0, None), ('eps inside the square root', 1e-8, None),
                                                        ('beta2 where beta1 belongs', 1.0, None), ('beta2 where beta1 belongs', 1e-8, 2.0)])
def test_adamw_bound_rejects(rng, mutation, scale, clip_factor):
    with pytest.raises(AssertionError):
        _adamw_run(rng, scale, 1e-4, mutation, clip_factor)


def test_adamw_emulation_follows_the_non_finite_rule(rng):
    var, m, v, grads = adamw_case(rng, 100, 1.0)
    for bad in (float('inf'), float('nan')):
        want = ref.adamw_steps(var, m, v, [grads[0]], None, float(B1), float(B2), float(EPS), 0.0, scales=[ref.clip_scale(bad, 1.0)],
                               lr_t=[1e-3])[0]
        assert all(np.isnan(want[k]).all() for k in ('var', 'm', 'v'))
        ref.assert_adamw_close(emu_adamw(var, grads[0], m, v, 1e-3, 0.0, bad, 1.0), want)
        with pytest.raises(AssertionError):                               # the kernel before the rule: scale 0 or 1, finite weights
            finite = emu_adamw(var, grads[0], m, v, 1e-3, 0.0, None)
            ref.assert_adamw_close(finite, want)


def _norm_run(rng, G, P, C, relu, fwd_mutation=None, bwd_mutation=None):
    x, gamma, beta, dy = norm_case(rng, G, P, C)
    got = emu_norm_forward(x, G, P, C, gamma, beta, relu, fwd_mutation)
    wf = ref.assert_norm_forward_close(got, x, G, P, C, gamma, beta, relu)
    y, mean, rstd, _ = got
    if relu:
        dy = np.where(y > 0, dy, f32(0)).astype(f32)
    wb = ref.assert_norm_backward_close(emu_norm_backward(x, dy, mean, rstd, gamma, G, P, C, bwd_mutation), x, dy, mean, rstd,
                                        gamma, G, P, C)
    return wf, wb


@pytest.mark.parametrize('kind,G,P,C', NORM_CASES)
@pytest.mark.parametrize('relu', [0, 1])
def test_norm_emulation_is_inside_the_bounds(rng, kind, G, P, C, relu):
    wf, wb = _norm_run(rng, G, P, C, relu)
    report(f'norm emulation {kind} ({G}, {P}, {C}) relu {relu}', forward_in_units_of_bound=wf, backward_in_units_of_bound=wb)


@pytest.mark.parametrize('mutation', ['unbiased variance', 'eps = 1e-5', 'one pixel dropped from one slice'])
def test_norm_forward_bound_rejects(rng, mutation):
    with pytest.raises(AssertionError):
        _norm_run(rng, 3, 300, 64, 0, fwd_mutation=mutation)


@pytest.mark.parametrize('mutation', ['mean dy dropped from dx', 'dgamma and dbeta swapped', 'one pixel dropped from one slice'])
def test_norm_backward_bound_rejects(rng, mutation):
    with pytest.raises(AssertionError):
        _norm_run(rng, 3, 300, 64, 0, bwd_mutation=mutation)


def _gates_run(rng, C, zr_mutation=None, r_mutation=None):
    M = 15
    a_zr, a_q, h, (d_hn, d_rh, dh0) = gate_case(rng, M, C)
    z, r, rh = emu_gate_zr(a_zr, h, C, zr_mutation)
    tol_s, tol_t = ref.activation_tolerance(a_zr, 'sigmoid'), ref.activation_tolerance(a_q, 'tanh')
    w = [ref.assert_gates_forward_close((z, r, rh), ref.gate_zr(a_zr, h, C), tol_s, 'gate_zr')]
    q, hn = emu_gate_q(a_q, z, h)
    w.append(ref.assert_gates_forward_close((q, hn), ref.gate_q(a_q, z, h), max(tol_s, tol_t), 'gate_q'))
    w.append(ref.assert_gates_backward_close(emu_gate_q_backward(d_hn, z, q, h), ref.gate_q_backward(d_hn, z, q, h), 'gate_q_bwd'))
    w.append(ref.assert_gates_backward_close(emu_gate_r_backward(d_rh, r, h, dh0, r_mutation), ref.gate_r_backward(d_rh, r, h, dh0),
                                             'gate_r_bwd'))
    return max(w)


@pytest.mark.parametrize('C', [128, 96])
def test_gate_emulation_is_inside_the_bounds(rng, C):
    report(f'gate emulation C {C}', worst_in_units_of_bound=_gates_run(rng, C))


def test_gate_bounds_reject(rng):
    with pytest.raises(AssertionError):
        _gates_run(rng, 96, zr_mutation='z and r halves swapped')
    with pytest.raises(AssertionError):
        _gates_run(rng, 96, r_mutation='dh overwritten')


def test_axpby_and_sumsq_bounds(rng):
    a, b = rng.normal(size=257).astype(f32), rng.normal(size=257).astype(f32)
    ref.assert_axpby_close(f32(0.25) * a + f32(-2.0) * b, ref.axpby(0.25, a, -2.0, b))
    ref.assert_axpby_close(np.maximum(f32(1.7) * a, f32(0)), ref.axpby_relu(float(f32(1.7)), a, 0.0))
    with pytest.raises(AssertionError):
        ref.assert_axpby_close(f32(0.25) * a + f32(2.0) * b, ref.axpby(0.25, a, -2.0, b))
    with pytest.raises(AssertionError):                                   # an fp32 accumulation is not the double path
        x = rng.normal(size=4097).astype(f32)
        ref.assert_sumsq_close(float(np.sum(x * x, dtype=f32)), ref.sumsq([x]), x.size)

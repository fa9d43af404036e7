"""The small kernels of the training step (csrc/backward.hip), each called through the C ABI with raw device pointers on the
current stream and compared with the float64 references of tests/train_kernels_ref.py through the comparison functions that
tests/test_train_kernels.py shows to reject subtly wrong kernels:

  raft_sumsq_f32, raft_sumsq_multi_f32                      the global norm of tf.clip_by_global_norm
  raft_adamw_step_f32, raft_adamw_step_multi_f32            tfa AdamW, alone and through training.AdamW.apply_gradients
  raft_norm_forward_f32, raft_norm_backward_f32             instance / batch normalisation in training form
  raft_gru_gate_zr_f32, _q_f32, _q_backward_f32, _r_backward_f32
  raft_axpby_f32, raft_axpby_relu_f32

Every bound is derived in the docstring of its ``assert_*_close`` or is a multiple of torch's own float32 error computed here;
every test prints its worst error in units of its bound.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import train_kernels_ref as ref
from conftest import report
from test_train_kernels import B1, B2, EPS, NORM_CASES, SCALES, adamw_case, gate_case, lr_t_of, norm_case

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = -12345.678
GUARD = 64


def _lib():
    from tf_raft_amd import _dev
    return _dev.lib()


def _call(name, *args):
    from tf_raft_amd import _dev
    from tf_raft_amd._ffi import check
    check(getattr(_dev.lib(), name)(*args, _dev.stream_ptr()), name)


def dev(a, dtype=torch.float32):
    from tf_raft_amd import _dev
    return _dev.to_device(np.ascontiguousarray(a), dtype=dtype)


def host(t):
    return t.detach().cpu().numpy()


def ptr(t):
    return None if t is None else t.data_ptr()


def ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def sizes(ts):
    return (C.c_int64 * len(ts))(*[t.numel() for t in ts])


def workspace(n):
    """Exactly ``n`` doubles of NaN followed by a guard region of a sentinel."""
    buf = torch.full((n + GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    buf[n:] = SENTINEL
    return buf


def guard_intact(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def empty_like(t, count=1):
    out = [torch.full_like(t, float('nan')) for _ in range(count)]
    return out[0] if count == 1 else out


# ------------------------------------------------------------------------------------------------ sum of squares

def _sumsq_input(rng, n, kind):
    """'plain' N(0, 1); 'huge' / 'tiny': every element around 1e20 / 1e-30, whose squares leave the float32 range."""
    if kind == 'plain':
        return rng.normal(size=n).astype(f32)
    x = (rng.uniform(0.5, 1.5, n) * (1e20 if kind == 'huge' else 1e-30)).astype(f32)
    x[0] = f32(1e20 if kind == 'huge' else 1e-30)
    return x


@pytest.mark.parametrize('n', [1, 255, 256, 257, 131071, 131075])
def test_sumsq_single_tensor(rng, n):
    """131075 = 512 workgroups x 256 + 3: a second grid-stride trip.  accumulate = 1 adds to a prefilled *out of the same
    magnitude (one more non-negative term: still inside n 2**-52)."""
    nws = int(_lib().raft_sumsq_workspace_doubles())
    worst = 0.0
    for kind in ('plain', 'huge', 'tiny'):
        x = _sumsq_input(rng, n, kind)
        want = ref.sumsq([x])
        assert 0 < want < float('inf')
        x_d = dev(x)
        for accumulate in (0, 1):
            pre = 0.37 * want
            results = []
            for _ in range(2):
                ws = workspace(nws)
                out = torch.full((1,), pre if accumulate else float('nan'), dtype=torch.float64, device='cuda')
                _call('raft_sumsq_f32', ptr(x_d), n, accumulate, ptr(out), ptr(ws))
                results.append(out.clone())
                assert guard_intact(ws, nws)
            assert torch.equal(results[0].view(torch.int64), results[1].view(torch.int64)), 'not bitwise repeatable'
            worst = max(worst, ref.assert_sumsq_close(float(results[0]), want + (pre if accumulate else 0.0), n,
                                                      f'sumsq n {n} {kind} accumulate {accumulate}'))
    report(f'raft_sumsq_f32 n {n}', worst_in_units_of_bound=worst)


MULTI_SIZES = (1, 2, 64, 255, 256, 257, 4097, 36864)


@pytest.mark.parametrize('count', [1, 63, 64, 65, 129, 154])
def test_sumsq_multi(rng, count):
    """64 tensors per launch: 63 / 64 / 65 / 129 / 154 around the chunk edges; 4097 = one past 16 workgroups x 256.  The
    workspace is exactly as long as the library says, NaN beforehand (a partial the final sum reads before it is written would
    make the result NaN) and followed by a guard."""
    xs = [(rng.uniform(0.5, 2.0) * rng.normal(size=MULTI_SIZES[k % len(MULTI_SIZES)])).astype(f32) for k in range(count)]
    n_total = sum(x.size for x in xs)
    want = ref.sumsq(xs)
    xs_d = [dev(x) for x in xs]
    nws = int(_lib().raft_sumsq_multi_workspace_doubles(count))
    assert nws == 16 * count
    results = []
    for _ in range(2):
        ws = workspace(nws)
        out = torch.full((1,), float('nan'), dtype=torch.float64, device='cuda')
        _call('raft_sumsq_multi_f32', ptrs(xs_d), sizes(xs_d), count, ptr(out), ptr(ws))
        results.append(out.clone())
        assert guard_intact(ws, nws)
        assert not bool(torch.isnan(ws[:nws]).any()), 'a partial was never written'
    assert torch.equal(results[0].view(torch.int64), results[1].view(torch.int64)), 'not bitwise repeatable'
    worst = ref.assert_sumsq_close(float(results[0]), want, n_total, f'sumsq_multi count {count}')
    ws1 = workspace(int(_lib().raft_sumsq_workspace_doubles()))
    chain = torch.full((1,), float('nan'), dtype=torch.float64, device='cuda')
    for k, x_d in enumerate(xs_d):
        _call('raft_sumsq_f32', ptr(x_d), x_d.numel(), 1 if k else 0, ptr(chain), ptr(ws1))
    worst = max(worst, ref.assert_sumsq_close(float(chain), want, n_total, f'sumsq chain count {count}'))
    report(f'raft_sumsq_multi_f32 count {count}', n_total=n_total, worst_in_units_of_bound=worst)


# ------------------------------------------------------------------------------------------------ AdamW

def _norm_sq(grads_d):
    """The device's own squared global norm, as training.AdamW.global_norm_sq computes it."""
    n = len(grads_d)
    nws = int(_lib().raft_sumsq_multi_workspace_doubles(n))
    ws = workspace(nws)
    out = torch.full((1,), float('nan'), dtype=torch.float64, device='cuda')
    _call('raft_sumsq_multi_f32', ptrs(grads_d), sizes(grads_d), n, ptr(out), ptr(ws))
    assert guard_intact(ws, nws)
    return out


def _adamw_single(state, grads_d, lr_t, wd, gnsq, clip):
    for (var, m, v), g in zip(state, grads_d):
        _call('raft_adamw_step_f32', ptr(var), ptr(g), ptr(m), ptr(v), var.numel(), float(lr_t), float(B1), float(B2), float(EPS),
              float(wd), ptr(gnsq), float(clip))


def _adamw_multi(state, grads_d, lr_t, wd, gnsq, clip):
    vs, ms, ss = ([s[k] for s in state] for k in range(3))
    _call('raft_adamw_step_multi_f32', ptrs(vs), ptrs(grads_d), ptrs(ms), ptrs(ss), sizes(vs), len(vs), float(lr_t), float(B1),
          float(B2), float(EPS), float(wd), ptr(gnsq), float(clip))


CLIP_CASES = ('none', 'inactive', 'equal', 'active')


@pytest.mark.parametrize('wd', [0.0, 1e-4])
@pytest.mark.parametrize('scale', SCALES)
def test_adamw_three_steps(rng, scale, wd):
    """Both kernels, three consecutive steps from non-zero slots, every clip case, the norm from the device's own
    raft_sumsq_multi_f32.  Each step is compared with the float64 step from the float32 state the kernel started from, with
    the hyperparameters rounded to float32 as the kernel receives them; the multi kernel must equal the single one bit for bit."""
    shapes = (1, 255, 257, 4099)
    worst = {}
    for clip_case in CLIP_CASES:
        cases = [adamw_case(rng, n, scale) for n in shapes]
        single = [[dev(t) for t in c[:3]] for c in cases]
        multi = [[dev(t) for t in c[:3]] for c in cases]
        w = 0.0
        for t in range(1, 4):
            before = [[host(x) for x in s] for s in single]
            grads = [c[3][t - 1] for c in cases]
            grads_d = [dev(g) for g in grads]
            lr_t = lr_t_of(4e-4, t)
            gnsq, clip, scales = None, 0.0, None
            if clip_case != 'none':
                gnsq = _norm_sq(grads_d)
                norm = math.sqrt(float(gnsq))
                ref.assert_sumsq_close(float(gnsq), ref.sumsq(grads), sum(shapes), 'global norm')
                clip = float(f32(norm * {'inactive': 2.0, 'equal': 1.0, 'active': 1.0 / 9.0}[clip_case]))
                scales = [ref.clip_scale(norm, clip)]
                if clip_case == 'equal':
                    assert f32(norm) == f32(clip)
            _adamw_single(single, grads_d, lr_t, wd, gnsq, clip)
            _adamw_multi(multi, grads_d, lr_t, wd, gnsq, clip)
            for k, n in enumerate(shapes):
                want = ref.adamw_steps(*before[k], [grads[k]], None, float(B1), float(B2), float(EPS), float(f32(wd)), scales=scales,
                                       lr_t=[float(lr_t)])[0]
                got = [host(x) for x in single[k]]
                w = max(w, ref.assert_adamw_close(got, want, f'adamw {clip_case} step {t} n {n}'))
                for a, b, name in zip(got, multi[k], ('var', 'm', 'v')):
                    assert np.array_equal(a.view(np.uint32), host(b).view(np.uint32)), f'multi != single: {name} {clip_case} step {t} n {n}'
        worst[clip_case] = w
    report(f'raft_adamw_step(_multi)_f32 scale {scale:g} wd {wd:g} [units of bound]', **worst)


def _trainable_shapes():
    from tf_raft_amd import weights as wm
    return [(k, v.shape) for k, v in wm.init_weights('raft').items() if 'moving' not in k]


def _device_case(shapes, seed, grad_norm=None):
    """On-device values for big tensor lists (torch is plumbing here): weights of magnitude in [0.05, 1], slots, gradients
    with one element in seven 0, optionally scaled to a global norm of about ``grad_norm``."""
    gen = torch.Generator(device='cuda').manual_seed(seed)
    total = sum(int(np.prod(s)) for _, s in shapes)
    out = []
    for _, s in shapes:
        r = lambda: torch.rand(tuple(s), generator=gen, device='cuda')              # noqa: E731
        var = (0.05 + 0.95 * r()) * torch.where(r() < 0.5, -1.0, 1.0)
        g = torch.randn(tuple(s), generator=gen, device='cuda')
        g.view(-1)[::7] = 0
        if grad_norm is not None:
            g *= grad_norm / math.sqrt(total * 6.0 / 7.0)
        out.append((var.contiguous(), (0.3 * torch.randn(tuple(s), generator=gen, device='cuda')).contiguous(),
                    (0.2 + r()).contiguous(), g.contiguous()))
    return out


@pytest.mark.parametrize('count', [1, 64, 65, 154])
def test_adamw_multi_equals_single_on_the_model_shapes(count):
    """The multi kernel claims the single kernel's arithmetic "statement for statement": bitwise equality tensor by tensor on
    the model's real trainable shapes (a 1-element and a 590 k-element tensor share a chunk), 64 / 65 at the chunk edge."""
    shapes = _trainable_shapes()
    assert len(shapes) == 154
    shapes = shapes[:count]
    case = _device_case(shapes, seed=count)
    grads_d = [c[3] for c in case]
    single = [[t.clone() for t in c[:3]] for c in case]
    multi = [[t.clone() for t in c[:3]] for c in case]
    gnsq = _norm_sq(grads_d)
    clip = 0.5 * math.sqrt(float(gnsq))
    _adamw_single(single, grads_d, lr_t_of(4e-4, 2), 1e-4, gnsq, clip)
    _adamw_multi(multi, grads_d, lr_t_of(4e-4, 2), 1e-4, gnsq, clip)
    for (name, _), s, m, c in zip(shapes, single, multi, case):
        for a, b, before in zip(s, m, c[:3]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
            assert not torch.equal(a, before), name                        # and the step did something
    sizes_ = sorted(int(np.prod(s)) for _, s in shapes)
    report(f'adamw multi == single, {count} tensors', smallest=sizes_[0], largest=sizes_[-1])


def test_adamw_apply_gradients_on_the_model_shapes():
    """training.AdamW.apply_gradients itself: 154 tensors in chunks of 64 / 64 / 26, CyclicalLearningRate, clip_norm = 1 under
    a gradient norm of about 9, three steps from the optimizer's own zero slots, each step against float64 on the state before it."""
    from tf_raft_amd import training
    shapes = _trainable_shapes()
    names = [k for k, _ in shapes]
    offs = np.cumsum([0] + [int(np.prod(s)) for _, s in shapes])
    flat = lambda ts: np.concatenate([host(t).ravel() for t in ts])                  # noqa: E731
    variables = {k: c[0] for (k, _), c in zip(shapes, _device_case(shapes, seed=7))}
    sched = training.CyclicalLearningRate(1e-4, 4e-4, step_size=2)
    opt = training.AdamW(weight_decay=1e-4, learning_rate=sched)
    worst = 0.0
    m = v = np.zeros(offs[-1], f32)
    for t in range(1, 4):
        grads = {k: c[3] for (k, _), c in zip(shapes, _device_case(shapes, seed=100 + t, grad_norm=9.0))}
        w, g = flat(variables.values()), flat(grads.values())
        lr = sched(t - 1)
        gn = opt.apply_gradients(grads, variables, clip_norm=1.0)
        norm_sq = float(np.sum(g.astype(np.float64) ** 2))
        assert 8.0 < math.sqrt(norm_sq) < 10.0
        ref.assert_sumsq_close(float(gn), norm_sq, g.size, f'global norm step {t}')
        lr_t = f32(lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))       # as apply_gradients forms it, rounded as the kernel receives it
        want = ref.adamw_steps(w, m, v, [g], None, float(B1), float(B2), float(EPS), float(f32(1e-4)),
                               scales=[ref.clip_scale(math.sqrt(float(gn)), 1.0)], lr_t=[float(lr_t)])[0]
        got = (flat(variables.values()), flat(opt._slots[k][0] for k in names), flat(opt._slots[k][1] for k in names))
        worst = max(worst, ref.assert_adamw_close(got, want, f'apply_gradients step {t}'))
        _, m, v = got
    assert opt.iterations == 3
    report('training.AdamW.apply_gradients, 154 tensors, 3 steps', n=int(offs[-1]), worst_in_units_of_bound=worst)


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
def test_non_finite_global_norm_sets_everything_to_nan(rng, bad):
    """tf.clip_by_global_norm: "if global_norm == infinity then the entries in t_list are all set to NaN", and a NaN norm
    propagates alike.  One bad element in ONE tensor: every element of every variable, m and v is NaN after the step, in both
    kernels and through training.AdamW."""
    from tf_raft_amd import training
    shapes = (1, 300, 4099)
    cases = [adamw_case(rng, n, 1.0) for n in shapes]
    grads = [c[3][0].copy() for c in cases]
    grads[1][17] = bad
    grads_d = [dev(g) for g in grads]
    gnsq = _norm_sq(grads_d)
    assert not math.isfinite(float(gnsq))
    for step in (_adamw_single, _adamw_multi):
        state = [[dev(t) for t in c[:3]] for c in cases]
        step(state, grads_d, lr_t_of(4e-4, 1), 1e-4, gnsq, 1.0)
        for n, s in zip(shapes, state):
            for t, name in zip(s, ('var', 'm', 'v')):
                assert bool(torch.isnan(t).all()), f'{step.__name__} n {n}: {name} has {int((~torch.isnan(t)).sum())} finite elements'
    variables = {f'w{k}': dev(c[0]) for k, c in enumerate(cases)}
    opt = training.AdamW(weight_decay=1e-4, learning_rate=4e-4)
    gn = opt.apply_gradients({f'w{k}': g for k, g in enumerate(grads_d)}, variables, clip_norm=1.0)
    assert not math.isfinite(float(gn))
    for k, t in variables.items():
        assert bool(torch.isnan(t).all()) and all(bool(torch.isnan(s).all()) for s in opt._slots[k]), k


# ------------------------------------------------------------------------------------------------ normalisation layers

@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('kind,G,P,C', NORM_CASES)
def test_norm_forward_and_backward(rng, kind, G, P, C, relu):
    """(2, 35, 96): fewer pixels than the 256 slices, last channel chunk 32 wide; (3, 300, 64): uneven slices; (2, 1, 32): one
    pixel; (1, 1031, 160): three ragged channel chunks.  Channel 3 has mean 100 over a spread of 0.01, channel 5 is constant.
    With relu the upstream is masked by raft_relu_backward_f32 as grad._norm_bwd does."""
    x, gamma, beta, dy = norm_case(rng, G, P, C)
    x_d, gamma_d, beta_d, dy_d = dev(x), dev(gamma), dev(beta), dev(dy)
    nws = int(_lib().raft_norm_workspace_doubles(G, C))
    ws = workspace(nws)
    y_d = empty_like(x_d)
    mean_d, rstd_d, var_d = (torch.full((G, C), float('nan'), device='cuda') for _ in range(3))
    _call('raft_norm_forward_f32', ptr(x_d), G, P, C, ptr(gamma_d), ptr(beta_d), 1e-3, relu, ptr(y_d), ptr(mean_d), ptr(rstd_d),
          ptr(var_d), ptr(ws))
    assert guard_intact(ws, nws)
    y, mean, rstd, var = host(y_d), host(mean_d), host(rstd_d), host(var_d)
    wf = ref.assert_norm_forward_close((y, mean, rstd, var), x, G, P, C, gamma, beta, relu, what=f'norm forward {kind} ({G}, {P}, {C})')
    if P == 1:
        assert np.array_equal(rstd, np.full((G, C), f32(1.0 / math.sqrt(np.float64(f32(1e-3)))))) and np.array_equal(var, np.zeros((G, C), f32))
    if relu:
        masked_d = empty_like(dy_d)
        _call('raft_relu_backward_f32', ptr(y_d), ptr(dy_d), ptr(masked_d), dy_d.numel())
        dy = host(masked_d)
        assert np.array_equal(dy, np.where(y > 0, dy_d.cpu().numpy(), f32(0)))
        dy_d = masked_d
    ws = workspace(nws)
    dx_d = empty_like(x_d)
    dg_d, db_d = (torch.full((C,), float('nan'), device='cuda') for _ in range(2))
    _call('raft_norm_backward_f32', ptr(x_d), ptr(dy_d), ptr(mean_d), ptr(rstd_d), ptr(gamma_d), G, P, C, ptr(dx_d), ptr(dg_d), ptr(db_d),
          ptr(ws))
    assert guard_intact(ws, nws)
    dx = host(dx_d)
    wb = ref.assert_norm_backward_close((dx, host(dg_d), host(db_d)), x, dy, mean, rstd, gamma, G, P, C,
                                        what=f'norm backward {kind} ({G}, {P}, {C})')
    if P == 1:
        assert np.array_equal(dx, np.zeros_like(dx))
    report(f'raft_norm_forward/backward_f32 {kind} ({G}, {P}, {C}) relu {relu}', forward_in_units_of_bound=wf, backward_in_units_of_bound=wb)


# ------------------------------------------------------------------------------------------------ gates, axpby

@pytest.mark.parametrize('C_', [128, 96])
def test_gru_gates(rng, C_):
    """a_zr is (M, 2C): z from the first C columns, r from the last.  Pre-activations N(0, 3) with planted +-20 and +-90: no
    NaN, sigmoid(+20), sigmoid(+90) and tanh of all four exactly +-1, sigmoid(-90) exactly 0 (sigmoid(-20) = 2e-9 is a
    float32 like any other).  The backward kernels are checked given the device's own z, r, q."""
    M = 15
    a_zr, a_q, h, (d_hn, d_rh, dh0) = gate_case(rng, M, C_)
    a_zr_d, a_q_d, h_d = dev(a_zr), dev(a_q), dev(h)
    z_d, r_d, rh_d, q_d, hn_d = empty_like(h_d, 5)
    _call('raft_gru_gate_zr_f32', ptr(a_zr_d), ptr(h_d), C_, M, ptr(z_d), ptr(r_d), ptr(rh_d))
    z, r, rh = host(z_d), host(r_d), host(rh_d)
    tol_s, tol_t = ref.activation_tolerance(a_zr, 'sigmoid'), ref.activation_tolerance(a_q, 'tanh')
    w_zr = ref.assert_gates_forward_close((z, r, rh), ref.gate_zr(a_zr, h, C_), tol_s, 'gate_zr')
    for got, a in ((z, a_zr[:, :C_]), (r, a_zr[:, C_:])):
        assert np.all(got[a >= 20] == 1) and np.all(got[a <= -90] == 0) and (a >= 20).sum() >= 2 and (a <= -90).sum() >= 1
    _call('raft_gru_gate_q_f32', ptr(a_q_d), ptr(z_d), ptr(h_d), M * C_, ptr(q_d), ptr(hn_d))
    q, hn = host(q_d), host(hn_d)
    w_q = ref.assert_gates_forward_close((q, hn), ref.gate_q(a_q, z, h), max(tol_s, tol_t), 'gate_q')
    assert np.all(q[a_q >= 20] == 1) and np.all(q[a_q <= -20] == -1) and (np.abs(a_q) >= 20).sum() >= 8
    d_hn_d, d_rh_d = dev(d_hn), dev(d_rh)
    dz_d, dq_d, dh_d, dr_d = empty_like(h_d, 4)
    _call('raft_gru_gate_q_backward_f32', ptr(d_hn_d), ptr(z_d), ptr(q_d), ptr(h_d), M * C_, ptr(dz_d), ptr(dq_d), ptr(dh_d))
    w_qb = ref.assert_gates_backward_close((host(dz_d), host(dq_d), host(dh_d)), ref.gate_q_backward(d_hn, z, q, h), 'gate_q_backward')
    acc_d = dev(dh0)
    _call('raft_gru_gate_r_backward_f32', ptr(d_rh_d), ptr(r_d), ptr(h_d), M * C_, ptr(dr_d), ptr(acc_d))
    w_rb = ref.assert_gates_backward_close((host(dr_d), host(acc_d)), ref.gate_r_backward(d_rh, r, h, dh0), 'gate_r_backward')
    report(f'GRU gates C {C_} [units of bound]', gate_zr=w_zr, gate_q=w_q, gate_q_backward=w_qb, gate_r_backward=w_rb,
           sigmoid_tolerance=tol_s, tanh_tolerance=tol_t)


@pytest.mark.parametrize('n', [1, 257])
def test_axpby(rng, n):
    """Factors whose products are exact (1, 0.25, -2: the sums the training step forms) with b, a general factor without b."""
    a, b = rng.normal(size=n).astype(f32), rng.normal(size=n).astype(f32)
    a_d, b_d = dev(a), dev(b)
    worst = 0.0
    for name, fn in (('raft_axpby_f32', ref.axpby), ('raft_axpby_relu_f32', ref.axpby_relu)):
        for alpha, beta, with_b in ((1.0, 1.0, True), (0.25, -2.0, True), (float(f32(1.7)), 0.0, False), (float(f32(-0.3)), 5.0, False)):
            out_d = empty_like(a_d)
            _call(name, alpha, ptr(a_d), beta, ptr(b_d) if with_b else None, ptr(out_d), n)
            worst = max(worst, ref.assert_axpby_close(host(out_d), fn(alpha, a, beta, b if with_b else None), f'{name} {alpha} {beta} {with_b}'))
    report(f'raft_axpby(_relu)_f32 n {n}', worst_in_spacings=worst)

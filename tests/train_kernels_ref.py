"""What the tests of the training step's small kernels share (csrc/backward.hip: sum of squares, AdamW, the normalisation layers,
the GRU gates, axpby): plain NumPy float64 references of each operation and ONE comparison function per kernel family that holds
the bound.  tests/test_train_kernels.py anchors the references to torch and shows that each bound rejects a subtly wrong kernel
(on fp32 emulations, no GPU); tests/test_gpu_train_kernels.py puts the device's results through the same functions.

Every ``assert_*_close`` raises AssertionError and otherwise returns the worst error it saw in units of its bound (<= 1).
``U`` = 2**-24 is the unit roundoff of float32: one rounding moves a value by at most ``U * |value|``.
"""
import math

import numpy as np

U = 2.0 ** -24
F32_EPS_NORM = float(np.float32(1e-3))          # eps of both normalisation layers as the kernel receives it


def f64(x):
    return np.asarray(x, dtype=np.float64)


def _worst(err, bound, what):
    """max(err / bound) with 0 / 0 = 0; NaN anywhere in ``err`` fails."""
    err, bound = np.broadcast_arrays(f64(err), f64(bound))
    if err.size == 0:
        return 0.0
    assert not np.isnan(err).any(), f'{what}: NaN where the reference is finite'
    assert not np.isnan(bound).any(), f'{what}: the bound itself is NaN'
    over = err > bound
    if over.any():
        k = int(np.argmax(np.where(over, err - bound, 0.0)))
        raise AssertionError(f'{what}: {int(over.sum())} of {err.size} outside the bound; furthest at flat index {k}: '
                             f'error {err.ravel()[k]:.6e} against bound {bound.ravel()[k]:.6e}')
    return float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0).max())


def ulps32(got, want):
    """|got - want| in units of the float32 spacing at ``want`` (the spacing at 0 is the smallest denormal)."""
    want = f64(want)
    return np.abs(f64(got) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ sum of squares, clipping

def sumsq(xs):
    """Sum of squares over a list of arrays, correctly rounded (a float32 squared is exact in float64; math.fsum is exact)."""
    return math.fsum(math.fsum((f64(x).ravel() ** 2).tolist()) for x in xs)


def assert_sumsq_close(got, want, n, what='sumsq'):
    """``n * 2**-52`` relative: every partial and the final value are float64 sums of exact squares, a sum of n terms in ANY
    order is within (n - 1) * 2**-53 relative of the exact one (all terms non-negative), and ``want`` is correctly rounded."""
    got, want = float(got), float(want)
    assert math.isfinite(got), f'{what}: {got}'
    return _worst(abs(got - want), n * 2.0 ** -52 * abs(want), what)


def clip_scale(norm, clip):
    """tf.clip_by_global_norm's factor: ``clip / max(norm, clip)``, and NaN for a non-finite norm (TF: "if global_norm ==
    infinity then the entries in t_list are all set to NaN"; a NaN norm propagates the same way)."""
    norm, clip = float(norm), float(clip)
    if not math.isfinite(norm):
        return float('nan')
    return clip / max(norm, clip)


# ------------------------------------------------------------------------------------------------ AdamW

def adamw_steps(var, m, v, grads, lr, beta1, beta2, eps, wd, t0=0, scales=None, lr_t=None):
    """tensorflow-addons 0.11.1 AdamW over Keras Adam of TF 2.3, float64, one dict per step:

        var -= wd * var                                  (decoupled, NOT scaled by the learning rate)
        g = grad * scale                                 (``scales[k]``: the factor of clip_by_global_norm, default 1)
        m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2
        var -= lr_t m / (sqrt(v) + eps),   lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t),  t = t0 + 1, t0 + 2, ...

    ``lr`` is a float or one per step; ``lr_t`` (one per step) replaces the computed value: the kernels receive lr_t as a
    float32.  Each dict has var, m, v after the step and the terms the bound is made of: ``w`` (var before), ``update``,
    ``m_terms`` = |beta1 m| + |(1 - beta1) g|."""
    var, m, v = f64(var).copy(), f64(m).copy(), f64(v).copy()
    out = []
    for k, grad in enumerate(grads):
        t = t0 + k + 1
        step_lr = float(lr[k] if isinstance(lr, (list, tuple)) else lr) if lr is not None else None
        lt = float(lr_t[k]) if lr_t is not None else step_lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        g = f64(grad) * (1.0 if scales is None else scales[k])
        w = var
        m_terms = np.abs(beta1 * m) + np.abs((1.0 - beta1) * g)
        m = beta1 * m + (1.0 - beta1) * g
        v = beta2 * v + (1.0 - beta2) * g * g
        update = lt * m / (np.sqrt(v) + eps)
        var = (w - wd * w) - update
        out.append(dict(var=var, m=m, v=v, w=w, update=update, m_terms=m_terms))
    return out


ADAMW_UNITS = 8.0


def assert_adamw_close(got, want, what='adamw'):
    """``got`` = (var, m, v) of the kernel after one step, ``want`` = that step's dict of ``adamw_steps`` evaluated on the same
    float32 inputs and float32-rounded hyperparameters.  Per element, in units of U = 2**-24:

        var  8 U (|w| + |update|)        m  8 U (|beta1 m| + |(1 - beta1) g|)        v  8 U |v|

    Rounding count of the kernel's statements (each rounding <= 1 U of its result, FMA contraction only removes some):
      g = grad * scale: the norm to float32, the division, the product = 3 (0 without clipping).
      m: g (3) + the product with 1 - beta1 (1) on the g term, the product (1) on the m term, the sum (1): <= 5 of m_terms.
      v: the g^2 term carries 2 * 3 + 2 products, the v term 1, the sum 1.  Where g^2 dominates AND the clip is active that
         is 9 in the worst case; the roundings are independent and each averages a quarter of its bound, the fp32 emulation
         (tests/test_train_kernels.py) stays under 2.2.
      var: w - wd w (2 of |w|), the final difference (1 of |w| + |update|), update = lr_t m / (sqrt(v) + eps): product,
         sqrt, sum, division (4) + half of v's error + m's error.  m's error is relative to m_terms, not to |m|: where the two
         terms of m cancel the update is small and its error is not small against it.  That part is covered by the |w| term
         as long as |w| >> lr, which is why the tests give every weight a magnitude of at least 0.05 (lr <= 1e-3):
         lr_t m_terms / (sqrt(v) + eps) <= ~10 lr there, under 1 U |w|.
    Where the reference is NaN (a non-finite global norm) the kernel's value must be NaN too."""
    worst = 0.0
    for name, g, bound in (('var', got[0], np.abs(want['w']) + np.abs(want['update'])), ('m', got[1], want['m_terms']),
                           ('v', got[2], np.abs(want['v']))):
        ref = want[name]
        g = f64(g)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(g), nan), f'{what} {name}: NaN in {int(np.isnan(g).sum())} places, reference in {int(nan.sum())}'
        ok = ~nan
        worst = max(worst, _worst(np.abs(g - ref)[ok], ADAMW_UNITS * U * np.broadcast_to(bound, ref.shape)[ok], f'{what} {name}'))
    return worst


# ------------------------------------------------------------------------------------------------ normalisation layers

def norm_forward(x, G, P, C, gamma, beta, eps, relu, mean=None, rstd=None):
    """tfa InstanceNormalization (G = B, P = H W) / Keras BatchNormalization on batch statistics (G = 1, P = B H W), x viewed
    as (G, P, C): ``y, mean, rstd, var`` with the BIASED variance and rstd = 1 / sqrt(var + eps).  With ``mean`` / ``rstd``
    given, y is evaluated with those (the apply kernel reads the float32 statistics)."""
    x = f64(x).reshape(G, P, C)
    mu = x.mean(axis=1)
    var = ((x - mu[:, None]) ** 2).mean(axis=1)
    rs = 1.0 / np.sqrt(var + eps)
    mu_y = mu if mean is None else f64(mean).reshape(G, C)
    rs_y = rs if rstd is None else f64(rstd).reshape(G, C)
    y = (x - mu_y[:, None]) * rs_y[:, None] * f64(gamma) + f64(beta)
    if relu:
        y = np.maximum(y, 0.0)
    return y, mu, rs, var


def norm_backward(x, dy, mean, rstd, gamma, G, P, C, terms=False):
    """``dx, dgamma, dbeta`` of y = xhat gamma + beta with xhat = (x - mean) rstd:
    dx = gamma rstd (dy - mean_P(dy) - xhat mean_P(dy xhat)),  dgamma = sum dy xhat,  dbeta = sum dy (over G and P).
    ``terms=True`` appends the magnitudes the bounds are made of."""
    x, dy = f64(x).reshape(G, P, C), f64(dy).reshape(G, P, C)
    mean, rstd, gamma = f64(mean).reshape(G, 1, C), f64(rstd).reshape(G, 1, C), f64(gamma)
    xh = (x - mean) * rstd
    m1 = dy.mean(axis=1, keepdims=True)
    m2 = (dy * xh).mean(axis=1, keepdims=True)
    dx = gamma * rstd * (dy - m1 - xh * m2)
    dgamma, dbeta = (dy * xh).sum(axis=(0, 1)), dy.sum(axis=(0, 1))
    if not terms:
        return dx, dgamma, dbeta
    return dx, dgamma, dbeta, dict(dx=np.abs(gamma * rstd) * (np.abs(dy) + np.abs(m1) + np.abs(xh) * np.abs(m2)),
                                   dgamma=np.abs(dy * xh).sum(axis=(0, 1)), dbeta=np.abs(dy).sum(axis=(0, 1)))


def assert_norm_forward_close(got, x, G, P, C, gamma, beta, relu, eps=F32_EPS_NORM, what='norm forward'):
    """``got`` = (y, mean, rstd, var) of the kernel.
    mean, rstd, var: within 2 float32 spacings of the float64 values (the spacing at 0 is the smallest denormal: a constant
      channel has var = 0 exactly).  The kernel sums x - x0 and its square in float64 with x0 the group's first pixel (error
      ~ P 2**-53 of sums that no longer cancel), forms the three in float64 and rounds each once: half a spacing.  The
      single-pass E[x^2] - mean^2 without the shift misses this bound: 4e-16 instead of 0 on the constant channel, up to 4
      spacings on a channel of mean 100 and spread 0.01.
    y: within 4 U (|xhat gamma| + |beta|) of the float64 value on the kernel's own float32 mean / rstd: x - mean (1),
      times rstd (1), times gamma (1), plus beta (1) = 4 on the first term, 1 on beta.  After a relu the bound is the same
      (max(., 0) is 1-Lipschitz and exact)."""
    y, mean, rstd, var = (f64(t) for t in got)
    _, mu, rs, vr = norm_forward(x, G, P, C, gamma, beta, eps, relu)
    worst = max(_worst(ulps32(mean.reshape(G, C), mu), 2.0, f'{what} mean'), _worst(ulps32(rstd.reshape(G, C), rs), 2.0, f'{what} rstd'),
                _worst(ulps32(var.reshape(G, C), vr), 2.0, f'{what} var'))
    want, _, _, _ = norm_forward(x, G, P, C, gamma, beta, eps, relu, mean=mean, rstd=rstd)
    xg = np.abs((f64(x).reshape(G, P, C) - mean.reshape(G, 1, C)) * rstd.reshape(G, 1, C) * f64(gamma))
    return max(worst, _worst(np.abs(y.reshape(G, P, C) - want), 4.0 * U * (xg + np.abs(f64(beta))), f'{what} y'))


def assert_norm_backward_close(got, x, dy, mean, rstd, gamma, G, P, C, what='norm backward'):
    """``got`` = (dx, dgamma, dbeta) of the kernel, against the float64 formula on the same float32 x, dy, mean, rstd, gamma.
    dx: 8 U |gamma rstd| (|dy| + |mean dy| + |xhat| |mean dy xhat|).  xhat = (x - mean) rstd: 2; each mean to float32: 1;
      xhat * mean: 1; two subtractions: 2; gamma * rstd and the last product: 2.  On the third term 2 + 1 + 1 + 1 + 2 = 7 and
      fewer on the others.  This holds because the means are float64 sums of float64 products: with float32 products
      dy ((x - mean) rstd) every term of a sum that mostly cancels carries 3 roundings, the error of mean(dy xhat) is then
      relative to mean |dy xhat| and not to |mean dy xhat|, and the kernel missed this bound by a factor 2 wherever a relu
      had zeroed dy.
    dgamma: 4 U sum |dy xhat|: float64 sums and products, 1 for the result (3 more per term with float32 products).
    dbeta: 2 U sum |dy|: float64 sums of the float32 inputs, 1 for the result."""
    dx, dgamma, dbeta, t = norm_backward(x, dy, mean, rstd, gamma, G, P, C, terms=True)
    return max(_worst(np.abs(f64(got[0]).reshape(G, P, C) - dx), 8.0 * U * t['dx'], f'{what} dx'),
               _worst(np.abs(f64(got[1]) - dgamma), 4.0 * U * t['dgamma'], f'{what} dgamma'),
               _worst(np.abs(f64(got[2]) - dbeta), 2.0 * U * t['dbeta'], f'{what} dbeta'))


# ------------------------------------------------------------------------------------------------ GRU gates, axpby

def sigmoid(a):
    a = f64(a)
    e = np.exp(-np.abs(a))
    return np.where(a >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def gate_zr(a_zr, h, C):
    """a_zr (M, 2C): z = sigmoid(a[:, :C]), r = sigmoid(a[:, C:]), rh = r h."""
    a = f64(a_zr).reshape(-1, 2 * C)
    z, r = sigmoid(a[:, :C]), sigmoid(a[:, C:])
    return z, r, r * f64(h).reshape(-1, C)


def gate_q(a_q, z, h):
    """q = tanh(a), h' = (1 - z) h + z q."""
    q = np.tanh(f64(a_q))
    return q, (1.0 - f64(z)) * f64(h) + f64(z) * q


def gate_q_backward(d_h_new, z, q, h):
    """dz_pre = dh' (q - h) z (1 - z),  dq_pre = dh' z (1 - q^2),  dh = dh' (1 - z)."""
    g, z, q, h = f64(d_h_new), f64(z), f64(q), f64(h)
    return g * (q - h) * z * (1.0 - z), g * z * (1.0 - q * q), g * (1.0 - z)


def gate_r_backward(d_rh, r, h, dh):
    """dr_pre = d(rh) h r (1 - r),  dh + d(rh) r  (the kernel ACCUMULATES into dh)."""
    g, r = f64(d_rh), f64(r)
    return g * f64(h) * r * (1.0 - r), f64(dh) + g * r


def activation_tolerance(a, name):
    """max(4 x the worst error of torch's float32 sigmoid / tanh against float64 on ``a``, 2**-23): how well a float32
    implementation of the function does on these inputs, not an assumption about ``__expf`` / ``tanhf``."""
    import torch
    t = torch.tensor(np.asarray(a, dtype=np.float32))
    fn = torch.sigmoid if name == 'sigmoid' else torch.tanh
    err = float((fn(t).double() - fn(t.double())).abs().max())
    return max(4.0 * err, 2.0 ** -23)


def assert_gates_forward_close(got, want, tol, what='gates'):
    """Forward gates: every output within ``tol`` (``activation_tolerance``) in absolute terms; |h| <= 1 in the tests, so the
    products r h and (1 - z) h + z q carry the activations' errors at most once each plus float32 roundings of values <= 1."""
    worst = 0.0
    for k, (g, w) in enumerate(zip(got, want)):
        g = f64(g).reshape(np.shape(w))
        assert np.isfinite(g).all(), f'{what} output {k}: not finite'
        worst = max(worst, _worst(np.abs(g - w), tol, f'{what} output {k}'))
    return worst


def assert_gates_backward_close(got, want, what='gates backward'):
    """The two backward kernels are products of their inputs: 6 U |value| per output against float64 on the same z, r, q.
    Longest chain dz_pre = g (q - h) z (1 - z): q - h (1), 1 - z (1), three products (3) = 5.  1 - q^2 and dh += g r are one
    fused multiply-add each in the kernel (one rounding of the RESULT, -ffp-contract=on)."""
    worst = 0.0
    for k, (g, w) in enumerate(zip(got, want)):
        worst = max(worst, _worst(np.abs(f64(g).reshape(np.shape(w)) - w), 6.0 * U * np.abs(w), f'{what} output {k}'))
    return worst


def axpby(alpha, a, beta, b=None, relu=False):
    """alpha a + beta b (b = None: alpha a), optionally through max(., 0)."""
    out = float(alpha) * f64(a) + (float(beta) * f64(b) if b is not None else 0.0)
    return np.maximum(out, 0.0) if relu else out


def axpby_relu(alpha, a, beta, b=None):
    return axpby(alpha, a, beta, b, relu=True)


def assert_axpby_close(got, want, what='axpby'):
    """Within 1 float32 spacing of the float64 result rounded to float32.  The tests use factors whose products are exact
    (powers of two) or a single product (b = NULL), so the kernel rounds once (half a spacing) with or without contraction."""
    w32 = f64(want).astype(np.float32)
    return _worst(ulps32(got, w32), 1.0, what)

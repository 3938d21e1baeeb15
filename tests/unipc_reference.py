"""A float64 restatement of UniPC (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion
Models"), data prediction, multistep, "bh1" / "bh2" (plain helper, no test in it).

Written from the formulas, as predictor and corrector with explicit differences D_k and numpy.linalg.solve; it never sees the library's
collapsed tables.  Notation for a level with cumulative alpha a: alpha = sqrt(a), sigma = sqrt(1 - a), lambda = ln(alpha / sigma).  A
step goes from the newest evaluated level s to the target t: h = lambda_t - lambda_s, hh = -h, phi1 = expm1(hh), B = hh ("bh1") or
expm1(hh) ("bh2"); m[0] is the x0 estimate at s, m[k] that at the earlier level earlier[k-1], r_k = (lambda_{earlier[k-1]} - lambda_s) / h,
D_k = (m[k] - m[0]) / r_k; g_1 = phi1/hh - 1, g_{i+1} = g_i/hh - 1/(i+1)!, b_i = g_i i! / B; R has rows i = 1..p equal to
(r_1^(i-1), ..., r_{p-1}^(i-1), 1).

``kernel`` restates one launch of dm3d_unipc_update (include/dm3d.h), order="f64" through predictor() / corrector(), order="f32" as the
individually rounded float32 operations the header documents, on coefficients this file collapses itself, by linearity: the
coefficient of an input is the restatement's answer to that input set to 1 and the others to 0.
"""
import math

import numpy as np

F = np.float32


def _lam(ab, i):
    a = float(ab[i])
    return math.log(math.sqrt(a) / math.sqrt(1.0 - a))


def _system(ab, s, t, earlier, variant):
    h = _lam(ab, t) - _lam(ab, s)
    hh = -h
    phi1 = math.expm1(hh)
    B = {"bh1": hh, "bh2": math.expm1(hh)}[variant]
    r = [(_lam(ab, e) - _lam(ab, s)) / h for e in earlier]
    p = len(earlier) + 1
    R = np.array([[rk ** (i - 1) for rk in r] + [1.0] for i in range(1, p + 1)])
    g, b = phi1 / hh - 1.0, []
    for i in range(1, p + 1):
        b.append(g * math.factorial(i) / B)
        g = g / hh - 1.0 / math.factorial(i + 1)
    sig = lambda i: math.sqrt(1.0 - float(ab[i]))
    return sig(t) / sig(s), math.sqrt(float(ab[t])), phi1, B, r, R, np.array(b)


def predictor(ab, s, t, x_s, m, earlier=(), variant="bh2"):
    """x_t^p of order p = 1 + len(earlier) (t < 0, clean: the x0 estimate m[0])."""
    if t < 0:
        return m[0] + 0.0 * x_s
    ratio, a_t, phi1, B, r, R, b = _system(ab, s, t, earlier, variant)
    p = len(earlier) + 1
    rho = [] if p == 1 else [0.5] if p == 2 else list(np.linalg.solve(R[:2, :2], b[:2]))
    out = ratio * x_s - a_t * phi1 * m[0]
    for k in range(1, p):
        out = out - a_t * B * rho[k - 1] * (m[k] - m[0]) / r[k - 1]
    return out


def corrector(ab, s, t, x_s, m, m_t, earlier=(), variant="bh2"):
    """x_t^c of order p = 1 + len(earlier): x_s the corrected state at s, m_t the x0 estimate the network gave on the predicted state at t."""
    ratio, a_t, phi1, B, r, R, b = _system(ab, s, t, earlier, variant)
    p = len(earlier) + 1
    rho = [0.5] if p == 1 else list(np.linalg.solve(R, b))
    acc = rho[p - 1] * (m_t - m[0])
    for k in range(1, p):
        acc = acc + rho[k - 1] * (m[k] - m[0]) / r[k - 1]
    return ratio * x_s - a_t * phi1 * m[0] - a_t * B * acc


def orders(n, order=2, lower_order_final=True):
    """Order of row r of an n-row chain (row n-1 runs first, row 0 steps to clean): step j = n-1-r has min(order, j+1), and with
    lower_order_final at most the steps between levels that are left, itself included (r; the step to clean is the x0 estimate)."""
    return [min(order, n - r, max(r, 1)) if lower_order_final else min(order, n - r) for r in range(n)]


def estimate(x, eps, a, clip=True, bound=None):
    """The x0 estimate of a level with cumulative alpha ``a``: clamp(x0, -1, 1), or clamp(x0, -s, s) / s under a dynamic bound s."""
    x0 = (x - math.sqrt(1.0 - a) * eps) / math.sqrt(a)
    if not clip:
        return x0
    return np.clip(x0, -1.0, 1.0) if bound is None else np.clip(x0, -bound, bound) / bound


def dynamic_bound(x0, ratio, cap=None):
    """Imagen's s of one volume: the ratio-quantile of |x0| (numpy's linear interpolation), raised to 1, capped."""
    s = max(float(np.quantile(np.abs(x0).reshape(-1), ratio)), 1.0)
    return s if cap is None else min(s, cap)


def chain(eps_fn, ab, taus, x_T, order=2, lower_order_final=True, variant="bh2", clip=True, threshold=None):
    """The whole chain in float64 over taus = tau_0 < ... < tau_{n-1}: eps_fn(x, t) is the model; returns the x0 estimate at tau_0.
    ``threshold`` = (ratio, cap): each volume's estimate is thresholded dynamically."""
    taus = [int(v) for v in taus]
    n = len(taus)
    p = orders(n, order, lower_order_final)
    x = np.asarray(x_T, dtype=np.float64)
    xc, m = None, []                                                    # corrected state of the level before; estimates, newest first
    for r in range(n - 1, -1, -1):
        s = taus[r]
        eps = np.asarray(eps_fn(x, s), dtype=np.float64)
        if threshold is None:
            m_s = estimate(x, eps, float(ab[s]), clip)
        else:
            raw = estimate(x, eps, float(ab[s]), False)
            m_s = np.stack([estimate(x[b], eps[b], float(ab[s]), True, dynamic_bound(raw[b], *threshold)) for b in range(len(x))])
        if r == 0:
            return m_s
        if r < n - 1:                                                   # the corrector at s, of the order of the step that produced s
            q = p[r + 1]
            xc = corrector(ab, taus[r + 1], s, xc, m, m_s, taus[r + 2:r + 1 + q], variant)
        else:
            xc = x
        m = [m_s] + m
        x = predictor(ab, s, taus[r - 1], xc, m, taus[r + 1:r + p[r]], variant)


def rows(ab, taus, order=2, lower_order_final=True, variant="bh2"):
    """[n, 10] float64 (p_x, p_0, p_1, p_2, k_x, k_0, k_1, k_2, k_t, rot) of every row of a chain, by linearity from predictor() and
    corrector(): rows n-1 and 0 have no corrector."""
    taus = [int(v) for v in taus]
    n = len(taus)
    p = orders(n, order, lower_order_final)
    out = np.zeros((n, 10))
    for r in range(n):
        out[r, :4] = predictor_row(ab, taus[r], taus[r - 1] if r > 0 else -1, taus[r + 1:r + p[r]], variant)
        if 0 < r < n - 1:
            out[r, 4:9] = corrector_row(ab, taus[r + 1], taus[r], taus[r + 2:r + 1 + p[r + 1]], variant)
        out[r, 9] = (n - 1 - r) % 3
    return out


def predictor_row(ab, s, t, earlier=(), variant="bh2"):
    unit = np.eye(4)
    return np.array([predictor(ab, s, t, unit[i, 0], list(unit[i, 1:2 + len(earlier)]), earlier, variant) for i in range(4)])


def corrector_row(ab, s, t, earlier=(), variant="bh2"):
    unit = np.eye(5)
    return np.array([corrector(ab, s, t, unit[i, 0], list(unit[i, 1:2 + len(earlier)]), unit[i, 4], earlier, variant) for i in range(5)])


def kernel(ab, x, eps, xc, hist, t, t_prev, t_hist, order, corrector_order, variant="bh2", clip=True, bound=None, float_order="f64"):
    """One launch on one sample: x the predicted state at level t, eps the model's noise there, xc the corrected state at t_hist[0],
    hist the x0 estimates at t_hist (newest first).  Returns (x_next, x_corr, x0).  float_order="f32": float32 inputs, the header's
    operations, each rounded."""
    a = float(ab[t])
    if float_order == "f64":
        x, eps = np.asarray(x, np.float64), np.asarray(eps, np.float64)
        hist = [np.asarray(h, np.float64) for h in hist]
        m = estimate(x, eps, a, clip, bound)
        c = x
        if corrector_order:
            c = corrector(ab, t_hist[0], t, np.asarray(xc, np.float64), hist, m, list(t_hist[1:corrector_order]), variant)
        return predictor(ab, t, t_prev, c, [m] + hist, list(t_hist[:order - 1]), variant), c, m
    p = predictor_row(ab, t, t_prev, list(t_hist[:order - 1]), variant).astype(F)
    k = corrector_row(ab, t_hist[0], t, list(t_hist[1:corrector_order]), variant).astype(F) if corrector_order else np.zeros(5, F)
    x, eps = np.asarray(x, F), np.asarray(eps, F)
    m = (x - F(math.sqrt(1.0 - a)) * eps) / F(math.sqrt(a))              # mul, sub, div, each rounded (numpy float32 arithmetic)
    if clip:
        keep = np.isnan(m)
        s = F(1.0) if bound is None else F(bound)
        b = np.clip(m, -s, s)
        b = b if bound is None else b / s
        m = np.where(keep, m, b).astype(F)
    c = x
    if corrector_order:
        c = None
        for coef, v in zip(k[:4], [xc] + list(hist[:3])):
            if coef != 0:
                term = coef * np.asarray(v, F)
                c = term if c is None else c + term
        c = k[4] * m if c is None else c + k[4] * m
    out = p[0] * c + p[1] * m
    for coef, v in zip(p[2:], hist[:2]):
        if coef != 0:
            out = out + coef * np.asarray(v, F)
    assert out.dtype == F and c.dtype == F and m.dtype == F
    return out, c, m

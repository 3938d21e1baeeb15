"""The host arithmetic of the samplers and of training: schedules, coefficient rows, threshold and guidance tables, the prediction
and objective tables (eps, v, x0; min-SNR), mask pooling and context dropout.  Pure functions of numbers and arrays: none needs the model, the library or a device.  ``diffusion`` re-exports every
public name."""
from __future__ import annotations

import math

import numpy as np
import torch


def _host(v):
    """``v`` as the host sees it: a tensor detached and on the CPU, anything else as it is."""
    return v.detach().cpu() if torch.is_tensor(v) else v


def _per_volume(name: str, v, B: int) -> np.ndarray:
    """One value or one per volume, finite, as float64 [B] (a broadcast view)."""
    a = np.asarray(_host(v), dtype=np.float64).reshape(-1)
    if a.size not in (1, B):
        raise ValueError(f"{name} must hold one value or one per volume ({B}), got {a.size}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be finite")
    return np.broadcast_to(a, (B,))


def ddim_timesteps(T: int, num_steps=None, timesteps=None) -> np.ndarray:
    """The DDIM schedule tau_0 < ... < tau_{S-1} in [0, T): ``timesteps`` as given (strictly increasing), or for ``num_steps`` = S
    tau_i = round(i (T-1) / (S-1)) (halves rounded up, in integers) for i = 0..S-1, and [T-1] for S = 1: always holds 0 and T-1.
    Neither given: every timestep (S = T)."""
    T = int(T)
    if num_steps is not None and timesteps is not None:
        raise ValueError("give num_steps or timesteps, not both")
    if timesteps is not None:
        ts = np.asarray(timesteps).reshape(-1)
        if ts.size == 0 or not np.all(ts == np.round(ts)) or ts.min() < 0 or ts.max() >= T or np.any(np.diff(ts) <= 0):
            raise ValueError(f"timesteps must be strictly increasing integers in [0, {T})")
        return ts.astype(np.int64)
    S = T if num_steps is None else int(num_steps)
    if not 1 <= S <= T:
        raise ValueError(f"num_steps must lie in [1, {T}], got {num_steps}")
    if S == 1:
        return np.array([T - 1], dtype=np.int64)
    i = np.arange(S, dtype=np.int64)
    return (2 * i * (T - 1) + (S - 1)) // (2 * (S - 1))


def ddim_coefficients(alpha_bar, src, dst, eta=0.0) -> np.ndarray:
    """float64 [n, 5] rows (sqrt(a), sqrt(1-a), a_x0, a_eps, sigma) of the DDIM steps src[r] -> dst[r] (include/dm3d.h,
    dm3d_ddim_desc): a = alpha_bar[src], a' = alpha_bar[dst] (1 where dst < 0), sigma = eta sqrt((1-a')/(1-a)) sqrt(1 - a/a'),
    a_x0 = sqrt(a'), a_eps = sqrt(max(1 - a' - sigma^2, 0)).  eta = 0 gives sigma = 0 for either direction (inversion: a' < a)."""
    ab = np.asarray(alpha_bar, dtype=np.float64)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    a = ab[src]
    ap = np.where(dst < 0, 1.0, ab[np.maximum(dst, 0)])
    sigma = np.zeros_like(a)
    if eta != 0:
        sigma = float(eta) * np.sqrt((1 - ap) / (1 - a)) * np.sqrt(1 - a / ap)
    a_eps = np.sqrt(np.maximum(1 - ap - sigma ** 2, 0.0))
    return np.stack([np.sqrt(a), np.sqrt(1 - a), np.sqrt(ap), a_eps, sigma], axis=1)


def dpm_coefficients(alpha_bar, src, dst, prev, order=2) -> np.ndarray:
    """float64 [n, 3] rows (c_x, c_0, c_1) of the DPM-Solver++(2M) steps src[r] -> dst[r] (include/dm3d.h, dm3d_dpm_desc):
    x' = c_x x + c_0 x0 + c_1 x0_prev.  With alpha = sqrt(a), sigma = sqrt(1-a), lambda = log(alpha/sigma) and h = lambda_dst -
    lambda_src: c_x = sigma_dst / sigma_src and A = alpha_dst (1 - e^-h); a first-order row is (c_x, A, 0), a second-order row with
    r = (lambda_src - lambda_prev) / h is (c_x, A (1 + 1/(2r)), -A / (2r)), ``prev[r]`` being the level the step before started from.
    ``prev[r] < 0`` or ``order`` = 1 makes row r first order; ``dst[r] < 0`` (clean, a' = 1) is (0, 1, 0) exactly.
    A level with a = 0 (the zero-terminal-SNR schedule's last) has lambda = -inf: a row from it has h = +inf and is
    (sigma_dst, alpha_dst, 0), first order whatever ``prev`` says; the row after it has r = inf, 1/(2r) = 0 and c_1 = 0, so the
    history is not read.  No row holds a NaN."""
    if order not in (1, 2):
        raise ValueError(f"solver_order must be 1 or 2, got {order!r}")
    ab = np.asarray(alpha_bar, dtype=np.float64)
    src, dst, prev = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (src, dst, prev))
    lam = lambda a: 0.5 * (np.log(a) - np.log1p(-a))            # log(sqrt(a) / sqrt(1-a)); -inf at a = 0
    a_s, a_t, a_p = ab[src], ab[np.maximum(dst, 0)], ab[np.maximum(prev, 0)]
    with np.errstate(divide="ignore", invalid="ignore"):
        h = lam(a_t) - lam(a_s)                                 # +inf from a level with a = 0: expm1(-h) = -1, A = alpha_dst
        c_x = np.sqrt((1 - a_t) / (1 - a_s))
        A = -np.sqrt(a_t) * np.expm1(-h)
        second = (prev >= 0) & (dst >= 0) & (order == 2) & (a_s > 0)
        g = np.where(second, h / (2 * (lam(a_s) - lam(a_p))), 0.0)          # 1 / (2r); 0 where lambda_prev = -inf
    out = np.stack([c_x, A * (1 + g), -A * g], axis=1)
    out[dst < 0] = (0.0, 1.0, 0.0)
    return out


def dpm_sde_coefficients(alpha_bar, src, dst, prev, order=2, eta=1.0) -> np.ndarray:
    """float64 [n, 4] rows (c_x, c_0, c_1, c_z) of the stochastic DPM-Solver++(2M) steps src[r] -> dst[r] (include/dm3d.h,
    dm3d_dpm_sde_desc): x' = c_x x + c_0 x0 + c_1 x0_prev + c_z z.  With alpha, sigma, lambda and h as dpm_coefficients and
    ``eta`` >= 0 (1: the solver of Lu et al. 2022, 0: the ODE solver): c_x = (sigma_dst / sigma_src) e^(-eta h),
    A = alpha_dst (1 - e^(-(1 + eta) h)) and c_z = sigma_dst sqrt(1 - e^(-2 eta h)); a first-order row is (c_x, A, 0, c_z), a
    second-order row (c_x, A (1 + g), -A g, c_z) with dpm_coefficients' g = 1 / (2r) (the midpoint form).  ``prev``, ``order`` and the row
    to clean, (0, 1, 0, 0) exactly, follow dpm_coefficients.  A row from a level with a = 0 (h = +inf) is written out, never through
    0 * inf: (sigma_dst, alpha_dst, 0, 0) at eta = 0 and (0, alpha_dst, 0, sigma_dst) at eta > 0; the row after it has g = 0.  At
    eta = 0 columns 0-2 are dpm_coefficients' own (that function is called) and column 3 is 0.  No row holds a NaN."""
    eta = float(eta)
    if not (eta >= 0 and math.isfinite(eta)):                   # (a NaN fails the comparison too)
        raise ValueError(f"sde_eta must be finite and >= 0, got {eta}")
    ode = dpm_coefficients(alpha_bar, src, dst, prev, order)
    out = np.zeros((len(ode), 4), dtype=np.float64)
    out[:, :3] = ode
    if eta == 0:
        return out
    ab = np.asarray(alpha_bar, dtype=np.float64)
    src, dst, prev = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (src, dst, prev))
    lam = lambda a: 0.5 * (np.log(a) - np.log1p(-a))            # dpm_coefficients' expressions
    a_s, a_t, a_p = ab[src], ab[np.maximum(dst, 0)], ab[np.maximum(prev, 0)]
    blind = a_s == 0                                            # lambda_src = -inf: nothing of x survives, all of z enters
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.where(blind, 0.0, lam(a_t) - lam(a_s))           # (a finite stand-in: the blind rows are written out below)
        c_x = np.sqrt((1 - a_t) / (1 - a_s)) * np.exp(-eta * h)
        A = -np.sqrt(a_t) * np.expm1(-(1 + eta) * h)
        c_z = np.sqrt(1 - a_t) * np.sqrt(-np.expm1(-2 * eta * h))
        second = (prev >= 0) & (dst >= 0) & (order == 2) & ~blind
        g = np.where(second, h / (2 * (lam(a_s) - lam(a_p))), 0.0)          # 1 / (2r); 0 where lambda_prev = -inf
    out = np.stack([c_x, A * (1 + g), -A * g, c_z], axis=1)
    zero = np.zeros_like(a_t)
    out[blind] = np.stack([zero, np.sqrt(a_t), zero, np.sqrt(1 - a_t)], axis=1)[blind]
    out[dst < 0] = (0.0, 1.0, 0.0, 0.0)
    return out


UNIPC_VARIANTS = ("bh1", "bh2")


def _check_unipc(order, variant):
    if order not in (1, 2, 3):
        raise ValueError(f"solver_order must be 1, 2 or 3 for sampler='unipc', got {order!r}")
    if variant not in UNIPC_VARIANTS:
        raise ValueError(f"unipc_variant must be 'bh1' or 'bh2', got {variant!r}")


def unipc_orders(n: int, order=2, lower_order_final=True) -> np.ndarray:
    """The order of every row of an n-row UniPC chain (row n-1 runs first, row 0 is the step to clean): step j = n-1-r, counted from
    the start, has order min(``order``, j+1), and with ``lower_order_final`` at most the number of steps left, itself included.  The
    steps counted are those between levels, r of them at row r: the step to clean returns the x0 estimate and has no order to lower.
    So the step into the schedule's lowest level (row 1) is first order, as in the DPM-Solver++ chain and for its reason: that step
    crosses a log-SNR gap several times the one before it."""
    r = np.arange(int(n), dtype=np.int64)
    p = np.minimum(int(order), n - r)
    return np.minimum(p, np.maximum(r, 1)) if lower_order_final else p


def unipc_system(alpha_bar, s, t, earlier, variant="bh2"):
    """What the predictor and the corrector of one UniPC step from level ``s`` to level ``t`` share (Zhao et al. 2023; the
    data-prediction form), in float64: (sigma_t/sigma_s, alpha_t, phi1, B, r, R, b) with h = lambda_t - lambda_s, hh = -h,
    phi1 = expm1(hh), B = hh ("bh1") or expm1(hh) ("bh2"), r_k = (lambda_{earlier[k-1]} - lambda_s) / h for the p-1 ``earlier`` levels,
    R the p x p matrix with rows (r_1^(i-1), ..., r_{p-1}^(i-1), 1) and b_i = g_i i! / B, g_1 = phi1/hh - 1, g_{i+1} = g_i/hh - 1/(i+1)!."""
    ab = np.asarray(alpha_bar, dtype=np.float64)
    lam = lambda i: 0.5 * (math.log(ab[i]) - math.log1p(-ab[i]))
    h = lam(t) - lam(s)
    hh = -h
    phi1 = math.expm1(hh)
    B = hh if variant == "bh1" else phi1
    r = np.array([(lam(e) - lam(s)) / h for e in earlier] + [1.0])
    p = len(r)
    R = np.stack([r ** i for i in range(p)])
    g, fact, b = phi1 / hh - 1.0, 1.0, []
    for i in range(1, p + 1):
        b.append(g * fact / B)
        fact *= i + 1
        g = g / hh - 1.0 / fact
    return math.sqrt((1 - ab[t]) / (1 - ab[s])), math.sqrt(ab[t]), phi1, B, r, R, np.array(b)


def unipc_predictor(alpha_bar, s, t, earlier=(), variant="bh2") -> np.ndarray:
    """float64 (p_x, p_0, p_1, p_2) of the UniPC predictor of order p = 1 + len(``earlier``) from level ``s`` to level ``t`` (t < 0:
    clean, (0, 1, 0, 0) exactly): x_t = p_x x_s + p_0 m_0 + p_1 m_1 + p_2 m_2, m_0 the x0 estimate at s and m_k that at earlier[k-1].
    It is x_t = (sigma_t/sigma_s) x_s - alpha_t phi1 m_0 - alpha_t B sum_k rho_k (m_k - m_0) / r_k collapsed, with rho = (1/2) at
    p = 2 and the solution of the leading 2 x 2 system of unipc_system's (R, b) at p = 3; p = 1 is the DDIM eta = 0 step."""
    out = np.zeros(4)
    if t < 0:
        out[1] = 1.0
        return out
    if len(earlier) > 2:
        raise ValueError("the predictor's order is at most 3")
    c_x, a_t, phi1, B, r, R, b = unipc_system(alpha_bar, s, t, earlier, variant)
    rho = np.zeros(0) if len(earlier) == 0 else np.array([0.5]) if len(earlier) == 1 else np.linalg.solve(R[:2, :2], b[:2])
    w = a_t * B * rho / r[:-1]
    out[0], out[1] = c_x, -a_t * phi1 + w.sum()
    out[2:2 + len(w)] = -w
    return out


def unipc_corrector(alpha_bar, s, t, earlier=(), variant="bh2") -> np.ndarray:
    """float64 (k_x, k_0, k_1, k_2, k_t) of the UniPC corrector of order p = 1 + len(``earlier``) at level ``t``, reached from level
    ``s``: x_t^c = k_x x_s + k_0 m_0 + k_1 m_1 + k_2 m_2 + k_t m_t, x_s the corrected state at s, m_t the x0 estimate the network
    gave on the predicted state at t.  It is x_t^c = (sigma_t/sigma_s) x_s - alpha_t phi1 m_0 - alpha_t B (sum_k rho_k (m_k - m_0) / r_k
    + rho_p (m_t - m_0)) collapsed, with rho = (1/2) at p = 1 and else the solution of unipc_system's R rho = b."""
    if len(earlier) > 2:
        raise ValueError("the corrector's order is at most 3")
    c_x, a_t, phi1, B, r, R, b = unipc_system(alpha_bar, s, t, earlier, variant)
    rho = np.array([0.5]) if len(earlier) == 0 else np.linalg.solve(R, b)
    w = a_t * B * rho / r                                        # (r_p = 1: the last entry is alpha_t B rho_p)
    out = np.zeros(5)
    out[0], out[1] = c_x, -a_t * phi1 + w.sum()
    out[2:2 + len(w) - 1] = -w[:-1]
    out[4] = -w[-1]
    return out


def unipc_coefficients(alpha_bar, taus, order=2, lower_order_final=True, variant="bh2") -> np.ndarray:
    """float64 [n, 10] rows (p_x, p_0, p_1, p_2, k_x, k_0, k_1, k_2, k_t, rot) of a UniPC chain over the schedule ``taus`` = tau_0 <
    ... < tau_{n-1} (include/dm3d.h, dm3d_unipc_desc): row r belongs to the launch after the U-Net pass at tau_r (row n-1 runs
    first).  Columns 0-3 are unipc_predictor's for the step tau_r -> tau_{r-1} (row 0: to clean) at the order unipc_orders gives the
    row; columns 4-8 unipc_corrector's at tau_r, reached from tau_{r+1}, at the order of the predictor that produced tau_r (row r+1's),
    all zero (no corrector) in row n-1, which nothing precedes, and in row 0, whose result is the x0 estimate alone.  rot = (n-1-r) % 3 is
    the history slot the row's estimate goes to.  A level with alpha_bar = 0 has no finite lambda and is an error."""
    _check_unipc(order, variant)
    ab = np.asarray(alpha_bar, dtype=np.float64)
    taus = np.asarray(taus, dtype=np.int64).reshape(-1)
    if np.any(ab[taus] <= 0):
        raise ValueError("sampler='unipc' needs alpha_bar > 0 at every level of the schedule (lambda = -inf breaks the corrector's h)")
    n = len(taus)
    orders = unipc_orders(n, order, lower_order_final)
    out = np.zeros((n, 10), dtype=np.float64)
    for r in range(n):
        out[r, :4] = unipc_predictor(ab, taus[r], taus[r - 1] if r > 0 else -1, taus[r + 1:r + orders[r]], variant)
        if 0 < r < n - 1:
            out[r, 4:9] = unipc_corrector(ab, taus[r + 1], taus[r], taus[r + 2:r + 1 + orders[r + 1]], variant)
        out[r, 9] = (n - 1 - r) % 3
    return out


def threshold_rank(per_sample: int, ratio) -> tuple:
    """(i, f) of the dynamic threshold's quantile (include/dm3d.h, dm3d_thresh_desc): q = ratio (N-1) in float64, i = floor(q) and
    f = float32(q - i), the weight of v_{i+1} in the interpolation between the order statistics v_i and v_{i+1} of N = per_sample
    magnitudes (numpy's "linear" quantile).  ratio = 1 gives (N-1, 0): the maximum."""
    q = float(ratio) * (int(per_sample) - 1)
    i = min(int(math.floor(q)), int(per_sample) - 1)
    return i, np.float32(q - i)


FLOAT32_MAX = float(np.finfo(np.float32).max)


def threshold_tables(B: int, per_sample: int, dynamic_threshold, threshold_max=None):
    """(rank int32 [B], frac float32 [B], smax float32 [B]) host tables of dm3d_thresh_desc, one ratio / cap broadcast or one per
    volume, validated: 0 < ratio <= 1, cap >= 1 (None: the largest finite float32), all finite."""
    p = _per_volume("dynamic_threshold", dynamic_threshold, B)
    cap = _per_volume("threshold_max", FLOAT32_MAX if threshold_max is None else threshold_max, B)
    if p.min() <= 0 or p.max() > 1:
        raise ValueError("dynamic_threshold must lie in (0, 1]")
    if cap.min() < 1 or cap.max() > FLOAT32_MAX:
        raise ValueError("threshold_max must be >= 1 (and a finite float32)")
    ranks = [threshold_rank(per_sample, v) for v in p]
    return (np.array([r[0] for r in ranks], dtype=np.int32), np.array([r[1] for r in ranks], dtype=np.float32),
            np.ascontiguousarray(cap.astype(np.float32)))


def guide_tables(B: int, guidance_scale, guidance_rescale):
    """(w, phi): float32 [B] host arrays of the guidance scale and rescale, one value broadcast or one per volume, validated."""
    w, phi = (np.ascontiguousarray(_per_volume(name, v, B).astype(np.float32))
              for name, v in (("guidance_scale", guidance_scale), ("guidance_rescale", guidance_rescale)))
    if phi.min() < 0 or phi.max() > 1:
        raise ValueError("guidance_rescale must lie in [0, 1]")
    return w, phi


PREDICTIONS = ("eps", "v", "x0")          # what the network's output is read as (DiffusionModel(prediction=))
LOSS_WEIGHTINGS = (None, "min_snr")       # compile(loss_weighting=)


def _check_prediction(prediction) -> str:
    if prediction not in PREDICTIONS:
        raise ValueError(f"prediction must be 'eps', 'v' or 'x0', got {prediction!r}")
    return prediction


def prediction_table(alpha_bar, prediction) -> np.ndarray:
    """float32 [T, 2] rows (c_p, c_x) of dm3d_pred_desc (include/dm3d.h): eps = c_p pred + c_x x_t at every timestep, in float64 from
    the float32 alpha_bar table the kernels use, rounded once.  With a = sqrt(alpha_bar) and s = sqrt(1 - alpha_bar): "v" (Salimans &
    Ho 2022, v = a z - s x0) gives (a, s), "x0" gives (-a/s, 1/s) and "eps" (1, 0)."""
    _check_prediction(prediction)
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    a, s = np.sqrt(ab), np.sqrt(1 - ab)
    if prediction == "v":
        rows = (a, s)
    elif prediction == "x0":
        rows = (-a / s, 1 / s)
    else:
        rows = (np.ones_like(a), np.zeros_like(a))
    return np.stack(rows, axis=1).astype(np.float32)


def frame_table(alpha_bar, prediction) -> np.ndarray:
    """float32 [T, 4] rows (k0x, k0p, kex, kep) of the update descriptors' ``frame`` (include/dm3d.h, dm3d_ddim_desc): at every
    timestep x0 = k0x x_t + k0p pred and eps = kex x_t + kep pred, in float64 from the float32 alpha_bar table the kernels use, rounded
    once.  With a = sqrt(alpha_bar) and s = sqrt(1 - alpha_bar): "v" gives (a, -s, s, a), no division anywhere; "x0" gives
    (0, 1, 1/s, -a/s), s > 0 at every timestep; "eps" gives (1/a, -s/a, 0, 1) and is an error where any alpha_bar is 0 (the
    zero-terminal-SNR schedule: eps carries no information about x0 there)."""
    _check_prediction(prediction)
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    a, s = np.sqrt(ab), np.sqrt(1 - ab)
    zero, one = np.zeros_like(a), np.ones_like(a)
    if prediction == "v":
        rows = (a, -s, s, a)
    elif prediction == "x0":
        rows = (zero, one, 1 / s, -a / s)
    else:
        if np.any(ab == 0):
            raise ValueError("the eps frame divides by sqrt(alpha_bar), which is 0 in this schedule: use prediction='v' or 'x0'")
        rows = (1 / a, -s / a, zero, one)
    return np.stack(rows, axis=1).astype(np.float32)


def objective_rows(alpha_bar, t, prediction, loss_weighting=None, snr_gamma=5.0) -> np.ndarray:
    """float32 [B, 4] rows (a_z, a_0, w, 0) of dm3d_loss_desc (include/dm3d.h) for the timesteps ``t``: the training target is
    a_z noise + a_0 x0 and w the sample's loss weight, in float64 from the float32 alpha_bar table, rounded once.  Targets, with
    a = sqrt(alpha_bar[t]) and s = sqrt(1 - alpha_bar[t]): "eps" (1, 0), "v" (a, -s), "x0" (0, 1).  w = 1 without ``loss_weighting``;
    "min_snr" (Hang et al. 2023) with SNR = alpha_bar / (1 - alpha_bar) and gamma = ``snr_gamma``: min(SNR, gamma) / SNR for eps,
    min(SNR, gamma) / (SNR + 1) for v and min(SNR, gamma) for x0 (one weight on the x0 error, written in each target's own units).
    At alpha_bar = 0 (the zero-terminal-SNR schedule's last timestep) the v and x0 rows are finite and SNR = 0: "min_snr" weighs that
    timestep 0 for both (x_t holds nothing of x0 there), no weighting weighs it 1."""
    _check_prediction(prediction)
    if loss_weighting not in LOSS_WEIGHTINGS:
        raise ValueError(f"loss_weighting must be None or 'min_snr', got {loss_weighting!r}")
    gamma = float(snr_gamma)
    if not gamma > 0:                                     # a NaN fails the comparison too
        raise ValueError(f"snr_gamma must be > 0, got {snr_gamma}")
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)[np.asarray(_host(t), dtype=np.int64).reshape(-1)]
    a, s = np.sqrt(ab), np.sqrt(1 - ab)
    rows = np.zeros((ab.size, 4), dtype=np.float64)
    if prediction == "v":
        rows[:, 0], rows[:, 1] = a, -s
    elif prediction == "x0":
        rows[:, 1] = 1.0
    else:
        rows[:, 0] = 1.0
    rows[:, 2] = 1.0
    if loss_weighting == "min_snr":
        snr = ab / (1 - ab)
        clipped = np.minimum(snr, gamma)
        rows[:, 2] = clipped / snr if prediction == "eps" else clipped / (snr + 1) if prediction == "v" else clipped
    return rows.astype(np.float32)


def edit_steps(strength, n: int) -> int:
    """The steps an edit keeps of an n-step schedule: floor(strength n + 1/2) for strength in (0, 1]; 0 steps is an error."""
    s = float(strength)
    if not 0 < s <= 1:                                    # a NaN fails the comparison too
        raise ValueError(f"strength must lie in (0, 1], got {strength}")
    k = int(math.floor(s * int(n) + 0.5))
    if k == 0:
        raise ValueError(f"strength {strength} keeps no step of a {n}-step schedule")
    return k


def edit_levels(alpha_bar, levels) -> np.ndarray:
    """float64 [n, 2] rows (sqrt(a'), sqrt(1-a')) of the known-latent levels (include/dm3d.h, dm3d_edit_desc): a' = alpha_bar[level],
    1 where level < 0 (clean)."""
    ab = np.asarray(alpha_bar, dtype=np.float64)
    lv = np.asarray(levels, dtype=np.int64)
    ap = np.where(lv < 0, 1.0, ab[np.maximum(lv, 0)])
    return np.stack([np.sqrt(ap), np.sqrt(1 - ap)], axis=1)


def latent_mask(mask, latent_shape) -> torch.Tensor:
    """An edit mask (1 = regenerate, 0 = keep, values in [0, 1]) at latent resolution: ``mask`` is [B|1, D', H', W'] or
    [B|1, D', H', W', 1] with (D', H', W') = k (D, H, W) for an integer k >= 1 (k = 4: a 128^3 image mask over a 32^3 latent),
    ``latent_shape`` = (B, D, H, W, C).  Each k^3 block is pooled by its max (a voxel any part of which is regenerated is
    regenerated) and a batch of one is broadcast: float32 [B, D, H, W] on the mask's device."""
    B, D, H, W = (int(v) for v in latent_shape[:4])
    m = (mask if torch.is_tensor(mask) else torch.as_tensor(np.asarray(mask))).to(torch.float32)
    if m.dim() == 5:
        if m.shape[-1] != 1:
            raise ValueError(f"a 5-D mask has one trailing channel, got {tuple(m.shape)}")
        m = m[..., 0]
    if m.dim() != 4 or m.shape[0] not in (1, B):
        raise ValueError(f"mask must be [B|1, D', H', W'(, 1)] with B = {B}, got {tuple(m.shape)}")
    k = m.shape[1] // D
    if k < 1 or tuple(m.shape[1:]) != (k * D, k * H, k * W):
        raise ValueError(f"mask extent {tuple(m.shape[1:])} is no integer multiple of the latent's {(D, H, W)}")
    if not bool(((m >= 0) & (m <= 1)).all()):
        raise ValueError("mask values must lie in [0, 1]")
    if k > 1:
        m = m.reshape(m.shape[0], D, k, H, k, W, k).amax(dim=(2, 4, 6))
    return m.expand(B, D, H, W).contiguous()


def context_dropout(ids, p, null_context, *, seed=None, drop=None) -> np.ndarray:
    """The context ids a train step runs on (int32 [B]): ``ids`` with each entry replaced by ``null_context`` where ``drop`` (bool
    [B]) says so; ``drop`` None draws it, one uniform per sample from numpy's default_rng(``seed``), dropped where it is < ``p``
    (p = 0: never, p = 1: always)."""
    ids = np.array(ids, dtype=np.int32).reshape(-1)
    if drop is None:
        if not 0 <= float(p) <= 1:                            # a NaN fails the comparison too
            raise ValueError(f"context_dropout must lie in [0, 1], got {p}")
        drop = np.random.default_rng(seed).random(ids.size) < float(p)
    drop = np.asarray(_host(drop))
    if drop.dtype != np.bool_ or drop.reshape(-1).size != ids.size:
        raise ValueError(f"drop must hold one bool per sample ({ids.size})")
    ids[drop.reshape(-1)] = int(null_context)
    return ids


def _indices(v, B: int) -> np.ndarray:
    """One timestep index, or one per sample, as int64 [B] on the host."""
    return np.broadcast_to(np.asarray(torch.as_tensor(v).reshape(-1).cpu(), dtype=np.int64), (B,))

"""The float64 chain reference of the sampler GPU tests (plain helper, no test in it): DDPM, DDIM and DPM-Solver++(2M) chains, ODE and
SDE, restated from the formulas (Song et al., eq. 12; Lu et al. 2022, Algorithm 2 in the data-prediction form and its SDE midpoint
form, DESIGN.md sections 4.13 and 4.14), with the models, weights, oracle network and schedules the tests build them on.  The UniPC
chain is tests/unipc_reference.py.

Notation for a level with cumulative alpha ab: alpha = sqrt(ab), sigma = sqrt(1 - ab), lambda = log(alpha / sigma).  A schedule is
sched[0] < ... < sched[n-1]; a chain steps from sched[n-1] down to sched[0] and then to clean (level -1).  ``ab`` is any table that
indexes to a number: the oracle's float32 Betas table as float64 (oracle_alpha_bar) or alpha_bar64.

x0_32 and the two bound32 are float32 restatements that are compared bitwise: their operations keep their order.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

F = np.float32
F32_MAX = float(np.finfo(np.float32).max)


# ---- models, weights, the oracle network -----------------------------------------------------------------------------------------------
def args(T, bs=1):
    return SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=bs)


def schedule(T, S):
    return [T - 1] if S == 1 else [int(math.floor(i * (T - 1) / (S - 1) + 0.5)) for i in range(S)]


_WEIGHTS = {}


def weights(size=8, C=4, scale=1.0, seed=0, conditional=True):
    """The synthetic weights of a configuration, built once; ``scale`` scales the output conv (a scaled set shares every other array)."""
    import dm3d_amd
    key = (size, C, scale, seed, conditional)
    if key not in _WEIGHTS:
        if scale != 1.0:
            W = weights(size, C, 1.0, seed, conditional)
            W = dict(W, **{k: W[k] * np.float32(scale) for k in ("out.conv.kernel", "out.conv.bias")})
        else:
            W = dm3d_amd.synthetic_weights(dm3d_amd.UNetConfig(img_size=size, img_channels=C, conditional=conditional), seed=seed)
        _WEIGHTS[key] = W
    return _WEIGHTS[key]


def cond_model(T, B, size=8, C=4, W=None, **kw):
    """(the conditional DiffusionModel, its weights)."""
    from dm3d_amd.networks import conditional_dm3d as cdm
    W = weights(size, C) if W is None else W
    return cdm.DiffusionModel(size, 1024, C, None, args(T, B), weights=W, **kw), W


def uncond_model(T, B=1, size=8, C=4, **kw):
    """(the unconditional DiffusionModel, its weights)."""
    from dm3d_amd.networks import dm3d
    W = weights(size, C, conditional=False)
    return dm3d.DiffusionModel(size, 1024, C, None, args(T, B), weights=W, **kw), W


_ORACLES = {}


def oracle(W, size=8, C=4, conditional=True):
    """The CPU oracle network on ``W`` (built once per weight set and configuration): net(x, t, context) in float64."""
    from oracle import ref_torch as rt
    key = (id(W), size, C, conditional)
    if key not in _ORACLES:
        ocfg = rt.UNetConfig(img_size=size, img_channels=C, conditional=conditional)
        Wt = {k: torch.from_numpy(v) for k, v in W.items()}
        net = lambda x, t, ctx=None: rt.unet_forward(Wt, ocfg, x.float(), torch.full((x.shape[0],), int(t), dtype=torch.int64), ctx).double()
        _ORACLES[key] = (W, net)                        # W is held: its id stays its own
    return _ORACLES[key][1]


# ---- schedules -----------------------------------------------------------------------------------------------------------------------
def oracle_betas(T):
    """The oracle's Betas: float32 tables, the ones the kernels read (the DDPM posterior step takes the whole object)."""
    from oracle import ref_torch as rt
    return rt.Betas(T)


def oracle_alpha_bar(T):
    """alpha_bar of the oracle's Betas table, float32; ``.double()`` for the float64 formulas."""
    return oracle_betas(T).alpha_bar


def alpha_bar64(T, ztsnr=False):
    """The linear schedule's alpha_bar (with Algorithm 1 of Lin et al. 2023 for ``ztsnr``), rounded to the float32 the kernels read."""
    r = np.sqrt(np.cumprod(1 - np.linspace(0.0001, 0.02, T), 0))
    if ztsnr:
        r = (r - r[-1]) * (r[0] / (r[0] - r[-1]))
    return (r ** 2).astype(F).astype(np.float64)


# ---- the x0 estimate and its bound ---------------------------------------------------------------------------------------------------
def x0_64(kind, x, pred, a):
    """The x0 estimate at cumulative alpha ``a`` of a network output read as ``kind`` ("eps" / "v" / "x0")."""
    x, pred, al, sg = x.double(), pred.double(), math.sqrt(a), math.sqrt(1 - a)
    return {"eps": lambda: (x - sg * pred) / al, "v": lambda: al * x - sg * pred, "x0": lambda: pred}[kind]()


def eps64(kind, x, pred, a):
    """The same output as eps."""
    x, pred, al, sg = x.double(), pred.double(), math.sqrt(a), math.sqrt(1 - a)
    return {"eps": lambda: pred, "v": lambda: sg * x + al * pred, "x0": lambda: (x - al * pred) / sg}[kind]()


def threshold64(x0, p, cap, bounds=None):
    """Dynamic thresholding of an estimate [B, ...]: s of a volume is the p-quantile of |x0| (numpy's linear one), raised to 1, capped;
    clamp(x0, -s, s) / s.  Each volume's s is appended to ``bounds``."""
    out = []
    for b in range(x0.shape[0]):
        s = min(max(float(np.quantile(x0[b].abs().numpy().reshape(-1), p)), 1.0), cap)
        if bounds is not None:
            bounds.append(s)
        out.append(x0[b].clamp(-s, s) / s)
    return torch.stack(out)


def bounded64(x0, clip=True, thr=None):
    """The estimate a step uses: thresholded (``thr`` = (p, cap, list of recorded bounds)), clamped to [-1, 1], or as it is."""
    if thr is not None:
        return threshold64(x0, *thr)
    return x0.clamp(-1, 1) if clip else x0


def x0_32(x, e, ab32, t):
    """(x - sqrt(1-a) eps) / sqrt(a) of one volume in float32: mul, sub, div, each rounded; the coefficients are the host table's
    (float64 square roots of the float32 alpha_bar, rounded once)."""
    a = np.float64(np.asarray(ab32)[t])
    sqab, sq1ab = np.float32(np.sqrt(a)), np.float32(np.sqrt(1 - a))
    x, e = np.asarray(x, dtype=np.float32).reshape(-1), np.asarray(e, dtype=np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        return (x - sq1ab * e) / sqab


def bound32(x0, p, smax=F32_MAX):
    """(s, s_raw) of one volume's float32 x0 at ratio p: np.sort puts a NaN last, as the kernel's bit-pattern order does."""
    v = np.sort(np.abs(x0))
    N = v.size
    q = float(p) * (N - 1)
    i = min(int(math.floor(q)), N - 1)
    f = np.float32(q - i)
    with np.errstate(all="ignore"):
        raw = np.float32(v[i] + np.float32(f * np.float32(v[min(i + 1, N - 1)] - v[i])))
    s = raw if np.isnan(raw) else np.minimum(np.maximum(raw, np.float32(1)), np.float32(smax))
    return np.float32(s), raw


def bound32_at(x0, rank, frac, smax):
    """dm3d_thresh_desc's s of one volume's float32 x0 from the table's own rank and fraction: v_i + f*(v_{i+1} - v_i), raised to 1,
    capped."""
    v = np.sort(np.abs(x0))
    i = min(int(rank), v.size - 1)
    raw = F(v[i] + F(F(frac) * F(v[min(i + 1, v.size - 1)] - v[i])))
    return F(min(max(raw, F(1)), F(smax)))


# ---- steps and their coefficient rows ------------------------------------------------------------------------------------------------
def ddim_update64(x0, eps, a, ap, eta=0.0, z=None):
    """The DDIM update from an estimate: alpha_bar a -> ap (1: clean)."""
    sigma = eta * math.sqrt((1 - ap) / (1 - a)) * math.sqrt(1 - a / ap) if eta else 0.0
    out = math.sqrt(ap) * x0 + math.sqrt(max(1 - ap - sigma * sigma, 0.0)) * eps
    return out + sigma * z.double() if sigma else out


def ddim64(x, eps, a, ap, eta=0.0, z=None, clip=True):
    """One DDIM step on eps: x at alpha_bar a -> alpha_bar ap (1: the x0 estimate)."""
    x, eps = x.double(), eps.double()
    return ddim_update64(bounded64(x0_64("eps", x, eps, a), clip), eps, a, ap, eta, z)


def dpm_row64(ab, s, t, p, eta=0.0):
    """(c_x, c_0, c_1, c_z) of the DPM-Solver++(2M) step from level s to t (t < 0: clean); p: the level the step before started from
    (p < 0: first order); eta: the SDE form's (0: the ODE solver, c_z = 0).  h = lambda_t - lambda_s; from a level with ab = 0 the
    limits h = inf are written out, and a history level with ab = 0 has g = 0 (r = inf: first order)."""
    if t < 0:
        return 0.0, 1.0, 0.0, 0.0
    al = lambda i: math.sqrt(float(ab[i]))
    sg = lambda i: math.sqrt(1.0 - float(ab[i]))
    if ab[s] == 0.0:
        return (sg(t), al(t), 0.0, 0.0) if eta == 0 else (0.0, al(t), 0.0, sg(t))
    lam = lambda i: math.log(al(i) / sg(i))
    h = lam(t) - lam(s)
    A = al(t) * (1.0 - math.exp(-(1.0 + eta) * h))
    g = 0.0 if p < 0 or ab[p] == 0.0 else h / (2.0 * (lam(s) - lam(p)))
    return sg(t) / sg(s) * math.exp(-eta * h), A * (1.0 + g), -A * g, sg(t) * math.sqrt(1.0 - math.exp(-2.0 * eta * h))


def dpm_update64(x, x0, ab, s, t, p=-1, hist=None, eta=0.0, z=None):
    """The DPM-Solver++ update from an estimate; ``hist`` the estimate of the step before, ``z`` the SDE form's noise."""
    c_x, c_0, c_1, c_z = dpm_row64(ab, s, t, p, eta)
    out = c_x * x + c_0 * x0
    if c_1 != 0:
        out = out + c_1 * hist.double()
    if c_z != 0:
        out = out + c_z * z.double()
    return out


def dpm64(x, eps, ab, s, t, p=-1, hist=None, clip=True, eta=0.0, z=None):
    """One step on eps in float64: (x at t, the x0 estimate)."""
    x = x.double()
    x0 = bounded64(x0_64("eps", x, eps, float(ab[s])), clip)
    return dpm_update64(x, x0, ab, s, t, p, hist, eta, z), x0


def prev_levels(sched, order=2, lower_order_final=True):
    """The order rule: p of the step from sched[i] (the first step, the step to clean and, with lower_order_final, the step into
    sched[0] are first order)."""
    n = len(sched)
    prev = list(sched[1:]) + [-1]
    if order == 1:
        prev = [-1] * n
    if lower_order_final and n > 1:
        prev[1] = -1
    return prev


# ---- chain pieces --------------------------------------------------------------------------------------------------------------------
def guide64(pos, neg, w, phi=0.0, factors=None):
    """neg + w (pos - neg), volume by volume, rescaled by f = phi std(pos) / std(guided) + 1 - phi (population standard deviations;
    f = 1 where std(guided) = 0) where phi != 0.  ``w`` and ``phi``: one value or one per volume; each f is appended to ``factors``."""
    pos, neg = pos.double(), neg.double()
    B = pos.shape[0]
    per_volume = lambda v: [float(u) for u in np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1), (B,))]
    out = []
    for b, (wb, pb) in enumerate(zip(per_volume(w), per_volume(phi))):
        g = neg[b] + wb * (pos[b] - neg[b])
        if pb != 0:
            sg = float(g.std(unbiased=False))
            f = pb * float(pos[b].std(unbiased=False)) / sg + (1 - pb) if sg > 0 else 1.0
            if factors is not None:
                factors.append(f)
            g = f * g
        out.append(g)
    return torch.stack(out)


def known64(x0, ab, level, z):
    """The known latent at ``level`` in float64 (-1: x0)."""
    if level < 0:
        return x0.double()
    a = float(ab[level])
    return math.sqrt(a) * x0.double() + math.sqrt(1 - a) * z.double()


def edit_blend64(x0, ab, sched, keep, known_noise):
    """An edit chain's ``blend(i, x)``: after the step from sched[i], the known latent at the level the step reached (row i of
    known_noise; row 0 clean) replaces x by the weight ``keep`` [B, D, H, W]."""
    w = keep.double().unsqueeze(-1)
    return lambda i, x: w * known64(x0, ab, sched[i - 1] if i > 0 else -1, known_noise[i]) + (1 - w) * x


def half_mask(B, size=8, slab=False):
    """Regenerate the lower half of D, keep the upper half; ``slab``: a fractional slab at the boundary (size 16: a mask over 8^3 latents)."""
    m = torch.zeros((B, size, size, size))
    h = size // 2
    m[:, :h] = 1.0
    if slab:
        m[:, h:h + 2] = 0.3
        m[:, h:h + 2, :, :h // 2] = 0.8
    return m


def chain64(net, ab, sched, x_start, solver="dpmpp", kind="eps", eta=0.0, noise=None, order=2, lower_order_final=True, clip=True,
            thr=None, blend=None, steps=None, states=None, betas=None):
    """The whole chain with float64 bookkeeping: steps from sched[-1] down to sched[0], then clean.  ``net(x, t)`` is the network's
    output (guided already, where the chain is), read as ``kind``; ``noise[i]`` the z of the step from sched[i].
    solver "ddpm": the oracle's posterior step on ``betas``, the oracle's Betas (z = 0 at t = 0, as the reference's loop);
    "ddim": eta is DDIM's, and the model's eps is carried on beside the bounded estimate;
    "dpmpp": ``order`` / ``lower_order_final`` set the rows, eta is the SDE form's, the history is the bounded estimate, before any blend.
    The estimate is thresholded (``thr`` = (p, cap, list): the bounds are recorded), clamped (``clip``) or left.  ``blend(i, x)`` (edit
    chains) follows the step from sched[i]; ``steps`` stops the chain early; ``states`` collects x after every step."""
    x, hist, prev = x_start.double(), None, prev_levels(sched, order, lower_order_final)
    for k, i in enumerate(range(len(sched) - 1, -1, -1)):
        if steps is not None and k == steps:
            break
        t, t_next = sched[i], (sched[i - 1] if i > 0 else -1)
        a = float(ab[t])
        pred = net(x, t)
        z = None if noise is None else noise[i]
        if solver == "ddpm":
            from oracle import ref_torch as rt
            z = z.double() if t > 0 else torch.zeros_like(x)
            x = rt.ddpm_step(betas, x, eps64(kind, x, pred, a), torch.full((x.shape[0],), t, dtype=torch.int64), z)
        else:
            x0 = bounded64(x0_64(kind, x, pred, a), clip, thr)
            if solver == "ddim":
                x = ddim_update64(x0, eps64(kind, x, pred, a), a, float(ab[t_next]) if t_next >= 0 else 1.0, eta, z)
            else:
                x, hist = dpm_update64(x, x0, ab, t, t_next, prev[i], hist, eta, z), x0
        if blend is not None:
            x = blend(i, x)
        if states is not None:
            states.append(x)
    return x

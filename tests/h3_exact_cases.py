"""Constructed operands on which the split-float16 (h3) contractions of the C ABI are EXACT (plain helper, numpy / torch-CPU only, no test
in it; tests/test_h3_exact_host.py checks it on the CPU, tests/test_gpu_h3_exact.py feeds it to the kernels).

Why.  The h3 mode splits x = hi + lo, hi = fp16(x), lo = fp16(x - hi), and forms a.b = al.bh + ah.bl + ah.bh into a
float32 accumulator.  The Gaussian parity tests hold max|err| / max|ref| to 2e-5; a cross term lost for one (tap, input channel) moves a
k3 Cin = 32 output by about 2e-6 of max|ref| and a whole 8-channel slot of a 64-byte record by about 6e-6: both pass there
(`gaussian_drop_error` below measures it).  Here every product and every partial sum is representable in float32, so the float64
reference and a correct kernel agree BIT FOR BIT in any summation order, and a lost, doubled or misplaced piece is a non-zero difference
of at least one quantum.  This is the contraction-axis counterpart of tests/attention_logit_cases.py and tests/norm_offset_cases.py.

Exactness budget.  A case is admissible when (1) every term a kernel may add into an output — the three products of every live (tap,
channel), bias, vec, res, a fused skip conv's products, the parts of a Cin split (partial sums of the same terms) — is an integer multiple
of one quantum q, and (2) sum|terms| / q < 2^21 per output, three bits under float32's 24.  Then every partial sum in ANY order is a multiple
of q below 2^21 q, i.e. a float32, and IEEE addition returns it unrounded.  `budget` computes q (from the operands' own binary quanta) and
the ratio for every case; sum|a||b| comes from the float64 reference applied to |x| and |w|.  For the Winograd-x form the ratio is computed
again on the transformed operands (inputs d0-d2, d1+d2, d2-d1, d1-d3; weights g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2 — quantum q/2); for the
UpSample parity sums |a||sum w| <= sum|a||w| term by term, so the plain ratio bounds it (Conv3DTranspose parities select taps, they sum
none).  `assert_lossless` checks fp16(v) + fp16(v - fp16(v)) == v on every value a kernel splits: activations, Winograd-transformed
activations, and weights / transformed weights / parity sums times 2^w_exp.

Patterns (all |values| <= 1; "coarse" = {0, +-1/2, +-1}; "fine" = odd multiples of 2^-12 in (1/2, 1), 12 significant bits, which float16
cannot hold, mixed with 3 % coarse values):
  hi       both operands coarse: only ah.bh is live.  The control: no split term, no path the Gaussian suite does not already hold.
  act-lo   activations fine (lo != 0 on >= 90 %, asserted), weights coarse (bl = 0, al.bl = 0): exercises al.bh.
  wgt-lo   the mirror image: exercises ah.bl.
  both-lo  both fine; NOT exact: the bar per output is 2^-21 sum|a||b| (the dropped al.bl at 2^-22 per product, as much again for the
           accumulation), per output and not max-normalised.  Its bias, vec and res are ZERO: the bar scales with the products alone
           and has no room for the float32 rounding of additive terms up to 12 on an output whose products sum to 1; the epilogue's
           additions are what the three exact patterns hold.

Sparse conv weights.  Output channel co has non-zero weights only at flat positions p = tap Cin + ci with (p + r) mod M == co mod M,
M = min(64, Cout) (M = 64 for every full column tile; a narrower conv takes M = Cout so that no (tap, ci) goes unused).  At Cout = 64
that is 14-27 non-zeros per output and every (tap, ci) is live in exactly one output channel of the tile.  The rotations r in {0, 1, 16,
21} move the assignment across both column maps (channel 16 ni + j and channel 4 j + ni).  Activations are dense over voxels, so every
halo and padding position takes part.  GEMM operands are dense; the fused MLP takes W0 with 4 and W1 with 8 non-zeros per row from {+-1}.

Epilogue operands: bias, vec, res and the skip kernel are multiples of 2^-4 (the skip kernel: signed powers of two from 1/4 to 4, at two
sparse positions per output, so that its products keep a quantum of 2^-14 under fine activations); PReLU slopes from {1/4, 1/2} (they
divide q by 4); ReLU as the case lists it.

Forms with an inexact step — the fused norm + SiLU prologue (direct kernel with `pro`, Winograd MODE 1) and post_* / DM3D_FMT_H2
output — run act-lo and wgt-lo with that step evaluated in float64, against the per-output bar ELEM_TOL sum|a||b| (ELEM_TOL = 1e-6, the
project's elementwise tolerance; a is the value the contraction sees, behind the prologue).  A lost cross term is 2^-12 of its product,
about 18x that per product.  The prologue's shift is 2.5 +- 0.2 (scale 0.5 .. 1.5), so that silu leaves no activation near zero and
even a corner output, with a few live taps, has sum|a||b| >= 1.  So that the bar, which scales with the products alone, also covers the float32 rounding of the additive
epilogue and of the consumer's step, those forms keep |bias|, |vec|, |res| <= 1/2 and the post scale in {1/4, 1/2}, |post shift| <= 1/4:
the step's argument is then at most sum|a||b| / 2 + 1 and an elementwise error of ELEM_TOL / 2 of it stays inside the bar wherever
sum|a||b| >= 1, which `budget` asserts for them.

Host model.  `h3_contract` emulates the contraction: both operands split, the three products formed in float32, summed one by one in a
caller-given permutation, with `drop=(term, tap, slot)` omitting one piece (term "al_bh" or "ah_bl", slot = ci // 8).  `wino_contract` is
the F(2,3)-x variant (transform, split, four term contractions, output pair); its `fold` argument adds tap (0,2)'s ah.bh and al.bh as
ONE term, as the pad step of DESIGN.md section 4.2 forms them inside one MFMA.

Not covered: dm3d_attn_front (layer norms sit in front of its contractions, so its operands cannot be constructed); the attention
kernels' logit axis has tests/test_gpu_attention_logits.py."""
import numpy as np
import torch

from guarded_buffers import h2_decode, h2_encode
from oracle import ref_kernels as rk
from oracle import ref_torch as rt

PATTERNS = ("hi", "act-lo", "wgt-lo", "both-lo")
EXACT = ("hi", "act-lo", "wgt-lo")
ROTATIONS = (0, 1, 16, 21)
BUDGET = 2.0 ** 21
BOTH_LO_TOL = 2.0 ** -21
ELEM_TOL = 1e-6
COARSE = np.array([0.0, 0.5, -0.5, 1.0, -1.0])
TERMS = ("al_bh", "ah_bl")

# Names of test_gpu_infer_kernels.CONV_CASES.  The exact list runs each case through `exact_form` (no prologue: the direct kernel's plain
# staging, Winograd MODE 0); H2_IN_TOO repeats a case behind a DM3D_FMT_H2 input (Winograd MODE 2).  The inexact list runs cases as listed.
EXACT_CONV = ("v3 td4 nct4 full 16B", "v3 td8 nct4 full 16B", "v3 td4 nct2 cout32", "v3 td4 nct1 cout8", "v3 td4 partial 6x5x7 cout40",
              "v3 td8 partial 6x5x7 cout40", "v3 dual input 16+12", "v3 H2 in", "v3 td4 full scalar (PReLU)", "v3 fused skip (skip_wpk)",
              "v3 Cin split", "wino Cin32", "wino Cin48 B2", "wino two-way Cin split", "wino skip tail (skip_wpk_frag)", "pack h3w 20->40",
              "tap k3 s2 5x6x8", "tap k1 full brick", "tap k1 partial 5x6x7", "tap k4 s2 6x8x4", "parity upsample 4^3", "parity transpose 4^3",
              "parity transpose 3x5x4")
H2_IN_TOO = ("wino Cin32", "wino Cin48 B2")
INEXACT_CONV = ("v3 td4 nct4 full 16B", "wino Cin32", "v3 td4 H2 out + post", "v3 post, float32 out", "wino H2 out + post")


# ---- values ------------------------------------------------------------------------------------------------------------------------------
def coarse(rng, *shape, nonzero=False):
    return rng.choice(COARSE[1:] if nonzero else COARSE, size=shape).astype(np.float32)


def fine(rng, *shape, nonzero=False):
    """Odd multiples of 2^-12 in (1/2, 1) with random sign (12 significant bits: lo != 0), 3 % coarse values among them."""
    m = (2 * rng.integers(1024, 2048, size=shape) + 1) * rng.choice([-1.0, 1.0], size=shape)
    v = (m * 2.0 ** -12).astype(np.float32)
    c = coarse(rng, *shape, nonzero=nonzero)
    return np.where(rng.random(shape) < 0.03, c, v).astype(np.float32)


def sixteenths(rng, *shape, bound=4.0):
    """Multiples of 2^-4 in [-bound, bound]."""
    n = int(bound * 16)
    return (rng.integers(-n, n + 1, size=shape) / 16.0).astype(np.float32)


def operand(rng, pattern, side, *shape, nonzero=False):
    """The values of one side ("act" or "wgt") of a contraction under a pattern."""
    lo = pattern == "both-lo" or pattern == side + "-lo"
    return (fine if lo else coarse)(rng, *shape, nonzero=nonzero)


def split16(v):
    """(hi, lo) of float32 values as float32 arrays: hi = fp16(v), lo = fp16(v - hi)."""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16).astype(np.float32)
    return hi, (v - hi).astype(np.float16).astype(np.float32)


def lo_share(v):
    return float((split16(v)[1] != 0).mean())


def assert_lossless(name, v):
    hi, lo = split16(v)
    v = np.asarray(v, np.float32)
    assert np.isfinite(hi).all() and np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), v.astype(np.float64)), f"{name}: hi + lo loses bits"


def quantum(*arrays):
    """The largest power of two that divides every entry of the arrays (1 for all-zero input)."""
    v = np.concatenate([np.zeros(1)] + [np.asarray(a, np.float64).ravel() for a in arrays if a is not None])
    v = v[v != 0]
    if v.size == 0:
        return 1.0
    for e in range(8, -41, -1):
        s = v * 2.0 ** -e
        if np.array_equal(s, np.rint(s)):
            return 2.0 ** e
    raise AssertionError("an operand is no multiple of 2^-40")


def w_exponent(*wmax):
    """The power of two that brings the largest weight into [2^13, 2^14) (ops.h3_weight_exponent)."""
    return int(13 - np.floor(np.log2(max(float(w) for w in wmax))))


# ---- convs -------------------------------------------------------------------------------------------------------------------------------
def modulus(cout):
    return min(64, cout)


def live_mask(taps, cin, cout, rot):
    """[taps * cin, cout] bool: position p = tap cin + ci is live for channel co iff (p + rot) mod M == co mod M."""
    M = modulus(cout)
    p = np.arange(taps * cin)[:, None]
    return (p + rot) % M == (np.arange(cout) % M)[None, :]


def live_positions(taps, cin, cout, rot, co):
    p = np.nonzero(live_mask(taps, cin, cout, rot)[:, co])[0]
    return [(int(q // cin), int(q % cin)) for q in p]


def out_dims(s):
    D, H, W = s["dims"]
    if s["up"] or s["tr"]:
        return 2 * D, 2 * H, 2 * W
    return tuple(-(-n // s["stride"]) for n in (D, H, W))


def exact_form(s, **kw):
    """The case without its inexact steps (no prologue, no post step, float32 output, no in_scale), plus overrides."""
    return dict(s, pro=None, post=False, out_h2=False, in_scale=False, **kw)


def is_inexact(s):
    return bool(s["pro"]) or s["post"] or s["out_h2"]


def _flat_kernel(s, k):
    """[taps * cin, cout] view of a case's Keras kernel in position order p = tap cin + ci."""
    cin, cout = s["c1"] + s["c2"], s["cout"]
    if s["tr"]:
        return k.transpose(0, 1, 2, 4, 3).reshape(64 * cin, cout)
    return k.reshape(-1, cout)


def conv_host(s, pattern, rot, seed=0):
    """The operands of case `s` (a test_gpu_infer_kernels._case dict) under a pattern and a rotation, with the keys _conv_host gives:
    numpy arrays, and h["base"], the float64 result without the residual and the consumer's post step.  Also h["abs"] = sum|a||b| per
    output (skip products included) and h["eps_abs"], the sum of |bias|, |vec|, |res|."""
    rng = np.random.default_rng([seed, rot, PATTERNS.index(pattern), sum(map(ord, s["name"]))])
    B, cin, cout = s["B"], s["c1"] + s["c2"], s["cout"]
    od = out_dims(s)
    small = is_inexact(s)
    eb = 0.0 if pattern == "both-lo" else 0.5 if small else 4.0       # (both-lo: see the module docstring)
    h = {"in_scale": None}
    x = operand(rng, pattern, "act", B, *s["dims"], cin)
    x1, x2 = np.ascontiguousarray(x[..., :s["c1"]]), (np.ascontiguousarray(x[..., s["c1"]:]) if s["c2"] else None)
    if s["x_h2"]:
        h["x1_words"] = h2_encode(x1)
        assert np.array_equal(h2_decode(h["x1_words"]), x1.astype(np.float64)), "DM3D_FMT_H2 does not hold the activations"
    h["x1"], h["x2"] = x1, x2
    taps = 64 if s["tr"] else s["ks"] ** 3
    flat = operand(rng, pattern, "wgt", taps * cin, cout, nonzero=True) * live_mask(taps, cin, cout, rot)
    if s["tr"]:
        h["kernel"] = np.ascontiguousarray(flat.reshape(4, 4, 4, cin, cout).transpose(0, 1, 2, 4, 3)).astype(np.float32)
    else:
        h["kernel"] = flat.reshape((s["ks"],) * 3 + (cin, cout)).astype(np.float32)
    h["bias"] = sixteenths(rng, cout, bound=eb) if s["bias"] else None
    if s["vec"]:
        h["vec"] = sixteenths(rng, B + 2, cout, bound=eb)
        h["vec_idx"] = ((np.arange(B) * 2 + 1) % (B + 2)).astype(np.int32)
    else:
        h["vec"] = h["vec_idx"] = None
    if s["pro"]:
        shape = (B, cin) if s["pro"] == "sample" else (cin,)
        h["pro"] = ((rng.random(shape) + 0.5).astype(np.float32), (2.5 + rng.standard_normal(shape) * 0.2).astype(np.float32))
    else:
        h["pro"] = None
    h["prelu"] = rng.choice([0.25, 0.5], size=od + (cout,)).astype(np.float32) if s["prelu"] else None
    skip = None
    if s["skip"]:
        _, sc1, sc2 = s["skip"]
        sx = operand(rng, pattern, "act", B, *s["dims"], sc1 + sc2)
        h["skip_x1"], h["skip_x2"] = np.ascontiguousarray(sx[..., :sc1]), (np.ascontiguousarray(sx[..., sc1:]) if sc2 else None)
        sk = rng.choice([0.25, 0.5, 1.0, 2.0, 4.0], size=(sc1 + sc2, cout)) * rng.choice([-1.0, 1.0], size=(sc1 + sc2, cout))
        keep = (np.arange(sc1 + sc2)[:, None] + rot) % ((sc1 + sc2) // 2) == (np.arange(cout) % ((sc1 + sc2) // 2))[None, :]
        h["skip_k"] = (sk * keep).astype(np.float32)
        skip = (sx, h["skip_k"])
    h["post"] = (rng.choice([0.25, 0.5], size=cout).astype(np.float32), sixteenths(rng, cout, bound=0.25)) if s["post"] else None
    h["res"] = sixteenths(rng, B, *od, cout, bound=eb) if s["res"] else None
    conv = dict(x2=x2, ksize=s["ks"], stride=s["stride"], upsample=s["up"], transpose=s["tr"])
    h["base"] = rk.conv3d_fused(x1, h["kernel"], bias=h["bias"], pro=h["pro"], vec=h["vec"], vec_idx=h["vec_idx"], relu=s["relu"],
                                prelu_alpha=h["prelu"], skip=skip, **conv).numpy()
    # what the contraction sees, in float64 (behind the prologue), and sum |a||b| per output from the same reference on absolute values
    a64 = _acts64(h, x)
    ax = np.abs(a64)
    h["abs"] = rk.conv3d_fused(ax[..., :s["c1"]], np.abs(h["kernel"]), x2=ax[..., s["c1"]:] if s["c2"] else None, ksize=s["ks"], stride=s["stride"],
                               upsample=s["up"], transpose=s["tr"], skip=(np.abs(skip[0]), np.abs(skip[1])) if skip else None).numpy()
    e = np.zeros((B,) + od + (cout,))
    if h["bias"] is not None:
        e += np.abs(h["bias"])
    if h["vec"] is not None:
        e += np.abs(h["vec"].astype(np.float64))[h["vec_idx"]][:, None, None, None, :]
    if h["res"] is not None:
        e += np.abs(h["res"])
    h["eps_abs"] = e
    h["w_exp"] = w_exponent(*([float(np.abs(h["kernel"]).max()) * (8.0 if s["up"] else 1.0)] + ([float(np.abs(h["skip_k"]).max())] if s["skip"] else [])))
    return h


def _acts64(h, x):
    a = x.astype(np.float64)
    if h["pro"] is not None:
        sc, sh = (p.astype(np.float64) for p in h["pro"])
        if sc.ndim == 2:
            sc, sh = sc[:, None, None, None, :], sh[:, None, None, None, :]
        a = rt._swish(torch.from_numpy(a * sc + sh)).numpy()
    return a


def conv_finish(h, res):
    """base + res, then the consumer's norm + SiLU in float64: what the launch stores."""
    y = h["base"] if res is None else h["base"] + res.astype(np.float64)
    if h["post"] is not None:
        y = rt._swish(torch.from_numpy(y * h["post"][0].astype(np.float64) + h["post"][1].astype(np.float64))).numpy()
    return y


def conv_x(h):
    return h["x1"] if h["x2"] is None else np.concatenate([h["x1"], h["x2"]], -1)


def up_parity_sums(k):
    """[8 parities, 8 taps, cin, cout]: the 2x2x2 kernels of a k3 conv on the nearest-2x upsampled tensor (csrc/dm3d_pack.hip, up_weight)."""
    sel = {(0, 0): (0, 0), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2, 2)}              # (parity, tap) -> inclusive range of k3 taps along an axis
    out = np.zeros((8, 8) + k.shape[3:], np.float64)
    for par in range(8):
        for tap in range(8):
            r = [sel[((par >> sh) & 1, (tap >> sh) & 1)] for sh in (2, 1, 0)]
            out[par, tap] = k[r[0][0]:r[0][1] + 1, r[1][0]:r[1][1] + 1, r[2][0]:r[2][1] + 1].astype(np.float64).sum((0, 1, 2))
    return out


def wino_weights(k):
    """[4 terms, 3, 3, cin, cout] float32, the packer's operations in its order: g0, ((g0 + g2) + g1) / 2, ((g0 + g2) - g1) / 2, g2."""
    g0, g1, g2 = (k[:, :, i].astype(np.float32) for i in range(3))
    return np.stack([g0, np.float32(0.5) * ((g0 + g2) + g1), np.float32(0.5) * ((g0 + g2) - g1), g2])


def wino_inputs(x):
    """[4 terms, B, D, H, W / 2, C] float32: d0 - d2, d1 + d2, d2 - d1, d1 - d3 of the x-padded rows, per output pair."""
    xp = np.pad(np.asarray(x, np.float32), ((0, 0), (0, 0), (0, 0), (1, 1), (0, 0)))
    d = [xp[:, :, :, i::2][:, :, :, :x.shape[3] // 2] for i in range(4)]
    return np.stack([d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]])


def _rows9(v):
    """[B, D, H, Wp, C] -> [voxels, 9 * C]: the (dz, dy) neighbourhood of every position, zero padded, position order (dz 3 + dy) C + ci."""
    B, D, H, Wp, Cn = v.shape
    vp = np.pad(v, ((0, 0), (1, 1), (1, 1), (0, 0), (0, 0)))
    cols = [vp[:, dz:dz + D, dy:dy + H] for dz in range(3) for dy in range(3)]
    return np.stack(cols, 4).reshape(B * D * H * Wp, 9 * Cn)


def budget(s, h, pattern):
    """Asserts the exactness budget and the lossless splits of a host dict; returns (q, worst ratio sum|terms| / q)."""
    name = f"{s['name']} / {pattern}"
    x = conv_x(h)
    cin = x.shape[-1]
    assert float(np.abs(x).max()) <= 1 and float(np.abs(h["kernel"]).max()) <= 1
    if pattern in ("act-lo", "both-lo"):
        assert lo_share(x) >= 0.9, f"{name}: lo != 0 on {lo_share(x):.2f} of the activations"
    if pattern in ("wgt-lo", "both-lo"):
        kf = _flat_kernel(s, h["kernel"])
        assert lo_share(kf[kf != 0]) >= 0.9, f"{name}: lo != 0 on {lo_share(kf[kf != 0]):.2f} of the live weights"
    scale = 2.0 ** h["w_exp"]
    if h["pro"] is None:
        assert_lossless(name + " activations", x)
    wk = up_parity_sums(h["kernel"]) if s["up"] else h["kernel"].astype(np.float64)
    assert float(np.abs(wk).max()) * scale < 2.0 ** 14
    assert_lossless(name + " weights", wk * scale)
    q = quantum(x) * quantum(h["kernel"])
    if s["skip"]:
        sx = h["skip_x1"] if h["skip_x2"] is None else np.concatenate([h["skip_x1"], h["skip_x2"]], -1)
        assert_lossless(name + " skip activations", sx)
        assert_lossless(name + " skip weights", h["skip_k"].astype(np.float64) * scale)
        q = min(q, quantum(sx) * quantum(h["skip_k"]))
    q = min(q, quantum(h["bias"], h["vec"], h["res"]))
    total = h["abs"] + h["eps_abs"]
    ratio = float(total.max()) / q
    if s["wino"] and h["pro"] is None:
        v, u = wino_inputs(x), wino_weights(h["kernel"])
        assert_lossless(name + " transformed activations", v)
        assert_lossless(name + " transformed weights", u.astype(np.float64) * scale)
        qw = min(quantum(v) * quantum(u), q)
        m = [np.abs(_rows9(v[t]).astype(np.float64)) @ np.abs(u[t].astype(np.float64)).reshape(9 * cin, -1) for t in range(4)]
        pair = np.maximum(m[0] + m[1] + m[2], m[1] + m[2] + m[3])                      # output 2j: terms 0-2; output 2j + 1: terms 1-3
        ratio = max(ratio, (float(pair.max()) + float(h["eps_abs"].max()) + (float((h["abs"] - _main_abs(s, h)).max()) if s["skip"] else 0.0)) / qw)
        q = qw
    if h["prelu"] is not None:
        q, ratio = q / 4, ratio * 4
    if pattern in EXACT and not is_inexact(s):
        assert ratio < BUDGET, f"{name}: sum|terms| / q = {ratio:.3g} exceeds 2^21"
    if is_inexact(s):
        assert float(h["abs"].min()) >= 1.0, f"{name}: an output with sum|a||b| = {float(h['abs'].min()):.3g} < 1 has no room for the elementwise step"
    return q, ratio


def _main_abs(s, h):
    x = np.abs(_acts64(h, conv_x(h)))
    return rk.conv3d_fused(x[..., :s["c1"]], np.abs(h["kernel"]), x2=x[..., s["c1"]:] if s["c2"] else None, ksize=s["ks"], stride=s["stride"],
                           upsample=s["up"], transpose=s["tr"]).numpy()


def conv_bar(s, h, pattern):
    """The per-output bound of a case that is not exact: [B, od, cout] float64."""
    if is_inexact(s):
        return ELEM_TOL * h["abs"]
    assert pattern == "both-lo"
    return BOTH_LO_TOL * h["abs"]


def explain(s, rot, got, ref, q):
    """The message of a failed exact comparison: first differing (voxel, co), the (tap, ci) live there, the difference in quanta."""
    bad = np.argwhere(got != ref)
    if bad.size == 0:
        return ""
    i = tuple(int(v) for v in bad[0])
    cin = s["c1"] + s["c2"]
    taps = 64 if s["tr"] else s["ks"] ** 3
    return (f"{s['name']} rotation {rot}: {len(bad)} of {got.size} outputs differ; first at (b, z, y, x) = {i[:-1]}, co = {i[-1]}: got {got[i]!r}, "
            f"reference {ref[i]!r}, difference {(float(got[i]) - float(ref[i])) / q:+.3g} q (q = 2^{int(np.log2(q))}); live (tap, ci) of that channel: "
            f"{live_positions(taps, cin, s['cout'], rot, i[-1])}")


# ---- im2col and the host model -----------------------------------------------------------------------------------------------------------
def same_pad(n, k, stride):
    """(before, after) of TensorFlow's SAME padding."""
    total = max((-(-n // stride) - 1) * stride + k - n, 0)
    return total // 2, total - total // 2


def im2col(s, x):
    """[voxels, taps * cin] float32 rows of a k1 / k3 / k4 'same' conv at stride 1 or 2, or of the k3 conv on the nearest-2x upsampled
    tensor; position order p = tap cin + ci, voxel order (b, z, y, x) of the output."""
    assert not s["tr"]
    x = np.asarray(x, np.float32)
    if s["up"]:
        x = x.repeat(2, 1).repeat(2, 2).repeat(2, 3)
    k, st = s["ks"], s["stride"]
    pads = [same_pad(n, k, st) for n in x.shape[1:4]]
    xp = np.pad(x, [(0, 0)] + pads + [(0, 0)])
    od = [-(-n // st) for n in x.shape[1:4]]
    cols = [xp[:, a:a + st * od[0]:st, b:b + st * od[1]:st, c:c + st * od[2]:st] for a in range(k) for b in range(k) for c in range(k)]
    return np.stack(cols, 4).reshape(-1, k ** 3 * x.shape[-1])


def h3_contract(A, W, cin, perm=None, drop=None, fold_taps=()):
    """The h3 contraction of A [rows, K] with W [K, cols] (float32, W already times 2^w_exp; position p = tap cin + ci): both operands
    split, ah.bh, al.bh and ah.bl formed in float32 for every live position of a column, and added one by one into a float32 accumulator
    in the order perm(n_terms) gives (None: as listed).  drop = (term, tap, slot) omits that piece for the channels ci // 8 == slot of the
    tap; the taps of fold_taps add ah.bh + al.bh as one term.  Returns float32 [rows, cols]."""
    ah, al = split16(A)
    wh, wl = split16(W)
    p = np.arange(A.shape[1])
    dropped = np.zeros(A.shape[1], bool) if drop is None else (p // cin == drop[1]) & ((p % cin) // 8 == drop[2])
    folded = np.isin(p // cin, list(fold_taps))
    out = np.zeros((A.shape[0], W.shape[1]), np.float32)
    for co in range(W.shape[1]):
        idx = np.nonzero(W[:, co])[0]
        hh, lh, hl = ah[:, idx] * wh[idx, co], al[:, idx] * wh[idx, co], ah[:, idx] * wl[idx, co]
        if drop is not None:
            (lh if drop[0] == "al_bh" else hl)[:, dropped[idx]] = 0
        f = folded[idx]
        terms = np.concatenate([hh[:, ~f], lh[:, ~f], hh[:, f] + lh[:, f], hl], 1)
        order = np.arange(terms.shape[1]) if perm is None else perm(terms.shape[1])
        acc = np.zeros(A.shape[0], np.float32)
        for j in order:
            acc = acc + terms[:, j]
        out[:, co] = acc
    return out


def wino_contract(x, kernel, w_exp, perm=None, drop=None, fold=True):
    """The Winograd F(2,3)-x form of a k3 stride-1 conv on x [B, D, H, W, C] (W even): transformed inputs and weights in float32, each
    split, the four term contractions over the nine (dz, dy) taps by `h3_contract` (tap (0,2) folded as the pad step does), and
    y(2j) = m0 + m1 + m2, y(2j + 1) = m1 - m2 - m3 in float32, times 2^-w_exp.  drop = (term, tap of 9, slot[, Winograd term])."""
    B, D, H, Wd, Cn = x.shape
    v, u = wino_inputs(x), wino_weights(kernel) * np.float32(2.0 ** w_exp)
    m = []
    for t in range(4):
        d = drop if drop is not None and (len(drop) < 4 or drop[3] == t) else None
        m.append(h3_contract(_rows9(v[t]), u[t].reshape(9 * Cn, -1), Cn, perm, None if d is None else d[:3], fold_taps=(2,) if fold else ()))
    y = np.stack([(m[0] + m[1]) + m[2], (m[1] - m[2]) - m[3]], 1)                         # [pairs, 2, cout]
    y = y.reshape(B, D, H, Wd // 2, 2, -1).reshape(B, D, H, Wd, -1)
    return y * np.float32(2.0 ** -w_exp)


def direct_contract(s, h, perm=None, drop=None):
    """The direct forms' contraction of a host dict (no epilogue): float32 [B, od, cout]."""
    A = im2col(s, conv_x(h))
    W = _flat_kernel(s, h["kernel"]) * np.float32(2.0 ** h["w_exp"])
    y = h3_contract(A, W, s["c1"] + s["c2"], perm, drop) * np.float32(2.0 ** -h["w_exp"])
    return y.reshape((s["B"],) + out_dims(s) + (s["cout"],))


def conv_only64(s, h):
    """The float64 convolution of a host dict without any epilogue."""
    return rk.conv3d_fused(h["x1"], h["kernel"], x2=h["x2"], ksize=s["ks"], stride=s["stride"], upsample=s["up"], transpose=s["tr"]).numpy()


def gaussian_drop_error(s, h, drop, ref_max=None, channels=8):
    """What dropping one piece costs on DENSE operands, as the Gaussian suite measures it: max|err| / max|ref| of the three-product sum
    without the piece (products and sums in float64: the accumulation's own 1e-7 is left out) against the float64 conv of a k3 stride-1
    case; h is test_gpu_infer_kernels._conv_host's dict, its prologue applied in float64 first.  ref_max: the max|ref| to normalise by
    (the suite's is that of the stored output, epilogue and residual included); None: the bare convolution's.  channels=1: drop[2] is one
    input channel, not a slot of eight."""
    x = _acts64(h, conv_x(h)).astype(np.float32)
    cin = x.shape[-1]
    A = im2col(dict(s, up=False), x)
    w_exp = w_exponent(float(np.abs(h["kernel"]).max()))
    W = (h["kernel"].reshape(-1, s["cout"]) * np.float32(2.0 ** w_exp)).astype(np.float32)
    (ah, al), (wh, wl) = (tuple(t.astype(np.float64) for t in split16(A))), (tuple(t.astype(np.float64) for t in split16(W)))
    ref = A.astype(np.float64) @ W.astype(np.float64)
    p = np.arange(A.shape[1])
    sel = (p // cin == drop[1]) & ((p % cin) // channels == drop[2])
    piece = (al[:, sel] @ wh[sel]) if drop[0] == "al_bh" else (ah[:, sel] @ wl[sel])
    got = ah @ wh + al @ wh + ah @ wl - piece
    return float(np.abs(got - ref).max() / (np.abs(ref).max() if ref_max is None else ref_max * 2.0 ** w_exp))


# ---- GEMM --------------------------------------------------------------------------------------------------------------------------------
def gemm_problem(pattern, m, n, k, batch, af, bf, bias, res, act, alpha, seed=0):
    """A dense dm3d_gemm_tn problem under a pattern, with the keys test_gpu_infer_kernels._gemm_problem gives (float32 output, H3), plus
    p["abs"] = sum|terms| per output, p["q"] and p["ratio"]."""
    rng = np.random.default_rng([seed, m, n, k, batch, af, bf, PATTERNS.index(pattern)])
    a, b = operand(rng, pattern, "act", batch, m, k), operand(rng, pattern, "wgt", batch, n, k)
    p = dict(m=m, n=n, k=k, batch=batch, af=af, bf=bf, of=0, prec=1, act=act, alpha=alpha, bcast_b=False, bias_m=bias == "m")
    p["a_words"], p["b_words"] = (h2_encode(a) if af else a), (h2_encode(b) if bf else b)
    for words, v, f in ((p["a_words"], a, af), (p["b_words"], b, bf)):
        assert not f or np.array_equal(h2_decode(words), v.astype(np.float64))
    p["a"], p["b"] = a, b
    eb = 0.0 if pattern == "both-lo" else 4.0
    p["bias"] = sixteenths(rng, m if bias == "m" else n, bound=eb) if bias else None
    p["res"] = sixteenths(rng, batch, m, n, bound=eb) if res >= 1 else None
    p["res2"] = sixteenths(rng, batch, m, n, bound=eb) if res >= 2 else None
    assert_lossless("gemm a", a), assert_lossless("gemm b", b)
    assert np.log2(abs(alpha)) == np.rint(np.log2(abs(alpha))), "alpha must be a power of two"
    prod = np.einsum("bmk,bnk->bmn", np.abs(a).astype(np.float64), np.abs(b).astype(np.float64))
    p["prod_abs"] = abs(alpha) * prod
    tot = p["prod_abs"].copy()
    if p["bias"] is not None:
        tot += np.abs(p["bias"])[:, None] if p["bias_m"] else np.abs(p["bias"])
    for r in (p["res"], p["res2"]):
        if r is not None:
            tot += np.abs(r)
    # the accumulator holds unscaled products (grid qa qb); behind alpha every term lies on the grid min(|alpha| qa qb, the epilogue's)
    qp = quantum(a) * quantum(b)
    p["q"] = min(qp * abs(alpha), quantum(p["bias"], p["res"], p["res2"]))
    p["ratio"] = max(float(prod.max()) / qp, float(tot.max()) / p["q"])
    if pattern in EXACT:
        assert p["ratio"] < BUDGET, f"gemm m{m} n{n} k{k} {pattern}: sum|terms| / q = {p['ratio']:.3g} exceeds 2^21"
    if pattern in ("act-lo", "both-lo"):
        assert lo_share(a) >= 0.9
    if pattern in ("wgt-lo", "both-lo"):
        assert lo_share(b) >= 0.9
    p["ref"] = rk.gemm_tn(a, b, alpha=alpha, bias=p["bias"], bias_along_m=p["bias_m"], kind=act, res=p["res"], res2=p["res2"]).numpy()
    return p


def explain_gemm(p, got, ref):
    bad = np.argwhere(got != ref)
    if bad.size == 0:
        return ""
    i = tuple(int(v) for v in bad[0])
    return (f"gemm m{p['m']} n{p['n']} k{p['k']}: {len(bad)} of {got.size} outputs differ; first at (batch, m, n) = {i}: got {got[i]!r}, reference "
            f"{ref[i]!r}, difference {(float(got[i]) - float(ref[i])) / p['q']:+.3g} q (q = 2^{int(np.log2(p['q']))})")


# ---- fused MLP ---------------------------------------------------------------------------------------------------------------------------
def mlp_problem(m, units=256, seed=0):
    """dm3d_mlp_fused operands: x fine (lo live in the first product), W0 [4u, u] with 4 and W1 [u, 4u] with 8 non-zeros per row from
    {+-1}, biases and residuals multiples of 2^-4 (|b0| <= 1/2).  The hidden activation relu(W0 x + b0) is then a multiple of 2^-12
    below 4.5 — 15 bits, its own re-split exact and its lo half live in the second product (non-zero on a third of the positive entries).  Returns the operands, the float64 result,
    q = 2^-12 and the worst sum|terms| / q of either layer."""
    rng = np.random.default_rng([seed, m, units])
    x = fine(rng, m, units)
    w0, w1 = np.zeros((4 * units, units), np.float32), np.zeros((units, 4 * units), np.float32)
    for j in range(4 * units):
        w0[j, (j + units // 4 * np.arange(4) + 7 * (j // units)) % units] = rng.choice([-1.0, 1.0], size=4)
    for j in range(units):
        w1[j, (j + units // 2 * np.arange(8)) % (4 * units)] = rng.choice([-1.0, 1.0], size=8)
    assert ((w0 != 0).sum(1) == 4).all() and ((w1 != 0).sum(1) == 8).all() and (w0 != 0).any(0).all() and (w1 != 0).any(0).all()
    p = dict(m=m, x=x, w0=w0, w1=w1, b0=sixteenths(rng, 4 * units, bound=0.5), b1=sixteenths(rng, units), r1=sixteenths(rng, m, units),
             r2=sixteenths(rng, m, units), w2=np.zeros((units, units), np.float32), b2=np.zeros(units, np.float32))
    hid = np.maximum(x.astype(np.float64) @ w0.astype(np.float64).T + p["b0"], 0.0)
    p["hidden_lo_share"] = lo_share(hid[hid > 0])
    assert lo_share(x) >= 0.9 and p["hidden_lo_share"] >= 0.25, "the hidden activation carries no lo part"
    assert_lossless("mlp x", x), assert_lossless("mlp hidden", hid)
    assert np.array_equal(hid.astype(np.float32).astype(np.float64), hid)
    p["q"] = quantum(x)
    t0 = np.abs(x).astype(np.float64) @ np.abs(w0).astype(np.float64).T + np.abs(p["b0"])
    t1 = hid @ np.abs(w1).astype(np.float64).T + np.abs(p["b1"]) + np.abs(p["r1"]) + np.abs(p["r2"])
    p["ratio"] = float(max(t0.max(), t1.max())) / p["q"]
    assert p["q"] == 2.0 ** -12 and p["ratio"] < BUDGET
    p["hidden"] = hid
    p["ref"] = rk.mlp_fused(x, w0, p["b0"], w1, p["b1"], p["r1"], p["r2"]).numpy()
    return p


def mlp_contract(p, perm=None, drop=None):
    """The fused MLP on the host model: both layers by `h3_contract` (one 'tap' of 4u or u channels), the hidden activation re-split."""
    u = p["w0"].shape[1]
    hid = np.maximum(h3_contract(p["x"], np.ascontiguousarray(p["w0"].T), u, perm, drop) + p["b0"], np.float32(0))
    y = h3_contract(hid, np.ascontiguousarray(p["w1"].T), 4 * u, perm)
    return ((y + p["b1"]) + p["r1"]) + p["r2"], hid

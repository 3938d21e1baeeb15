"""GPU parity of the inference entries of the C ABI, one kernel at a time, called through ctypes as a host would, with EVERY device buffer
inside guard bands (tests/guarded_buffers.py) and compared with the float64 restatements of oracle/ref_kernels.py / oracle/ref_torch.py.

What the guard bands see.  Outputs, in-place buffers and scratch sit between 4096 sentinel words, and the gaps of a leading dimension
larger than its matrix hold the same word: a store outside the payload fails `get()`.  Inputs sit between 4096 words 0x7fc07fc0 (a NaN as
float32 and as either float16 half), gaps included: a read outside the payload THAT REACHES A RESULT makes the result non-finite, and every
test asserts finiteness before it measures the error; inputs are also asserted unwritten.  A stray read whose value is masked afterwards
still breaks the ABI but cannot be seen this way.

Entries and forms covered
  dm3d_conv3d_ndhwc   16x16x32 kernel (conv3d_igemm_h3v3): 4- and 8-slice bricks; column forms NCT 4 / 2 / 1 (cout 64 / 32 / 8); epilogue
                      branches full brick 16-byte, full brick scalar (PReLU), partial brick (6x5x7, cout 40); dual input; per-sample
                      prologue vectors; DM3D_FMT_H2 output with post_*; DM3D_FMT_H2 input; fused skip conv (skip_wpk; skip_wpk_frag behind
                      the Winograd-x form); Cin split through split_counters + scratch (tickets zero afterwards).  Winograd-x form: Cin 32,
                      48, two-way Cin split, skip tail.  TAP-layout kernel: k3 stride 2 on 5x6x8, k1 (full and partial bricks), k4 stride 2.
                      Parity forms: upsample, transpose 4^3 -> 8^3 and 3x5x4.  float32 kernel: plain, ragged, stride 2.
                      Every case first asserts dm3d_conv_tile_form() / dm3d_conv_weight_layout() name the form it is listed for.
  packers             dm3d_pack_weights (zero padding and contents exact), _h3, _h3p (modes 0, 1 and 2), _up, _up_h3, _convt, _convt_h3, _h3w,
                      _skip_h3p, _skip_h3f, each at ragged channel counts from cin {4, 20, 48} x cout {8, 40, 72}; dm3d_pack_mlp_weights,
                      dm3d_pack_front_weights.  Each writes into a guarded buffer of exactly the queried size that starts out full of the
                      poison word, is read back (pads intact) and handed to the conv / MLP / front launch as a poisoned-pad input: padding
                      the header calls zero and a packer left unwritten makes that launch's result non-finite.  Not seen this way: the
                      padding of output channels past cout, whose products are never stored.
  dm3d_gemm_tn        F32, and H3 with every a_fmt / b_fmt / out_fmt; lda, ldb, ldo, ldr larger than the matrices; bias along n / m; res,
                      res2; each act; alpha; stride_b = 0.   dm3d_gemm_tn_group: 1-4 problems of different m, n, k, batch, each against
                      float64 and bitwise against the same descriptor issued alone.
  dm3d_attention      three-launch form (lq 64, lk 48; broadcast keys; scratch guarded) and fused form (c 256, lq 128, lk 32 / 96,
                      scratch NULL);  dm3d_attention_group: self + broadcast cross pass, fused and fallback, bitwise against single calls.
  dm3d_mlp_fused, dm3d_attn_front; dm3d_layernorm3[_h2], dm3d_softmax_rows[_h2], dm3d_affine_act, dm3d_split_h2, dm3d_vq_assign,
  dm3d_gather_rows, dm3d_randn, dm3d_range_check, dm3d_ddpm_update (clamped t, seed_dev, all seven tables poisoned around).  The N(0,1)
  stream dm3d_randn and dm3d_ddpm_update draw is held to a host reference element by element in tests/test_gpu_philox.py, not here.
  The range guard (range_flag / range_limit), guard site by guard site (every DM3D_AMAX of the sources has a plant case that reaches it,
  the Winograd-x form's ragged-cout branch and both GEMM tile forms included): plant -> 1 (some plants negative), control -> exactly 0,
  limit 0 means 65504, and the lanes a partial tile masks must not speak.

Not reached at a small shape: the Winograd-x and 8-slice forms' own launch thresholds (512 workgroups) — the per-call knobs
DM3D_CONV_WIDE_WGS / DM3D_CONV_WINO_MINCHUNKS / DM3D_CONV_WINO_SPLIT_MINCHUNKS admit the small grids, as in test_gpu_wino.py; the
128 x 128 tile form of the H3 GEMM (taken from 256 tiles of that size up) runs under the per-call knob DM3D_GEMM_MR=2, and no query names
the tile form a GEMM launch took, so those cases rest on the knob; the grouped GEMM and the attention entries run the 64 x 64 form only.
Without a plant case of their own: PReLU on a partial brick and PReLU behind the Winograd-x form (other instantiations of branches that
have one).  Not covered: dm3d_conv_desc.gn_stats (normalisation statistics: tests/test_gpu_round4.py); the logit axis of the attention and
softmax entries (constructed score rows, the fused kernel's lazy running maximum, the float16 floor of the probabilities:
tests/test_gpu_attention_logits.py).

Tolerances (max |err| / max |ref|), the project's: contractions 2e-5, row kernels 3e-6, elementwise 1e-6, data movement bitwise.
The worst error per entry is printed at the end of the module (docs/EXPERIMENTS.md records a run)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from guarded_buffers import IN, OUT, POISON_WORD, Guarded, h2_decode, h2_encode
from oracle import ref_kernels as rk
from oracle import ref_torch as rt

pytestmark = pytest.mark.gpu

LAYER_TOL, ROW_TOL, ELEM_TOL = 2e-5, 3e-6, 1e-6
NONE, RELU, SILU = 0, 1, 2
F32, H3 = 0, 1
FF32, FH2 = 0, 1
WORST = {}
CONV_KNOBS = ("DM3D_CONV_WIDE_WGS", "DM3D_CONV_WINO_MINCHUNKS", "DM3D_CONV_WINO", "DM3D_CONV_V3_TD", "DM3D_CONV_WINO_SPLIT_MINCHUNKS",
              "DM3D_CONV_WINO_GRID")


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    yield torch.device("cuda:0")
    for name in sorted(WORST):
        print(f"worst error {name}: {WORST[name]:.2e}")


@pytest.fixture()
def rng(request):
    return np.random.default_rng(sum(map(ord, request.node.name)))


def _lib_():
    from dm3d_amd import _lib
    return _lib


def _call(name, *args):
    lib = _lib_()
    lib.check(getattr(lib.lib(), name)(*args, None), name)


def _err(name, got, ref, scale=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output (a read outside an operand's extent?)"
    e = float(np.abs(got - ref).max() / max(float(np.abs(ref).max()) if scale is None else scale, 1e-30))
    WORST[name] = max(WORST.get(name, 0.0), e)
    print(f"{name}: {e:.2e}")
    return e


def _f32(rng, *shape, mean=0.0, std=1.0):
    return (rng.standard_normal(shape) * std + mean).astype(np.float32)


def _gin(dev, arr):
    return Guarded(arr, dev, IN)


def _gout(dev, arr):
    return Guarded(arr, dev, OUT)


def _exp_for(*wmax):
    """The power of two that brings the largest weight into [2^13, 2^14) (ops.h3_weight_exponent)."""
    m = max(float(w) for w in wmax)
    return int(13 - np.floor(np.log2(m)))


# ======================================================================================================================================
# 1. Conv3D
# ======================================================================================================================================
def _case(name, form, layout, B=1, dims=(8, 8, 8), c1=32, c2=0, cout=64, ks=3, stride=1, prec=H3, **kw):
    d = dict(name=name, form=form, layout=layout, B=B, dims=dims, c1=c1, c2=c2, cout=cout, ks=ks, stride=stride, prec=prec, up=False, tr=False,
             bias=True, vec=True, pro="batch", res=True, relu=True, prelu=False, skip=None, x_h2=False, out_h2=False, post=False, wino=False,
             split=False, env={}, in_scale=False, h3p_direct=False)
    d.update(kw)
    return d


WIDE = {"DM3D_CONV_WIDE_WGS": "1"}
SMALL_GRIDS = {"DM3D_CONV_WIDE_WGS": "1", "DM3D_CONV_WINO_MINCHUNKS": "1"}
PAIR, TAP = 1, 0

CONV_CASES = [
    _case("v3 td4 nct4 full 16B", 4, PAIR, B=2),
    _case("v3 td8 nct4 full 16B", 8, PAIR, B=2, env=WIDE),
    _case("v3 td4 nct2 cout32", 4, PAIR, cout=32),
    _case("v3 td4 nct1 cout8", 4, PAIR, cout=8),
    _case("v3 td4 full scalar (PReLU)", 4, PAIR, prelu=True),
    _case("v3 td8 full scalar (PReLU)", 8, PAIR, prelu=True, env=WIDE),
    _case("v3 td4 partial 6x5x7 cout40", 4, PAIR, B=2, dims=(6, 5, 7), c1=20, cout=40),
    _case("v3 td8 partial 6x5x7 cout40", 8, PAIR, dims=(6, 5, 7), c1=20, cout=40, env=WIDE),
    _case("v3 dual input 16+12", 4, PAIR, c1=16, c2=12),
    _case("v3 per-sample prologue", 4, PAIR, B=2, c1=16, c2=12, pro="sample"),
    _case("v3 td4 H2 out + post", 4, PAIR, B=2, out_h2=True, post=True),
    _case("v3 td8 H2 out + post", 8, PAIR, out_h2=True, post=True, env=WIDE),
    _case("v3 post, float32 out", 4, PAIR, post=True),
    _case("v3 H2 in", 4, PAIR, x_h2=True, pro=None),
    _case("v3 fused skip (skip_wpk)", 4, PAIR, skip=("lds", 16, 12), relu=False),
    _case("v3 Cin split", 4, PAIR, c1=64, split=True),
    _case("wino Cin32", 10, PAIR, wino=True, env=SMALL_GRIDS),
    _case("wino Cin48 B2", 10, PAIR, B=2, c1=48, wino=True, env=SMALL_GRIDS),
    _case("wino two-way Cin split", 10, PAIR, c1=64, wino=True, split=True, env=dict(SMALL_GRIDS, DM3D_CONV_WINO_SPLIT_MINCHUNKS="4")),
    _case("wino skip tail (skip_wpk_frag)", 10, PAIR, wino=True, skip=("frag", 40, 0), relu=False, env=SMALL_GRIDS),
    _case("wino H2 out + post", 10, PAIR, wino=True, out_h2=True, post=True, env=SMALL_GRIDS),
    _case("tap k3 s2 5x6x8", 0, TAP, B=2, dims=(5, 6, 8), c1=20, cout=40, stride=2),
    _case("tap k1 full brick", 0, TAP, dims=(4, 8, 8), c1=20, cout=64, ks=1),
    _case("tap k1 partial 5x6x7", 0, TAP, B=2, dims=(5, 6, 7), c1=20, cout=40, ks=1, in_scale=True),
    _case("tap k4 s2 6x8x4", 0, TAP, dims=(6, 8, 4), c1=8, cout=24, ks=4, stride=2),
    _case("parity upsample 4^3", 4, PAIR, dims=(4, 4, 4), c1=16, up=True),
    _case("parity transpose 4^3", 4, PAIR, dims=(4, 4, 4), c1=16, cout=24, ks=4, stride=2, tr=True),
    _case("parity transpose 3x5x4", 4, PAIR, B=2, dims=(3, 5, 4), c1=16, cout=24, ks=4, stride=2, tr=True),
    _case("f32 plain", 0, None, c1=16, prec=F32),
    _case("f32 ragged 6x5x7", 0, None, B=2, dims=(6, 5, 7), c1=20, cout=40, prec=F32, in_scale=True),
    _case("f32 stride 2 5x6x8", 0, None, dims=(5, 6, 8), c1=20, cout=40, stride=2, prec=F32),
    _case("f32 upsample", 0, None, dims=(3, 4, 5), c1=8, cout=24, up=True, prec=F32),
    _case("f32 transpose", 0, None, dims=(3, 4, 5), c1=8, cout=24, ks=4, stride=2, tr=True, prec=F32),
]
# packers over ragged channel counts, one conv each (in_scale where the entry takes it)
CONV_CASES += [_case(f"pack h3p {ci}->{co}", 4, PAIR, dims=(4, 8, 8), c1=ci, cout=co, in_scale=True) for ci, co in ((4, 8), (20, 40), (48, 72))]
CONV_CASES += [_case(f"pack h3 k1 {ci}->{co}", 0, TAP, dims=(4, 8, 8), c1=ci, cout=co, ks=1, in_scale=True) for ci, co in ((4, 72), (48, 8))]
CONV_CASES += [_case(f"pack h3w {ci}->{co}", 10, PAIR, c1=ci, cout=co, wino=True, in_scale=True, env=SMALL_GRIDS) for ci, co in ((20, 40), (48, 72))]
CONV_CASES += [
    _case("pack up_h3 20->40", 4, PAIR, dims=(3, 4, 5), c1=20, cout=40, up=True),
    _case("pack h3p mode 1 48->8", 4, PAIR, dims=(3, 4, 5), c1=48, cout=8, up=True, h3p_direct=True),
    _case("pack convt_h3 4->72", 4, PAIR, dims=(3, 4, 5), c1=4, cout=72, ks=4, stride=2, tr=True),
    _case("pack h3p mode 2 20->40", 4, PAIR, dims=(3, 4, 5), c1=20, cout=40, ks=4, stride=2, tr=True, h3p_direct=True),
    _case("pack up 20->40", 0, None, dims=(3, 4, 5), c1=20, cout=40, up=True, prec=F32),
    _case("pack up 48->8", 0, None, dims=(3, 4, 5), c1=48, cout=8, up=True, prec=F32),
    _case("pack convt 4->72", 0, None, dims=(3, 4, 5), c1=4, cout=72, ks=4, stride=2, tr=True, prec=F32),
    _case("pack convt 20->40", 0, None, dims=(3, 4, 5), c1=20, cout=40, ks=4, stride=2, tr=True, prec=F32),
    _case("pack skip_h3p 20->40", 4, PAIR, dims=(4, 8, 8), cout=40, skip=("lds", 20, 0), relu=False),
    _case("pack skip_h3p 4->72", 4, PAIR, dims=(4, 8, 8), cout=72, skip=("lds", 4, 0), relu=False),
    _case("pack skip_h3f 48->40", 10, PAIR, cout=40, wino=True, skip=("frag", 48, 0), relu=False, env=SMALL_GRIDS),
    _case("pack skip_h3f 20->72", 10, PAIR, cout=72, wino=True, skip=("frag", 20, 0), relu=False, env=SMALL_GRIDS),
]
CONV_BY_NAME = {c["name"]: c for c in CONV_CASES}
assert len(CONV_BY_NAME) == len(CONV_CASES)


def _out_dims(s):
    D, H, W = s["dims"]
    if s["up"] or s["tr"]:
        return 2 * D, 2 * H, 2 * W
    return tuple(-(-n // s["stride"]) for n in (D, H, W))


def _conv_host(s, rng):
    """The operands of a case as numpy arrays, and its float64 result without the residual and the consumer's post step."""
    B, cin, cout = s["B"], s["c1"] + s["c2"], s["cout"]
    od = _out_dims(s)
    h = {}
    x1 = _f32(rng, B, *s["dims"], s["c1"])
    if s["x_h2"]:
        h["x1_words"] = h2_encode(x1)
        x1 = h2_decode(h["x1_words"])                         # the values the buffer holds
    h["x1"] = x1
    h["x2"] = _f32(rng, B, *s["dims"], s["c2"]) if s["c2"] else None
    taps = s["ks"] ** 3
    kshape = (4, 4, 4, cout, cin) if s["tr"] else (s["ks"],) * 3 + (cin, cout)
    h["kernel"] = _f32(rng, *kshape, std=1.0 / np.sqrt(taps * cin / (8.0 if s["up"] else 1.0)))
    h["in_scale"] = (rng.random(cin) + 0.5).astype(np.float32) if s["in_scale"] else None
    h["bias"] = _f32(rng, cout) if s["bias"] else None
    if s["vec"]:
        h["vec"] = _f32(rng, B + 2, cout)                     # [rows, vec_ld] with vec_ld = cout + 8: the gap is poison
        h["vec_idx"] = ((np.arange(B) * 2 + 1) % (B + 2)).astype(np.int32)
    else:
        h["vec"] = h["vec_idx"] = None
    if s["pro"]:
        shape = (B, cin) if s["pro"] == "sample" else (cin,)
        h["pro"] = ((rng.random(shape) + 0.5).astype(np.float32), _f32(rng, *shape, std=0.2))
    else:
        h["pro"] = None
    h["prelu"] = (rng.random(od + (cout,)) * 0.5).astype(np.float32) if s["prelu"] else None
    if s["skip"]:
        _, sc1, sc2 = s["skip"]
        h["skip_x1"], h["skip_x2"] = _f32(rng, B, *s["dims"], sc1), (_f32(rng, B, *s["dims"], sc2) if sc2 else None)
        h["skip_k"] = _f32(rng, sc1 + sc2, cout, std=0.2)
    h["post"] = ((rng.random(cout) + 0.5).astype(np.float32), _f32(rng, cout, std=0.2)) if s["post"] else None
    h["res"] = _f32(rng, B, *od, cout) if s["res"] else None
    k64 = rk.f64(h["kernel"])
    if h["in_scale"] is not None:
        k64 = k64 * rk.f64(h["in_scale"])[:, None]
    skip = None
    if s["skip"]:
        sx = h["skip_x1"] if h["skip_x2"] is None else np.concatenate([h["skip_x1"], h["skip_x2"]], -1)
        skip = (sx, h["skip_k"])
    h["base"] = rk.conv3d_fused(h["x1"], k64, x2=h["x2"], ksize=s["ks"], stride=s["stride"], upsample=s["up"], transpose=s["tr"], bias=h["bias"],
                                pro=h["pro"], vec=h["vec"], vec_idx=h["vec_idx"], relu=s["relu"], prelu_alpha=h["prelu"], skip=skip).numpy()
    return h


def _conv_finish(h, res):
    """base + res, then the consumer's norm + SiLU: what the launch stores."""
    y = h["base"] if res is None else h["base"] + res.astype(np.float64)
    if h["post"] is not None:
        y = rt._swish(torch.from_numpy(y * h["post"][0].astype(np.float64) + h["post"][1].astype(np.float64))).numpy()
    return y


_CONV_HOSTS = {}


def _conv_host_cached(s):
    if s["name"] not in _CONV_HOSTS:
        _CONV_HOSTS[s["name"]] = _conv_host(s, np.random.default_rng(sum(map(ord, s["name"]))))
    return _CONV_HOSTS[s["name"]]


def _pack(dev, entry, nbytes, *args_before, args_after=()):
    """Runs a packer into a guarded buffer of exactly nbytes, checks the pads, and returns the image re-uploaded as an input."""
    assert nbytes > 0 and nbytes % 4 == 0
    # prefilled with the poison word (a float16 NaN in either half): padding the header calls zero that a packer left unwritten reaches the
    # launch that reads the image — a padded input channel or tap multiplies into every output — and makes its result non-finite
    img = _gout(dev, np.full(nbytes // 4, POISON_WORD, np.uint32))
    _call(entry, *args_before, img.ptr, *args_after)
    return _gin(dev, img.get())


def _conv_weights(dev, s, h):
    """Every weight image the case needs, each packed into a buffer of exactly the size its query returns."""
    lib = _lib_().lib()
    cin, cout, taps = s["c1"] + s["c2"], s["cout"], s["ks"] ** 3
    k = _gin(dev, h["kernel"])
    sc = _gin(dev, h["in_scale"]) if h["in_scale"] is not None else None
    scp = sc.ptr if sc else None
    w = {"w_exp": 0, "keep": [k, sc]}
    parity = s["up"] or s["tr"]
    if s["prec"] == F32:
        if parity:
            w["wpk"] = _pack(dev, "dm3d_pack_weights_up" if s["up"] else "dm3d_pack_weights_convt", 4 * lib.dm3d_packed_weight_up_elems(cin, cout), k.ptr, cin, cout)
        else:
            w["wpk"] = _pack(dev, "dm3d_pack_weights", 4 * lib.dm3d_packed_weight_elems(taps, cin, cout), k.ptr, taps, cin, cout, scp)
    else:
        wmax = float(np.abs(h["kernel"]).max()) * (float(h["in_scale"].max()) if sc else 1.0) * (8.0 if s["up"] else 1.0)
        if s["skip"]:
            wmax = max(wmax, float(np.abs(h["skip_k"]).max()))
        e = w["w_exp"] = _exp_for(wmax)
        if parity and s["h3p_direct"]:                       # dm3d_pack_weights_h3p modes 1 / 2: eight parity images of eight taps
            nb = 8 * lib.dm3d_packed_weight_h3p_bytes(8, cin, cout)
            assert nb == lib.dm3d_packed_weight_up_h3_bytes(cin, cout)
            w["wpk"] = _pack(dev, "dm3d_pack_weights_h3p", nb, k.ptr, 8, cin, cout, e, None, args_after=(1 if s["up"] else 2,))
        elif parity:
            w["wpk"] = _pack(dev, "dm3d_pack_weights_up_h3" if s["up"] else "dm3d_pack_weights_convt_h3", lib.dm3d_packed_weight_up_h3_bytes(cin, cout),
                             k.ptr, cin, cout, e)
        elif s["layout"] == PAIR:
            w["wpk"] = _pack(dev, "dm3d_pack_weights_h3p", lib.dm3d_packed_weight_h3p_bytes(taps, cin, cout), k.ptr, taps, cin, cout, e, scp, args_after=(0,))
        else:
            w["wpk"] = _pack(dev, "dm3d_pack_weights_h3", lib.dm3d_packed_weight_h3_bytes(taps, cin, cout), k.ptr, taps, cin, cout, e, scp)
        if s["wino"]:
            w["wino"] = _pack(dev, "dm3d_pack_weights_h3w", lib.dm3d_packed_weight_h3w_bytes(cin, cout), k.ptr, cin, cout, e, scp)
        if s["skip"]:
            sk = _gin(dev, h["skip_k"])
            sc_in = s["skip"][1] + s["skip"][2]
            nb = lib.dm3d_packed_weight_skip_h3p_bytes(sc_in, cout)
            w["skip"] = _pack(dev, "dm3d_pack_weights_skip_h3p", nb, sk.ptr, sc_in, cout, e)
            if s["skip"][0] == "frag":
                w["skip_frag"] = _pack(dev, "dm3d_pack_weights_skip_h3f", nb, sk.ptr, sc_in, cout, e)
            w["keep"].append(sk)
    return w


def _conv_launch(dev, monkeypatch, s, h, res, limit=None):
    """One guarded launch of a case with the residual `res`; returns (stored values as float64, range flag or None)."""
    lib = _lib_()
    for v in CONV_KNOBS:
        monkeypatch.delenv(v, raising=False)
    for key, val in s["env"].items():
        monkeypatch.setenv(key, val)
    B, cout = s["B"], s["cout"]
    od = _out_dims(s)
    w = _conv_weights(dev, s, h)
    ins = {"x1": _gin(dev, h["x1_words"] if s["x_h2"] else h["x1"])}
    d = lib.ConvDesc()
    d.x1, d.c1, d.c2, d.batch = ins["x1"].ptr, s["c1"], s["c2"], B
    if s["c2"]:
        ins["x2"] = _gin(dev, h["x2"])
        d.x2 = ins["x2"].ptr
    d.in_d, d.in_h, d.in_w = s["dims"]
    d.upsample, d.ksize, d.stride, d.transpose = int(s["up"]), s["ks"], s["stride"], int(s["tr"])
    d.wpk, d.cout, d.precision, d.w_exp = w["wpk"].ptr, cout, s["prec"], w["w_exp"]
    if s["prec"] == H3:
        d.w_layout = lib.lib().dm3d_conv_weight_layout(s["ks"], s["stride"], int(s["up"]), int(s["tr"]), cout)
        assert d.w_layout == s["layout"], f"{s['name']}: weight layout {d.w_layout}"
    if h["bias"] is not None:
        ins["bias"] = _gin(dev, h["bias"])
        d.bias = ins["bias"].ptr
    if h["vec"] is not None:
        ins["vec"] = Guarded.matrix(h["vec"], cout + 8, dev, IN)
        ins["vec_idx"] = _gin(dev, h["vec_idx"])
        d.vec, d.vec_idx, d.vec_ld = ins["vec"].ptr, ins["vec_idx"].ptr, cout + 8
    if h["pro"] is not None:
        ins["ps"], ins["pt"] = _gin(dev, h["pro"][0]), _gin(dev, h["pro"][1])
        d.pro_scale, d.pro_shift = ins["ps"].ptr, ins["pt"].ptr
        d.pro_batch_stride = s["c1"] + s["c2"] if s["pro"] == "sample" else 0
    d.relu = int(s["relu"])
    if h["prelu"] is not None:
        ins["prelu"] = _gin(dev, h["prelu"])
        d.prelu_alpha = ins["prelu"].ptr
    if res is not None:
        ins["res"] = _gin(dev, res)
        d.res = ins["res"].ptr
    if s["skip"]:
        ins["sx1"] = _gin(dev, h["skip_x1"])
        d.skip_x1, d.skip_c1, d.skip_c2, d.skip_wpk = ins["sx1"].ptr, s["skip"][1], s["skip"][2], w["skip"].ptr
        if s["skip"][2]:
            ins["sx2"] = _gin(dev, h["skip_x2"])
            d.skip_x2 = ins["sx2"].ptr
        if "skip_frag" in w:
            d.skip_wpk_frag = w["skip_frag"].ptr
    if s["x_h2"]:
        d.x1_fmt = FH2
    if s["out_h2"]:
        d.out_fmt = FH2
    if h["post"] is not None:
        ins["qs"], ins["qt"] = _gin(dev, h["post"][0]), _gin(dev, h["post"][1])
        d.post_scale, d.post_shift = ins["qs"].ptr, ins["qt"].ptr
    if s["wino"]:
        d.wpk_wino = w["wino"].ptr
    out = _gout(dev, np.zeros((B,) + od + (cout,), np.float32))
    d.out = out.ptr
    scratch = counters = None
    if s["split"]:
        probe = _gout(dev, np.zeros(4, np.int32))
        d.split_counters, d.split_counter_words = probe.ptr, 1 << 20     # (the queries answer for a descriptor that provides tickets)
        need, words = lib.lib().dm3d_conv_scratch_bytes(C.byref(d)), lib.lib().dm3d_conv_split_counter_words(C.byref(d))
        assert need > 0 and words > 0, f"{s['name']}: the descriptor does not split"
        scratch, counters = _gout(dev, np.full(need // 4, 7.0, np.float32)), _gout(dev, np.zeros(words, np.int32))
        d.scratch, d.scratch_bytes, d.split_counters, d.split_counter_words = scratch.ptr, need, counters.ptr, words
    flag = None
    if limit is not None:
        flag = _gout(dev, np.zeros(1, np.int32))
        d.range_flag, d.range_limit = flag.ptr, limit
    form = lib.lib().dm3d_conv_tile_form(C.byref(d))
    assert form == s["form"], f"{s['name']}: resolves to tile form {form}, listed for {s['form']}"
    lib.check(lib.lib().dm3d_conv3d_ndhwc(C.byref(d), None), "conv3d")
    got = out.get()
    got = h2_decode(got.reshape(-1, cout)).reshape(got.shape) if s["out_h2"] else got.astype(np.float64)
    if s["split"]:
        # (the queries answer for every form the geometry could take: that THIS launch split shows in the parts' accumulator tiles)
        assert (scratch.get() != 7.0).any(), f"{s['name']}: the launch did not split (scratch was not written)"
        assert not counters.get().any(), "split_counters must be zero after the launch"
    for b in list(ins.values()) + [w[k] for k in ("wpk", "wino", "skip", "skip_frag") if k in w]:
        b.unchanged()
    return got, (None if flag is None else int(flag.get()[0]))


@pytest.mark.parametrize("name", [c["name"] for c in CONV_CASES])
def test_conv3d(dev, monkeypatch, name):
    s = CONV_BY_NAME[name]
    h = _conv_host_cached(s)
    got, _ = _conv_launch(dev, monkeypatch, s, h, h["res"])
    key = "dm3d_conv3d_ndhwc " + ("f32" if s["prec"] == F32 else {0: "h3 TAP kernel", 4: "h3 16x16x32", 8: "h3 16x16x32", 10: "h3 Winograd-x"}[s["form"]])
    assert _err(key, got, _conv_finish(h, h["res"])) < LAYER_TOL


def test_pack_weights_zero_padding_and_contents(dev, rng):
    """dm3d_pack_weights: [taps][CoutPad][CinPad], K contiguous per output channel, zero padded, rows scaled by in_scale."""
    lib = _lib_().lib()
    for taps, cin, cout in ((27, 4, 8), (1, 20, 40), (8, 48, 72)):
        k, sc = _f32(rng, taps, cin, cout), (rng.random(cin) + 0.5).astype(np.float32)
        n = lib.dm3d_packed_weight_elems(taps, cin, cout)
        cip, cop = -(-cin // 16) * 16, -(-cout // 64) * 64
        assert n == taps * cip * cop
        bk, bs, img = _gin(dev, k), _gin(dev, sc), _gout(dev, np.full(n, 7.0, np.float32))
        _call("dm3d_pack_weights", bk.ptr, taps, cin, cout, bs.ptr, img.ptr)
        exp = np.zeros((taps, cop, cip), np.float32)
        exp[:, :cout, :cin] = (k * sc[None, :, None]).transpose(0, 2, 1)
        assert np.array_equal(img.get().reshape(taps, cop, cip), exp)
        bk.unchanged(), bs.unchanged()
    WORST.setdefault("dm3d_pack_weights (bitwise)", 0.0)


# ======================================================================================================================================
# 2. GEMM
# ======================================================================================================================================
def _gemm_problem(rng, m, n, k, batch, af, bf, of, prec, bias, res, act, alpha, bcast_b):
    """Host operands (values as the buffers hold them) and the float64 result of one descriptor."""
    a, b = _f32(rng, batch, m, k), _f32(rng, 1 if bcast_b else batch, n, k)
    p = dict(m=m, n=n, k=k, batch=batch, af=af, bf=bf, of=of, prec=prec, act=act, alpha=alpha, bcast_b=bcast_b, bias_m=bias == "m")
    p["a_words"], p["b_words"] = (h2_encode(a) if af else a), (h2_encode(b) if bf else b)
    if af:
        a = h2_decode(p["a_words"])
    if bf:
        b = h2_decode(p["b_words"])
    p["a"], p["b"] = a, b
    p["bias"] = _f32(rng, m if bias == "m" else n) if bias else None
    p["res"] = _f32(rng, batch, m, n) if res >= 1 else None
    p["res2"] = _f32(rng, batch, m, n) if res >= 2 else None
    return p


def _gemm_ref(p):
    return rk.gemm_tn(p["a"], p["b"], alpha=p["alpha"], bias=p["bias"], bias_along_m=p["bias_m"], kind=p["act"], res=p["res"], res2=p["res2"]).numpy()


def _gemm_desc(dev, p, limit=None):
    """A descriptor over freshly uploaded guarded buffers, every leading dimension strictly larger than its matrix."""
    lib = _lib_()
    m, n, k = p["m"], p["n"], p["k"]
    lda, ldb, ldr = k + 16, k + 32, n + 4
    ldo = n + 16 if p["of"] else n + 3
    bufs = dict(a=Guarded.matrix(p["a_words"], lda, dev, IN), b=Guarded.matrix(p["b_words"], ldb, dev, IN),
                out=Guarded.matrix(np.zeros((p["batch"], m, n), np.float32), ldo, dev, OUT))
    d = lib.GemmDesc()
    d.a, d.lda, d.stride_a = bufs["a"].ptr, lda, m * lda
    d.b, d.ldb, d.stride_b = bufs["b"].ptr, ldb, 0 if p["bcast_b"] else n * ldb
    d.out, d.ldo, d.stride_o = bufs["out"].ptr, ldo, m * ldo
    d.m, d.n, d.k, d.batch, d.alpha, d.act = m, n, k, p["batch"], p["alpha"], p["act"]
    if p["bias"] is not None:
        bufs["bias"] = _gin(dev, p["bias"])
        d.bias, d.bias_along_m = bufs["bias"].ptr, int(p["bias_m"])
    if p["res"] is not None:
        bufs["res"] = Guarded.matrix(p["res"], ldr, dev, IN)
        d.res, d.ldr, d.stride_r = bufs["res"].ptr, ldr, m * ldr
    if p["res2"] is not None:
        bufs["res2"] = Guarded.matrix(p["res2"], ldr, dev, IN)
        d.res2 = bufs["res2"].ptr
    d.precision, d.a_fmt, d.b_fmt, d.out_fmt = p["prec"], p["af"], p["bf"], p["of"]
    if limit is not None:
        bufs["flag"] = _gout(dev, np.zeros(1, np.int32))
        d.range_flag, d.range_limit = bufs["flag"].ptr, limit
    return d, bufs


def _gemm_result(p, bufs):
    """The stored matrix (raw words and float64 values), after the guards were checked."""
    raw = bufs["out"].get()[..., :p["n"]]
    for key in ("a", "b", "bias", "res", "res2"):
        if key in bufs:
            bufs[key].unchanged()
    return raw, (h2_decode(raw.reshape(-1, p["n"])).reshape(raw.shape) if p["of"] else raw.astype(np.float64))


def _gemm_cases():
    Ms, Ns, Ks = (1, 127, 129, 200), (16, 48, 144), (16, 48, 272)
    cases = []
    for i, (af, bf, of) in enumerate(itertools.product((FF32, FH2), repeat=3)):
        for j in range(3):
            v = i + j
            cases.append((Ms[(i + j) % 4], Ns[(i + 2 * j) % 3], Ks[(i // 2 + j) % 3], (1, 3, 2)[v % 3], af, bf, of, H3, (None, "n", "m")[v % 3], (v + j) % 3,
                          (v + 1) % 3, (1.0, 0.37)[v % 2], v % 3 == 1))
    for i, (m, n) in enumerate(itertools.product(Ms, (16, 48, 70, 144))):
        cases.append((m, n, Ks[i % 3], (1, 2)[i % 2], FF32, FF32, FF32, F32, (None, "n", "m")[i % 3], i % 3, (i + 2) % 3, (1.0, -1.5)[i % 2], i % 4 == 1))
    return cases


def _gemm_id(c):
    m, n, k, batch, af, bf, of, prec, bias, res, act, alpha, bc = c
    return f"{'h3' if prec else 'f32'}-m{m}n{n}k{k}b{batch}-a{af}b{bf}o{of}-bias{bias}-res{res}-act{act}-alpha{alpha}-bcast{int(bc)}"


@pytest.mark.parametrize("case", _gemm_cases(), ids=_gemm_id)
def test_gemm_tn(dev, rng, case):
    m, n, k, batch, af, bf, of, prec, bias, res, act, alpha, bc = case
    p = _gemm_problem(rng, m, n, k, batch, af, bf, of, prec, bias, res, act, alpha, bc and batch > 1)
    d, bufs = _gemm_desc(dev, p)
    lib = _lib_()
    lib.check(lib.lib().dm3d_gemm_tn(C.byref(d), None), "gemm_tn")
    _, got = _gemm_result(p, bufs)
    assert _err("dm3d_gemm_tn " + ("h3" if prec else "f32"), got, _gemm_ref(p)) < LAYER_TOL


@pytest.mark.parametrize("m,n,k,of", [(200, 144, 272, FF32), (129, 48, 16, FH2), (256, 128, 48, FF32)])
def test_gemm_tn_h3_128_tile_form(dev, rng, monkeypatch, m, n, k, of):
    """DM3D_GEMM_MR=2 (read per call) forces the 128 x 128 tile form, which a launch otherwise takes from 256 such tiles up."""
    monkeypatch.setenv("DM3D_GEMM_MR", "2")
    p = _gemm_problem(rng, m, n, k, 2, FH2, FF32, of, H3, "m", 2, SILU, 0.37, False)
    d, bufs = _gemm_desc(dev, p)
    lib = _lib_()
    lib.check(lib.lib().dm3d_gemm_tn(C.byref(d), None), "gemm_tn")
    assert _err("dm3d_gemm_tn h3 128x128 tiles", _gemm_result(p, bufs)[1], _gemm_ref(p)) < LAYER_TOL


GROUP_PROBLEMS = [(200, 16, 48, 2, "n", 1, RELU), (65, 48, 16, 1, "m", 2, NONE), (1, 1, 272, 3, None, 0, SILU), (129, 144, 32, 1, "n", 1, NONE)]


@pytest.mark.parametrize("fmt", [FF32, FH2], ids=["f32 operands", "H2 operands"])
@pytest.mark.parametrize("count", [1, 2, 3, 4])
def test_gemm_tn_group(dev, rng, count, fmt):
    """Problems of different m, n, k and batch in one launch: each against its own float64 product and bitwise against the same descriptor
    issued alone; every problem's output has guard bands of its own, so a block that lands in the wrong problem is caught."""
    lib = _lib_()
    probs = [_gemm_problem(rng, m, n, k, batch, fmt, fmt, FF32, H3, bias, res, act, 0.5 + i, False)
             for i, (m, n, k, batch, bias, res, act) in enumerate(GROUP_PROBLEMS[:count])]
    descs, bufs = zip(*(_gemm_desc(dev, p) for p in probs))
    arr = (lib.GemmDesc * count)(*descs)
    lib.check(lib.lib().dm3d_gemm_tn_group(arr, count, None), "gemm_tn_group")
    for p, b in zip(probs, bufs):
        raw, got = _gemm_result(p, b)
        assert _err("dm3d_gemm_tn_group", got, _gemm_ref(p)) < LAYER_TOL
        d1, b1 = _gemm_desc(dev, p)
        lib.check(lib.lib().dm3d_gemm_tn(C.byref(d1), None), "gemm_tn")
        assert np.array_equal(raw.view(np.int32), _gemm_result(p, b1)[0].view(np.int32)), "a grouped problem differs from the same descriptor issued alone"


# ======================================================================================================================================
# 3. Attention
# ======================================================================================================================================
def _attn_problem(rng, B, lq, lk, c, fmt, bcast, res=True):
    q, k, v = _f32(rng, B, lq, c, std=0.7), _f32(rng, 1 if bcast else B, lk, c, std=0.7), _f32(rng, 1 if bcast else B, lk, c)
    vt = np.ascontiguousarray(v.transpose(0, 2, 1))
    p = dict(B=B, lq=lq, lk=lk, c=c, fmt=fmt, bcast=bcast, scale=float(c) ** -0.5)
    p["qw"], p["kw"], p["vtw"] = (h2_encode(t) if fmt else t for t in (q, k, vt))
    if fmt:
        q, k, vt = h2_decode(p["qw"]), h2_decode(p["kw"]), h2_decode(p["vtw"])
    p["res"] = _f32(rng, B, lq, c) if res else None
    p["ref"] = rk.attention(q, k, np.asarray(vt).transpose(0, 2, 1), p["scale"], p["res"]).numpy()
    return p


def _attn_desc(dev, p, prec):
    lib = _lib_()
    c, lq, lk = p["c"], p["lq"], p["lk"]
    ldq, ldk, ldv, ldo = c + 16, c + 32, lk + 16, c + 8
    bufs = dict(q=Guarded.matrix(p["qw"], ldq, dev, IN), k=Guarded.matrix(p["kw"], ldk, dev, IN), vt=Guarded.matrix(p["vtw"], ldv, dev, IN),
                out=Guarded.matrix(np.zeros((p["B"], lq, c), np.float32), ldo, dev, OUT))
    d = lib.AttentionDesc()
    d.q, d.ldq = bufs["q"].ptr, ldq
    d.k, d.ldk, d.stride_k = bufs["k"].ptr, ldk, 0 if p["bcast"] else lk * ldk
    d.vt, d.ldv, d.stride_vt = bufs["vt"].ptr, ldv, 0 if p["bcast"] else c * ldv
    d.out, d.ldo = bufs["out"].ptr, ldo
    if p["res"] is not None:
        bufs["res"] = Guarded.matrix(p["res"], ldo, dev, IN)
        d.res = bufs["res"].ptr
    d.batch, d.lq, d.lk, d.c, d.scale, d.precision, d.fmt = p["B"], lq, lk, c, p["scale"], prec, p["fmt"]
    return d, bufs


def _attn_result(p, bufs):
    got = bufs["out"].get()[..., :p["c"]]
    for key in ("q", "k", "vt", "res"):
        if key in bufs:
            bufs[key].unchanged()
    return got


def _attn_scratch(dev, p):
    n = _lib_().lib().dm3d_attention_workspace_bytes(p["B"], p["lq"], p["lk"])
    assert n > 0
    return _gout(dev, np.zeros(n // 4, np.float32))


@pytest.mark.parametrize("prec,fmt", [(F32, FF32), (H3, FF32), (H3, FH2)], ids=["f32", "h3", "h3 H2 operands"])
@pytest.mark.parametrize("bcast", [False, True], ids=["own keys", "broadcast keys"])
def test_attention_three_launch_form(dev, rng, prec, fmt, bcast):
    lib = _lib_()
    p = _attn_problem(rng, 2, 64, 48, 32, fmt, bcast)
    d, bufs = _attn_desc(dev, p, prec)
    scratch = _attn_scratch(dev, p)
    lib.check(lib.lib().dm3d_attention(C.byref(d), scratch.ptr, None), "attention")
    assert _err("dm3d_attention three launches", _attn_result(p, bufs), p["ref"]) < LAYER_TOL
    scratch.get()


@pytest.mark.parametrize("lk", [32, 96])
@pytest.mark.parametrize("bcast", [False, True], ids=["own keys", "broadcast keys"])
def test_attention_fused_form(dev, rng, lk, bcast):
    lib = _lib_()
    p = _attn_problem(rng, 2, 128, lk, 256, FH2, bcast)
    d, bufs = _attn_desc(dev, p, H3)
    lib.check(lib.lib().dm3d_attention(C.byref(d), None, None), "attention")            # scratch NULL: only the fused form accepts it
    assert _err("dm3d_attention fused", _attn_result(p, bufs), p["ref"]) < LAYER_TOL


@pytest.mark.parametrize("form", ["fused", "fallback"])
def test_attention_group(dev, rng, form):
    """A self pass and a broadcast cross pass in one call, against float64 and bitwise against the two passes issued singly."""
    lib = _lib_()
    B, lq, lk, c = (2, 128, 32, 256) if form == "fused" else (2, 64, 48, 64)
    probs = [_attn_problem(rng, B, lq, lk, c, FH2, False), _attn_problem(rng, B, lq, lk, c, FH2, True)]
    descs, bufs = zip(*(_attn_desc(dev, p, H3) for p in probs))
    scratch = _attn_scratch(dev, probs[0])
    arr = (lib.AttentionDesc * 2)(*descs)
    lib.check(lib.lib().dm3d_attention_group(arr, 2, None if form == "fused" else scratch.ptr, None), "attention_group")
    scratch.get()
    for p, b in zip(probs, bufs):
        got = _attn_result(p, b)
        assert _err("dm3d_attention_group " + form, got, p["ref"]) < LAYER_TOL
        d1, b1 = _attn_desc(dev, p, H3)
        s1 = _attn_scratch(dev, p)
        lib.check(lib.lib().dm3d_attention(C.byref(d1), None if form == "fused" else s1.ptr, None), "attention")
        assert np.array_equal(got.view(np.int32), _attn_result(p, b1).view(np.int32)), "a grouped pass differs from the same pass issued alone"
        s1.get()


# ======================================================================================================================================
# 4. dm3d_mlp_fused, dm3d_attn_front
# ======================================================================================================================================
U = 256
_MLP_W = {}


def _h2_weight(dev, w, entry, *args):
    """float32 [n, k] weight -> its DM3D_FMT_H2 rows -> the operand-fragment image of `entry`, packed into a buffer of the source's byte count."""
    words = h2_encode(w)
    src = _gin(dev, words)
    img = _pack(dev, entry, words.size * 4, src.ptr, *args)
    src.unchanged()
    return img, h2_decode(words)


def _mlp_weights(dev):
    if not _MLP_W:
        g = np.random.default_rng(41)
        _MLP_W["h"] = dict(w0=_f32(g, 4 * U, U, std=1 / 16), b0=_f32(g, 4 * U, std=0.1), w1=_f32(g, U, 4 * U, std=1 / 32), b1=_f32(g, U, std=0.1),
                           w2=_f32(g, U, U, std=1 / 16), b2=_f32(g, U, std=0.1))
    h = _MLP_W["h"]
    img, val = {}, {}
    img["w0"], val["w0"] = _h2_weight(dev, h["w0"], "dm3d_pack_mlp_weights", U, 0)
    img["w1"], val["w1"] = _h2_weight(dev, h["w1"], "dm3d_pack_mlp_weights", U, 1)
    img["w2"], val["w2"] = _h2_weight(dev, h["w2"], "dm3d_pack_front_weights", U, U)
    for k in ("b0", "b1", "b2"):
        img[k], val[k] = _gin(dev, h[k]), h[k]
    return img, val


def _mlp_launch(dev, m, out_h2, tail, x, r1, r2, r3, limit=None):
    lib = _lib_()
    img, val = _mlp_weights(dev)
    xw = h2_encode(x)
    ldx, ldr, ldr3 = U + 16, U + 4, U + 8
    ldo = U + 16 if out_h2 else U + 12
    bufs = dict(x=Guarded.matrix(xw, ldx, dev, IN), r1=Guarded.matrix(r1, ldr, dev, IN), r2=Guarded.matrix(r2, ldr, dev, IN),
                out=Guarded.matrix(np.zeros((m, U), np.float32), ldo, dev, OUT))
    d = lib.MlpDesc()
    d.x, d.ldx, d.w0, d.b0, d.w1, d.b1 = bufs["x"].ptr, ldx, img["w0"].ptr, img["b0"].ptr, img["w1"].ptr, img["b1"].ptr
    d.res, d.res2, d.ldr = bufs["r1"].ptr, bufs["r2"].ptr, ldr
    d.out, d.ldo, d.out_fmt, d.m, d.units = bufs["out"].ptr, ldo, FH2 if out_h2 else FF32, m, U
    if tail:
        bufs["r3"] = Guarded.matrix(r3, ldr3, dev, IN)
        d.w2, d.b2, d.res3, d.ldr3 = img["w2"].ptr, img["b2"].ptr, bufs["r3"].ptr, ldr3
    flag = None
    if limit is not None:
        flag = _gout(dev, np.zeros(1, np.int32))
        d.range_flag, d.range_limit = flag.ptr, limit
    lib.check(lib.lib().dm3d_mlp_fused(C.byref(d), None), "mlp_fused")
    raw = bufs["out"].get()[:, :U]
    got = h2_decode(raw) if out_h2 else raw.astype(np.float64)
    for b in list(img.values()) + [bufs[k] for k in bufs if k != "out"]:
        b.unchanged()
    ref = rk.mlp_fused(h2_decode(xw), val["w0"], val["b0"], val["w1"], val["b1"], r1, r2, (val["w2"], val["b2"], r3) if tail else None).numpy()
    return got, ref, (None if flag is None else int(flag.get()[0]))


@pytest.mark.parametrize("m", [64, 200])
@pytest.mark.parametrize("form", ["f32 out", "H2 out", "w2 tail"])
def test_mlp_fused(dev, rng, m, form):
    x, r1, r2, r3 = _f32(rng, m, U), _f32(rng, m, U), _f32(rng, m, U), _f32(rng, m, U)
    got, ref, _ = _mlp_launch(dev, m, form == "H2 out", form == "w2 tail", x, r1, r2, r3)
    assert _err("dm3d_mlp_fused " + form, got, ref) < LAYER_TOL


_FRONT_NAMES = ("y", "qk", "vt", "q2", "n3")


def _front_host(rng, m):
    h = dict(x=_f32(rng, m, U, std=2.0), w_in=_f32(rng, U, U, std=1 / 16), b_in=_f32(rng, U, std=0.1), w_qk=_f32(rng, 2 * U, U, std=1 / 16),
             b_qk=_f32(rng, 2 * U, std=0.1), w_v=_f32(rng, U, U, std=1 / 16), b_v=_f32(rng, U, std=0.1))
    h["norms"] = [((rng.random(U) + 0.5).astype(np.float32), _f32(rng, U, std=0.2)) for _ in range(3)]
    return h


def _front_launch(dev, m, h, limit=None):
    lib = _lib_()
    img, val = {}, {}
    for k, n in (("w_in", U), ("w_qk", 2 * U), ("w_v", U)):
        img[k], val[k] = _h2_weight(dev, h[k], "dm3d_pack_front_weights", n, U)
    ins = {k: _gin(dev, h[k]) for k in ("b_in", "b_qk", "b_v")}
    for i, (g, b) in enumerate(h["norms"]):
        ins[f"g{i + 1}"], ins[f"be{i + 1}"] = _gin(dev, g), _gin(dev, b)
    ldx, ld = U + 4, dict(y=U + 8, qk=2 * U + 16, vt=m + 16, q2=U + 16, n3=U + 32)
    ins["x"] = Guarded.matrix(h["x"], ldx, dev, IN)
    shapes = dict(y=(m, U), qk=(m, 2 * U), vt=(U, m), q2=(m, U), n3=(m, U))
    outs = {k: Guarded.matrix(np.zeros(shapes[k], np.float32), ld[k], dev, OUT) for k in _FRONT_NAMES}
    d = lib.AttnFrontDesc()
    d.x, d.ldx = ins["x"].ptr, ldx
    d.w_in, d.b_in, d.w_qk, d.b_qk, d.w_v, d.b_v = img["w_in"].ptr, ins["b_in"].ptr, img["w_qk"].ptr, ins["b_qk"].ptr, img["w_v"].ptr, ins["b_v"].ptr
    d.g1, d.be1, d.g2, d.be2, d.g3, d.be3 = (ins[k].ptr for k in ("g1", "be1", "g2", "be2", "g3", "be3"))
    d.eps = 1e-3
    d.y, d.ldy, d.qk, d.ldqk, d.vt, d.ldvt = outs["y"].ptr, ld["y"], outs["qk"].ptr, ld["qk"], outs["vt"].ptr, ld["vt"]
    d.q2, d.ldq2, d.n3, d.ldn3, d.m, d.units = outs["q2"].ptr, ld["q2"], outs["n3"].ptr, ld["n3"], m, U
    flag = None
    if limit is not None:
        flag = _gout(dev, np.zeros(1, np.int32))
        d.range_flag, d.range_limit = flag.ptr, limit
    lib.check(lib.lib().dm3d_attn_front(C.byref(d), None), "attn_front")
    got = {}
    for k in _FRONT_NAMES:
        raw = outs[k].get()[:, :shapes[k][1]]
        got[k] = raw.astype(np.float64) if k == "y" else h2_decode(raw)
    for b in list(img.values()) + list(ins.values()):
        b.unchanged()
    ref = rk.attn_front(h["x"], val["w_in"], h["b_in"], val["w_qk"], h["b_qk"], val["w_v"], h["b_v"], h["norms"], 1e-3)
    return got, {k: v.numpy() for k, v in ref.items()}, (None if flag is None else int(flag.get()[0]))


@pytest.mark.parametrize("mr", ["1", "2"], ids=["32-row tiles", "64-row tiles"])
@pytest.mark.parametrize("m", [64, 128])
def test_attn_front(dev, rng, monkeypatch, m, mr):
    monkeypatch.setenv("DM3D_FRONT_MR", mr)
    got, ref, _ = _front_launch(dev, m, _front_host(rng, m))
    for k in _FRONT_NAMES:
        assert _err("dm3d_attn_front " + k, got[k], ref[k]) < LAYER_TOL


# ======================================================================================================================================
# 5. Row kernels and small entries
# ======================================================================================================================================
LN3_CASES = [(c, rows, h2) for h2 in (False, True) for c in (4, 48, 256, 1024) for rows in (1, 5, 1025) if not (h2 and c % 16)]     # H2 rows: whole records


@pytest.mark.parametrize("c,rows,h2", LN3_CASES)
def test_layernorm3(dev, rng, c, rows, h2):
    nout = 1 + (c // 4 + rows) % 3
    x = _f32(rng, rows, c, mean=0.3, std=2.0)
    params = [((rng.random(c) + 0.5).astype(np.float32), _f32(rng, c)) for _ in range(nout)]
    bx = _gin(dev, x)
    pb = [(_gin(dev, g), _gin(dev, b)) for g, b in params]
    outs = [_gout(dev, np.zeros((rows, c), np.float32)) for _ in range(nout)]
    args = []
    for i in range(3):
        args += [pb[i][0].ptr, pb[i][1].ptr, outs[i].ptr] if i < nout else [None, None, None]
    _call("dm3d_layernorm3_h2" if h2 else "dm3d_layernorm3", bx.ptr, rows, c, 1e-3, *args)
    for (g, b), o in zip(params, outs):
        got = h2_decode(o.get()) if h2 else o.get()
        assert _err("dm3d_layernorm3" + ("_h2" if h2 else ""), got, rk.layernorm(x, g, b, 1e-3).numpy()) < ROW_TOL
    bx.unchanged()
    for g, b in pb:
        g.unchanged(), b.unchanged()


SOFTMAX_CASES = [(cols, h2) for h2 in (False, True) for cols in (8, 16, 100, 1024, 1040, 4112) if not (h2 and cols % 16)]     # H2 rows: whole records


@pytest.mark.parametrize("cols,h2", SOFTMAX_CASES)
def test_softmax_rows(dev, rng, cols, h2):
    rows, ld = 6, cols + 16
    s = _f32(rng, rows, cols, std=4.0)
    s[1, :] = 0.0
    s[1, cols // 2] = 90.0                                    # one dominant logit
    s[2, :] = -3.25                                           # equal logits
    s[3, cols - 1] = 60.0                                     # the dominant one is the row's last element
    ref = torch.softmax(rk.f64(s), -1).numpy()
    buf = Guarded.matrix(s, ld, dev, OUT)
    _call("dm3d_softmax_rows_h2" if h2 else "dm3d_softmax_rows", buf.ptr, rows, cols, ld)
    raw = buf.get()[:, :cols]
    got = h2_decode(raw) if h2 else raw
    assert _err("dm3d_softmax_rows" + ("_h2" if h2 else ""), got, ref) < ROW_TOL
    # rows sum to 1: float32 within 1e-5; a DM3D_FMT_H2 element is hi + lo with lo a float16 that is subnormal below 6e-5 (step 2^-24), so each
    # of the cols probabilities may be off by 2^-25 on top of that (the format's own rounding, whatever kernel writes it)
    assert np.abs(np.asarray(got, np.float64).sum(-1) - 1).max() < 1e-5 + (cols * 2.0 ** -25 if h2 else 0.0)


@pytest.mark.parametrize("rows,c,act,affine", [(33, 64, SILU, False), (1, 4, RELU, False), (7, 20, NONE, False), (1031, 36, SILU, True), (5, 1028, RELU, True)])
def test_affine_act(dev, rng, rows, c, act, affine):
    x, sc, sh = _f32(rng, rows, c, std=3), (rng.random(c) + 0.5).astype(np.float32), _f32(rng, c)
    bx, bs, bh, y = _gin(dev, x), _gin(dev, sc), _gin(dev, sh), _gout(dev, np.zeros((rows, c), np.float32))
    _call("dm3d_affine_act", bx.ptr, y.ptr, rows, c, bs.ptr if affine else None, bh.ptr if affine else None, act)
    if not affine and act == NONE:
        assert np.array_equal(y.get(), x)                     # identity: a bitwise copy
    assert _err("dm3d_affine_act", y.get(), rk.affine_act(x, sc if affine else None, sh, act).numpy()) < ELEM_TOL
    bx.unchanged(), bs.unchanged(), bh.unchanged()


@pytest.mark.parametrize("rows,k,exp2", [(7, 40, 0), (1, 4, 3), (300, 100, -2), (5, 48, 0), (3, 272, 1)])
def test_split_h2(dev, rng, rows, k, exp2):
    kp = -(-k // 16) * 16
    ld_src, ld_dst = k + 4, kp + 16
    x = _f32(rng, rows, k, std=3)
    src = Guarded.matrix(x, ld_src, dev, IN)
    dst = Guarded.matrix(np.full((rows, kp), 7, np.int32), ld_dst, dev, OUT)
    _call("dm3d_split_h2", src.ptr, rows, k, ld_src, exp2, dst.ptr, ld_dst)
    words = dst.get()[:, :kp]
    val = h2_decode(words)
    assert _err("dm3d_split_h2", val[:, :k], x.astype(np.float64) * 2.0 ** exp2) < ELEM_TOL
    halves = np.ascontiguousarray(words).view(np.uint16).reshape(rows, kp // 16, 2, 2, 8)          # [record][hi | lo][slot][8]
    pad = np.zeros((kp,), bool)
    pad[k:] = True
    assert not halves.transpose(0, 2, 1, 3, 4).reshape(rows, 2, kp)[:, :, pad].any(), "columns k..round_up(k, 16) must be exactly zero"
    src.unchanged()


def test_vq_assign(dev, rng):
    rows, dd, k = 70, 8, 20
    E = _f32(rng, dd, k)
    E[:, 11] = E[:, 5]                                        # an exact tie: the lowest index wins
    z = (E.T[rng.integers(0, k, rows)] + _f32(rng, rows, dd, std=0.01)).astype(np.float32)
    z[:6] = E[:, 5]
    sim = (z.astype(np.float64) @ E.astype(np.float64)).astype(np.float32)
    esq = (E.astype(np.float64) ** 2).sum(0).astype(np.float32)
    ref, dist = rk.vq_assign_f32(z, sim, esq)
    part = np.partition(dist, 2, -1)
    assert ((part[:, 2] - part[:, 0]) > 1e-3 * np.abs(dist).max()).all()       # apart from the planted tie the winner is clear
    bz, bs, be, idx = _gin(dev, z), _gin(dev, sim), _gin(dev, esq), _gout(dev, np.full(rows, -7, np.int32))
    _call("dm3d_vq_assign", bz.ptr, rows, dd, bs.ptr, k, be.ptr, idx.ptr)
    got = idx.get()
    assert np.array_equal(got, ref) and (got[:6] == 5).all() and 11 not in got
    bz.unchanged(), bs.unchanged(), be.unchanged()
    WORST.setdefault("dm3d_vq_assign (exact)", 0.0)


@pytest.mark.parametrize("rows,c,table_rows", [(5, 4, 3), (70, 36, 9), (1000, 260, 2)])
def test_gather_rows(dev, rng, rows, c, table_rows):
    table = _f32(rng, table_rows, c)
    idx = rng.integers(0, table_rows, rows).astype(np.int32)
    idx[:4] = [-1, table_rows, 2 ** 31 - 1, -2 ** 31]        # clamped to the first / last row: never outside the table
    bt, bi, out = _gin(dev, table), _gin(dev, idx), _gout(dev, np.zeros((rows, c), np.float32))
    _call("dm3d_gather_rows", bt.ptr, table_rows, bi.ptr, out.ptr, rows, c)
    assert np.array_equal(out.get(), rk.gather_rows(table, idx))
    bt.unchanged(), bi.unchanged()
    WORST.setdefault("dm3d_gather_rows (bitwise)", 0.0)


def test_randn_same_draw_whatever_the_length(dev):
    lib = _lib_()
    draws = {}
    for n in (4, 1028, 4 * 1024 + 4, 4 * 70001):               # one element quad; ragged last blocks
        buf = _gout(dev, np.zeros(n, np.float32))
        lib.check(lib.lib().dm3d_randn(buf.ptr, n, 1234567, 3, None), "randn")
        draws[n] = buf.get()
        assert np.isfinite(draws[n]).all()
    longest = draws[4 * 70001]
    for n, x in draws.items():
        assert np.array_equal(x, longest[:n]), n
    assert abs(float(longest.mean())) < 0.02 and abs(float(longest.std()) - 1) < 0.02
    WORST.setdefault("dm3d_randn (bitwise)", 0.0)


def test_range_check(dev, rng):
    limit = np.float32(100.0)
    base = np.clip(_f32(rng, 4 * 1031, std=20), -99, 99)

    def flag_after(x, n=None, start=0):
        bx, bf = _gin(dev, x), _gout(dev, np.array([start], np.int32))
        _call("dm3d_range_check", bx.ptr, x.size if n is None else n, float(limit), bf.ptr)
        bx.unchanged()
        return int(bf.get()[0])

    assert flag_after(base) == 0 and flag_after(base, start=1) == 1
    assert flag_after(base[:4]) == 0                           # the poison behind four elements is not looked at
    for bad in (np.nan, np.inf, np.nextafter(limit, np.float32(np.inf)), -np.float32(101)):
        x = base.copy()
        x[-1] = bad
        assert flag_after(x) == 1 and flag_after(x, n=x.size - 4) == 0, bad
    WORST.setdefault("dm3d_range_check (exact)", 0.0)


# ======================================================================================================================================
# 7. dm3d_ddpm_update
# ======================================================================================================================================
T_STEPS = 50


def _ddpm(dev, x, eps, t, mode, noise=None, seed=0, seed_dev=None):
    lib = _lib_()
    tab = rt.Betas(T_STEPS)
    B, per = x.shape
    bufs = dict(x=_gout(dev, x) if mode == 1 else _gin(dev, x), eps=_gin(dev, eps), t=_gin(dev, np.asarray(t, np.int32)))
    d = lib.DdpmDesc()
    d.x, d.eps, d.t, d.batch, d.per_sample, d.timesteps, d.mode, d.seed = bufs["x"].ptr, bufs["eps"].ptr, bufs["t"].ptr, B, per, T_STEPS, mode, seed
    for name in ("beta", "sqrt_alpha", "alpha_bar", "alpha_bar_prev", "sqrt_alpha_bar", "sqrt_alpha_bar_prev", "sqrt_one_minus_alpha_bar"):
        bufs[name] = _gin(dev, getattr(tab, name).numpy())     # each table in an allocation of its own, poison on both sides
        setattr(d, name, bufs[name].ptr)
    if noise is not None:
        bufs["noise"] = _gin(dev, noise)
        d.noise = bufs["noise"].ptr
    if seed_dev is not None:
        bufs["seed_dev"] = _gin(dev, np.array([seed_dev, 0], np.uint64))
        d.seed_dev = bufs["seed_dev"].ptr
    if mode == 0:
        bufs["mean"], bufs["var"] = _gout(dev, np.zeros((B, per), np.float32)), _gout(dev, np.zeros(B, np.float32))
        d.mean_out, d.var_out = bufs["mean"].ptr, bufs["var"].ptr
    lib.check(lib.lib().dm3d_ddpm_update(C.byref(d), None), "ddpm_update")
    res = (bufs["mean"].get(), bufs["var"].get()) if mode == 0 else (bufs["x"].get(),)
    for k, b in bufs.items():
        if b.role == IN:
            b.unchanged()
    return res


@pytest.mark.parametrize("per", [4, 1028, 4 * 8 * 8 * 8])
def test_ddpm_update(dev, rng, per):
    B, T = 4, T_STEPS
    x, eps, z = _f32(rng, B, per), _f32(rng, B, per), _f32(rng, B, per)
    t_out, t_in = [-5, 0, T - 1, T + 3], [0, 0, T - 1, T - 1]
    mean_r, var_r, step_r = rk.ddpm_update(rt.Betas(T), x, eps, t_in, z)
    mean, var = _ddpm(dev, x, eps, t_in, 0)
    assert _err("dm3d_ddpm_update mean", mean, mean_r.numpy()) < ELEM_TOL
    assert _err("dm3d_ddpm_update var", var, var_r.numpy()) < ELEM_TOL
    step, = _ddpm(dev, x, eps, t_in, 1, noise=z)
    assert _err("dm3d_ddpm_update step", step, step_r.numpy()) < ELEM_TOL
    # t is clamped to [0, timesteps) before any table is indexed (the tables' neighbours are poison)
    mean_c, var_c = _ddpm(dev, x, eps, t_out, 0)
    assert np.array_equal(mean_c.view(np.int32), mean.view(np.int32)) and np.array_equal(var_c.view(np.int32), var.view(np.int32))
    assert np.array_equal(_ddpm(dev, x, eps, t_out, 1, noise=z)[0].view(np.int32), step.view(np.int32))
    # in-kernel Philox: seed_dev holding s is seed = s
    a, = _ddpm(dev, x, eps, t_in, 1, seed=987654321)
    b, = _ddpm(dev, x, eps, t_in, 1, seed=5, seed_dev=987654321)
    c, = _ddpm(dev, x, eps, t_in, 1, seed=5)
    assert np.isfinite(a).all() and np.array_equal(a.view(np.int32), b.view(np.int32)) and not np.array_equal(a, c)


# ======================================================================================================================================
# 8. The range guard, epilogue by epilogue
# ======================================================================================================================================
L = 500.0


def _sign(where, allowed=True):
    """-1 for the plants at the end of the first sample, where the epilogue can store a negative value at all."""
    return -1.0 if allowed and where == "end of first sample" else 1.0


def _conditions(ref, pos, limit):
    """The two reference-side conditions of a plant, from float64 alone: the planted value is at least twice the limit, every other one at
    most half of it."""
    ref = np.asarray(ref, np.float64)
    assert abs(ref[pos]) >= 2 * limit, (abs(ref[pos]), limit)
    rest = np.abs(ref)
    rest[pos] = 0
    assert rest.max() <= limit / 2, (rest.max(), limit)


def _guard_rounds(run, base, pos, inverse=lambda v: v, sign=1.0):
    """`run(res, limit) -> (ref, flag)` with the residual `res` built here: base["res"] plus, at `pos`, what makes the stored value T
    (base["nores"]: the float64 result without the residual; `inverse`: T -> the value in front of a consumer's post step).
    `sign` = -1 plants -T: the guard looks at magnitudes.  Plant (T = 3L against L) -> 1; control (the same plant under 4L) -> exactly 0; limit 0 is 65504: 7.0e4 -> 1, 6.0e4 -> 0."""
    for target, limit, want in ((3 * L, L, 1), (3 * L, 4 * L, 0), (7.0e4, 0.0, 1), (6.0e4, 0.0, 0)):
        res = base["res"].copy()
        res[pos] = np.float32(inverse(sign * target) - base["nores"][pos])
        ref, flag = run(res, limit)
        if limit == L:
            _conditions(ref, pos, L)
        else:                                                  # the operands' side of the other rounds: the plant is what it is meant to be
            rest = np.abs(ref)
            rest[pos] = 0
            assert abs(ref[pos] - sign * target) <= 0.01 * target and rest.max() <= L / 2, (ref[pos], rest.max())
        assert flag == want, f"stored {target:g} under range_limit {limit:g}: flag {flag}, expected {want}"


GUARD_CONVS = ["v3 td4 nct4 full 16B", "v3 td8 nct4 full 16B", "v3 td4 nct2 cout32", "v3 td4 nct1 cout8", "v3 td4 full scalar (PReLU)",
               "v3 td4 partial 6x5x7 cout40", "v3 td8 partial 6x5x7 cout40", "v3 td4 H2 out + post", "v3 post, float32 out", "v3 fused skip (skip_wpk)",
               "v3 Cin split", "wino Cin48 B2", "wino two-way Cin split", "wino skip tail (skip_wpk_frag)", "wino H2 out + post",
               "tap k3 s2 5x6x8", "tap k1 full brick", "tap k1 partial 5x6x7", "tap k4 s2 6x8x4", "parity upsample 4^3", "parity transpose 3x5x4",
               # the Winograd-x form's general epilogue branch (ragged cout: the plant at "last" sits in the last valid channel), and the
               # 8-slice instantiations of the scalar and the DM3D_FMT_H2 full-brick branches
               "pack h3w 20->40", "pack h3w 48->72", "v3 td8 full scalar (PReLU)", "v3 td8 H2 out + post"]


def _positions(shape):
    """First element; last element of the tensor (the last valid voxel and channel of a partial brick or tile, in the last sample); the last
    channel of the first sample's last voxel."""
    first, last = (0,) * len(shape), tuple(n - 1 for n in shape)
    return {"first": first, "last": last, "end of first sample": (0,) + last[1:]}


@pytest.mark.parametrize("where", ["first", "last", "end of first sample"])
@pytest.mark.parametrize("name", GUARD_CONVS)
def test_range_guard_conv(dev, monkeypatch, name, where):
    s = CONV_BY_NAME[name]
    h = _conv_host_cached(s)
    pos = _positions(h["res"].shape)[where]
    inverse = (lambda v: v)
    if h["post"] is not None:                                  # the guard looks at what is stored: behind post_* and SiLU (silu(u) = u up there)
        inverse = lambda v: (v - float(h["post"][1][pos[-1]])) / float(h["post"][0][pos[-1]])

    def run(res, limit):
        _, flag = _conv_launch(dev, monkeypatch, s, h, res, limit)
        return _conv_finish(h, res), flag

    _guard_rounds(run, dict(res=h["res"], nores=h["base"]), pos, inverse, _sign(where, h["post"] is None))       # (SiLU stores nothing below -0.28)


@pytest.mark.parametrize("name", ["v3 td4 partial 6x5x7 cout40", "v3 td8 partial 6x5x7 cout40", "tap k1 partial 5x6x7", "pack h3w 20->40"])
def test_range_guard_conv_partial_brick_masked_lanes(dev, monkeypatch, name):
    """The lanes a partial brick masks read clamped addresses: the bias of the last valid channel and the residual of element 0 of a slice.
    The last channel carries res = +3L in every voxel, cancelled by bias = -3L; channel 0 (where a clamped residual address lands)
    carries res = -3L and bias = +3L.  Every true output stays below L/2, while a lane that combined the clamped operands would see 6L:
    only output values count (include/dm3d.h), so the flag stays 0."""
    s = dict(CONV_BY_NAME[name], relu=False, name=name + ", adversarial")
    h = _conv_host_cached(s)
    bias, res = h["bias"].copy(), h["res"].copy()
    bias[-1] -= np.float32(3 * L)
    bias[0] += np.float32(3 * L)
    res[..., -1] += np.float32(3 * L)
    res[..., 0] -= np.float32(3 * L)
    g = dict(h, bias=bias, base=h["base"] + (bias.astype(np.float64) - h["bias"]))        # no ReLU / PReLU: the bias enters linearly
    ref = _conv_finish(g, res)
    assert np.abs(ref).max() <= L / 2 and np.abs(res[..., -1]).min() >= 2 * L and np.abs(res[..., 0]).min() >= 2 * L
    got, flag = _conv_launch(dev, monkeypatch, s, g, res, L)
    assert _err("dm3d_conv3d_ndhwc masked lanes", got, ref, scale=3 * L) < LAYER_TOL
    assert flag == 0, "a masked lane of a partial brick raised the range flag"


GUARD_GEMMS = [("full tile", 128, 64, FF32, None), ("partial tile", 200, 48, FF32, None), ("partial tile, H2 out", 200, 48, FH2, None), ("one row", 1, 16, FF32, None),
               ("128x128 tiles, full", 128, 128, FF32, "2"), ("128x128 tiles, partial", 200, 144, FH2, "2")]


@pytest.mark.parametrize("where", ["first", "last", "end of first sample"])
@pytest.mark.parametrize("case", GUARD_GEMMS, ids=[c[0] for c in GUARD_GEMMS])
def test_range_guard_gemm(dev, rng, monkeypatch, case, where):
    _, m, n, of, mr = case
    lib = _lib_()
    monkeypatch.delenv("DM3D_GEMM_MR", raising=False)
    if mr:
        monkeypatch.setenv("DM3D_GEMM_MR", mr)                  # read per call: 2 forces the 128 x 128 tile form a launch takes from 256 tiles up
    p = _gemm_problem(rng, m, n, 48, 2, FF32, FH2, of, H3, "n", 1, NONE, 0.25, False)
    nores = _gemm_ref(dict(p, res=None))
    pos = _positions(nores.shape)[where]

    def run(res, limit):
        q = dict(p, res=res)
        d, bufs = _gemm_desc(dev, q, limit)
        lib.check(lib.lib().dm3d_gemm_tn(C.byref(d), None), "gemm_tn")
        _gemm_result(q, bufs)
        return _gemm_ref(q), int(bufs["flag"].get()[0])

    _guard_rounds(run, dict(res=p["res"], nores=nores), pos, sign=_sign(where))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_range_guard_gemm_group_of_three(dev, rng, which):
    """Each problem of a group carries its own flag: the plant in problem `which` raises that one and no other."""
    lib = _lib_()
    probs = [_gemm_problem(rng, m, n, k, batch, FF32, FF32, FF32, H3, bias, 1, NONE, 0.25, False) for m, n, k, batch, bias, _, _ in GROUP_PROBLEMS[:3]]
    refs = []
    for i, p in enumerate(probs):
        if i == which:
            nores = _gemm_ref(dict(p, res=None))
            pos = tuple(n - 1 for n in nores.shape)
            p["res"][pos] = np.float32(3 * L - nores[pos])
        refs.append(_gemm_ref(p))
        if i == which:
            _conditions(refs[i], pos, L)
        else:
            assert np.abs(refs[i]).max() <= L / 2
    descs, bufs = zip(*(_gemm_desc(dev, p, L) for p in probs))
    lib.check(lib.lib().dm3d_gemm_tn_group((lib.GemmDesc * 3)(*descs), 3, None), "gemm_tn_group")
    for i, (p, b) in enumerate(zip(probs, bufs)):
        _gemm_result(p, b)
        assert int(b["flag"].get()[0]) == int(i == which), f"problem {i}"


def test_range_guard_gemm_partial_tile_masked_lanes(dev, rng):
    """m = 200, n = 48: the lanes past the edge of the last tile load clamped rows and columns.  The last valid row carries res = +3L and
    its neighbour res = -3L, each cancelled by its own product (that row of A is a scaled row of B, and B's rows are orthogonal), so every
    true output stays below L/2; a lane that paired one row's product with the other's residual would see 6L.  The flag must stay 0."""
    lib = _lib_()
    m, n, k = 200, 48, 48
    p = _gemm_problem(rng, m, n, k, 1, FF32, FF32, FF32, H3, None, 1, NONE, 1.0, False)
    b = np.zeros((1, n, k), np.float32)
    b[0, np.arange(n), np.arange(n)] = 2.0                     # orthogonal rows: A[r] . B[j] = 2 A[r][j]
    p["b"] = p["b_words"] = b
    for row, sign in ((m - 1, 1.0), (m - 2, -1.0)):
        p["a"][0, row, :] = np.float32(-sign * 1.5 * L)         # the product is -+3L in every column
        p["res"][0, row, :] += np.float32(sign * 3 * L)
    p["a_words"] = p["a"]
    ref = _gemm_ref(p)
    assert np.abs(ref).max() <= L / 2 and np.abs(p["res"][0, m - 2:]).min() >= 2 * L
    d, bufs = _gemm_desc(dev, p, L)
    lib.check(lib.lib().dm3d_gemm_tn(C.byref(d), None), "gemm_tn")
    _, got = _gemm_result(p, bufs)
    assert _err("dm3d_gemm_tn h3", got, ref, scale=3 * L) < LAYER_TOL
    assert int(bufs["flag"].get()[0]) == 0, "a masked lane of a partial tile raised the range flag"


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("form", ["f32 out", "H2 out", "w2 tail"])
def test_range_guard_mlp(dev, rng, form, where):
    m = 200
    x, r1, r2, r3 = _f32(rng, m, U), _f32(rng, m, U), _f32(rng, m, U), _f32(rng, m, U)
    tail = form == "w2 tail"
    img_val = _mlp_weights(dev)[1]
    base = rk.mlp_fused(h2_decode(h2_encode(x)), img_val["w0"], img_val["b0"], img_val["w1"], img_val["b1"], r1, r2 if tail else None,
                        (img_val["w2"], img_val["b2"], None) if tail else None).numpy()
    pos = _positions(base.shape)[where]

    def run(res, limit):
        _, ref, flag = _mlp_launch(dev, m, form == "H2 out", tail, x, r1, r2 if tail else res, res if tail else r3, limit)
        return ref, flag

    _guard_rounds(run, dict(res=r3 if tail else r2, nores=base), pos, sign=_sign("end of first sample", where == "last"))


@pytest.mark.parametrize("out", ["y", "qk", "vt", "q2", "n3"])
def test_range_guard_attn_front(dev, rng, monkeypatch, out):
    """Each of the five outputs has a guard site of its own and no residual: the plant goes through the operand that adds into that output
    alone — b_in for y (behind the ReLU), b_qk's key half for qk, b_v for vt, beta3 for n3, and a large row of W_qk's query half seen only
    through norm2 for q2 (beta2 aligned with it, beta1 orthogonal to it)."""
    monkeypatch.delenv("DM3D_FRONT_MR", raising=False)
    m = 64
    h = _front_host(rng, m)
    col = U - 1

    def plant(target):
        g = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in h.items()}
        g["norms"] = [(a.copy(), b.copy()) for a, b in h["norms"]]
        if out == "qk":
            g["b_qk"][2 * U - 1] = target
        elif out == "vt":
            g["b_v"][col] = target
        elif out == "n3":
            g["norms"][2][1][col] = target
        elif out == "y":
            g["b_in"][col] = target                            # y's column is `target`-sized in every row; the norms absorb it (LayerNormalization)
        else:                                                  # q2 = n2 . W_q^T + b_q: one query row that only norm2's beta excites
            g["norms"][1][1][:] = 0.0
            g["norms"][1][1][7] = target / 64.0
            g["norms"][1][0][7] = 0.0                          # n2's column 7 is exactly beta2[7]
            g["norms"][0][1][7] = 0.0
            g["norms"][0][0][7] = 0.0                          # n1 (the source of q|k and v) is exactly 0 in that column
            g["w_qk"][col, :] = 0.0
            g["w_qk"][col, 7] = 64.0
        return g

    sign = -1.0 if out in ("vt", "n3") else 1.0                # (y sits behind a ReLU; two of the others carry the negative plants)
    for target, limit, want in ((3 * L, L, 1), (3 * L, 4 * L, 0), (7.0e4, 0.0, 1), (6.0e4, 0.0, 0)):
        g = plant(np.float32(sign * target))
        got, ref, flag = _front_launch(dev, m, g, limit)
        eff = limit if limit > 0 else 65504.0
        peak = {k: float(np.abs(v).max()) for k, v in ref.items()}
        others = max(v for k, v in peak.items() if k != out)
        assert others <= L / 2 and abs(peak[out] - target) <= 0.02 * target, peak             # from the float64 reference alone
        assert (peak[out] > eff) == bool(want)
        assert flag == want, f"{out}: target {target:g} under limit {limit:g}: flag {flag}, expected {want}; peaks {peak}"

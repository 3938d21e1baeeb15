"""The split-float16 (h3) kernels of the C ABI on operands whose sums are EXACT (tests/h3_exact_cases.py: constructions, budget, proofs).
Every product and partial sum of an exact pattern is a float32, so a correct kernel returns the float64 reference bit for bit, in any
summation order, with the lo pieces live; a lost, doubled or misplaced hi / lo piece at ONE (tap, input channel) is a difference of at
least one quantum, where the Gaussian parity tests (2e-5 of max|ref|) leave room for it.

Harness: the cases, launch, packers and guard bands of tests/test_gpu_infer_kernels.py (imported; every buffer guarded, every conv case
asserts dm3d_conv_tile_form / dm3d_conv_weight_layout), with the host dict built by h3_exact_cases.conv_host.
  convs     every form listed in h3_exact_cases.EXACT_CONV without its inexact steps (direct 16x16x32 kernel td4 / td8, NCT 4 / 2 / 1,
            partial bricks, dual input, H2 input, PReLU, fused skip conv, Cin split; Winograd-x MODE 0 and, behind an H2 input, MODE 2,
            Cin split, skip tail, ragged cout 40; TAP kernel; parity forms), each with patterns hi, act-lo, wgt-lo (array_equal) and
            both-lo (2^-21 sum|a||b| per output) under rotations 0, 1, 16, 21; the prologue / post / H2-output forms under
            ELEM_TOL sum|a||b| per output.
  GEMM      dm3d_gemm_tn H3, dense operands, k 16 / 48 / 272 at 129 x 48 and 200 x 144, every a_fmt / b_fmt, alpha a power of two, bias
            along n and m, res, res2; the 128-tile form (DM3D_GEMM_MR=2); dm3d_gemm_tn_group with three problems.
  fused MLP dm3d_mlp_fused, units 256, m 64 / 200, float32 out: the hidden activation's own lo half is live in the second product.
The hi pattern is the control: no split term is live in it, so a whole-quantum difference THERE would say the MFMA's internal adder does
not keep 21 bits under its largest addend, not that a kernel lost a piece (docs/EXPERIMENTS.md records the run).
Not covered: dm3d_attn_front (layer norms in front of its contractions); the attention kernels' logit axis has
tests/test_gpu_attention_logits.py."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import h3_exact_cases as hx
import test_gpu_infer_kernels as tk

pytestmark = pytest.mark.gpu
RECORD = {}


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    yield torch.device("cuda:0")
    for name in sorted(RECORD):
        print(f"h3 exact {name}: {RECORD[name]}")


def _note(name, differing=0, total=0, share=None):
    r = RECORD.setdefault(name, {"differing": 0, "outputs": 0})
    r["differing"] += differing
    r["outputs"] += total
    if share is not None:
        r["worst share of bar"] = round(max(r.get("worst share of bar", 0.0), share), 3)


def _share(got, ref, bar):
    assert np.isfinite(got).all(), "non-finite output (a read outside an operand's extent?)"
    return float((np.abs(got - ref) / np.maximum(bar, 1e-300)).max())


EXACT_CASES = [(n, hx.exact_form(tk.CONV_BY_NAME[n])) for n in hx.EXACT_CONV]
EXACT_CASES += [(n + " (H2 in)", hx.exact_form(tk.CONV_BY_NAME[n], x_h2=True)) for n in hx.H2_IN_TOO]


@pytest.mark.parametrize("name,s", EXACT_CASES, ids=[n for n, _ in EXACT_CASES])
def test_conv3d_exact(dev, monkeypatch, name, s):
    for pattern, rot in itertools.product(hx.PATTERNS, hx.ROTATIONS):
        h = hx.conv_host(s, pattern, rot)
        q, _ = hx.budget(s, h, pattern)
        got, _ = tk._conv_launch(dev, monkeypatch, s, h, h["res"])
        ref = hx.conv_finish(h, h["res"])
        if pattern in hx.EXACT:
            ref32 = ref.astype(np.float32).astype(np.float64)
            bad = int((got != ref32).sum())
            _note(f"conv {name} / {pattern}", bad, got.size)
            print(f"conv {name} / {pattern} / rotation {rot}: {bad} of {got.size} outputs differ")
            assert np.array_equal(got, ref32), f"{pattern}: " + hx.explain(s, rot, got, ref32, q)
        else:
            share = _share(got, ref, hx.conv_bar(s, h, pattern))
            _note(f"conv {name} / {pattern}", share=share)
            print(f"conv {name} / {pattern} / rotation {rot}: worst error {share:.3f} of 2^-21 sum|a||b|")
            assert share <= 1.0


@pytest.mark.parametrize("name", hx.INEXACT_CONV)
def test_conv3d_inexact_step_forms(dev, monkeypatch, name):
    """Prologue (norm + SiLU in front), post step and DM3D_FMT_H2 output: act-lo and wgt-lo against ELEM_TOL sum|a||b| per output."""
    s = tk.CONV_BY_NAME[name]
    for pattern, rot in itertools.product(("act-lo", "wgt-lo"), hx.ROTATIONS):
        h = hx.conv_host(s, pattern, rot)
        hx.budget(s, h, pattern)
        got, _ = tk._conv_launch(dev, monkeypatch, s, h, h["res"])
        share = _share(got, hx.conv_finish(h, h["res"]), hx.conv_bar(s, h, pattern))
        _note(f"conv (inexact step) {name} / {pattern}", share=share)
        print(f"conv (inexact step) {name} / {pattern} / rotation {rot}: worst error {share:.3f} of ELEM_TOL sum|a||b|")
        assert share <= 1.0


# ---- GEMM --------------------------------------------------------------------------------------------------------------------------------
def _gemm_variants(m, n, k):
    """Every a_fmt / b_fmt, with the epilogue moving along: (af, bf, bias, res, act, alpha, batch)."""
    for i, (af, bf) in enumerate(itertools.product((tk.FF32, tk.FH2), repeat=2)):
        yield af, bf, ("n", "m", None, "n")[i], (2, 1, 2, 0)[i], (tk.NONE, tk.RELU)[i % 2], (1.0, 0.5, 2.0, 0.25)[i], (1, 2)[i % 2]


def _gemm_check(dev, p, pattern, name, launch):
    d, bufs = tk._gemm_desc(dev, p)
    launch(d)
    _, got = tk._gemm_result(p, bufs)
    if pattern in hx.EXACT:
        ref32 = p["ref"].astype(np.float32).astype(np.float64)
        assert np.array_equal(ref32, p["ref"])
        _note(f"{name} / {pattern}", int((got != ref32).sum()), got.size)
        assert np.array_equal(got, ref32), f"{pattern}: " + hx.explain_gemm(p, got, ref32)
    else:
        share = _share(got, p["ref"], hx.BOTH_LO_TOL * p["prod_abs"])
        _note(f"{name} / {pattern}", share=share)
        assert share <= 1.0


def _single(d):
    lib = tk._lib_()
    lib.check(lib.lib().dm3d_gemm_tn(C.byref(d), None), "gemm_tn")


@pytest.mark.parametrize("k", [16, 48, 272])
@pytest.mark.parametrize("m,n", [(129, 48), (200, 144)])
def test_gemm_tn_exact(dev, m, n, k):
    for pattern in hx.PATTERNS:
        for af, bf, bias, res, act, alpha, batch in _gemm_variants(m, n, k):
            _gemm_check(dev, hx.gemm_problem(pattern, m, n, k, batch, af, bf, bias, res, act, alpha), pattern, f"gemm_tn m{m} n{n} k{k}", _single)


@pytest.mark.parametrize("m,n,k", [(200, 144, 272), (129, 48, 16), (256, 128, 48)])
def test_gemm_tn_exact_128_tile_form(dev, monkeypatch, m, n, k):
    """DM3D_GEMM_MR=2 (read per call) forces the 128 x 128 tile form."""
    monkeypatch.setenv("DM3D_GEMM_MR", "2")
    for pattern in hx.PATTERNS:
        _gemm_check(dev, hx.gemm_problem(pattern, m, n, k, 2, tk.FH2, tk.FF32, "m", 2, tk.RELU, 0.5), pattern, "gemm_tn 128x128 tiles", _single)


def test_gemm_tn_group_exact(dev):
    lib = tk._lib_()
    for pattern, fmt in itertools.product(hx.PATTERNS, (tk.FF32, tk.FH2)):             # (a group shares its operand formats)
        probs = [hx.gemm_problem(pattern, m, n, k, batch, fmt, fmt, bias, res, act, alpha)
                 for m, n, k, batch, bias, res, act, alpha in ((200, 16, 48, 2, "n", 1, tk.RELU, 0.5), (65, 48, 16, 1, "m", 2, tk.NONE, 2.0),
                                                                (129, 144, 272, 1, "n", 1, tk.NONE, 1.0))]
        descs, bufs = zip(*(tk._gemm_desc(dev, p) for p in probs))
        arr = (lib.GemmDesc * 3)(*descs)
        lib.check(lib.lib().dm3d_gemm_tn_group(arr, 3, None), "gemm_tn_group")
        for p, b in zip(probs, bufs):
            _, got = tk._gemm_result(p, b)
            if pattern in hx.EXACT:
                ref32 = p["ref"].astype(np.float32).astype(np.float64)
                _note(f"gemm_tn_group / {pattern}", int((got != ref32).sum()), got.size)
                assert np.array_equal(got, ref32), f"{pattern}: " + hx.explain_gemm(p, got, ref32)
            else:
                share = _share(got, p["ref"], hx.BOTH_LO_TOL * p["prod_abs"])
                _note(f"gemm_tn_group / {pattern}", share=share)
                assert share <= 1.0


# ---- fused MLP ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [64, 200])
def test_mlp_fused_exact(dev, monkeypatch, m):
    p = hx.mlp_problem(m, tk.U)
    monkeypatch.setitem(tk._MLP_W, "h", {k: p[k] for k in ("w0", "b0", "w1", "b1", "w2", "b2")})
    got, ref, _ = tk._mlp_launch(dev, m, False, False, p["x"], p["r1"], p["r2"], None)
    assert np.array_equal(ref, p["ref"]) and np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    bad = np.argwhere(got != ref)
    _note("mlp_fused", len(bad), got.size)
    msg = ""
    if len(bad):
        i = tuple(int(v) for v in bad[0])
        msg = (f"{len(bad)} of {got.size} outputs differ; first at (row, unit) = {i}: got {got[i]!r}, reference {ref[i]!r}, difference "
               f"{(got[i] - ref[i]) / p['q']:+.3g} q (q = 2^-12); hidden units live there: {np.nonzero(p['w1'][i[1]])[0].tolist()}")
    assert not len(bad), msg

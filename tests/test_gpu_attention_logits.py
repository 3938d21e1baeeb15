"""GPU parity of dm3d_attention (fused and three-launch form), dm3d_attention_group and dm3d_softmax_rows[_h2] along the LOGIT axis: score
rows built by tests/attention_logit_cases.py (equal logits, a single one, stairs that move the fused kernel's lazy running maximum on
every tile / every second tile / never, one lane of a wave moving alone, every lane with its own history, a tail sitting just above or
just below the float16 split's rounding point, a common shift of +-64), against float64 on guarded buffers.

Shapes, strides, formats and tile forms are the business of tests/test_gpu_infer_kernels.py, whose descriptor and guarded-buffer plumbing
(`_attn_desc`, `_attn_result`, `_attn_scratch`, `_err`) is used here as it stands.  What each pattern drives inside attn_fused_h3 is
asserted on the CPU, on a model of the documented rule (tests/test_attention_logits_host.py); nothing here reads the kernel's state.

Every bound is attention_logit_cases.bound: the project's bar (LAYER_TOL for the attention entries, ROW_TOL for softmax_rows), the
float32 rounding of the score, and — for tail_floor alone, where the probabilities pass through float16 hi + lo — the format's floor of
2^-25 per probability.  Each test prints its error beside the bound and the terms the bound consisted of (docs/EXPERIMENTS.md records
a run)."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_logit_cases as lc
import test_gpu_infer_kernels as ik
from guarded_buffers import OUT, Guarded, h2_decode
from oracle import ref_kernels as rk

pytestmark = pytest.mark.gpu

F32, H3, FF32, FH2 = ik.F32, ik.H3, ik.FF32, ik.FH2
assert (lc.LAYER_TOL, lc.ROW_TOL) == (ik.LAYER_TOL, ik.ROW_TOL), "attention_logit_cases restates the project's bars"
RECORD = []


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    yield torch.device("cuda:0")
    for line in RECORD:
        print(line)


def _within(entry, what, name, got, ref, S, h2, v=None, scale=None):
    """Asserts got within bound of ref (finiteness first: ik._err); prints error, bound and the bound's terms."""
    total, terms = lc.bound(entry, name, S, h2, v, ref)
    e = ik._err(f"{what} {name}", got, ref, scale)
    RECORD.append(f"| {what} | {name} | {S.shape[-1]} | {e:.2e} | {total:.2e} | {lc.describe(terms)} |"
                  + (f" {e / terms['floor']:.2f} |" if terms["floor"] else " |"))
    print(f"    bound {total:.2e} = {lc.describe(terms)}")
    assert e < total, (what, name, e, total)
    return e


def _run_attention(dev, p, prec, scratch=True):
    lib = ik._lib_()
    d, bufs = ik._attn_desc(dev, p, prec)
    s = ik._attn_scratch(dev, p) if scratch else None
    lib.check(lib.lib().dm3d_attention(C.byref(d), s.ptr if s else None, None), "attention")
    got = ik._attn_result(p, bufs)                              # pads and gaps of the output intact, every input unchanged
    if s:
        s.get()
    return got


def _fused_cases():
    out = []
    for lk in (32, 64, 256, 4096):
        for name in lc.pattern_names(lk, lc.LONG_PATTERNS if lk == 4096 else None):
            for kind in (("zero_mean", "with_mean") if name.startswith(lc.FLOOR_PATTERNS) else ("zero_mean",)):
                out.append((name, lk, kind))
    return out


# ======================================================================================================================================
# dm3d_attention, fused form: B = 1, lq = 128 (one workgroup, four waves of 32 queries), c = 256, H2 operands, scratch NULL, residual
# ======================================================================================================================================
@pytest.mark.parametrize("name,lk,kind", _fused_cases())
def test_attention_fused(dev, name, lk, kind):
    p = lc.attention_problem(name, 1, 128, lk, 256, FH2, False, kind)
    got = _run_attention(dev, p, H3, scratch=False)             # scratch NULL: only the fused form accepts it
    _within("attention", f"fused {kind}", name, got, p["ref"], p["S"], True, p["v"])


def test_attention_fused_two_samples_broadcast_keys(dev):
    p = lc.attention_problem("mixed_wave", 2, 128, 64, 256, FH2, True)
    got = _run_attention(dev, p, H3, scratch=False)
    _within("attention", "fused B=2 broadcast keys", "mixed_wave", got, p["ref"], p["S"], True, p["v"])


def test_reference_is_the_projects(dev):
    """The float64 reference of attention_logit_cases (numpy) is oracle/ref_kernels.attention on the same decoded operands."""
    p = lc.attention_problem("mixed_wave", 2, 128, 64, 256, FH2, True)
    ref = rk.attention(h2_decode(p["qw"]), h2_decode(p["kw"]), h2_decode(p["vtw"]).transpose(0, 2, 1), p["scale"], p["res"]).numpy()
    assert np.abs(ref - p["ref"]).max() < 1e-12 * np.abs(ref).max()


# ======================================================================================================================================
# dm3d_attention, three-launch form: B = 2, lq = 64, c = 32, own keys, scratch guarded
# ======================================================================================================================================
THREE_PATTERNS = ["flat(0)", "flat(-3.25)", "one_hot(0)", "one_hot(31)", "one_hot(32)", "one_hot(last)", "stairs_up(8.5)", "mixed_wave",
                  "tail_floor(17.2)", "tail_floor(17.4)", "offset(+64)", "offset(-64)"]
THREE_FORMS = {"f32": (F32, FF32), "h3": (H3, FF32), "h3 H2 operands": (H3, FH2)}


@pytest.mark.parametrize("name", THREE_PATTERNS)
@pytest.mark.parametrize("lk", [48, 112])
@pytest.mark.parametrize("form", list(THREE_FORMS))
def test_attention_three_launch(dev, form, lk, name):
    prec, fmt = THREE_FORMS[form]
    p = lc.attention_problem(name, 2, 64, lk, 32, fmt, False)
    got = _run_attention(dev, p, prec)
    _within("attention", f"three launches {form}", name, got, p["ref"], p["S"], fmt == FH2, p["v"])


# ======================================================================================================================================
# dm3d_attention_group: a mixed_wave self pass and a tail_floor broadcast pass in one call
# ======================================================================================================================================
@pytest.mark.parametrize("form", ["fused", "fallback"])
def test_attention_group(dev, form):
    lib = ik._lib_()
    B, lq, lk, c = (2, 128, 64, 256) if form == "fused" else (2, 64, 48, 64)
    probs = [lc.attention_problem("mixed_wave", B, lq, lk, c, FH2, False), lc.attention_problem("tail_floor(17.2)", B, lq, lk, c, FH2, True, "with_mean")]
    descs, bufs = zip(*(ik._attn_desc(dev, p, H3) for p in probs))
    scratch = ik._attn_scratch(dev, probs[0])
    arr = (lib.AttentionDesc * 2)(*descs)
    lib.check(lib.lib().dm3d_attention_group(arr, 2, None if form == "fused" else scratch.ptr, None), "attention_group")
    scratch.get()
    for p, b in zip(probs, bufs):
        got = ik._attn_result(p, b)
        _within("attention", f"group {form}", p["name"], got, p["ref"], p["S"], True, p["v"])
        alone = _run_attention(dev, p, H3, scratch=form != "fused")
        assert np.array_equal(got.view(np.int32), alone.view(np.int32)), "a grouped pass differs from the same pass issued alone"


# ======================================================================================================================================
# A common shift of the logits: the output moves by no more than twice the float32 rounding of the shifted score
# ======================================================================================================================================
def _shift_invariance(dev, what, B, lq, lk, c, prec, fmt, scratch):
    base = lc.attention_problem("mixed_wave", B, lq, lk, c, fmt, False)
    got0 = _run_attention(dev, base, prec, scratch)
    for name in ("offset(+64)", "offset(-64)"):
        p = lc.attention_problem(name, B, lq, lk, c, fmt, False)
        assert np.array_equal(p["vtw"], base["vtw"]) and np.array_equal(p["res"], base["res"]) and np.array_equal(p["S"], base["S"] + (64 if "+" in name else -64))
        got = _run_attention(dev, p, prec, scratch)
        allowed = 2.0 * lc.score_term(p["S"])
        e = ik._err(f"{what} {name} against mixed_wave", got, got0, float(np.abs(base["ref"]).max()))
        RECORD.append(f"| {what} | {name} against mixed_wave | {lk} | {e:.2e} | {allowed:.2e} | 2 x score {lc.score_term(p['S']):.2e} | |")
        print(f"    allowed {allowed:.2e} = 2 x score term {lc.score_term(p['S']):.2e}")
        assert e <= allowed


@pytest.mark.parametrize("lk", [32, 64, 256])
def test_shift_invariance_fused(dev, lk):
    _shift_invariance(dev, "fused", 1, 128, lk, 256, H3, FH2, False)


@pytest.mark.parametrize("lk", [48, 112])
@pytest.mark.parametrize("form", list(THREE_FORMS))
def test_shift_invariance_three_launch(dev, form, lk):
    _shift_invariance(dev, f"three launches {form}", 2, 64, lk, 32, *THREE_FORMS[form], True)


# ======================================================================================================================================
# dm3d_softmax_rows[_h2]: one pattern per row, every NE instantiation of softmax_rows_kernel (1, 4, 8, 16) and both streaming kernels
# ======================================================================================================================================
SOFTMAX_COLS = (8, 64, 100, 256, 512, 1024, 1040, 4112)


@pytest.mark.parametrize("cols,h2", [(cols, h2) for h2 in (False, True) for cols in SOFTMAX_COLS if not (h2 and cols % 16)])       # H2 rows: whole records
def test_softmax_rows(dev, cols, h2):
    entry = "dm3d_softmax_rows_h2" if h2 else "dm3d_softmax_rows"
    names, S = lc.softmax_rows_matrix(cols)
    ref = lc.softmax64(S)
    buf = Guarded.matrix(S.astype(np.float32), cols + 16, dev, OUT)              # in place: the scores are the output buffer
    ik._call(entry, buf.ptr, len(names), cols, cols + 16)
    raw = buf.get()[:, :cols]                                                    # pads and the ld gap intact
    got = np.asarray(h2_decode(raw) if h2 else raw, np.float64)
    assert np.isfinite(got).all()
    for i, n in enumerate(names):                                                # each row against the matrix's max |ref| (1: the one_hot rows), as test_softmax_rows does
        _within("softmax_rows", entry, n, got[i:i + 1], ref[i:i + 1], S[i:i + 1], h2, scale=float(ref.max()))
        if not h2:                                                               # float32 rows also against their OWN maximum (1 / cols for a flat row)
            _within("softmax_rows", entry + " per row", n, got[i:i + 1], ref[i:i + 1], S[i:i + 1], h2)
    # rows sum to 1: float32 within 1e-5; a DM3D_FMT_H2 element may be off by 2^-25 on top of that (tests/test_gpu_infer_kernels.py::test_softmax_rows)
    assert np.abs(got.sum(-1) - 1).max() < 1e-5 + (cols * lc.H2_FLOOR if h2 else 0.0)
    for i, n in enumerate(names):
        if n.startswith("flat"):
            words = raw[i].view(np.int16).reshape(-1, 2, 16) if h2 else raw[i].view(np.int32).reshape(1, 1, -1)      # H2 record: 16 hi, 16 lo
            assert (words == words[:1, :, :1]).all(), f"{n}: equal logits, unequal probabilities"
    # a common shift: the rows offset(+-64) are stairs_up(7.5) + 64 and stairs_down(8.5) - 64
    for shifted, plain in (("offset(+64)", "stairs_up(7.5)"), ("offset(-64)", "stairs_down(8.5)")):
        i, j = names.index(shifted), names.index(plain)
        e = ik._err(f"{entry} {shifted} against {plain}", got[i], got[j], float(ref.max()))
        assert e <= 2.0 * lc.score_term(S[i])

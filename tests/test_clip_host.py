"""CPU tier of global-norm clipping and gradient accumulation: the dm3d_grad_scale / dm3d_adam_scaled ABI and its host checks, the
argument rules of compile(global_clipnorm=, grad_accum_steps=) and Trainer.set_clipping's cycle bookkeeping (no kernel is launched)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_entries_are_declared_exported_and_bound(built_library, tmp_path):
    from dm3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dm3d.h")).read()
    assert re.search(r"\bint\s+dm3d_grad_scale\s*\(const dm3d_gradscale_desc\* d, void\* stream\);", header)
    assert re.search(r"\bint\s+dm3d_adam_scaled\s*\(float\* w, const float\* g, float\* m, float\* v, float\* ema", header)
    handle = ctypes.CDLL(built_library)
    assert hasattr(handle, "dm3d_grad_scale") and hasattr(handle, "dm3d_adam_scaled")
    res, args = _lib.SIGNATURES["dm3d_grad_scale"]
    assert res is ctypes.c_int and len(args) == 2 and args[0]._type_ is _lib.GradScaleDesc and args[1] is ctypes.c_void_p
    res, args = _lib.SIGNATURES["dm3d_adam_scaled"]
    assert res is ctypes.c_int and len(args) == 13 and args[5] is ctypes.c_int64 and args[6:11] == [ctypes.c_float] * 5
    assert args[11] is ctypes.c_void_p and args[12] is ctypes.c_void_p
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111                         # additive: the version stays
    # the descriptor as the C compiler lays it out == the ctypes mirror, and the partial count is mirrored
    fields = ("g", "n", "partials", "state", "clip_norm", "pre_scale")
    assert fields == tuple(n for n, _ in _lib.GradScaleDesc._fields_)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dm3d.h"\nint main(void){printf("%d %zu' + " %zu" * len(fields)
                   + '\\n", DM3D_GRADNORM_PARTIAL_BLOCKS, sizeof(dm3d_gradscale_desc), '
                   + ", ".join(f"offsetof(dm3d_gradscale_desc, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert vals[0] == _lib.GRADNORM_PARTIAL_BLOCKS == 1024
    assert vals[1] == ctypes.sizeof(_lib.GradScaleDesc) == 40
    assert vals[2:] == [getattr(_lib.GradScaleDesc, f).offset for f in fields]


def _refused(lib, entry, call, cases):
    failures = []
    for what, args in cases:
        lib.dm3d_fill(None, 0, 0.0, None)                           # leaves a known message behind
        stale = lib.dm3d_last_error()
        rc = call(args)
        msg = lib.dm3d_last_error()
        if rc != -1 or not msg or msg == stale or entry.encode() not in msg:
            failures.append(f"dm3d_{entry}({what}): rc {rc}, message {msg!r}")
    return failures


def test_grad_scale_refuses_bad_arguments(built_library):
    """Every documented precondition is checked before anything is launched: DM3D_EINVAL and a fresh message naming the entry, with no
    GPU in the machine (the pointers are made-up addresses nothing may dereference)."""
    from dm3d_amd import _lib
    lib = _lib.lib()
    ptrs = dict(g=0x10000, partials=0x20000, state=0x30000)
    ok = dict(**ptrs, n=1024, clip_norm=1.0, pre_scale=1.0)
    bad = [(f"{k} null", {k: None}) for k in ptrs] + [(f"{k} misaligned", {k: ptrs[k] + 4}) for k in ptrs]
    bad += [(f"n = {n}", dict(n=n)) for n in (0, 6, -4)]
    bad += [(f"clip_norm {c}", dict(clip_norm=c)) for c in (0.0, -1.0, NAN)]
    bad += [(f"pre_scale {p}", dict(pre_scale=p)) for p in (0.0, -1.0, NAN, INF)]

    def call(override):
        d = _lib.GradScaleDesc()
        for k, v in {**ok, **override}.items():
            setattr(d, k, v)
        return lib.dm3d_grad_scale(ctypes.byref(d), None)

    failures = _refused(lib, "grad_scale", call, bad)
    failures += _refused(lib, "grad_scale", lambda _: lib.dm3d_grad_scale(None, None), [("null descriptor", None)])
    assert not failures, "\n".join(failures)


def test_adam_scaled_refuses_bad_arguments(built_library):
    """As test_adam_ema_refuses_bad_arguments, with ``state`` beside the five buffers.  ema = NULL is no error: with every other
    argument in order the argument checks pass, which shows here as the refusal of the NEXT bad argument (n) instead of ema's."""
    from dm3d_amd import _lib
    lib = _lib.lib()
    ptrs = dict(w=0x10000, g=0x20000, m=0x30000, v=0x40000, ema=0x50000, state=0x60000)
    ok = dict(**ptrs, n=1024, lr_t=1e-4, beta1=0.9, beta2=0.999, eps=1e-7, ema_rate=0.1)
    bad = [(f"{k} null", {k: None}) for k in ptrs if k != "ema"] + [(f"{k} misaligned", {k: ptrs[k] + 4}) for k in ptrs]
    bad += [(f"n = {n}", dict(n=n)) for n in (0, 6, -4)]
    bad += [(f"ema_rate {r}", dict(ema_rate=r)) for r in (-0.1, 1.5, NAN, INF)]
    bad += [("ema == w", dict(ema=ptrs["w"])), ("ema == g", dict(ema=ptrs["g"])), ("ema == m", dict(ema=ptrs["m"])),
            ("ema == v", dict(ema=ptrs["v"])), ("ema inside w", dict(ema=ptrs["w"] + 16)), ("ema ends inside v", dict(ema=ptrs["v"] - 16, n=8))]
    bad += [(f"state inside {k}", dict(state=ptrs[k] + 32)) for k in ("w", "m", "v", "ema")]
    bad += [("state == w, no ema", dict(state=ptrs["w"], ema=None)), ("state is the end of m", dict(state=ptrs["m"] + 4 * 1024 - 16))]

    def call(override):
        a = {**ok, **override}
        return lib.dm3d_adam_scaled(a["w"], a["g"], a["m"], a["v"], a["ema"], a["n"], a["lr_t"], a["beta1"], a["beta2"], a["eps"],
                                    a["ema_rate"], a["state"], None)

    failures = _refused(lib, "adam_scaled", call, bad)
    assert not failures, "\n".join(failures)
    # ema = NULL passes the pointer checks: the message is the one about n, not one about a null or overlapping pointer
    lib.dm3d_fill(None, 0, 0.0, None)
    assert call(dict(ema=None, n=6)) == -1
    msg = lib.dm3d_last_error()
    assert b"adam_scaled: n=6" in msg, msg
    assert call(dict(ema=None, ema_rate=2.0)) == -1 and b"ema_rate" in lib.dm3d_last_error()


def test_compile_rules_for_clipping_and_accumulation():
    from test_ema_host import _model
    m = _model(context_dim=2)
    assert (m._global_clipnorm, m._grad_accum_steps) == (None, 1)
    m.compile(optimizer=1e-3, ema_decay=0.5, global_clipnorm=2.0, grad_accum_steps=3)
    kept = (m.optimizer, m._ema_decay, m._global_clipnorm, m._grad_accum_steps)
    assert kept == (1e-3, 0.5, 2.0, 3) and isinstance(m._grad_accum_steps, int)
    for kw in ([dict(global_clipnorm=c) for c in (0, -1, NAN, INF)] + [dict(grad_accum_steps=k) for k in (0, -1, 1.5, True)]):
        with pytest.raises(ValueError):
            m.compile(optimizer=7e-3, ema_decay=0.9, **kw)
        assert (m.optimizer, m._ema_decay, m._global_clipnorm, m._grad_accum_steps) == kept, kw       # a refused compile() changes nothing
    m.compile(global_clipnorm=0.5)
    assert (m._global_clipnorm, m._grad_accum_steps, m._ema_decay) == (0.5, 1, None)
    m.compile(grad_accum_steps=4)
    assert (m._global_clipnorm, m._grad_accum_steps) == (None, 4)
    m.compile()                                                                               # the defaults switch both off again
    assert (m._global_clipnorm, m._grad_accum_steps) == (None, 1)
    assert m._training_settings() == (1e-4, None, True)                                       # the tuple's shape is as before


def test_accumulation_cycle_bookkeeping():
    """Trainer.set_clipping / micro_step / micro_step_done on a bare object (no device): call j of k adds iff j > 0 and ends the cycle
    iff j = k - 1; a call that never reports done is not counted; a change of k in mid-cycle waits for the next cycle; the rules are
    compile()'s."""
    from dm3d_amd.train import Trainer
    tr = object.__new__(Trainer)
    tr.accum_pos, tr.cycle_steps = 0, 1

    def call():
        place = tr.micro_step()
        tr.micro_step_done()
        return place
    tr.set_clipping()
    assert (tr.global_clipnorm, tr.accum_steps, tr.cycle_steps) == (None, 1, 1)
    assert [call() for _ in range(2)] == [(False, True)] * 2
    tr.set_clipping(1.0, 3)
    assert (tr.global_clipnorm, tr.cycle_steps) == (1.0, 3)
    assert [call() for _ in range(4)] == [(False, False), (True, False), (True, True), (False, False)]
    assert tr.micro_step() == tr.micro_step() == (True, False) and tr.accum_pos == 1       # a call that raised is taken again
    tr.set_clipping(None, 2)                                        # in mid-cycle (one call of three done): the cycle keeps its k
    assert (tr.accum_steps, tr.cycle_steps) == (2, 3)
    assert [call() for _ in range(4)] == [(True, False), (True, True), (False, False), (True, True)]
    assert tr.cycle_steps == 2
    for bad in (dict(global_clipnorm=0.0), dict(global_clipnorm=INF), dict(global_clipnorm=NAN), dict(accum_steps=0), dict(accum_steps=2.5)):
        with pytest.raises(ValueError):
            tr.set_clipping(**bad)
    assert (tr.global_clipnorm, tr.accum_steps) == (None, 2)

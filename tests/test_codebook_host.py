"""CPU tier of the codebook entries (no kernel is launched): dm3d_code_stats, dm3d_code_usage, dm3d_codebook_ema and
dm3d_codebook_replace are declared, exported and bound and refuse every documented bad argument; csrc/dm3d_codebook.hip compiles for
gfx950 without spill or scratch; the numpy restatement the GPU tests compare against (tests/codebook_reference.py) meets closed forms
and math.fsum; the shuffle is a permutation; the chain of the EMA tests keeps its assignments apart; the Python wrappers refuse what
they document."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import codebook_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 0x10000                                   # an aligned non-null "pointer": nothing is launched, so nothing dereferences it
ENTRIES = {"code_stats": "dm3d_code_stats", "code_usage": "dm3d_code_usage", "codebook_ema": "dm3d_codebook_ema",
           "codebook_replace": "dm3d_codebook_replace"}
ALL = tuple(ENTRIES)
STATS, USAGE, EMA, REPLACE = (("code_stats",), ("code_usage",), ("codebook_ema",), ("codebook_replace",))
DIMMED = ("code_stats", "codebook_ema", "codebook_replace")

# rows 10, dim 8, k 12: z 320 bytes, idx 40, counts 48, sums 768, codebook and ema_w 384, the vectors over k 48
OK = dict(z=A, idx=A + 0x1000, rows=10, dim=8, k=12, counts=A + 0x2000, sums=A + 0x3000, invalid=A + 0x4000, eps=1e-10,
          perplexity=A + 0x5000, active=A + 0x6000, used_accum=A + 0x7000, cluster_size=A + 0x8000, ema_w=A + 0x9000, codebook=A + 0xA000,
          esq=A + 0xB000, decay=0.99, epsilon=1e-5, used=A + 0xC000, num_batches=10, draw=0, threshold=0.01, noise_scale=1e-12, seed=7,
          used_count=A + 0xD000, unused_count=A + 0xE000, map=A + 0xF000)
BAD = [
    (ALL, dict(k=0), "k=0 (at least 1)"), (ALL, dict(k=4097), "k=4097 exceeds DM3D_CODEBOOK_MAX_K=4096"),
    (DIMMED, dict(dim=0), "dim=0 (at least 4)"), (DIMMED, dict(dim=1028), "dim=1028 exceeds DM3D_CODEBOOK_MAX_DIM=1024"),
    (DIMMED, dict(dim=6), "dim=6 must be a multiple of 4"),
    (STATS + USAGE, dict(rows=0), "rows=0 (at least 1)"), (STATS + USAGE, dict(rows=(1 << 30) + 1), "rows=1073741825 exceeds DM3D_CODEBOOK_MAX_ROWS=1073741824"),
    (STATS, dict(z=0), "z must be non-null"), (STATS, dict(idx=0), "idx must be non-null"), (STATS, dict(counts=0), "counts must be non-null"),
    (STATS, dict(sums=0), "sums must be non-null"), (STATS, dict(invalid=0), "invalid must be non-null"),
    (STATS, dict(z=A + 2), "z must be 4-byte aligned"), (STATS, dict(idx=A + 0x1001), "idx must be 4-byte aligned"),
    (STATS, dict(sums=A + 0x3004), "sums must be 8-byte aligned"), (STATS, dict(counts=A + 0x2002), "counts must be 4-byte aligned"),
    (STATS, dict(counts=A + 316), "z overlaps counts"), (STATS, dict(sums=A + 0x1000 + 32), "idx overlaps sums"),
    (STATS, dict(invalid=A + 0x3000 + 764), "sums overlaps invalid"), (STATS, dict(invalid=A + 0x2000 + 44), "counts overlaps invalid"),
    (USAGE, dict(eps=-1.0), "eps=-1 (at least 0)"), (USAGE, dict(eps=float("nan")), "eps=nan"),
    (USAGE, dict(counts=0), "counts must be non-null"), (USAGE, dict(perplexity=0), "perplexity must be non-null"),
    (USAGE, dict(active=0), "active must be non-null"), (USAGE, dict(perplexity=A + 0x5004), "perplexity must be 8-byte aligned"),
    (USAGE, dict(used_accum=A + 0x7001), "used_accum must be 4-byte aligned"), (USAGE, dict(used_accum=A + 0x2000 + 44), "counts overlaps used_accum"),
    (USAGE, dict(active=A + 0x5004), "perplexity overlaps active"),
    (EMA, dict(decay=1.5), "decay=1.5 (0 to 1)"), (EMA, dict(decay=-0.1), "decay=-0.1 (0 to 1)"), (EMA, dict(decay=float("nan")), "decay=nan"),
    (EMA, dict(epsilon=-1.0), "epsilon=-1 (at least 0)"),
    (EMA, dict(counts=0), "counts must be non-null"), (EMA, dict(sums=0), "sums must be non-null"), (EMA, dict(cluster_size=0), "cluster_size must be non-null"),
    (EMA, dict(ema_w=0), "ema_w must be non-null"), (EMA, dict(codebook=0), "codebook must be non-null"), (EMA, dict(esq=0), "esq must be non-null"),
    (EMA, dict(ema_w=A + 0x9004), "ema_w must be 16-byte aligned"), (EMA, dict(codebook=A + 0xA008), "codebook must be 16-byte aligned"),
    (EMA, dict(sums=A + 0x3004), "sums must be 8-byte aligned"), (EMA, dict(esq=A + 0xB002), "esq must be 4-byte aligned"),
    (EMA, dict(codebook=A + 0x9000 + 368), "ema_w overlaps codebook"), (EMA, dict(esq=A + 0x3000 + 764), "sums overlaps esq"),
    (EMA, dict(cluster_size=A + 0x2000 + 44), "counts overlaps cluster_size"), (EMA, dict(esq=A + 0xA000), "codebook overlaps esq"),
    (REPLACE, dict(num_batches=0), "num_batches=0 (at least 1)"), (REPLACE, dict(threshold=float("nan")), "threshold is NaN"),
    (REPLACE, dict(noise_scale=float("inf")), "noise_scale must be finite"), (REPLACE, dict(noise_scale=float("nan")), "noise_scale must be finite"),
    (REPLACE, dict(ema_w=0), "cluster_size and ema_w are given together or not at all"),
    (REPLACE, dict(cluster_size=0), "cluster_size and ema_w are given together or not at all"),
    (REPLACE, dict(codebook=0), "codebook must be non-null"), (REPLACE, dict(esq=0), "esq must be non-null"), (REPLACE, dict(used=0), "used must be non-null"),
    (REPLACE, dict(used_count=0), "used_count must be non-null"), (REPLACE, dict(unused_count=0), "unused_count must be non-null"),
    (REPLACE, dict(map=0), "map must be non-null"), (REPLACE, dict(codebook=A + 0xA004), "codebook must be 16-byte aligned"),
    (REPLACE, dict(map=A + 0xF002), "map must be 4-byte aligned"), (REPLACE, dict(ema_w=A + 0x9008), "ema_w must be 16-byte aligned"),
    (REPLACE, dict(map=A + 0xC000 + 44), "used overlaps map"), (REPLACE, dict(unused_count=A + 0xD000), "used_count overlaps unused_count"),
    (REPLACE, dict(esq=A + 0xA000 + 380), "codebook overlaps esq"), (REPLACE, dict(ema_w=A + 0xA000 - 368), "codebook overlaps ema_w"),
    (REPLACE, dict(cluster_size=A + 0xF000 + 44), "map overlaps cluster_size"),
]


def _desc(_lib, **override):
    d = _lib.CodebookDesc()
    for k, v in {**OK, **override}.items():
        setattr(d, k, v)
    return d


def test_entries_are_declared_exported_and_bound(built_library, tmp_path):
    from dm3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dm3d.h")).read()
    handle = C.CDLL(built_library)
    for name in ENTRIES.values():
        assert re.search(r"\bint %s\(const dm3d_codebook_desc\* d, void\* stream\);" % name, header), name
        assert hasattr(handle, name), name
        assert _lib.SIGNATURES[name] == (C.c_int, [C.POINTER(_lib.CodebookDesc), C.c_void_p]), name
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111 and "#define DM3D_VERSION 111 " in header
    # the ctypes mirror has the header's fields, in its order, with its types
    body = re.search(r"typedef struct dm3d_codebook_desc \{(.*?)\} dm3d_codebook_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in (s.strip() for s in body.split(";")):
        if decl:
            ctype, names = decl.removeprefix("const ").split(" ", 1)
            fields += [(n.strip(" *"), ctype + ("*" if "*" in ctype + names else "")) for n in names.split(",")]
    kinds = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
    assert [f[0] for f in fields] == [f[0] for f in _lib.CodebookDesc._fields_]
    for (name, ctype), (_, mirror) in zip(fields, _lib.CodebookDesc._fields_):
        assert mirror is (C.c_void_p if ctype.endswith("*") else kinds[ctype]), (name, ctype, mirror)
    for name, value in (("MAX_K", 4096), ("MAX_DIM", 1024), ("MAX_ROWS", 1 << 30), ("SLICE", 64), ("BATCH", 16)):
        assert f"#define DM3D_CODEBOOK_{name} {value}\n" in header and getattr(_lib, "CODEBOOK_" + name) == value, name
    assert (cr.MAX_K, cr.MAX_DIM, cr.MAX_ROWS) == (_lib.CODEBOOK_MAX_K, _lib.CODEBOOK_MAX_DIM, _lib.CODEBOOK_MAX_ROWS)
    for name, value in (("DM3D_STREAM_CODEBOOK", cr.STREAM_CODEBOOK), ("DM3D_STREAM_CODEBOOK_SHUFFLE", cr.STREAM_CODEBOOK_SHUFFLE)):
        assert f"#define {name} 0x{value:X}\n" in header, name
    assert (_lib.STREAM_CODEBOOK, _lib.STREAM_CODEBOOK_SHUFFLE) == (cr.STREAM_CODEBOOK, cr.STREAM_CODEBOOK_SHUFFLE)
    from oracle import ref_philox
    taken = {v for n, v in vars(ref_philox).items() if n.startswith("STREAM_") and not n.startswith("STREAM_ID")} | {_lib.STREAM_AUGMENT}
    assert not {cr.STREAM_CODEBOOK, cr.STREAM_CODEBOOK_SHUFFLE} & taken                    # no other entry shares a draw
    # the mirror's size is the compiler's
    cc = next((p for p in ("/usr/bin/cc", "/usr/bin/gcc", "/usr/bin/clang", "/opt/rocm/llvm/bin/clang") if os.path.exists(p)), None)
    if cc is not None:
        import subprocess
        src, exe = tmp_path / "size.c", tmp_path / "size"
        src.write_text('#include <stdio.h>\n#include "dm3d.h"\nint main(void) { printf("%zu\\n", sizeof(dm3d_codebook_desc)); return 0; }\n')
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        assert int(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout) == C.sizeof(_lib.CodebookDesc)
    assert C.sizeof(_lib.CodebookDesc) == 192


def test_entries_refuse_bad_arguments(built_library):
    """Every documented precondition is checked before anything is launched: DM3D_EINVAL and a message that starts with the entry's short
    name and names the fault, with no GPU in the machine."""
    from dm3d_amd import _lib
    lib = _lib.lib()
    failures = []
    for entries, override, words in BAD:
        for short in entries:
            lib.dm3d_fill(None, 0, 0.0, None)                       # leaves a known message behind
            rc = getattr(lib, ENTRIES[short])(C.byref(_desc(_lib, **override)), None)
            msg = (lib.dm3d_last_error() or b"").decode()
            if rc != -1 or not msg.startswith(short + ":") or words not in msg:
                failures.append(f"{ENTRIES[short]}({override}): rc {rc}, message {msg!r}, wanted {words!r}")
    for short, name in ENTRIES.items():
        if getattr(lib, name)(None, None) != -1 or f"{short}: null descriptor".encode() not in lib.dm3d_last_error():
            failures.append(f"{name}(NULL)")
    assert not failures, "\n".join(failures)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_codebook_kernels_compile_without_spill_or_scratch(tmp_path):
    """The gfx950 listing of csrc/dm3d_codebook.hip (the library's flags), read by its metadata alone: every kernel is there, none with
    a spilled register or a private segment, each within the 64 KiB of static LDS."""
    import subprocess
    out = str(tmp_path / "dm3d_codebook.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function",
                    "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(ROOT, "3d-condtional-stable-diffusion_amd", "csrc", "dm3d_codebook.hip"),
                    "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    rows = re.findall(r"\.group_segment_fixed_size:\s+(\d+)[\s\S]*?\.name:\s+(\S+)[\s\S]*?\.private_segment_fixed_size:\s+(\d+)[\s\S]*?"
                      r"\.sgpr_spill_count:\s+(\d+)[\s\S]*?\.vgpr_spill_count:\s+(\d+)", text)
    names = [r[1] for r in rows]
    kernels = ["code_stats_kernel", "code_usage_kernel", "codebook_ema_kernel", "replace_plan_kernel", "replace_apply_kernel"]
    for k in kernels:
        assert any(k in n for n in names), (k, names)
    assert len(rows) == len(kernels), names
    assert all(int(a) == 0 and int(b) == 0 and int(c) == 0 for _, _, a, b, c in rows), rows
    assert all(int(lds) <= 64 * 1024 for lds, *_ in rows), rows


# ---- the restatement against closed forms ------------------------------------------------------------------------------------------------
def test_dlog_and_dexp_are_a_log_and_an_exp():
    """The stated operations against the host's libm (itself within an ulp) at 1e-15 relative, over what dm3d_code_usage feeds them:
    p + eps in [1e-10, 1 + 1e-10] and -sum in [0, log 4096]."""
    rng = np.random.default_rng(0)
    xs = np.concatenate([10.0 ** rng.uniform(-10, 0, 20000), [1e-10, 1.0, 1.0 + 1e-10, 0.5, cr.SQRT_HALF, np.nextafter(cr.SQRT_HALF, 0)]])
    for x in xs.tolist():
        want = math.log(x)
        assert abs(cr.dlog(x) - want) <= 1e-15 * abs(want) + (1e-26 if x == 1.0 else 0.0), x
    assert cr.dlog(1.0) == 0.0
    for y in np.concatenate([rng.uniform(-1e-6, math.log(4096.0), 20000), [0.0, math.log(4096.0), 0.5 * cr.LN2]]).tolist():
        assert abs(cr.dexp(y) - math.exp(y)) <= 1e-15 * math.exp(y), y
    assert cr.dexp(0.0) == 1.0


def test_usage_closed_forms():
    for k in (1, 5, 33, 512, 4096):
        perp, active = cr.code_usage(np.full(k, 3, np.int32), 3 * k)                    # uniform usage: perplexity K
        assert abs(perp - k) <= 1e-12 * k + 1e-8 * k * k and active == k, (k, perp)    # eps = 1e-10 inside the log moves it by K^2 eps
        one = np.zeros(k, np.int32)
        one[k // 2] = 700
        perp, active = cr.code_usage(one, 700)                                          # one code: perplexity 1
        assert abs(perp - 1.0) <= 1e-9 and active == 1, (k, perp)
    perp, active = cr.code_usage(np.full(64, 2, np.int32), 128, eps=0.0)
    assert abs(perp - 64.0) <= 64 * 1e-14 and active == 64


def test_stats_closed_forms_and_fsum():
    """A constant member set sums to count * v exactly while count * v is representable; every sum is within count * 2^-52 of math.fsum,
    relative to the sum of the absolute values (n - 1 sequential adds err by at most (n - 1) * 2^-53 of it: Higham, Accuracy and
    Stability of Numerical Algorithms, 4.2).  A float32 accumulation of the offset case misses that bar a thousand times over."""
    v = np.array([0.5, -3.25, 1000.0, 2.0 ** -20], np.float32)
    idx = np.array([2, 0, 2, 2, 1, 2, -1, 3, 2], np.int32)
    counts, sums, invalid = cr.code_stats(np.tile(v, (9, 1)), idx, 3)
    assert counts.tolist() == [1, 1, 5] and invalid == 2
    assert np.array_equal(sums, counts[:, None].astype(np.float64) * v.astype(np.float64))
    counts, sums, _ = cr.code_stats(np.tile(v, (9, 1)), idx, 5)
    assert counts.tolist() == [1, 1, 5, 1, 0] and not sums[4].any()
    for shape in cr.SHAPES:
        for kind in cr.KINDS:
            z, idx = cr.stats_case(shape, kind)
            k = shape[2]
            counts, sums, invalid = cr.code_stats(z, idx, k)
            valid = (idx >= 0) & (idx < k)
            assert counts.sum() + invalid == shape[0] and np.array_equal(counts, np.bincount(idx[valid], minlength=k))
            if kind == "empty":
                assert counts[1] == 0 and not sums[1].any()
            if kind == "one":
                assert counts[k // 2] == shape[0] and (np.delete(counts, k // 2) == 0).all()
            if kind == "invalid":
                assert invalid >= shape[0] // 7
            for c in np.flatnonzero(counts)[:8].tolist() + [int(counts.argmax())]:
                rows = z[idx == c].astype(np.float64)
                for f in (0, shape[1] - 1):
                    exact, scale = math.fsum(rows[:, f].tolist()), math.fsum(np.abs(rows[:, f]).tolist())
                    assert abs(sums[c, f] - exact) <= counts[c] * 2.0 ** -52 * scale, (shape, kind, c, f)
            if kind == "offset":                                                        # what a float32 accumulation would lose
                c = int(counts.argmax())
                f32 = np.cumsum(z[idx == c], axis=0, dtype=np.float32)[-1]
                assert np.abs(f32.astype(np.float64) - sums[c]).max() > 1e3 * counts[c] * 2.0 ** -52 * np.abs(sums[c]).max()


def test_ema_restatement_against_the_literal_rule():
    """One update on random state: wherever N' > 0 the restatement is the literal float64 rule within float32 rounding; N' == 0 keeps row
    and esq; esq is numpy's (emb ** 2).sum(axis=0, dtype=float32) on the [D, K] layout."""
    for shape in cr.SHAPES:
        z, idx = cr.ema_stats_case(shape)
        size, ema_w, book, esq = cr.ema_state(shape)
        counts, sums, _ = cr.code_stats(z, idx, shape[2])
        n_size, n_w, n_book, n_esq = cr.codebook_ema(size, ema_w, book, esq, counts, sums, 0.99, 1e-5)
        dead = n_size == 0
        assert dead[0] and dead[-1] and dead.sum() == 2
        assert np.array_equal(n_book[dead], book[dead]) and np.array_equal(n_esq[dead], esq[dead]) and np.isfinite(n_book).all()
        live = ~dead
        valid = (idx >= 0) & (idx < shape[2])
        l_size, l_w, l_emb = cr.ema_literal(size[live], ema_w[live].T, book[live].T, z[valid], np.searchsorted(np.flatnonzero(live), idx[valid]),
                                            0.99, 1e-5, np.float64)
        assert np.allclose(n_size[live], l_size, rtol=1e-6, atol=0) and np.allclose(n_w[live], l_w.T, rtol=1e-5, atol=1e-6)
        assert np.allclose(n_book[live], l_emb.T, rtol=1e-5, atol=1e-6)
        emb = np.ascontiguousarray(n_book.T)
        assert np.array_equal(n_esq[live], (emb ** 2).sum(axis=0, dtype=np.float32)[live])


def test_chain_keeps_its_assignments_apart():
    """The input condition of the chained EMA test: on exactly its inputs the float64 literal chain's smallest relative gap between the
    best and the second-best distance, over every row of every step, stays above 0.05, so no assignment can flip between float32 and
    float64; the float32 chain picks the same indices, and every code is used in every step."""
    assert (cr.CHAIN_STEPS, cr.CHAIN_K, cr.CHAIN_DIM, cr.CHAIN_ROWS, cr.CHAIN_DECAY, cr.CHAIN_GAP) == (6, 16, 8, 512, 0.9, 0.05)
    c64, c32 = cr.literal_chain(np.float64), cr.literal_chain(np.float32)
    for step, ((i64, gap, e64), (i32, _, e32)) in enumerate(zip(c64, c32)):
        print(f"step {step}: smallest relative gap {gap:.4f}, float32 against float64 literal {np.abs(e32 - e64).max():.3e}")
        assert gap > cr.CHAIN_GAP, (step, gap)
        assert np.array_equal(i64, i32) and len(set(i64.tolist())) == cr.CHAIN_K
    # the restatement in the stated order follows the same chain
    batches, codebook = cr.chain_inputs()
    state = cr.chain_start(codebook)
    for z, (i64, _, e64) in zip(batches, c64):
        idx, _ = cr.assign(z, state[2].T)
        assert np.array_equal(idx, i64)
        counts, sums, _ = cr.code_stats(z, idx, cr.CHAIN_K)
        state = cr.codebook_ema(*state, counts, sums, cr.CHAIN_DECAY, cr.CHAIN_EPSILON)
        assert np.abs(state[2].T - e64).max() < 1e-5


def test_shuffle_is_a_permutation_and_the_plan_follows_the_branches():
    for entries in (1, 2, 30, 1020, 4096):
        order = cr.shuffle_order(entries, 0, 7)
        assert sorted(order.tolist()) == list(range(entries))
        assert np.array_equal(order, cr.shuffle_order(entries, 0, 7))
        if entries > 2:
            assert not np.array_equal(order, np.arange(entries)) and not np.array_equal(order, cr.shuffle_order(entries, 1, 7))
            assert not np.array_equal(order, cr.shuffle_order(entries, 0, 8))
    for k in (33, 1024):
        for kind in ("most", "few", "none"):
            used = cr.used_case(k, kind)
            plan, nu, nv = cr.replace_plan(used, 10, 0.01, 0, 7)
            dead = used == 0
            assert nu == (~dead).sum() and nv == dead.sum() and nu + nv == k
            if kind == "none":
                assert nu == 0 and np.array_equal(plan, np.arange(k))
                continue
            assert (plan[~dead] == -1).all() and (~dead)[plan[dead]].all()            # used rows stay; every source is a used code
            u, v = np.flatnonzero(~dead), np.flatnonzero(dead)
            if kind == "most":
                assert nu >= nv and np.array_equal(plan[v], u[:nv])
            else:
                assert 0 < nu < nv
                tiled = np.tile(u, nv // nu + 1)
                taken = np.sort(plan[v])                                                # a prefix of a permutation of the tiled list
                assert nv < tiled.size <= k and all((taken == c).sum() <= nv // nu + 1 for c in u)
                assert not np.array_equal(plan[v], tiled[:nv])


def test_python_wrappers_refuse_what_they_document():
    from dm3d_amd import codebook, ops
    from dm3d_amd.networks.vqvae3d_monai import VQVAE
    from dm3d_amd.networks.vqgan import VQGAN
    assert all(callable(getattr(ops, n)) for n in ("code_stats", "code_usage", "codebook_ema", "codebook_replace"))
    assert all(callable(getattr(cls, n)) for cls in (VQVAE, VQGAN) for n in ("fit_codebook", "codebook_usage"))
    z, idx = torch.zeros(10, 8), torch.zeros(10, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"z must be a float32 tensor \[rows, D\]"):
        ops.code_stats(torch.zeros(10), idx, 4)
    with pytest.raises(ValueError, match=r"z must be a float32 tensor \[rows, D\]"):
        ops.code_stats(z.double(), idx, 4)
    with pytest.raises(ValueError, match="K=4097 codes; 1 to 4096 are taken"):
        ops.code_stats(z, idx, 4097)
    with pytest.raises(ValueError, match="D=6; a multiple of 4 from 4 to 1024 is taken"):
        ops.code_stats(torch.zeros(10, 6), idx, 4)
    with pytest.raises(ValueError, match="D=1028; a multiple of 4 from 4 to 1024 is taken"):
        ops.code_stats(torch.zeros(10, 1028), idx, 4)
    with pytest.raises(ValueError, match="z must be a contiguous device tensor: the codebook kernels have no CPU path"):
        ops.code_stats(z, idx, 4)
    counts = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"counts must be an int32 tensor \[K\]"):
        ops.code_usage(torch.zeros(2, 2), 10)
    with pytest.raises(ValueError, match="rows must be an integer from 1 to 1073741824"):
        ops.code_usage(counts, 0)
    with pytest.raises(ValueError, match="eps must be at least 0"):
        ops.code_usage(counts, 10, eps=-1.0)
    with pytest.raises(ValueError, match=r"counts must be a int32 tensor \[4\], got torch.int64"):
        ops.code_usage(counts.long(), 10)
    with pytest.raises(ValueError, match="counts must be a contiguous device tensor"):
        ops.code_usage(counts, 10)
    book, esq, size = torch.zeros(4, 8), torch.zeros(4), torch.zeros(4)
    with pytest.raises(ValueError, match=r"codebook must be a float32 tensor \[K, D\]"):
        ops.codebook_ema(torch.zeros(4), esq, size, book, counts, torch.zeros(4, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"esq must be a float32 tensor \[4\]"):
        ops.codebook_ema(book, torch.zeros(5), size, book, counts, torch.zeros(4, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="codebook must be a contiguous device tensor"):
        ops.codebook_ema(book, esq, size, book.clone(), counts, torch.zeros(4, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="cluster_size and ema_w are given together or not at all"):
        ops.codebook_replace(book, esq, counts, 10, cluster_size=size)
    # the checks that follow the tensors' own: a stand-in that passes for a device tensor, so they are reached without a GPU
    from unittest import mock
    with mock.patch.object(ops, "_dev_tensor", lambda t, name, dtype, shape, device=True: t):
        with pytest.raises(ValueError, match=r"decay must lie in \[0, 1\], got 1.5"):
            ops.codebook_ema(book, esq, size, book.clone(), counts, torch.zeros(4, 8, dtype=torch.float64), decay=1.5)
        with pytest.raises(ValueError, match="epsilon must be at least 0"):
            ops.codebook_ema(book, esq, size, book.clone(), counts, torch.zeros(4, 8, dtype=torch.float64), epsilon=-1e-5)
        with pytest.raises(ValueError, match="num_batches must be an integer of at least 1, got 0"):
            ops.codebook_replace(book, esq, counts, 0)
        with pytest.raises(ValueError, match="noise_scale must be finite"):
            ops.codebook_replace(book, esq, counts, 10, noise_scale=float("inf"))
    with pytest.raises(ValueError, match="num_embeddings=5000; 1 to 4096 are taken"):
        codebook.EMACodebook(5000, 8)
    with pytest.raises(ValueError, match="embedding_dim=6; a multiple of 4 from 4 to 1024 is taken"):
        codebook.EMACodebook(16, 6)
    with pytest.raises(ValueError, match=r"decay must lie in \[0, 1\]"):
        codebook.EMACodebook(16, 8, decay=2.0)
    assert codebook.USAGE_EPS == cr.EPS == 1e-10 and codebook.NOISE_SCALE == 1e-12

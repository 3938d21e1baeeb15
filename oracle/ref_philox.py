"""Host reference of the N(0,1) stream the drawing kernels share (include/dm3d.h, "What seeded means"): Philox4x32-10 written from the
paper (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) in numpy uint64 arithmetic, the float32
uniform mapping restated operation by operation, and Box-Muller with log, sqrt, cos and sin taken in float64.  numpy only.

A round of Philox4x32 maps the counter (c0, c1, c2, c3) under the key (k0, k1) to
    (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0)),     M0 = 0xD2511F53, M1 = 0xCD9E8D57,
and the key is bumped by the Weyl constants (0x9E3779B9, 0xBB67AE85) between rounds; ten rounds.  tests/test_philox_host.py holds
this to the known-answer vectors of the Random123 distribution.

`normal4(..., order="f64")` is what the GPU tests compare every drawn element with; order="f32" evaluates the four library calls in
numpy float32 instead (the host libm's roundings: orientation, not the device's bits)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

# word 3 of the counter: one constant per drawing entry, so that no two entries ever share a draw
STREAM_RANDN, STREAM_DDPM, STREAM_DDIM, STREAM_DPM_SDE, STREAM_EDIT = 0x5EED, 0xD1F0, 0xDD1A, 0x5DE2, 0xED17
# word 2 of the host's own dm3d_randn calls
STREAM_ID_X_T, STREAM_ID_TRAIN_NOISE = 0x7FFFFFFF, 0x7FFFFFFE

TWO_PI_F32 = np.float32(6.283185307179586)
TWO_M32_F32 = np.float32(2.0 ** -32)


def _u64(v):
    """A Python int or an array of non-negative integers below 2^32 as uint64 (negative int32 words are taken modulo 2^32)."""
    if isinstance(v, (int, np.integer)):
        return np.uint64(int(v) & MASK32)
    a = np.asarray(v)
    if a.dtype.kind == "i":
        a = a.astype(np.int64) & MASK32
    return a.astype(np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words and key words (ints or arrays below 2^32, broadcast together) -> four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(v) for v in (c0, c1, c2, c3, k0, k1)))
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                      # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def uniforms(c0, c1, c2, c3):
    """The four float32 uniforms of an output block: ((float)c + 0.5f) * 2^-32 in (0, 1] for the radius words 0 and 2,
    (float)c * 2^-32 in [0, 1] for the angle words 1 and 3; convert, add, multiply, each rounded to float32."""
    half = np.float32(0.5)
    f = [np.asarray(c, np.uint32).astype(np.float32) for c in (c0, c1, c2, c3)]
    return (f[0] + half) * TWO_M32_F32, f[1] * TWO_M32_F32, (f[2] + half) * TWO_M32_F32, f[3] * TWO_M32_F32


def box_muller(u0, u1, u2, u3, order="f64"):
    """[n, 4]: (r0 cos a1, r0 sin a1, r1 cos a3, r1 sin a3), r = sqrt(-2 log u), a = float32(2 pi) * u rounded to float32."""
    assert order in ("f64", "f32")
    a1, a3 = TWO_PI_F32 * np.asarray(u1, np.float32), TWO_PI_F32 * np.asarray(u3, np.float32)
    assert a1.dtype == np.float32 and a3.dtype == np.float32
    t = np.float64 if order == "f64" else np.float32
    u0, u2, a1, a3 = (np.asarray(v).astype(t) for v in (u0, u2, a1, a3))
    r0, r1 = np.sqrt(t(-2.0) * np.log(u0)), np.sqrt(t(-2.0) * np.log(u2))
    return np.stack([r0 * np.cos(a1), r0 * np.sin(a1), r1 * np.cos(a3), r1 * np.sin(a3)], -1)


def normal4(idx, s0, s1, seed, order="f64"):
    """Four N(0,1) draws for each 128-bit counter (idx low word, idx high word, s0, s1) under the 64-bit key `seed` (taken modulo
    2^64; low word first).  idx: uint64 array of float4 indices; s0 and s1: ints or arrays that broadcast against it.  Returns [n, 4],
    float64 (order "f64") or float32 (order "f32")."""
    idx = np.asarray(idx, np.uint64).reshape(-1)
    seed = int(seed) & (2 ** 64 - 1)
    c = philox4x32_10(idx & np.uint64(MASK32), idx >> np.uint64(32), s0, s1, seed & MASK32, seed >> 32)
    return box_muller(*uniforms(*c), order=order)


def _batched(batch, per_sample, word2, stream, seed, order):
    """z of [batch, per_sample]: float4 i of sample b has counter b * per4 + i; word2 is one int or one per sample."""
    assert per_sample % 4 == 0
    per4 = per_sample // 4
    idx = np.arange(batch * per4, dtype=np.uint64)
    w2 = np.repeat(_u64(np.broadcast_to(np.asarray(word2, np.int64), (batch,))), per4)
    return normal4(idx, w2, stream, seed, order).reshape(batch, per_sample)


def randn(n, seed, stream_id=0, order="f64"):
    """dm3d_randn: [n]."""
    assert n % 4 == 0
    return normal4(np.arange(n // 4, dtype=np.uint64), stream_id, STREAM_RANDN, seed, order).reshape(n)


def ddpm(batch, per_sample, t, seed, order="f64"):
    """dm3d_ddpm_update, mode 1: t the (clamped) timestep of each sample; a sample with t == 0 draws nothing (zeros)."""
    t = np.broadcast_to(np.asarray(t, np.int64), (batch,))
    z = _batched(batch, per_sample, t, STREAM_DDPM, seed, order)
    z[t == 0] = 0
    return z


def ddim(batch, per_sample, tau, seed, order="f64"):
    """dm3d_ddim_update[_frame]: tau the timestep each sample steps from, tau_table[clamp(pos[b])]."""
    return _batched(batch, per_sample, tau, STREAM_DDIM, seed, order)


def dpm_sde(batch, per_sample, tau, seed, order="f64"):
    """dm3d_dpm_sde_update[_frame]: as ddim, under its own stream constant."""
    return _batched(batch, per_sample, tau, STREAM_DPM_SDE, seed, order)


def edit(batch, per_sample, level, seed, order="f64"):
    """dm3d_edit_update: level the level timestep of each sample's row, (int32)levels[clamp(pos[b])][2]."""
    return _batched(batch, per_sample, level, STREAM_EDIT, seed, order)

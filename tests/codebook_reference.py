"""What the codebook tests share (plain helper, no test in it): a numpy restatement of dm3d_code_stats, dm3d_code_usage,
dm3d_codebook_ema and dm3d_codebook_replace in exactly the orders include/dm3d.h states, a second, literal restatement of the
reference's VectorQuantizerEMA update in TensorFlow's operation order (float32 and float64), and the inputs of the tests.

Orders.  np.cumsum is a sequential accumulation, so ``cumsum(..)[-1]`` is "one add at a time from 0"; elementwise numpy arithmetic on
float32 arrays rounds every operation to float32; dlog and dexp are written out in Python floats (IEEE doubles) operation by operation.
The one thing that cannot be restated to the bit is the N(0,1) draw of dm3d_codebook_replace, whose logf / sqrtf / sincosf are the device
library's: ``replace_plan`` gives everything up to the draw exactly, ``replace_noise`` the float64 draw of oracle/ref_philox.py, and the
tests hold a replaced row to ``row_bar`` (tests/philox_cases.py's bar on z, scaled, plus the two float32 roundings)."""
import math

import numpy as np

from oracle import ref_philox

MAX_K, MAX_DIM, MAX_ROWS = 4096, 1024, 1 << 30
STREAM_CODEBOOK, STREAM_CODEBOOK_SHUFFLE = 0xC0DE, 0xC0D5
EPS = 1e-10                                   # what _quantize adds inside the log
SHAPES = ((77, 4, 33), (513, 132, 128), (4099, 8, 1024), (3000, 64, 5))          # (rows, D, K)
KINDS = ("random", "empty", "one", "invalid", "offset")
F32, F64 = np.float32, np.float64


def shape_id(shape):
    return "x".join(str(v) for v in shape)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def stats_case(shape, kind):
    """(z float32 [rows, D], idx int32 [rows]) of one case.  "empty": code 1 has no member; "one": every row in one code; "invalid":
    every seventh row holds -1 or K; "offset": the values sit on 1000, so a float32 accumulation loses what a float64 one keeps."""
    rows, dim, k = shape
    rng = np.random.default_rng([rows, dim, k, KINDS.index(kind)])
    z = rng.standard_normal((rows, dim)).astype(F32)
    idx = rng.integers(0, k, rows).astype(np.int32)
    if kind == "empty":
        idx[idx == 1] = 0
    elif kind == "one":
        idx[:] = k // 2
    elif kind == "invalid":
        idx[::7] = np.where(np.arange(len(idx[::7])) % 2 == 0, -1, k)
        idx[3] = np.iinfo(np.int32).min
        idx[5] = np.iinfo(np.int32).max
    elif kind == "offset":
        z = (z + F32(1000.0)).astype(F32)
    return z, idx


def ema_state(shape, seed=0):
    """(cluster_size [K], ema_w [K, D], codebook [K, D], esq [K]) float32 to start an update from.  Codes 0 and K - 1 have cluster size 0."""
    _, dim, k = shape
    rng = np.random.default_rng([dim, k, seed, 77])
    size = rng.uniform(0.5, 40.0, k).astype(F32)
    size[0] = size[k - 1] = 0.0
    ema_w = rng.standard_normal((k, dim)).astype(F32)
    codebook = rng.standard_normal((k, dim)).astype(F32)
    return size, ema_w, codebook, esq_of(codebook)


def ema_stats_case(shape):
    """The random case with the rows of codes 0 and K - 1 moved to code 1 (so that, with ``ema_state``, N' is exactly 0 there)."""
    z, idx = stats_case(shape, "random")
    k = shape[2]
    if k > 2:
        idx[(idx == 0) | (idx == k - 1)] = 1
    return z, idx


# ---- dm3d_code_stats ----------------------------------------------------------------------------------------------------------------------
def code_stats(z, idx, k):
    """(counts int32 [k], sums float64 [k, D], invalid int32): sums[c] adds the member rows of c in ascending row order, one at a time."""
    z, idx = np.asarray(z, F32), np.asarray(idx, np.int32)
    counts, sums = np.zeros(k, np.int32), np.zeros((k, z.shape[1]), F64)
    for c in range(k):
        members = np.flatnonzero(idx == c)
        counts[c] = members.size
        if members.size:
            sums[c] = np.cumsum(z[members].astype(F64), axis=0)[-1]
    return counts, sums, np.int32(((idx < 0) | (idx >= k)).sum())


# ---- dm3d_code_usage ------------------------------------------------------------------------------------------------------------------------
SQRT_HALF = 0.70710678118654757
LN2, LN2_HI, LN2_LO, LOG2E = 0.69314718055994529, 0.693147180369123816490, 1.90821492927058770002e-10, 1.4426950408889634


def dlog(x):
    m, e = math.frexp(float(x))
    if m < SQRT_HALF:
        m, e = m * 2.0, e - 1
    s = (m - 1.0) / (m + 1.0)
    w = s * s
    p = 1.0 / 25.0
    for j in range(23, 2, -2):
        p = p * w + 1.0 / j
    p = p * w + 1.0
    return e * LN2 + (2.0 * s) * p


def dexp(y):
    y = float(y)
    n = float(np.rint(y * LOG2E))
    r = (y - n * LN2_HI) - n * LN2_LO
    q = 1.0 / math.factorial(14)
    for j in range(13, 0, -1):
        q = q * r + 1.0 / math.factorial(j)
    q = q * r + 1.0
    return math.ldexp(q, int(n))


def code_usage(counts, rows, eps=EPS):
    """(perplexity float64, active int32)."""
    s = 0.0
    for n in np.asarray(counts).tolist():
        p = float(n) / float(rows)
        s = s + p * dlog(p + eps)
    return F64(dexp(-s)), np.int32((np.asarray(counts) > 0).sum())


# ---- dm3d_codebook_ema ------------------------------------------------------------------------------------------------------------------------
def esq_of(codebook):
    """esq [K] of a [K, D] float32 codebook: float32, sequential in d, multiply and add rounded separately."""
    e = np.asarray(codebook, F32)
    return np.cumsum(e * e, axis=1, dtype=F32)[:, -1].astype(F32)


def codebook_ema(size, ema_w, codebook, esq, counts, sums, decay, epsilon):
    """The four arrays after one update ([K], [K, D], [K, D], [K], float32); the inputs are left alone."""
    decay, epsilon = F32(decay), F32(epsilon)
    om = F32(1.0) - decay
    size_new = (np.asarray(size, F32) * decay + om * np.asarray(counts).astype(F32)).astype(F32)
    w_new = (np.asarray(ema_w, F32) * decay + om * np.asarray(sums, F64).astype(F32)).astype(F32)
    n = np.cumsum(size_new.astype(F64))[-1]
    g = F32(n / (n + F64(epsilon)))
    live = size_new != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        e = ((w_new / size_new[:, None]).astype(F32) * g).astype(F32)
    book = np.where(live[:, None], e, np.asarray(codebook, F32)).astype(F32)
    return size_new, w_new, book, np.where(live, esq_of(book), np.asarray(esq, F32)).astype(F32)


def ema_literal(size, ema_w, emb, inputs, indices, decay, epsilon, dtype):
    """VectorQuantizerEMA.call's training branch (emavqvae.py:213-222) as TensorFlow evaluates it, in ``dtype``: [D, K] layouts, one-hot
    encodings, two matmuls, reduce_sum, and ((ema_w / cluster_size) * n) / (n + epsilon).  Returns (cluster_size, ema_w, embeddings)."""
    t = dtype
    k = emb.shape[1]
    encodings = np.eye(k, dtype=t)[np.asarray(indices)]
    flat = np.asarray(inputs).astype(t)
    size_new = np.asarray(size).astype(t) * t(decay) + t(1 - decay) * encodings.sum(axis=0, dtype=t)
    dw = flat.T @ encodings                                            # the reference's dw is [K, D] for an [D, K] ema_w; the transposed product is what its shapes need
    w_new = np.asarray(ema_w).astype(t) * t(decay) + t(1 - decay) * dw
    n = size_new.sum(dtype=t)
    emb_new = w_new / size_new.reshape(1, -1) * n / (n + t(epsilon))
    return size_new.astype(t), w_new.astype(t), emb_new.astype(t)


def assign(z, emb, dtype=F64):
    """(indices, smallest relative gap) of the reference's argmin over |z|^2 + |e|^2 - 2 z.e in ``dtype``; emb is [D, K].  The gap of a row
    is (second smallest - smallest) / second smallest distance."""
    z, emb = np.asarray(z).astype(dtype), np.asarray(emb).astype(dtype)
    dist = (z ** 2).sum(axis=1, keepdims=True) + (emb ** 2).sum(axis=0) - 2 * (z @ emb)
    two = np.partition(dist, 1, axis=1)[:, :2]
    return dist.argmin(axis=1).astype(np.int32), float(((two[:, 1] - two[:, 0]) / two[:, 1]).min())


# the chain of the EMA tests: six steps at decay 0.9
CHAIN_STEPS, CHAIN_K, CHAIN_DIM, CHAIN_ROWS, CHAIN_DECAY, CHAIN_EPSILON, CHAIN_GAP = 6, 16, 8, 512, 0.9, 1e-5, 0.05


def chain_inputs():
    """(batches [steps, rows, D] float32, codebook [K, D] float32): rows drawn 0.3 * noise around centres of scale 3, the codebook
    started 0.5 * noise from the centres."""
    rng = np.random.default_rng(20240611)
    centres = 3.0 * rng.standard_normal((CHAIN_K, CHAIN_DIM))
    owner = rng.integers(0, CHAIN_K, (CHAIN_STEPS, CHAIN_ROWS))
    batches = (centres[owner] + 0.3 * rng.standard_normal((CHAIN_STEPS, CHAIN_ROWS, CHAIN_DIM))).astype(F32)
    codebook = (centres + 0.5 * rng.standard_normal((CHAIN_K, CHAIN_DIM))).astype(F32)
    return batches, codebook


def chain_start(codebook):
    """What VQVAE.fit_codebook starts from for a given [K, D] codebook: cluster sizes 1, ema_w = the codebook."""
    book = np.asarray(codebook, F32)
    return np.ones(book.shape[0], F32), book.copy(), book.copy(), esq_of(book)


def literal_chain(dtype):
    """The literal restatement over the chain in ``dtype``: per step (indices, gap, embeddings [D, K] after the step)."""
    batches, codebook = chain_inputs()
    size, ema_w, emb = np.ones(CHAIN_K, dtype), codebook.T.astype(dtype), codebook.T.astype(dtype)
    out = []
    for z in batches:
        idx, gap = assign(z, emb, dtype)
        size, ema_w, emb = ema_literal(size, ema_w, emb, z, idx, CHAIN_DECAY, CHAIN_EPSILON, dtype)
        out.append((idx, gap, emb))
    return out


# ---- dm3d_codebook_replace ----------------------------------------------------------------------------------------------------------------------
def shuffle_order(entries, draw, seed):
    """The order the tiled list of ``entries`` entries is read in: positions sorted ascending by (Philox key, position)."""
    seed = int(seed) & (2 ** 64 - 1)
    key = ref_philox.philox4x32_10(np.arange(entries, dtype=np.uint64), 0, int(draw) & 0xFFFFFFFF, STREAM_CODEBOOK_SHUFFLE, seed & 0xFFFFFFFF, seed >> 32)[0]
    return np.lexsort((np.arange(entries), key.astype(np.uint64)))


def replace_plan(used, num_batches, threshold, draw, seed):
    """(map int32 [K], used_count, unused_count): map[c] is the source of c, c itself where only noise is added, -1 where the row stays."""
    used = np.asarray(used, np.int32)
    k = used.size
    dead = used.astype(F64) / F64(num_batches) < F64(threshold)
    u, v = np.flatnonzero(~dead), np.flatnonzero(dead)
    plan = np.full(k, -1, np.int32)
    if u.size == 0:
        plan[:] = np.arange(k)
    elif u.size >= v.size:
        plan[v] = u[:v.size]
    else:
        tiled = np.tile(u, v.size // u.size + 1)
        assert v.size < tiled.size <= k
        plan[v] = tiled[shuffle_order(tiled.size, draw, seed)][:v.size]
    return plan, np.int32(u.size), np.int32(v.size)


def replace_noise(k, dim, draw, seed):
    """z [K, D] float64: the N(0,1) draw of every element, float4 c * (D / 4) + f / 4 under the counter (index, draw, DM3D_STREAM_CODEBOOK)."""
    assert dim % 4 == 0
    return ref_philox.normal4(np.arange(k * dim // 4, dtype=np.uint64), int(draw) & 0xFFFFFFFF, STREAM_CODEBOOK, seed).reshape(k, dim)


def replace_rows(codebook, plan, noise_scale, draw, seed):
    """The [K, D] float64 codebook a replacement aims at: codebook[map[c]] + float32(noise_scale) * z[c] where map[c] >= 0."""
    book = np.asarray(codebook, F32).astype(F64)
    z = replace_noise(book.shape[0], book.shape[1], draw, seed)
    out = book.copy()
    hit = plan >= 0
    out[hit] = book[plan[hit]] + F64(F32(noise_scale)) * z[hit]
    return out


def row_bar(codebook, noise_scale, z_bar):
    """The bar on |device row - replace_rows| per element: the draw's own bar scaled, the product's rounding (relative 2^-24 of a value
    below 8 |noise_scale|: |z| < 8 for float32 Box-Muller) and the sum's rounding (half an ulp of a value below max|row| + 8 |noise_scale|)."""
    s = abs(float(F32(noise_scale)))
    top = float(np.abs(np.asarray(codebook, F64)).max()) + 8.0 * s
    return s * z_bar + 8.0 * s * 2.0 ** -24 + top * 2.0 ** -24


def used_case(k, kind, seed=0):
    """used int32 [K] for num_batches = 10 and threshold 0.01 (a code is unused where used == 0)."""
    rng = np.random.default_rng([k, seed, ("most", "few", "none").index(kind)])
    used = rng.integers(1, 50, k).astype(np.int32)
    if kind == "most":                          # |U| >= |V|: a third unused
        used[rng.permutation(k)[:k // 3]] = 0
    elif kind == "few":                         # 0 < |U| < |V|: five used (tiled and shuffled)
        keep = rng.permutation(k)[:5]
        mask = np.ones(k, bool)
        mask[keep] = False
        used[mask] = 0
    else:
        used[:] = 0
    return used

"""GPU parity of the codebook entries (include/dm3d.h, dm3d_codebook_desc) against the numpy restatement of tests/codebook_reference.py,
and of what is built on them: ``EMACodebook``, ``VQVAE.fit_codebook`` and ``VQVAE.codebook_usage``.

The raw-ABI cases call dm3d_code_stats, dm3d_code_usage, dm3d_codebook_ema and dm3d_codebook_replace through ctypes with every device
buffer guarded (tests/guarded_buffers.py).  The kernels run the restatement's operations in the restatement's order, so counts, sums,
perplexity, cluster sizes, moving averages, codebook and esq must equal it bit for bit, with inputs unchanged, guards intact and a
second run bitwise the first.  The one exception is the N(0,1) draw dm3d_codebook_replace adds, whose logf / sqrtf / sincosf are the
device library's: which row goes where, the counts, the copied EMA state and esq (by the stated rule on the device's own rows) are
exact, and a replaced row is held to codebook_reference.row_bar around source + noise_scale * z with z the float64 reference draw.

Shapes (rows, D, K): 77 x 4 x 33 (one partial 64-row group, one lane group), 513 x 132 x 128 (three feature slices, the last partial),
4099 x 8 x 1024 (seventeen 256-row rounds, more codes than rows in a round), 3000 x 64 x 5 (queues that fill and drain many times)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import codebook_reference as cr
from guarded_buffers import IN, OUT, Guarded
from philox_cases import Z_BAR

pytestmark = pytest.mark.gpu

STATS_PARAMS = [(shape, kind) for shape in cr.SHAPES for kind in cr.KINDS]
STATS_IDS = [f"{cr.shape_id(s)}-{k}" for s, k in STATS_PARAMS]


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


class _Call:
    """One descriptor over guarded buffers: ``give`` an input, ``out`` an output or in-place buffer (with its start values), ``run``."""

    def __init__(self, dev, **scalars):
        from dm3d_amd import _lib
        self.dev, self.ins, self.outs = dev, [], {}
        self.d = _lib.CodebookDesc()
        for k, v in scalars.items():
            setattr(self.d, k, v)

    def give(self, field, arr):
        self.ins.append(Guarded(arr, self.dev, IN))
        setattr(self.d, field, self.ins[-1].ptr)

    def out(self, field, start):
        self.outs[field] = Guarded(start, self.dev, OUT)
        setattr(self.d, field, self.outs[field].ptr)

    def run(self, entry):
        from dm3d_amd import _lib
        _lib.check(getattr(_lib.lib(), "dm3d_" + entry)(C.byref(self.d), None), entry)
        torch.cuda.synchronize()
        for g in self.ins:
            g.unchanged()
        return {k: g.get() for k, g in self.outs.items()}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _twice(make, entry):
    """The outputs of one run, after checking that a second run on fresh buffers is bitwise the first."""
    first, again = make().run(entry), make().run(entry)
    assert all(_same(first[k], again[k]) for k in first), entry
    return first


@functools.lru_cache(maxsize=None)
def _stats_reference(shape, kind):
    z, idx = cr.stats_case(shape, kind) if kind != "ema" else cr.ema_stats_case(shape)
    return (z, idx) + cr.code_stats(z, idx, shape[2])


def _stats_call(dev, z, idx, k):
    c = _Call(dev, rows=z.shape[0], dim=z.shape[1], k=k)
    c.give("z", z)
    c.give("idx", idx)
    c.out("counts", np.full(k, -7, np.int32))
    c.out("sums", np.full((k, z.shape[1]), np.nan, np.float64))
    c.out("invalid", np.full(1, -7, np.int32))
    return c


@pytest.mark.parametrize("shape,kind", STATS_PARAMS, ids=STATS_IDS)
def test_code_stats_and_usage_equal_the_restatement(dev, shape, kind):
    rows, dim, k = shape
    z, idx, counts, sums, invalid = _stats_reference(shape, kind)
    got = _twice(lambda: _stats_call(dev, z, idx, k), "code_stats")
    assert _same(got["counts"], counts), np.flatnonzero(got["counts"] != counts)[:8]
    assert got["invalid"][0] == invalid
    assert _same(got["sums"], sums), np.abs(got["sums"] - sums).max()
    if kind == "invalid":
        assert invalid > 0 and counts.sum() == rows - invalid
    # usage of these counts, and used_accum across two calls
    start = np.arange(k, dtype=np.int32) * 3
    perp, active = cr.code_usage(counts, rows)
    accum = Guarded(start, dev, OUT)
    for call in (1, 2):
        c = _Call(dev, rows=rows, k=k, eps=cr.EPS)
        c.give("counts", counts)
        c.out("perplexity", np.full(1, np.nan, np.float64))
        c.out("active", np.full(1, -7, np.int32))
        c.d.used_accum = accum.ptr
        res = c.run("code_usage")
        assert _same(res["perplexity"][0], perp), (res["perplexity"][0], perp)
        assert res["active"][0] == active
        assert _same(accum.get(), start + call * counts)
    c = _Call(dev, rows=rows, k=k, eps=cr.EPS)                      # without used_accum
    c.give("counts", counts)
    c.out("perplexity", np.full(1, np.nan, np.float64))
    c.out("active", np.full(1, -7, np.int32))
    assert _same(c.run("code_usage")["perplexity"][0], perp)
    print(f"{cr.shape_id(shape)} {kind}: perplexity {perp:.6f}, active {active} of {k}, invalid {invalid}")


def _ema_call(dev, state, counts, sums, decay, epsilon):
    size, ema_w, book, esq = state
    c = _Call(dev, dim=book.shape[1], k=book.shape[0], decay=decay, epsilon=epsilon)
    c.give("counts", counts)
    c.give("sums", sums)
    c.out("cluster_size", size)
    c.out("ema_w", ema_w)
    c.out("codebook", book)
    c.out("esq", esq)
    return c


def _check_ema(got, want):
    for name, ref in zip(("cluster_size", "ema_w", "codebook", "esq"), want):
        assert _same(got[name], ref), (name, np.abs(got[name].astype(np.float64) - ref).max())


@pytest.mark.parametrize("shape", cr.SHAPES, ids=[cr.shape_id(s) for s in cr.SHAPES])
def test_codebook_ema_equals_the_restatement(dev, shape):
    _, _, counts, sums, _ = _stats_reference(shape, "ema")
    state = cr.ema_state(shape)
    want = cr.codebook_ema(*state, counts, sums, 0.99, 1e-5)
    got = _twice(lambda: _ema_call(dev, state, counts, sums, 0.99, 1e-5), "codebook_ema")
    _check_ema(got, want)
    dead = want[0] == 0                                              # N' == 0: the code keeps its row and its esq
    assert dead.sum() == 2 and _same(got["codebook"][dead], state[2][dead]) and _same(got["esq"][dead], state[3][dead])
    assert np.isfinite(got["codebook"]).all()


def test_ema_chain_follows_the_restatement_and_the_float64_rule(dev):
    """Six chained steps at decay 0.9 (16 codes, D = 8, 512 rows a step; tests/test_codebook_host.py holds the input condition): counts,
    sums and state bitwise the restatement's at every step, and the codebook within four times the float32 literal restatement's own
    error of the float64 literal restatement (measured on an MI355X, worst of the six steps: the device 9.6e-7, the float32 literal
    restatement 1.38e-6; at the last step 8.03e-7 against 7.83e-7)."""
    batches, codebook = cr.chain_inputs()
    c64, c32 = cr.literal_chain(np.float64), cr.literal_chain(np.float32)
    state = cr.chain_start(codebook)
    dev_state = state
    for step, z in enumerate(batches):
        idx, _ = cr.assign(z, state[2].T)
        assert np.array_equal(idx, c64[step][0])
        counts, sums, _ = cr.code_stats(z, idx, cr.CHAIN_K)
        stats = _stats_call(dev, z, idx, cr.CHAIN_K).run("code_stats")
        assert _same(stats["counts"], counts) and _same(stats["sums"], sums), step
        state = cr.codebook_ema(*state, counts, sums, cr.CHAIN_DECAY, cr.CHAIN_EPSILON)
        got = _ema_call(dev, dev_state, stats["counts"], stats["sums"], cr.CHAIN_DECAY, cr.CHAIN_EPSILON).run("codebook_ema")
        _check_ema(got, state)
        dev_state = (got["cluster_size"], got["ema_w"], got["codebook"], got["esq"])
        err = np.abs(got["codebook"].T.astype(np.float64) - c64[step][2]).max()
        err32 = np.abs(c32[step][2].astype(np.float64) - c64[step][2]).max()
        print(f"step {step}: device against float64 literal {err:.3e}, float32 literal against it {err32:.3e}")
        assert err <= 4.0 * err32, (step, err, err32)


REPLACE_PARAMS = [(k, dim, kind, ema) for k, dim in ((33, 12), (1024, 260)) for kind in ("most", "few", "none") for ema in (True,)] + [(33, 12, "most", False)]


@pytest.mark.parametrize("k,dim,kind,ema", REPLACE_PARAMS, ids=[f"{k}x{d}-{kind}{'' if e else '-no-ema'}" for k, d, kind, e in REPLACE_PARAMS])
def test_codebook_replace(dev, k, dim, kind, ema):
    noise_scale, seed, draw, batches, threshold = 0.01, 0x0123456789ABCDEF, 3, 10, 0.01
    rng = np.random.default_rng([k, dim, 5])
    book = rng.standard_normal((k, dim)).astype(np.float32)
    esq = cr.esq_of(book)
    size = rng.uniform(1.0, 30.0, k).astype(np.float32)
    ema_w = rng.standard_normal((k, dim)).astype(np.float32)
    used = cr.used_case(k, kind)
    plan, nu, nv = cr.replace_plan(used, batches, threshold, draw, seed)

    def make():
        c = _Call(dev, dim=dim, k=k, num_batches=batches, threshold=threshold, noise_scale=noise_scale, seed=seed, draw=draw)
        c.out("codebook", book)
        c.out("esq", esq)
        c.out("used", used)
        c.out("used_count", np.full(1, -7, np.int32))
        c.out("unused_count", np.full(1, -7, np.int32))
        c.out("map", np.full(k, -7, np.int32))
        if ema:
            c.out("cluster_size", size)
            c.out("ema_w", ema_w)
        return c
    got = _twice(make, "codebook_replace")
    assert got["used_count"][0] == nu and got["unused_count"][0] == nv and not got["used"].any()
    assert _same(got["map"], plan), np.flatnonzero(got["map"] != plan)[:8]
    stay, hit = plan < 0, plan >= 0
    assert hit.sum() == (k if kind == "none" else nv)
    assert _same(got["codebook"][stay], book[stay]) and _same(got["esq"][stay], esq[stay])          # sources (and every used row) untouched
    want = cr.replace_rows(book, plan, noise_scale, draw, seed)
    bar = cr.row_bar(book, noise_scale, Z_BAR)
    err = np.abs(got["codebook"].astype(np.float64) - want)[hit].max()
    print(f"K={k} D={dim} {kind}: used {nu}, unused {nv}, worst |row - (source + s z_f64)| {err:.3e}, bar {bar:.3e}")
    assert err < bar
    moved = (got["codebook"][hit].astype(np.float64) - book[plan[hit]]) / noise_scale                # the normal stream shows
    assert 0.75 < moved.std() < 1.25 and abs(moved.mean()) < 0.3
    assert _same(got["esq"], cr.esq_of(got["codebook"]))                                             # esq by the stated rule, on the device's own rows
    if ema:
        copied = hit & (plan != np.arange(k))
        want_size, want_w = size.copy(), ema_w.copy()
        want_size[copied], want_w[copied] = size[plan[copied]], ema_w[plan[copied]]
        assert _same(got["cluster_size"], want_size) and _same(got["ema_w"], want_w)
        assert copied.sum() == (0 if kind == "none" else nv)


def test_ema_codebook_follows_the_restatement(dev, tmp_path):
    from dm3d_amd.codebook import EMACodebook
    batches, codebook = cr.chain_inputs()
    start = cr.chain_start(codebook)
    layer = EMACodebook(cr.CHAIN_K, cr.CHAIN_DIM, commitment_cost=6, decay=cr.CHAIN_DECAY, epsilon=cr.CHAIN_EPSILON, device=dev, seed=0)
    fresh = layer.state_dict()
    assert fresh["embeddings"].shape == (cr.CHAIN_DIM, cr.CHAIN_K) and np.abs(fresh["embeddings"]).max() <= 0.05 and not fresh["ema_cluster_size"].any()
    layer.load_state_dict({"embeddings": start[2].T, "ema_cluster_size": start[0], "ema_w": start[1].T})
    state, used = start, np.zeros(cr.CHAIN_K, np.int32)
    for z in batches[:3]:
        x = torch.from_numpy(z.reshape(2, 16, 16, cr.CHAIN_DIM)).to(dev)
        loss, q, indices, perplexity = layer(x, training=True)
        idx, _ = cr.assign(z, state[2].T)
        assert tuple(indices.shape) == (2, 16, 16) and indices.dtype == torch.int32 and np.array_equal(indices.cpu().numpy().reshape(-1), idx)
        assert tuple(q.shape) == tuple(x.shape) and _same(q.cpu().numpy().reshape(-1, cr.CHAIN_DIM), state[2][idx])      # the codes before the update
        counts, sums, _ = cr.code_stats(z, idx, cr.CHAIN_K)
        assert _same(perplexity.cpu().numpy(), cr.code_usage(counts, z.shape[0])[0])
        mse = ((state[2][idx].astype(np.float64) - z.astype(np.float64)) ** 2).sum() / z.size
        assert loss.dtype == torch.float64 and abs(float(loss) - 6 * mse) <= z.size * 2.0 ** -52 * 6 * mse                # a float64 sum in another order
        state, used = cr.codebook_ema(*state, counts, sums, cr.CHAIN_DECAY, cr.CHAIN_EPSILON), used + counts
        sd = layer.state_dict()
        assert _same(sd["embeddings"], np.ascontiguousarray(state[2].T)) and _same(sd["ema_cluster_size"], state[0])
        assert _same(sd["ema_w"], np.ascontiguousarray(state[1].T)) and _same(layer.esq.cpu().numpy(), state[3])
        assert _same(layer.codebooks_used.cpu().numpy(), used)
    # training=False changes no state
    before = layer.state_dict()
    out = layer(torch.from_numpy(batches[3].reshape(2, 16, 16, cr.CHAIN_DIM)).to(dev), training=False)
    assert np.array_equal(out[2].cpu().numpy().reshape(-1), cr.assign(batches[3], state[2].T)[0])
    after = layer.state_dict()
    assert all(_same(before[k], after[k]) for k in before) and _same(layer.esq.cpu().numpy(), state[3])
    # .npz round trip
    path = tmp_path / "codebook.npz"
    np.savez(path, **after)
    other = EMACodebook(cr.CHAIN_K, cr.CHAIN_DIM, decay=cr.CHAIN_DECAY, epsilon=cr.CHAIN_EPSILON, device=dev, seed=5)
    other.load_state_dict(dict(np.load(path)))
    again = other.state_dict()
    assert all(_same(after[k], again[k]) for k in after) and _same(other.esq.cpu().numpy(), state[3])
    # replacement through the layer: nothing is unused after three batches that use every code
    counts = layer.replace_unused_codebooks(3)
    assert int(counts.used_count) == cr.CHAIN_K and int(counts.unused_count) == 0 and not layer.codebooks_used.any()
    assert _same(layer.state_dict()["embeddings"], after["embeddings"])
    with pytest.raises(ValueError, match=r"inputs must be a float32 tensor \[\.\.\., 8\]"):
        layer(torch.zeros(4, 7, device=dev))


def _small_vqvae(dev, weights=None):
    from dm3d_amd.networks.vqvae3d_monai import VQVAE
    from oracle import ref_torch as rt
    if weights is None:
        cfg = rt.VQVAEConfig(in_channels=1, out_channels=1, num_channels=(16, 32), num_res_layers=2, num_res_channels=(16, 32),
                             num_embeddings=64, embedding_dim=8, input_size=32)
        weights = {k: v.numpy() for k, v in rt.vqvae_synthetic_weights(cfg, seed=1).items()}
    return VQVAE(1, 1, (16, 32), 2, (16, 32), downsample_parameters=((2, 4, 1, "same"),) * 2, upsample_parameters=((2, 4, 1, "same", 0),) * 2,
                 num_embeddings=64, embedding_dim=8, dropout=None, input_size=32, weights=weights, device=dev)


def test_fit_codebook_and_usage_on_the_small_vqvae(dev):
    from dm3d_amd import ops
    g = torch.Generator().manual_seed(8)
    xs = [torch.rand(2, 32, 32, 32, 1, generator=g).to(dev) for _ in range(2)]
    # a model that never calls the new methods quantizes as before
    plain = _small_vqvae(dev)
    emb0 = plain.state["vq.embeddings"].copy()
    lat = [plain.encoder(x) for x in xs]
    q, perp = plain.quantizer(lat[0])
    idx0 = plain.last_indices
    book0 = torch.from_numpy(np.ascontiguousarray(emb0.T)).to(dev)
    probs = torch.bincount(idx0.long(), minlength=64).float() / idx0.numel()
    assert torch.equal(q.reshape(-1, 8), book0[idx0.long()]) and torch.equal(perp, torch.exp(-(probs * torch.log(probs + 1e-10)).sum()))
    assert torch.equal(plain.P["vq.codebook_t"], book0) and _same(plain.state["vq.embeddings"], emb0)
    # usage: counts over both batches
    usage = plain.codebook_usage(xs)
    both = torch.cat([plain.get_code_indices(z.reshape(-1, 8)) for z in lat]).cpu().numpy()
    assert usage["rows"] == 2 * 2 * 8 * 8 * 8 == usage["counts"].sum() and np.array_equal(usage["counts"], np.bincount(both, minlength=64))
    assert usage["active_codes"] == (usage["counts"] > 0).sum() and usage["dead_codes"] == np.flatnonzero(usage["counts"] == 0).tolist()
    assert usage["perplexity"] == cr.code_usage(usage["counts"], usage["rows"])[0]
    # the fit: the restatement driven with the device's own latents and the device's own assignment to the restated codebook
    model = _small_vqvae(dev)
    report = model.fit_codebook(xs, decay=0.9, epsilon=1e-5)
    state = cr.chain_start(emb0.T)
    for i, z in enumerate(lat):
        flat = z.reshape(-1, 8)
        idx = ops.vq_assign(flat, torch.from_numpy(state[2]).to(dev), torch.from_numpy(state[3]).to(dev)).cpu().numpy()
        counts, sums, _ = cr.code_stats(flat.cpu().numpy(), idx, 64)
        perp_i, active_i = cr.code_usage(counts, flat.shape[0])
        assert report["perplexity"][i] == perp_i and report["active_codes"][i] == active_i
        mse = ((state[2][idx].astype(np.float64) - flat.cpu().numpy().astype(np.float64)) ** 2).sum() / flat.numel()
        assert abs(report["quantize_loss"][i] - 1.25 * mse) <= flat.numel() * 2.0 ** -52 * 1.25 * mse
        state = cr.codebook_ema(*state, counts, sums, 0.9, 1e-5)
    assert report["batches"] == 2 and report["replacements"] == 0
    assert _same(model.P["vq.codebook_t"].cpu().numpy(), state[2]) and _same(model.P["vq.esq"].cpu().numpy(), state[3])
    assert _same(model.state["vq.embeddings"], np.ascontiguousarray(state[2].T)) and not _same(model.state["vq.embeddings"], emb0)
    # a fresh model loaded from the returned state picks the same codes
    fresh = _small_vqvae(dev, weights=model.state)
    fresh.prepare()
    assert torch.equal(fresh.P["vq.codebook_t"], model.P["vq.codebook_t"]) and torch.equal(fresh.P["vq.esq"], model.P["vq.esq"])
    qa, _ = model.quantizer(lat[1])
    qb, _ = fresh.quantizer(lat[1])
    assert torch.equal(model.last_indices, fresh.last_indices) and torch.equal(qa, qb)
    # a second fit from the same start repeats bitwise; replacement every batch runs and reports
    twin = _small_vqvae(dev)
    twin.fit_codebook(xs, decay=0.9, epsilon=1e-5)
    assert torch.equal(twin.P["vq.codebook_t"], model.P["vq.codebook_t"])
    swapped = _small_vqvae(dev)
    rep = swapped.fit_codebook(xs, decay=0.9, replace_every=1, discarding_threshold=1.0, seed=3)
    assert rep["replacements"] == 2 and np.isfinite(swapped.state["vq.embeddings"]).all() and torch.isfinite(swapped.P["vq.esq"]).all()
    assert _same(swapped.P["vq.esq"].cpu().numpy(), cr.esq_of(swapped.P["vq.codebook_t"].cpu().numpy()))

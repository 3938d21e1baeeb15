"""GPU parity of the distribution-metric entries (include/dm3d.h, dm3d_dist_desc) against the numpy restatement of
tests/distribution_reference.py.

The raw-ABI cases call dm3d_feature_moments, dm3d_knn_radius, dm3d_prdc_counts and dm3d_poly_mmd through ctypes with every device buffer
guarded (tests/guarded_buffers.py).  The kernels run the restatement's operations in the restatement's order, so every output — mean,
covariance, radii, the three integer vectors, the three kernel sums — must equal it bit for bit, with inputs unchanged, guards intact
and a second run bitwise the first.  The shapes are the smallest at which the tiling can go wrong: 65 rows against 127 (tile 64), one
case inside a single tile, D = 1, 31, 33 and 70 (chunk 32), k = 1, 5, 16, row tables that permute, that repeat a row and NULL, exact
duplicates inside each set and one row shared between the sets, 1 and 3 subsets."""
import ctypes as C

import numpy as np
import pytest
import torch

import distribution_reference as dr
from guarded_buffers import IN, OUT, Guarded

pytestmark = pytest.mark.gpu

PARAMS = [(case, kind) for case in dr.CASES for kind in dr.TABLES]
IDS = [f"{dr.case_id(case)}-{kind}" for case, kind in PARAMS]
RANK_DEFICIENT = "rank-deficient"


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _sets(case, kind):
    """(real matrix, fake matrix, real table, fake table, real rows read, fake rows read) of one case."""
    n, m, _ = case
    real, fake = dr.clouds(case)
    tx, ty = dr.table(kind, n, real.shape[0], 11), dr.table(kind, m, fake.shape[0], 12)
    return real, fake, tx, ty, dr.gathered(real, tx, n), dr.gathered(fake, ty, m)


class _Call:
    """One descriptor over guarded buffers: inputs on construction, outputs by ``out``, then ``run`` checks inputs and returns outputs."""

    def __init__(self, dev, x, tx, n, y=None, ty=None, m=0):
        from dm3d_amd import _lib
        self.dev, self.ins, self.outs = dev, [], {}
        self.d = d = _lib.DistDesc()
        d.x, d.nx, d.dim, d.n = self._in(x), x.shape[0], x.shape[1], n
        d.rows_x = 0 if tx is None else self._in(tx)
        if y is not None:
            d.y, d.ny, d.m = self._in(y), y.shape[0], m
            d.rows_y = 0 if ty is None else self._in(ty)

    def _in(self, arr):
        self.ins.append(Guarded(arr, self.dev, IN))
        return self.ins[-1].ptr

    def give(self, field, arr):
        setattr(self.d, field, self._in(arr))

    def out(self, field, shape, dtype):
        fill = np.full(shape, -7, dtype) if np.issubdtype(dtype, np.integer) else np.full(shape, np.nan, dtype)
        self.outs[field] = Guarded(fill, self.dev, OUT)
        setattr(self.d, field, self.outs[field].ptr)

    def run(self, entry):
        from dm3d_amd import _lib
        _lib.check(getattr(_lib.lib(), "dm3d_" + entry)(C.byref(self.d), None), entry)
        torch.cuda.synchronize()
        for g in self.ins:
            g.unchanged()
        return {k: g.get() for k, g in self.outs.items()}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _twice(make, entry):
    """The outputs of one run, after checking that a second run on fresh buffers is bitwise the first."""
    first, again = make().run(entry), make().run(entry)
    assert all(_same(first[k], again[k]) for k in first), entry
    return first


@pytest.mark.parametrize("case,kind", PARAMS, ids=IDS)
def test_moments_equal_the_restatement(dev, case, kind):
    real, _, tx, _, x, _ = _sets(case, kind)
    n, dim = x.shape

    def make():
        c = _Call(dev, real, tx, n)
        c.out("mean", (dim,), np.float64)
        c.out("cov", (dim, dim), np.float64)
        return c
    got = _twice(make, "feature_moments")
    mean, cov = dr.feature_moments(x)
    assert _same(got["mean"], mean), np.abs(got["mean"] - mean).max()
    assert _same(got["cov"], cov), np.abs(got["cov"] - cov).max()
    assert np.array_equal(got["cov"], got["cov"].T)


@pytest.mark.parametrize("case,kind", PARAMS, ids=IDS)
def test_radii_and_counts_equal_the_restatement(dev, case, kind):
    real, fake, tx, ty, x, y = _sets(case, kind)
    n, m = x.shape[0], y.shape[0]
    for k in dr.KS:
        radii = []
        for mat, tab, rows in ((real, tx, n), (fake, ty, m)):
            def make():
                c = _Call(dev, mat, tab, rows)
                c.d.k = k
                c.out("radius", (rows,), np.float64)
                return c
            radii.append(_twice(make, "knn_radius")["radius"])
        rx, ry = dr.knn_radius(x, k), dr.knn_radius(y, k)
        assert _same(radii[0], rx) and _same(radii[1], ry), (k, np.abs(radii[0] - rx).max(), np.abs(radii[1] - ry).max())
        if k == 1 and kind != "permute":
            assert (rx == 0.0).sum() >= 2                                       # the duplicate rows (a repeating table adds more)

        def make():
            c = _Call(dev, real, tx, n, fake, ty, m)
            c.give("radius_x", rx)
            c.give("radius_y", ry)
            c.out("count_y", (m,), np.int32)
            c.out("near_x", (n,), np.int32)
            c.out("cover_x", (n,), np.int32)
            return c
        got = _twice(make, "prdc_counts")
        count, near, cover = dr.prdc_counts(x, y, rx, ry)
        assert _same(got["count_y"], count), (k, int((got["count_y"] != count).sum()))
        assert _same(got["near_x"], near) and _same(got["cover_x"], cover), k


@pytest.mark.parametrize("case", dr.CASES, ids=[dr.case_id(c) for c in dr.CASES])
def test_kernel_sums_equal_the_restatement(dev, case):
    n, m, _ = case
    real, fake = dr.clouds(case)
    for subsets, kind in ((1, None), (1, "permute"), (3, "permute"), (3, "repeat")):
        tx = None if kind is None else np.stack([dr.table(kind, n, real.shape[0], 20 + s) for s in range(subsets)])
        ty = None if kind is None else np.stack([dr.table(kind, m, fake.shape[0], 30 + s) for s in range(subsets)])

        def make():
            c = _Call(dev, real, tx, n, fake, ty, m)
            c.d.subsets = subsets
            c.out("sums", (subsets, 3), np.float64)
            c.out("work", (subsets * (2 * n + m),), np.float64)
            c.d.work_elems = subsets * (2 * n + m)
            return c
        got = _twice(make, "poly_mmd")["sums"]
        want = np.stack([dr.poly_mmd(dr.gathered(real, None if tx is None else tx[s], n), dr.gathered(fake, None if ty is None else ty[s], m))
                         for s in range(subsets)])
        assert _same(got, want), (subsets, kind, got.tolist(), want.tolist())


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def test_scores_through_the_wrappers(dev):
    """prdc, mmd2 and kid form their values from the kernels' outputs with correctly rounded float64 operations in the restatement's
    order (integer counts are exact; divisions go through a device divisor; kid's mean and variance over subsets are the moments
    kernel's sequential sums; the square root is correctly rounded), so they equal it to the last bit too."""
    from dm3d_amd import metrics, ops
    case = dr.MAIN_CASES[2]
    n, m, dim = case
    x, y = dr.clouds(case)[0][:n], dr.clouds(case)[1][:m]
    tx, ty = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(y.copy()).to(dev)
    for k in dr.KS:
        got, want = metrics.prdc(tx, ty, nearest_k=k), dr.prdc(x, y, k)
        assert set(got) == {"precision", "recall", "density", "coverage"}
        for key, v in got.items():
            assert v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda and _bits(v) == np.float64(want[key]).tobytes(), (k, key, float(v), want[key])
    v = metrics.mmd2(tx, ty)
    assert v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda and _bits(v) == np.float64(dr.mmd2(x, y)).tobytes(), (float(v), dr.mmd2(x, y))
    for subsets, size, seed in ((3, 20, 0), (1, 1000, 5), (4, 64, 2)):
        mean, std = metrics.kid(tx, ty, num_subsets=subsets, subset_size=size, seed=seed)
        wm, ws = dr.kid(x, y, subsets, size, seed)
        assert mean.dtype == std.dtype == torch.float64 and mean.is_cuda and std.is_cuda
        assert _bits(mean) == np.float64(wm).tobytes() and _bits(std) == np.float64(ws).tobytes(), (float(mean), wm, float(std), ws)
    # float32 features are widened exactly; a row table reads a resample in place
    x32, y32 = x.astype(np.float32), y.astype(np.float32)
    f32 = metrics.prdc(torch.from_numpy(x32).to(dev), torch.from_numpy(y32).to(dev), nearest_k=5)
    want = dr.prdc(x32.astype(np.float64), y32.astype(np.float64), 5)
    assert all(_bits(f32[key]) == np.float64(want[key]).tobytes() for key in want)
    rows = torch.from_numpy(dr.table("repeat", 40, n, 4).astype(np.int64)).to(dev)
    mom = ops.feature_moments(torch.from_numpy(x32).to(dev), rows)
    wmean, wcov = dr.feature_moments(x32.astype(np.float64)[rows.cpu().numpy()])
    assert _bits(mom.mean) == wmean.tobytes() and _bits(mom.cov) == wcov.tobytes()
    assert _bits(ops.knn_radius(tx, 5, rows)) == dr.knn_radius(x[rows.cpu().numpy()], 5).tobytes()
    # all seven numbers in one call
    out = metrics.distribution_metrics(tx, ty, nearest_k=5, num_subsets=3, subset_size=20, seed=0)
    assert set(out) == {"frechet_distance", "kid_mean", "kid_std", "precision", "recall", "density", "coverage"}
    assert all(v.dtype == torch.float64 and v.dim() == 0 and bool(torch.isfinite(v)) for v in out.values())
    assert _bits(out["kid_mean"]) == np.float64(dr.kid(x, y, 3, 20, 0)[0]).tobytes() and _bits(out["recall"]) == np.float64(dr.prdc(x, y, 5)["recall"]).tobytes()


def frechet_inputs():
    """{name: (real, fake)}: every case, one rank-deficient pair (23 and 40 rows of 70 features) and one pair fake = real."""
    out = {dr.case_id(c): (dr.clouds(c)[0][:c[0]], dr.clouds(c)[1][:c[1]]) for c in dr.CASES}
    big = dr.clouds(dr.MAIN_CASES[3])
    out[RANK_DEFICIENT] = (big[0][:23], big[1][:40])
    out["same"] = (dr.clouds(dr.MAIN_CASES[2])[0][:65],) * 2
    return out


def frechet_bars(inputs):
    """(relative bar, absolute bar, {name: symmetric-form value}): four times the largest disagreement between the restatement's two
    evaluations of the trace term, relative to the distance over the pairs of different sets, and absolute over all pairs."""
    sym = {k: dr.frechet(*v) for k, v in inputs.items()}
    gap = {k: abs(sym[k] - dr.frechet(*v, how="product")) for k, v in inputs.items()}
    return 4.0 * max(gap[k] / sym[k] for k in inputs if k != "same"), 4.0 * max(gap.values()), sym


def test_frechet_distance(dev):
    """The moments are bitwise the restatement's (above), so only the host tail can differ: torch.linalg.eigh / eigvalsh against
    numpy's.  Its bar is not chosen but measured: the restatement evaluates the trace term from the eigenvalues of the symmetric form
    S1^(1/2) S2 S1^(1/2) and from those of the plain product S1 S2, and the bar is four times their largest disagreement over the test
    inputs — relative to the distance, 1.2e-7 on these inputs (the largest gap, 3.1e-8 of a distance of 584, is the pair of 23 and
    40 rows of 70 features, rank-deficient, whose zero eigenvalues come out as rounding noise of either sign before the square root;
    full-rank pairs disagree by 1e-14 or less) — and, for fake = real, where the distance is 0, the same factor on the largest
    absolute gap (7.2e-5 here; the tail gives 5e-12).  Measured on the host: torch's tail is off the restatement's symmetric form by
    2.9e-8 relative on the rank-deficient pair, 1.7e-10 on the 65 x 70 one and at most 2e-14 elsewhere."""
    from dm3d_amd import metrics
    inputs = frechet_inputs()
    rel_bar, abs_bar, sym = frechet_bars(inputs)
    print(f"frechet bars: relative {rel_bar:.3e}, absolute {abs_bar:.3e}")
    assert 0.0 < rel_bar < 1e-6
    for name, (x, y) in inputs.items():
        got = metrics.frechet_distance(torch.from_numpy(x.copy()).to(dev), torch.from_numpy(y.copy()).to(dev))
        assert got.dtype == torch.float64 and got.dim() == 0
        err = abs(float(got) - sym[name])
        print(f"frechet {name}: {float(got):.17g} against {sym[name]:.17g}, off by {err:.3e}")
        if name == "same":
            assert abs(float(got)) <= abs_bar, (float(got), abs_bar)
        else:
            assert err <= rel_bar * sym[name], (name, float(got), sym[name], rel_bar)
    x, y = inputs[RANK_DEFICIENT]
    assert x.shape[0] < x.shape[1] and np.linalg.matrix_rank(dr.feature_moments(x)[1]) < x.shape[1]


def test_encoder_features(dev):
    """The default features are the pooled encoder output: against plain torch pooling of ``_encode`` on the same device, within four
    times what pooling that output in float32 instead of float64 changes (measured here); distribution_metrics takes them as they are."""
    from dm3d_amd import metrics
    from dm3d_amd.networks.vqvae3d_monai import VQVAE
    from oracle import ref_torch as rt
    cfg = rt.VQVAEConfig(in_channels=1, out_channels=1, num_channels=(16, 32), num_res_layers=2, num_res_channels=(16, 32),
                         num_embeddings=64, embedding_dim=8, input_size=32)
    W = rt.vqvae_synthetic_weights(cfg, seed=1)
    vq = VQVAE(1, 1, (16, 32), 2, (16, 32), downsample_parameters=((2, 4, 1, "same"),) * 2,
               upsample_parameters=((2, 4, 1, "same", 0),) * 2, num_embeddings=64, embedding_dim=8, dropout=None,
               input_size=32, weights={k: v.numpy() for k, v in W.items()}, precision="fp32")
    g = torch.Generator().manual_seed(8)
    vols = torch.rand(7, 32, 32, 32, 1, generator=g)
    z = torch.cat([vq._encode(vols[at:at + 3].to(dev)) for at in (0, 3, 6)])    # the batches encoder_features is asked for below
    assert tuple(z.shape) == (7, 8, 8, 8, 8)
    flat64, flat32 = z.double().reshape(7, -1, 8), z.reshape(7, -1, 8)
    want = {"mean": flat64.mean(1), "mean_std": torch.cat([flat64.mean(1), flat64.std(1, unbiased=False)], 1)}
    low = {"mean": flat32.mean(1).double(), "mean_std": torch.cat([flat32.mean(1), flat32.std(1, unbiased=False)], 1).double()}
    feats = {}
    for pool in ("mean", "mean_std"):
        bar = 4.0 * float((low[pool] - want[pool]).abs().max())
        got = feats[pool] = metrics.encoder_features(vq, vols, pool=pool, batch_size=3)            # batches of 3, 3 and 1
        assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (7, 8 if pool == "mean" else 16)
        err = float((got - want[pool]).abs().max())
        print(f"encoder_features {pool}: off by {err:.3e}, bar {bar:.3e}")
        assert bar > 0.0 and err <= bar
    real, fake = feats["mean_std"][:4], feats["mean_std"][3:]
    out = metrics.distribution_metrics(real, fake, nearest_k=2, num_subsets=2, subset_size=3, seed=0)
    assert set(out) == {"frechet_distance", "kid_mean", "kid_std", "precision", "recall", "density", "coverage"}
    assert all(v.dtype == torch.float64 and v.dim() == 0 and bool(torch.isfinite(v)) for v in out.values()), out

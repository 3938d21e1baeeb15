"""numpy float64 restatement of the distribution-metric entries (include/dm3d.h, dm3d_dist_desc) and of the public scores built on them
(plain helper, no test in it; tests/test_distribution_host.py checks it against closed forms, tests/test_gpu_distribution.py holds the
kernels to it bit for bit).

The operation order is the header's: a pair's sum over the feature axis is an explicit loop over f = 0 .. D-1 with the multiply and the
add as separate numpy operations (numpy fuses nothing), vectorised across pairs; sums over rows and over pairs are explicit loops in
index order.  Also here: the inputs of the GPU tests, so that the host tests can check on the CPU that they show something."""
import numpy as np
import torch

TILE, CHUNK = 64, 32                                # DM3D_DIST_TILE, DM3D_DIST_CHUNK: the kernel's row / column tile and feature chunk
MAX_K = 16


# ---- the entries -------------------------------------------------------------------------------------------------------------------------
def sqdist(x, y):
    """d2[i, j] = sum_f (x[i, f] - y[j, f])^2, sequential in f."""
    acc = np.zeros((x.shape[0], y.shape[0]), np.float64)
    for f in range(x.shape[1]):
        t = x[:, f, None] - y[None, :, f]
        acc = acc + t * t
    return acc


def dots(x, y):
    """sum_f x[i, f] * y[j, f], sequential in f."""
    acc = np.zeros((x.shape[0], y.shape[0]), np.float64)
    for f in range(x.shape[1]):
        acc = acc + x[:, f, None] * y[None, :, f]
    return acc


def feature_moments(x):
    """(mean [D], unbiased cov [D, D]), both sums sequential over the rows."""
    n, dim = x.shape
    s = np.zeros(dim, np.float64)
    for p in range(n):
        s = s + x[p]
    mean = s / np.float64(n)
    c = x - mean
    acc = np.zeros((dim, dim), np.float64)
    for p in range(n):
        acc = acc + c[p][:, None] * c[p][None, :]
    return mean, acc / np.float64(n - 1)


def knn_radius(x, k):
    """The (k + 1)-th smallest entry of every row of the set's own squared-distance matrix, self included (the prdc package's rule)."""
    assert 1 <= k <= MAX_K and k < x.shape[0]
    return np.sort(sqdist(x, x), axis=1)[:, k].copy()


def prdc_counts(real, fake, radius_real, radius_fake):
    """(count_fake int32 [M], near_real int32 [N], cover_real int32 [N]), strict < throughout."""
    d2 = sqdist(real, fake)
    count = (d2 < radius_real[:, None]).sum(axis=0).astype(np.int32)
    near = (d2 < radius_fake[None, :]).any(axis=1).astype(np.int32)
    cover = (d2.min(axis=1) < radius_real).astype(np.int32)
    return count, near, cover


def kernel_sum(x, y, skip_diagonal):
    """sum_i (sum_j k(x_i, y_j)), k = t * t * t with t = dot / D + 1; the row sums run over j in index order (j = i left out with
    ``skip_diagonal``), their sum over i in index order."""
    t = dots(x, y) / np.float64(x.shape[1]) + 1.0
    k = (t * t) * t
    rows = np.zeros(x.shape[0], np.float64)
    idx = np.arange(x.shape[0])
    for j in range(y.shape[0]):
        added = rows + k[:, j]
        rows = np.where(idx != j, added, rows) if skip_diagonal else added
    total = np.float64(0.0)
    for i in range(x.shape[0]):
        total = total + rows[i]
    return total


def poly_mmd(x, y):
    """The three sums of one subset: float64 [3]."""
    return np.array([kernel_sum(x, x, True), kernel_sum(y, y, True), kernel_sum(x, y, False)], np.float64)


# ---- the scores --------------------------------------------------------------------------------------------------------------------------
def mmd2_of(sums, n, m):
    return (sums[0] / np.float64(n * (n - 1)) + sums[1] / np.float64(m * (m - 1))) - (2.0 * sums[2]) / np.float64(n * m)


def mmd2(x, y):
    return mmd2_of(poly_mmd(x, y), x.shape[0], y.shape[0])


def kid_subsets(n_real, n_fake, num_subsets, subset_size, seed):
    """The documented draw: one seeded host generator; per subset randperm(n_real)[:m], then randperm(n_fake)[:m]."""
    m = min(subset_size, n_real, n_fake)
    g = torch.Generator().manual_seed(seed)
    a, b = [], []
    for _ in range(num_subsets):
        a.append(torch.randperm(n_real, generator=g)[:m].numpy().astype(np.int32))
        b.append(torch.randperm(n_fake, generator=g)[:m].numpy().astype(np.int32))
    return np.stack(a), np.stack(b)


def kid(x, y, num_subsets, subset_size, seed):
    """(mean, population std) of the unbiased MMD^2 over the subsets: sequential sums in subset order, std = sqrt(var1 * ((S-1)/S))."""
    ta, tb = kid_subsets(x.shape[0], y.shape[0], num_subsets, subset_size, seed)
    m = ta.shape[1]
    vals = np.array([mmd2_of(poly_mmd(x[a], y[b]), m, m) for a, b in zip(ta, tb)], np.float64)
    if num_subsets == 1:
        return vals[0], np.float64(0.0)
    mean, cov = feature_moments(vals[:, None])
    return mean[0], np.sqrt(cov[0, 0] * (np.float64(num_subsets - 1) / np.float64(num_subsets)))


def prdc(real, fake, k):
    count, near, cover = prdc_counts(real, fake, knn_radius(real, k), knn_radius(fake, k))
    n, m = real.shape[0], fake.shape[0]
    return {"precision": np.float64((count > 0).sum()) / np.float64(m), "recall": np.float64(near.sum()) / np.float64(n),
            "density": np.float64(count.sum()) / np.float64(k * m), "coverage": np.float64(cover.sum()) / np.float64(n)}


def frechet_from_moments(mu1, s1, mu2, s2, how="symmetric"):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2).  The trace term two ways: the eigenvalues of the symmetric form
    S1^(1/2) S2 S1^(1/2) (what the package computes), or those of the plain product S1 S2; negative ones are taken as 0."""
    if how == "symmetric":
        w, v = np.linalg.eigh(s1)
        root = (v * np.sqrt(np.maximum(w, 0.0))) @ v.T
        form = root @ s2 @ root
        ev = np.linalg.eigvalsh((form + form.T) * 0.5)
    else:
        ev = np.linalg.eigvals(s1 @ s2).real
    d = mu1 - mu2
    return (d * d).sum() + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.maximum(ev, 0.0)).sum()


def frechet(x, y, how="symmetric"):
    return frechet_from_moments(*feature_moments(x), *feature_moments(y), how=how)


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------------
SPARE = 5                                           # matrix rows beyond the rows a case reads: a table reaches them, NULL does not
# (N, M, D): N = R + 1 against M = 2C - 1 at D in {1, Dc - 1, Dc + 1, three chunks}; one case inside a single tile
MAIN_CASES = ((TILE + 1, 2 * TILE - 1, 1), (TILE + 1, 2 * TILE - 1, CHUNK - 1), (TILE + 1, 2 * TILE - 1, CHUNK + 1), (TILE + 1, 2 * TILE - 1, 2 * CHUNK + 6))
SMALL_CASE = (23, 40, 7)
CASES = MAIN_CASES + (SMALL_CASE,)
KS = (1, 5, 16)
TABLES = (None, "permute", "repeat")
_cache = {}


def clouds(case):
    """(real [N + SPARE, D], fake [M + SPARE, D]) float64: two overlapping Gaussian clouds with shifted means and unequal scales, a
    third of each moved away to opposite sides.  Each set holds an exact duplicate (rows 3 and 10 of real, 5 and 6 of fake) and the
    sets share a row (fake 0 is real 7)."""
    if case not in _cache:
        n, m, dim = case
        rng = np.random.default_rng(1000 * n + 10 * m + dim)
        real = rng.standard_normal((n + SPARE, dim))
        fake = 0.9 * rng.standard_normal((m + SPARE, dim)) + 0.3 / np.sqrt(dim)
        away = 3.0 + 3.0 / np.sqrt(dim)              # a third of each set lies where the other set has nothing: no score is 0 or 1
        real[rng.random(n + SPARE) < 0.35] += away
        fake[rng.random(m + SPARE) < 0.35] -= away
        real[10] = real[3]
        fake[6] = fake[5]
        fake[0] = real[7]
        real.setflags(write=False)
        fake.setflags(write=False)
        _cache[case] = (real, fake)
    return _cache[case]


def table(kind, count, rows, seed):
    """An int32 row table of ``count`` entries into a matrix of ``rows`` rows: None, a permutation (distinct rows, the spare ones
    among them) or a draw with replacement whose first two entries repeat one row."""
    if kind is None:
        return None
    rng = np.random.default_rng(seed)
    if kind == "permute":
        return rng.permutation(rows)[:count].astype(np.int32)
    t = rng.integers(0, rows, count).astype(np.int32)
    t[1] = t[0]
    return t


def gathered(mat, tab, count):
    return mat[:count] if tab is None else mat[tab]


def case_id(case):
    return "n%d-m%d-d%d" % case

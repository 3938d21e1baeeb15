"""The authority of the connected-component entries (plain helper, no test in it; tests/test_components_host.py checks it on the CPU
against closed forms and scipy, tests/test_gpu_components.py holds the kernels to it): the definitions restated in numpy, int64.  It
imports nothing from the package and nothing from scipy.

    mask          value > threshold (NaN is background), per volume and channel of a channel window (first, count)
    connectivity  6, 18, 26: neighbours differ by at most 1 on every axis and on at most 1, 2, 3 axes; nothing connects round the border
    labels        0 at the background; 1 + the rank of a component's smallest raster index among its volume's components
    largest       (label, size) of the component with the most voxels, the lowest label on a tie, (0, 0) for an empty mask
    filters       largest: that component's voxels; min_size n: the voxels of every component with at least n voxels; fill_holes: the
                  mask and every background voxel whose 6-connected background component touches no face of the volume

Labelling is union-find over the list of neighbouring voxel pairs: every root with a smaller root across some pair is hung under the
smallest such root, and all paths are flattened, until no pair has two roots.  A root is always the smallest index of its tree.  Every
comparison of the GPU tests is an equality."""
import functools

import numpy as np

THRESHOLD = 0.5
CX, X0C, NC = 3, 1, 2                           # x [B, D, H, W, 3] read through the window (1, 2): the channel stride is exercised
BATCH = 2
CONNECTIVITIES = (6, 18, 26)
MIN_SIZES = (1, 2, 5)
BRICK = (8, 8, 64)                              # the kernel's brick (d, h, w): what the corner and edge pairs straddle

# (d, h, w): the shapes of tests/mask_reference.py.  (17, 33, 65) crosses a brick edge on every axis (8 on d and h, 64 on w) and leaves
# one voxel past it; (3, 130, 6) and (130, 3, 5) cross sixteen of them on h and on d.  No further shape is needed for the brick.
SHAPES = ((1, 1, 1), (1, 9, 1), (5, 7, 9), (17, 33, 65), (3, 130, 6), (130, 3, 5))
# the mask kinds at position (b, c) = divmod(index, 2) of a case
GROUPS = {"blobs": ("ellipsoids", "speckle15", "speckle30", "speckle50"),
          "paths": ("checker", "serpentine", "serpentine_cut", "comb"),
          "touch": ("corner_pair", "edge_pair", "tie", "ellipsoids2"),
          "holes": ("shell", "shell_tunnel", "shell_diagonal", "nans"),
          "edges": ("full", "empty", "single", "speckle30b")}
CASES = tuple((s, g) for s in SHAPES for g in GROUPS)


def case_id(case):
    return "x".join(map(str, case[0])) + "-" + case[1]


# ---- the definitions -----------------------------------------------------------------------------------------------------------------
def masks(t, first, count, threshold=THRESHOLD):
    """[B, D, H, W, C] values -> bool [B, count, D, H, W]: the binarised channel window."""
    with np.errstate(invalid="ignore"):
        m = np.asarray(t)[..., first:first + count] > np.float32(threshold)
    return np.ascontiguousarray(np.moveaxis(m, -1, 1))


def offsets(connectivity):
    """Half of the neighbourhood: the offsets (dz, dy, dx) that point forward in raster order."""
    axes = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) > (0, 0, 0) and (dz != 0) + (dy != 0) + (dx != 0) <= axes]


def roots(m, connectivity):
    """One volume [D, H, W] bool -> int64 [D, H, W]: at every voxel the smallest raster index of its component (its own at the background)."""
    idx = np.arange(m.size, dtype=np.int64).reshape(m.shape)
    ea, eb = [], []
    for off in offsets(connectivity):
        sa = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip(off, m.shape))
        sb = tuple(slice(max(0, o), n - max(0, -o)) for o, n in zip(off, m.shape))
        both = m[sa] & m[sb]
        ea.append(idx[sa][both]), eb.append(idx[sb][both])
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    parent = np.arange(m.size, dtype=np.int64)
    while True:
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        ra, rb = parent[ea], parent[eb]
        differ = ra != rb
        if not differ.any():
            return parent.reshape(m.shape)
        np.minimum.at(parent, np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ])


def label(m, connectivity):
    """One volume -> (labels int64 [D, H, W], count)."""
    r = roots(m, connectivity)
    found = np.unique(r[m])
    out = np.zeros(m.shape, np.int64)
    out[m] = np.searchsorted(found, r[m]) + 1
    return out, len(found)


def largest(labels):
    """(label, size): the most voxels, the lowest label on a tie, (0, 0) without a component."""
    sizes = np.bincount(labels.reshape(-1))[1:]
    if not len(sizes):
        return 0, 0
    best = 0
    for i, s in enumerate(sizes.tolist()):
        if s > sizes[best]:
            best = i
    return best + 1, int(sizes[best])


def keep_largest(m, connectivity):
    labels, _ = label(m, connectivity)
    best, _ = largest(labels)
    return (labels == best) & m


def keep_min_size(m, connectivity, n):
    labels, _ = label(m, connectivity)
    sizes = np.bincount(labels.reshape(-1))
    return m & (sizes[labels] >= n)


def fill_holes(m):
    """The mask and the background components (6-connected) that touch no face of the volume."""
    labels, _ = label(~m, 6)
    face = np.zeros(m.shape, bool)
    for axis in range(3):
        sl = [slice(None)] * 3
        for end in (0, -1):
            sl[axis] = end
            face[tuple(sl)] = True
    open_labels = np.unique(labels[face & ~m])
    return m | ((labels > 0) & ~np.isin(labels, open_labels))


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
def _grid(shape):
    return np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")


def _ellipsoids(shape, rng, count):
    z, y, x = _grid(shape)
    m = np.zeros(shape, bool)
    for _ in range(count):
        c = [rng.uniform(0, n - 1) for n in shape]
        r = [max(0.8, rng.uniform(0.15, 0.3) * n) for n in shape]
        m |= ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0
        m[tuple(int(round(v)) for v in c)] = True
    return m


def solid(shape):
    """The ellipsoid about the volume's centre with radii of 0.4 extents."""
    z, y, x = _grid(shape)
    c = [(n - 1) / 2.0 for n in shape]
    r = [max(0.8, 0.4 * n) for n in shape]
    return ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0


def _erode(m):
    p = np.pad(m, 1, constant_values=False)
    return p[1:-1, 1:-1, 1:-1] & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:]


def shell(shape):
    """The solid ellipsoid without its twofold 6-erosion: two voxels thick along every face-connected path, so watertight at 6."""
    s = solid(shape)
    return s & ~_erode(_erode(s))


def straddle(shape):
    """The point the corner and edge pairs touch at: the kernel's first brick corner where the volume reaches past it, else the middle."""
    return tuple(b if n > b else n // 2 for n, b in zip(shape, BRICK))


def serpentine(shape, cut=False):
    """One voxel thick: the even rows of every even plane, joined at alternating ends by one voxel of the odd rows, the planes joined by
    one voxel of the odd planes at alternating ends of the path.  ``cut`` removes one voxel from the middle of the middle row."""
    d, h, w = shape
    m = np.zeros(shape, bool)
    m[::2, ::2, :] = True
    for y in range(1, h - 1, 2):
        m[::2, y, (w - 1) if (y // 2) % 2 == 0 else 0] = True
    last_row = (h - 1) // 2 * 2
    last_x = (w - 1) if (last_row // 2) % 2 == 0 else 0                          # where a plane's path ends
    for z in range(1, d - 1, 2):
        if (z // 2) % 2 == 0:
            m[z, last_row, last_x] = True
        else:
            m[z, 0, 0] = True
    if cut:
        m[(d - 1) // 4 * 2, (h - 1) // 4 * 2, w // 2] = False
    return m


def mask_of(kind, shape, seed=0):
    """bool [D, H, W], fixed seeds."""
    rng = np.random.default_rng([seed, sum(map(ord, kind))] + list(shape))
    d, h, w = shape
    if kind in ("ellipsoids", "ellipsoids2"):
        return _ellipsoids(shape, rng, 3)
    if kind.startswith("speckle"):
        return rng.random(shape) < int(kind[7:9]) / 100.0
    if kind == "nans":                                                          # values_of puts NaN over a part of every background: here all of it
        return rng.random(shape) < 0.4
    if kind == "checker":
        z, y, x = np.indices(shape)
        return (z + y + x) % 2 == 0
    if kind in ("serpentine", "serpentine_cut"):
        return serpentine(shape, kind.endswith("cut"))
    if kind == "comb":                                                          # teeth along d that join only in the last plane
        m = np.zeros(shape, bool)
        m[:, ::2, ::2] = True
        m[-1] = True
        return m
    if kind in ("corner_pair", "edge_pair"):
        a, b, c = straddle(shape)
        m = np.zeros(shape, bool)
        if kind == "corner_pair":
            m[max(0, a - 2):a, max(0, b - 2):b, max(0, c - 2):c] = True
            m[a:a + 2, b:b + 2, c:c + 2] = True
        else:
            m[max(0, a - 2):a, max(0, b - 2):b, max(0, c - 2):c + 2] = True
            m[a:a + 2, b:b + 2, max(0, c - 2):c + 2] = True
        return m
    if kind == "tie":                                                           # two components of 8 voxels where the volume has the room
        m = np.zeros(shape, bool)
        m[:2, :2, :2] = True
        m[-2:, -2:, -2:] = True
        return m
    if kind == "shell":
        return shell(shape)
    if kind == "shell_tunnel":                                                  # a face-connected tunnel, one voxel wide, from the centre to the face x = 0
        m = shell(shape)
        m[(d - 1) // 2, (h - 1) // 2, :(w - 1) // 2 + 1] = False
        return m
    if kind == "shell_diagonal":                                                # the cavity (1, 1, 1) meets the open corner voxel (0, 0, 0) only diagonally
        m = np.ones(shape, bool)
        m[0, 0, 0] = False
        if min(shape) >= 3:
            m[1, 1, 1] = False
        return m
    if kind == "full":
        return np.ones(shape, bool)
    if kind == "single":
        m = np.zeros(shape, bool)
        m[tuple(int(rng.integers(0, n)) for n in shape)] = True
        return m
    assert kind == "empty", kind
    return np.zeros(shape, bool)


def values_of(m, rng, all_nan=False):
    """float32 values whose binarisation at THRESHOLD is m: the mask in (0.5, 1], the background in [0, 0.5] with exact 0.5 and NaN in it."""
    u = rng.random(m.shape)
    v = np.where(m, 0.5 + 0.5 * (1.0 - u) + 1e-3, 0.5 * u).astype(np.float32)
    bg = np.flatnonzero(~m.reshape(-1))
    flat = v.reshape(-1)
    flat[bg[::7]] = 0.5                                                         # not above the threshold
    flat[bg if all_nan else bg[3::11]] = np.nan                                 # background
    return v


@functools.lru_cache(maxsize=None)
def make_case(case):
    """x [B, D, H, W, CX] float32; the channels outside the window hold values on both sides of the threshold."""
    shape, group = case
    rng = np.random.default_rng([11] + list(shape) + [len(group), ord(group[0])])
    x = rng.random((BATCH,) + shape + (CX,)).astype(np.float32)
    for i, kind in enumerate(GROUPS[group]):
        b, c = divmod(i, NC)
        x[b, ..., X0C + c] = values_of(mask_of(kind, shape), rng, all_nan=kind == "nans")
    x.setflags(write=False)
    return x


def _per_volume(m, fn):
    return np.stack([np.stack([fn(m[b, c]) for c in range(m.shape[1])]) for b in range(m.shape[0])])


def ndhwc(planar):
    """bool [B, nc, D, H, W] -> float32 [B, D, H, W, nc]: what a filter entry writes."""
    return np.ascontiguousarray(np.moveaxis(planar, 1, -1)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(case, connectivity):
    """dict: m (bool [B, nc, D, H, W]), labels (int64, same shape), count (int64 [B, nc]), largest (int64 [B, nc, 2]), filters: a dict
    of bool [B, nc, D, H, W] under "largest", ("min_size", n) for n of MIN_SIZES, and "fill_holes"."""
    x = make_case(case)
    m = masks(x, X0C, NC)
    for i, kind in enumerate(GROUPS[case[1]]):
        b, c = divmod(i, NC)
        assert np.array_equal(m[b, c], mask_of(kind, case[0])), kind
    labels = _per_volume(m, lambda v: label(v, connectivity)[0])
    count = labels.reshape(BATCH, NC, -1).max(-1)
    big = np.array([[largest(labels[b, c]) for c in range(NC)] for b in range(BATCH)], np.int64)
    filters = {"largest": _per_volume(m, lambda v: keep_largest(v, connectivity)), "fill_holes": _per_volume(m, fill_holes)}
    for n in MIN_SIZES:
        filters[("min_size", n)] = _per_volume(m, lambda v: keep_min_size(v, connectivity, n))
    return dict(m=m, labels=labels, count=count, largest=big, filters=filters)


def clean(m, *, keep_largest_=True, fill=True, min_size=None, connectivity=6):
    """One volume through the stages in the order min_size, largest, fill_holes."""
    if min_size is not None:
        m = keep_min_size(m, connectivity, min_size)
    if keep_largest_:
        m = keep_largest(m, connectivity)
    if fill:
        m = fill_holes(m)
    return m

"""What the GPU tests of the in-kernel N(0,1) stream share (plain helper, no test in it): the seeds, the bar on z, and the comparison
of a device draw with oracle/ref_philox.py's float64 evaluation, element by element.

The bar.  The counter, the key and the float32 uniforms are restated exactly, so a device draw differs from the float64 reference
only by the device library's logf, sqrtf, sinf and cosf, none of them correctly rounded, and the two products' roundings.  The worst
|z_device - z_f64| over every case of tests/test_gpu_philox.py and of section 3 of tests/test_gpu_sampler_kernels.py was measured on
an MI355X (docs/EXPERIMENTS.md, "The Philox stream against a host reference": per entry), and Z_BAR is four times that worst value:
the counters of the cases sample the arguments near u -> 1 and near multiples of pi/2 only sparsely.  It is an absolute error on z and
must stay below Z_BAR_CAP = 1e-5, a condition and no measurement: a wrong counter or key word gives an error of order 1, a wrong
uniform mapping or angle at least 1e-3 on most elements."""
import numpy as np

SEEDS = [0, 1, 987654321, 1 << 32, 0x0123456789ABCDEF, 1 << 63, (1 << 64) - 1]
SEED64 = 0x0123456789ABCDEF              # the seed of the cases that need one: both key words count
Z_BAR_CAP = 1e-5
Z_BAR = 4 * 5.94e-7                      # four times the worst measured error (dm3d_randn's; the other entries 4.5e-7 to 5.4e-7)
assert Z_BAR <= Z_BAR_CAP


def seed_words(seed):
    """The key as a chain writes it into its int64 seed buffer: seed - 2^64 from 2^63 up (one element; 8 bytes for seed_dev)."""
    seed = int(seed) & (2 ** 64 - 1)
    return np.array([seed - (1 << 64) if seed >= (1 << 63) else seed], np.int64)


def z_close(worst, name, got, ref, bar=Z_BAR):
    """Every element of the device draw `got` (float32, or float64 where a test had to recover it) against the float64 reference `ref`
    (same shape) at the absolute bar (a scalar or one per element); the worst error is printed and kept in `worst` under 'philox <name>'."""
    got, ref = np.asarray(got), np.asarray(ref, np.float64)
    assert got.dtype in (np.float32, np.float64) and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
    assert np.isfinite(got).all(), name
    err = np.abs(got.astype(np.float64) - ref)
    e = float(err.max())
    key = f"philox {name} (|z - z_f64|)"
    worst[key] = max(worst.get(key, 0.0), e)
    print(f"{key}: {e:.3e}")
    bad = err >= bar
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} elements off by more than the bar, worst {e:.3e}, first at {np.argwhere(bad)[0].tolist()}"


def independent(a, b):
    """Two draws that share nothing: var(a - b) = 2."""
    return float((np.asarray(a, np.float64) - np.asarray(b, np.float64)).std()) > 1.0

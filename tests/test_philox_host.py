"""The host reference of the kernels' N(0,1) stream (oracle/ref_philox.py) on its own, without a GPU: the Philox4x32-10 known-answer
vectors of the Random123 distribution, the edges of the float32 uniform mapping, the sensitivity of the draw to every counter and key
word (the high word of the float4 index included, which no GPU test reaches: it needs more than 2^34 elements), the moments and
correlations of the reference over 2^20 counters, and the counter layout of the five per-entry helpers."""
import numpy as np
import pytest

from oracle import ref_philox as rp

KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.fixture(scope="module")
def million():
    """The reference over 2^20 counters, [2^20, 4] float64: computed once, read by the tests below, never written."""
    z = rp.normal4(np.arange(1 << 20, dtype=np.uint64), 517, rp.STREAM_DDIM, 987654321)
    z.setflags(write=False)
    return z


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answers(ctr, key, want):
    got = rp.philox4x32_10(*ctr, *key)
    assert all(g.dtype == np.uint32 for g in got)
    assert tuple(int(g) for g in got) == want
    # the same through arrays, next to another counter: no lane sees its neighbour
    arr = rp.philox4x32_10(*(np.array([c, 7], np.uint32) for c in ctr), *key)
    assert tuple(int(g[0]) for g in arr) == want


def test_known_answer_through_normal4():
    """normal4 splits idx and seed low word first: the third vector's counter and key, put together as 64-bit values."""
    idx = np.array([(0x85A308D3 << 32) | 0x243F6A88], np.uint64)
    seed = (0x299F31D0 << 32) | 0xA4093822
    want = rp.box_muller(*rp.uniforms(*(np.array([w], np.uint32) for w in KAT[2][2])))
    assert np.array_equal(rp.normal4(idx, 0x13198A2E, 0x03707344, seed), want)
    assert np.array_equal(rp.normal4(idx, 0x13198A2E, 0x03707344, seed - (1 << 64)), want)      # a key held as a negative int64


def test_uniform_edges():
    words = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF], np.uint32)
    u0, u1, u2, u3 = rp.uniforms(words, words, words, words)
    assert all(u.dtype == np.float32 for u in (u0, u1, u2, u3))
    assert np.array_equal(u0, u2) and np.array_equal(u1, u3)
    assert u0[0] == np.float32(2.0 ** -33) and u1[0] == 0
    assert u0[-1] == np.float32(1.0) and u1[-1] == np.float32(1.0)
    assert (u0 > 0).all() and (u0 <= 1).all() and (u1 >= 0).all() and (u1 <= 1).all()
    # the largest word below which the float32 conversion does not round up to 2^32
    assert u0[4] < 1 and u0[5] == 1
    z = rp.box_muller(u0, u1, u2, u3)
    assert np.isfinite(z).all()
    r_max = np.sqrt(-2 * np.log(2.0 ** -33))
    assert abs(z[0, 0] - r_max) < 1e-12 and z[0, 1] == 0                     # c = 0: the largest radius, angle 0
    assert (z[-1] == 0).all()                                                # c = 0xffffffff: u0 == 1, r == 0
    # u1 == 1: the angle is the float32 2 pi, whose sine is not 0
    one = np.float32(1.0)
    z1 = rp.box_muller(np.float32(0.5), one, np.float32(0.5), one)
    r = np.sqrt(-2 * np.log(0.5))
    assert z1[0] == r * np.cos(np.float64(rp.TWO_PI_F32)) and z1[1] == r * np.sin(np.float64(rp.TWO_PI_F32)) and z1[1] != 0
    # no word gives u0 == 0: the mapping is monotone and its smallest value is positive
    assert np.all(np.diff(rp.uniforms(np.arange(0, 1 << 12, dtype=np.uint32), 0, 0, 0)[0]) > 0)


def test_every_counter_and_key_word_counts():
    n = 4096
    idx = np.arange(n, dtype=np.uint64)
    s0, s1, seed = 517, rp.STREAM_DDIM, 0x0123456789ABCDEF
    base = rp.normal4(idx, s0, s1, seed)
    others = {"idx low word": rp.normal4(idx + np.uint64(n), s0, s1, seed),
              "idx high word": rp.normal4(idx + np.uint64(1 << 32), s0, s1, seed),
              "s0": rp.normal4(idx, s0 + 1, s1, seed),
              "s1": rp.normal4(idx, s0, s1 + 1, seed),
              "key low word": rp.normal4(idx, s0, s1, seed ^ 1),
              "key high word": rp.normal4(idx, s0, s1, seed ^ (1 << 40)),
              "s0 and s1 swapped": rp.normal4(idx, s1, s0, seed)}
    for name, z in others.items():
        assert float((base - z).std()) > 1.0, name                           # independent draws: var(a - b) = 2


def test_moments_and_correlations(million):
    z = million
    assert np.isfinite(z).all()
    assert abs(float(z.mean())) < 5e-3 and abs(float(z.std()) - 1) < 5e-3
    for k in range(4):
        assert abs(float(z[:, k].mean())) < 5e-3 and abs(float(z[:, k].std()) - 1) < 5e-3, k
    corr = np.corrcoef(z.T)
    print("correlations of the four lanes:\n", corr)
    assert np.abs(corr - np.eye(4)).max() < 5e-3                             # the two normals of a pair, and the two pairs
    # neighbouring counters are uncorrelated too
    assert abs(float(np.corrcoef(z[:-1, 0], z[1:, 0])[0, 1])) < 5e-3


def test_f32_order_is_close_to_f64(million):
    z32 = rp.normal4(np.arange(1 << 16, dtype=np.uint64), 517, rp.STREAM_DDIM, 987654321, order="f32")
    assert z32.dtype == np.float32
    err = float(np.abs(z32 - million[:1 << 16]).max())
    print(f"float32 host libm against float64: {err:.2e}")
    assert err < 5e-6


def test_helpers_layout():
    P, seed = 1004, (1 << 63) + 12345
    for fn, stream in ((rp.ddpm, rp.STREAM_DDPM), (rp.ddim, rp.STREAM_DDIM), (rp.dpm_sde, rp.STREAM_DPM_SDE), (rp.edit, rp.STREAM_EDIT)):
        a, b = fn(4, P, 517, seed), fn(1, 4 * P, 517, seed)
        assert a.shape == (4, P) and np.array_equal(a.reshape(-1), b.reshape(-1)), fn.__name__
        assert np.array_equal(b.reshape(-1, 4), rp.normal4(np.arange(P, dtype=np.uint64), 517, stream, seed)), fn.__name__
        # one word 2 per sample: sample b keeps its own float4 indices b * per4 ...
        taus = np.array([3, 517, 999, 517])
        c = fn(4, P, taus, seed)
        assert np.array_equal(c[1], a[1]) and np.array_equal(c[3], a[3]) and float((c[0] - a[0]).std()) > 1 and float((c[2] - a[2]).std()) > 1
        want = rp.normal4(np.arange(2 * (P // 4), 3 * (P // 4), dtype=np.uint64), 999, stream, seed)
        assert np.array_equal(c[2], want.reshape(-1)), fn.__name__
    flat = rp.randn(4 * P, seed, 0x7FFFFFFF)
    assert np.array_equal(flat.reshape(-1, 4), rp.normal4(np.arange(P, dtype=np.uint64), 0x7FFFFFFF, rp.STREAM_RANDN, seed))
    assert np.array_equal(rp.randn(8, seed, 0x7FFFFFFF), flat[:8])           # a shorter tensor is a prefix
    assert float((rp.randn(4 * P, seed, 0xFFFFFFFF) - flat).std()) > 1
    # the five constants are five
    assert len({rp.STREAM_RANDN, rp.STREAM_DDPM, rp.STREAM_DDIM, rp.STREAM_DPM_SDE, rp.STREAM_EDIT}) == 5
    # ddpm: t == 0 draws nothing; a negative level (the clean row's -1) is the word 0xffffffff
    z = rp.ddpm(2, 8, [0, 5], seed)
    assert (z[0] == 0).all() and (z[1] != 0).all()
    assert np.array_equal(rp.edit(1, 8, -1, seed), rp.edit(1, 8, 0xFFFFFFFF, seed))

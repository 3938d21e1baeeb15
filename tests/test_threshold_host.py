"""CPU tier of dynamic thresholding (dm3d_x0_threshold, the x0_bound field of the DDIM / DPM-Solver++ descriptors, the
dynamic_threshold / threshold_max keywords): the ABI, the argument rules, the host rank table and the kernels' build (no kernel is launched)."""
import ctypes
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d-condtional-stable-diffusion_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SHAPE = (2, 8, 8, 8, 4)


def _model(T=20, B=2):
    from dm3d_amd.networks import conditional_dm3d
    return conditional_dm3d.DiffusionModel(8, 1024, 4, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B),
                                           device="cpu")


def test_abi_entries_exported(built_library):
    from dm3d_amd import _lib
    handle = ctypes.CDLL(built_library)
    for name in ("dm3d_x0_threshold", "dm3d_x0_threshold_scratch_bytes"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111                         # additive: the version stays


@pytest.mark.parametrize("c_name,mirror", [("dm3d_thresh_desc", "ThreshDesc"), ("dm3d_ddim_desc", "DdimDesc"), ("dm3d_dpm_desc", "DpmDesc")])
def test_struct_layouts_match_the_ctypes_mirrors(c_name, mirror, tmp_path):
    from dm3d_amd import _lib
    cls = getattr(_lib, mirror)
    fields = [name for name, _ in cls._fields_]
    if mirror != "ThreshDesc":
        assert fields[-1] == "x0_bound"                                                  # appended: every older offset stays
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dm3d.h"\nint main(){printf("%zu", sizeof(' + c_name + '));\n'
                   + "".join(f'printf(" %zu", offsetof({c_name}, {f}));\n' for f in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, *offs = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert size == ctypes.sizeof(cls)
    assert offs == [getattr(cls, f).offset for f in fields]


def test_plain_c_program_calls_the_threshold_entry(built_library, tmp_path):
    """A C99 translation unit including only dm3d.h links; a null or empty descriptor is refused before any device call."""
    src = tmp_path / "thr.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "dm3d.h"
int main(void) {
    dm3d_thresh_desc d;
    memset(&d, 0, sizeof d);
    int rc0 = dm3d_x0_threshold(NULL, NULL);
    printf("%d|%s\n", rc0, dm3d_last_error());
    int rc1 = dm3d_x0_threshold(&d, NULL);
    printf("%d|%s\n", rc1, dm3d_last_error());
    printf("%lld\n", (long long)dm3d_x0_threshold_scratch_bytes(2, 2048));
    return 0;
}
''')
    exe = tmp_path / "thr"
    libdir = os.path.dirname(built_library)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-ldm3d_hip", f"-Wl,-rpath,{libdir}"], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for line in lines[:2]:
        rc, text = line.split("|", 1)
        assert int(rc) != 0 and "thresh" in text
    assert "null descriptor" in lines[0] and "non-null" in lines[1]
    assert int(lines[2]) >= 2 * 2048 * 4


def test_threshold_argument_validation_needs_no_gpu(built_library):
    from dm3d_amd import _lib

    def refused(d, word):
        return _lib.lib().dm3d_x0_threshold(ctypes.byref(d), None) != 0 and word in _lib.lib().dm3d_last_error()

    def desc():
        d = _lib.ThreshDesc()
        d.x = d.eps = d.coef = d.pos = d.rank = d.frac = d.smax = d.bound = d.scratch = 4096
        d.batch, d.per_sample, d.rows = 2, 8, 4
        return d

    d = desc()
    d.per_sample = 6
    assert refused(d, b"per_sample")
    d = desc()
    d.batch = 65536
    assert refused(d, b"batch")
    d = desc()
    d.rows = 0
    assert refused(d, b"rows")
    for name in ("rank", "frac", "smax", "bound", "scratch"):
        d = desc()
        setattr(d, name, None)
        assert refused(d, b"non-null") and name.encode() in _lib.lib().dm3d_last_error(), name
    for name in ("x", "eps", "coef", "pos"):
        d = desc()
        setattr(d, name, None)
        assert refused(d, b"non-null"), name
    for name in ("x", "eps", "coef", "scratch"):
        d = desc()
        setattr(d, name, 4100)
        assert refused(d, b"aligned"), name
    # the extended update descriptors still refuse what they refused, with x0_bound set or not
    u = _lib.DpmDesc()
    u.x = u.eps = u.coef = u.pos = u.hist = u.x0_bound = 4096
    u.batch, u.per_sample, u.rows, u.mode = 2, 6, 4, 1
    assert _lib.lib().dm3d_dpm_update(ctypes.byref(u), None) != 0 and b"per_sample" in _lib.lib().dm3d_last_error()


def test_scratch_bytes_is_monotone(built_library):
    from dm3d_amd import _lib
    f = _lib.lib().dm3d_x0_threshold_scratch_bytes
    for per in (4, 2048, 262144):
        sizes = [f(b, per) for b in (1, 2, 3, 32, 64)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    for b in (1, 32):
        sizes = [f(b, per) for per in (4, 8, 2048, 2052, 262144)]
        assert all(a < b_ for a, b_ in zip(sizes, sizes[1:]))
        assert all(s % 16 == 0 for s in sizes)
    assert f(32, 262144) >= 32 * 262144 * 4                                             # room for the stashed magnitudes


@pytest.mark.parametrize("N,p,i,f", [
    (4, 0.5, 1, 0.5),                                     # q = 1.5
    (2048, 0.995, 2036, 0.7650000000001),                 # q = 0.995 * 2047 = 2036.765 in float64; q - i as float64 prints it
    (2048, 1.0, 2047, 0.0),                               # the maximum: v_{i+1} is never needed
    (262144, 0.995, 260832, 0.28500000000349246),         # q = 260832.285
])
def test_host_rank_table(N, p, i, f):
    """f is float32(q - i) with q and the difference in float64: one rounding, so the comparison is exact (q in float32 would give
    0.76501465 and 0.28125 for the two 0.995 cases)."""
    from dm3d_amd.diffusion import threshold_rank, threshold_tables
    gi, gf = threshold_rank(N, p)
    assert gi == i and isinstance(gf, np.float32)
    assert gf == np.float32(f) and 0 <= float(gf) < 1
    if p == 1.0:
        assert gi == N - 1 and float(gf) == 0.0
    rank, frac, smax = threshold_tables(3, N, p)
    assert rank.dtype == np.int32 and frac.dtype == np.float32 and smax.dtype == np.float32
    assert rank.tolist() == [i] * 3 and frac.tolist() == [float(gf)] * 3
    assert np.all(smax == np.finfo(np.float32).max)
    rank, frac, smax = threshold_tables(2, N, [p, 1.0], [1.0, 7.5])
    assert rank.tolist() == [i, N - 1] and frac[1] == 0 and smax.tolist() == [1.0, 7.5]


def test_generate_edit_and_sampler_argument_rules():
    m = _model(20)
    x0 = np.zeros(SHAPE, np.float32)
    calls = (lambda **kw: m.generate(SHAPE, context_value=1, **{"sampler" if k == "kind" else k: v for k, v in kw.items()}),
             lambda **kw: m.edit(x0, 1, **{"sampler" if k == "kind" else k: v for k, v in kw.items()}),
             lambda **kw: m.sampler(SHAPE, 1, **kw))
    for g in calls:
        with pytest.raises(ValueError, match="belong to"):
            g(dynamic_threshold=0.99)                                                    # the DDPM chain
        with pytest.raises(ValueError, match="clip_x0"):
            g(kind="ddim", num_steps=5, clip_x0=False, dynamic_threshold=0.99)
        with pytest.raises(ValueError, match="clip_x0"):
            g(kind="dpmpp", num_steps=5, clip_x0=False, dynamic_threshold=0.99)
        for kind in ("ddpm", "ddim", "dpmpp"):
            with pytest.raises(ValueError, match="needs dynamic_threshold"):
                g(kind=kind, threshold_max=2.0, **({} if kind == "ddpm" else dict(num_steps=5)))
        for kind in ("ddim", "dpmpp"):
            for p in (0.0, -0.1, 1.0001, float("nan"), float("inf"), [0.5, 0.0]):
                with pytest.raises(ValueError, match="dynamic_threshold"):
                    g(kind=kind, num_steps=5, dynamic_threshold=p)
            for cap in (0.999, 0.0, -1.0, float("nan"), float("inf"), 1e39, [2.0, 0.5]):
                with pytest.raises(ValueError, match="threshold_max"):
                    g(kind=kind, num_steps=5, dynamic_threshold=0.99, threshold_max=cap)
            with pytest.raises(ValueError, match="one value or one per volume"):
                g(kind=kind, num_steps=5, dynamic_threshold=[0.9, 0.9, 0.9])
            with pytest.raises(ValueError, match="one value or one per volume"):
                g(kind=kind, num_steps=5, dynamic_threshold=0.9, threshold_max=[2.0, 2.0, 2.0])


def test_single_call_argument_rules():
    m = _model(20)
    x = np.zeros(SHAPE, np.float32)
    with pytest.raises(ValueError, match="clip_x0"):
        m.ddim_step(x, x, 5, 3, clip_x0=False, dynamic_threshold=0.9)
    with pytest.raises(ValueError, match="clip_x0"):
        m.dpm_step(x, x, 5, 3, clip_x0=False, dynamic_threshold=0.9)
    with pytest.raises(ValueError, match="needs dynamic_threshold"):
        m.ddim_step(x, x, 5, 3, threshold_max=2.0)
    with pytest.raises(ValueError, match="needs dynamic_threshold"):
        m.dpm_step(x, x, 5, 3, threshold_max=2.0)
    with pytest.raises(ValueError, match="dynamic_threshold"):
        m.x0_threshold(x, x, 5, 1.5)
    with pytest.raises(ValueError, match="threshold_max"):
        m.x0_threshold(x, x, 5, 0.9, 0.5)
    with pytest.raises(ValueError):
        m.x0_threshold(x, x, 20, 0.9)                                                    # t outside the schedule
    with pytest.raises(ValueError):
        m.x0_threshold(x, x[:1], 5, 0.9)
    with pytest.raises(ValueError, match="one value or one per volume"):
        m.x0_threshold(x, x, 5, [0.9, 0.9, 0.9])


def test_signatures_and_graph_kinds():
    from dm3d_amd import diffusion
    from dm3d_amd.networks import conditional_dm3d
    M = conditional_dm3d.DiffusionModel
    for fn in (M.generate, M.edit, M.sampler, M.ddim_step, M.dpm_step):
        p = inspect.signature(fn).parameters
        for name in ("dynamic_threshold", "threshold_max"):
            assert p[name].kind == inspect.Parameter.KEYWORD_ONLY and p[name].default is None
    assert list(inspect.signature(M.x0_threshold).parameters)[1:6] == ["x_t", "pred_noise", "t", "dynamic_threshold", "threshold_max"]
    assert len(diffusion._CHAINS) == 12 and all(len(k) == 3 for k in diffusion._CHAINS)  # no new classes, no fourth axis
    # the graph key: a plain chain's is its KIND as before, a thresholded chain's is its own
    for cls in (diffusion.DdimSampler, diffusion.DpmEditSampler, diffusion.GuidedDpmSampler, diffusion.GuidedDdimEditSampler):
        plain, thr = SimpleNamespace(KIND=cls.KIND, threshold=None), SimpleNamespace(KIND=cls.KIND, threshold=(1, 2, 3))
        assert diffusion.Sampler.graph_kind.fget(plain) == cls.KIND
        assert diffusion.Sampler.graph_kind.fget(thr) not in {c.KIND for c in diffusion._CHAINS.values()}
    assert diffusion.Sampler.threshold is None


class _Stub:
    """Records what generate_sharded asks of DiffusionModel.generate."""
    device = torch.device("cpu")

    def generate(self, shape, last_step=0, context_value=None, **kw):
        self.shape, self.kw = tuple(shape), kw
        return torch.zeros(shape)


def test_generate_sharded_forwards_the_keywords():
    from dm3d_amd import parallel
    m = _Stub()
    parallel.generate_sharded(m, (5, 2, 2, 2, 4), 0, 1, seed=7, sampler="ddim", num_steps=8, dynamic_threshold=0.995, threshold_max=4.0)
    assert m.shape == (5, 2, 2, 2, 4)
    assert m.kw == dict(seed=7, sampler="ddim", num_steps=8, dynamic_threshold=0.995, threshold_max=4.0)
    per = [0.9, 0.91, 0.92, 0.93, 0.94]
    parallel.generate_sharded(m, (5, 2, 2, 2, 4), 0, 1, sampler="dpmpp", num_steps=8, dynamic_threshold=per, threshold_max=np.arange(1, 6.0))
    assert np.asarray(m.kw["dynamic_threshold"]).tolist() == per and np.asarray(m.kw["threshold_max"]).tolist() == [1, 2, 3, 4, 5]
    with pytest.raises(ValueError, match="dynamic_threshold"):
        parallel.generate_sharded(m, (5, 2, 2, 2, 4), 0, 1, sampler="ddim", dynamic_threshold=[0.9, 0.9])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_build_without_scratch_or_spills(tmp_path):
    """The five selection kernels for gfx950: no scratch, no spill, LDS within the 16 KiB of pass 1's histogram; the update kernels
    with the x0_bound path: still no scratch, no spill, no LDS."""
    found = {}
    for name in ("dm3d_thresh", "dm3d_ddim", "dm3d_dpm"):
        out = str(tmp_path / (name + ".s"))
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function",
                        "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(CSRC, name + ".hip"), "-o", out], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
        for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)[\s\S]*?\.name:\s+(\S+)[\s\S]*?\.private_segment_fixed_size:\s+(\d+)"
                             r"[\s\S]*?\.sgpr_spill_count:\s+(\d+)[\s\S]*?\.vgpr_count:\s+(\d+)[\s\S]*?\.vgpr_spill_count:\s+(\d+)", text):
            lds, kname, private, sspill, vgpr, vspill = m.groups()
            found[kname] = dict(lds=int(lds), private=int(private), sspill=int(sspill), vgpr=int(vgpr), vspill=int(vspill))
    thresh = {k: v for k, v in found.items() if "thresh_" in k}
    assert len(thresh) == 5, sorted(found)
    for k, v in thresh.items():
        assert v["private"] == 0 and v["sspill"] == 0 and v["vspill"] == 0 and v["lds"] <= 16384 and v["vgpr"] <= 64, (k, v)
    updates = {k: v for k, v in found.items() if "ddim_kernel" in k or "dpm_kernel" in k}
    assert len(updates) == 2
    for k, v in updates.items():
        assert v["private"] == 0 and v["vspill"] == 0 and v["lds"] == 0 and v["vgpr"] <= 64, (k, v)

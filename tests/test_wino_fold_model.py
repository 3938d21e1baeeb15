"""The pad step's mixed A fragment of the Winograd-x conv (dm3d_conv_h3w.hip: lane half 0 the hi piece of tap (0, 2), half 1 the lo piece of
the same records) in the LDS model of tools/lds_model.py: conflict-free in the layout the kernel uses, like every other fragment read."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lds_model as m          # noqa: E402


def test_mixed_fragment_reads_conflict_free():
    perm, s = (0, 1, 3, 2), (0, 0, 2, 2)
    for wave in range(4):
        for g in (0, 1):
            addr = m.a_read_mixed(wave, g, perm, s)
            assert m.cycles_read_b128(addr) == 4
            hi = m.a_read(wave, 3, 0, g, perm, s)
            assert addr[:32] == hi[:32] and all(addr[32 + l] == hi[l] ^ 32 for l in range(32))


def test_kernel_source_reads_the_modelled_addresses():
    src = open(os.path.join(ROOT, "3d-condtional-stable-diffusion_amd", "csrc", "dm3d_conv_h3w.hip")).read()
    assert "v_subrev_u32 %0, %2, %1" in src and '"n"(DZB)' in src, "half 1 steps back from the voxels of (1, 2) to those of (0, 2)"
    assert "v_xor_b32 %0, 32, %0" in src, "... and takes their lo piece"
    assert "0xffffffff00000000ull" in src, "... in lanes 32-63 only"

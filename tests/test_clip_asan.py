"""CPU-only: the host halves of dm3d_grad_scale, dm3d_adam_scaled and dm3d_adam_ema under AddressSanitizer, in a stand-alone program (the pattern of
tests/test_host_asan.py).  Nothing here needs a device, and no device code is instrumented."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clip_entries_host_side_under_address_sanitizer(tmp_path):
    """The two translation units the entries need (dm3d_train.hip and dm3d_api.hip: the error text) rebuilt with the sanitizer on the
    host code only (-fno-gpu-sanitize), linked into a library of their own and driven by tests/clip_asan.c: every documented
    precondition of the three entries on heap buffers of exactly the documented sizes.  Each call is refused with a message naming the
    entry, and the program ends without a sanitizer report."""
    csrc = os.path.join(ROOT, "3d-condtional-stable-diffusion_amd", "csrc")
    srcs = ["dm3d_train.hip", "dm3d_api.hip"]
    flags = ["-O1", "-g", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
             "-Wno-unused-function", "-Wno-option-ignored", "-ffp-contract=off", "-fsanitize=address", "-fno-gpu-sanitize",
             "-fno-omit-frame-pointer"]
    procs = [subprocess.Popen(["/opt/rocm/bin/hipcc", *flags, "-c", os.path.join(csrc, f), "-o", str(tmp_path / (f + ".o"))],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for f in srcs]
    for f, p in zip(srcs, procs):
        out, _ = p.communicate()
        assert p.returncode == 0, f + "\n" + out
    so = tmp_path / "libdm3d_clip.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "-shared", "-fPIC", "--offload-arch=gfx950", "-fsanitize=address", "-fno-gpu-sanitize",
                    "-Wno-option-ignored", "-o", str(so)] + [str(tmp_path / (f + ".o")) for f in srcs], check=True, capture_output=True)
    exe = tmp_path / "clip_asan"
    subprocess.run(["/opt/rocm/lib/llvm/bin/clang", "-fsanitize=address", "-fno-gpu-sanitize", "-g", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "clip_asan.c"), "-o", str(exe), "-L", str(tmp_path), "-ldm3d_clip", "-lm",
                    f"-Wl,-rpath,{tmp_path}"], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    got = re.search(r"refused (\d+) of (\d+);", r.stdout)
    assert got and got.group(1) == got.group(2) == "68", r.stdout
    assert "AddressSanitizer" not in r.stderr

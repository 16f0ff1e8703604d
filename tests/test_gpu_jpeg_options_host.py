"""GPU: a 4:4:4 file with optimised tables and a restart marker per MCU row from a host with no Python and no torch in the process --
examples/jpeg_options_host.cpp is built with hipcc and run against the in-tree libnesr_hip.so (nesr_jpeg_scratch_bytes_ex,
nesr_jpeg_encode_ex_u8).  The file it writes is the specification's (tests/jpeg_options_ref.py), byte for byte, and the length and
FNV-1a hash it prints are that file's, also when its first output buffer is too small."""
import os
import shutil
import subprocess

import pytest

from tests import jpeg_cases, jpeg_options_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & (2 ** 64 - 1)
    return h


def test_cpp_host_writes_the_specifications_file(tmp_path, cuda_device):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "jpeg_options_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "jpeg_options_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    for (kind, h, w, q, cap) in (("impulses", 200, 333, 95, None), ("impulses", 200, 333, 30, None), ("noise", 37, 53, 100, 1000)):
        src, dst = tmp_path / "in.raw", tmp_path / "out.jpg"
        img = jpeg_cases.content(kind, h, w, 3)
        img.tofile(src)
        cmd = ["timeout", "-k", "10", "60", exe, lib, str(src), str(h), str(w), str(q), str(dst)] + ([str(cap)] if cap else [])
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=90)
        assert out.returncode == 0, out.stdout + out.stderr
        print(out.stdout)
        want = jpeg_options_ref.encode_jpeg(img, q, "rgb", "4:4:4", True, -(-w // 8))
        assert f"the file needs {len(want)} bytes" in out.stdout
        assert f"{len(want)} bytes, fnv1a {_fnv1a(want):016x}" in out.stdout
        assert ("did not fit" in out.stdout) == (len(want) > (cap or h * w * 3 // 2 + 4096))
        with open(dst, "rb") as f:
            assert f.read() == want, (kind, h, w, q)

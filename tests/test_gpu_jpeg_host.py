"""GPU: cv2.imwrite's JPEG file from a host with no Python and no torch in the process -- examples/jpeg_host.cpp is built with hipcc
(only for hipMalloc / hipMemcpy) and run against the in-tree libnesr_hip.so: nesr_jpeg_scratch_bytes, nesr_jpeg_header,
nesr_jpeg_encode_u8.  The file it writes is the specification's (tests/jpeg_ref.py), byte for byte, also when its first output
buffer is too small and it runs again at the size the device reported."""
import os
import shutil
import subprocess

import pytest

from tests import jpeg_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_host_writes_the_specifications_file(tmp_path, cuda_device):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "jpeg_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "jpeg_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    for (kind, h, w, c, q, cap) in (("impulses", 200, 333, 3, 95, None), ("noise", 37, 53, 1, 30, None), ("noise", 37, 53, 3, 100, 1000)):
        src, dst = tmp_path / "in.raw", tmp_path / "out.jpg"
        jpeg_cases.content(kind, h, w, c).tofile(src)
        cmd = ["timeout", "-k", "10", "60", exe, lib, str(src), str(h), str(w), str(c), str(q), str(dst)] + ([str(cap)] if cap else [])
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=90)
        assert out.returncode == 0, out.stdout + out.stderr
        print(out.stdout)
        want = jpeg_cases.spec(kind, h, w, c, q)[0]
        assert f"the file needs {len(want)} bytes ({623 if c == 3 else 328} of them the header)" in out.stdout
        assert ("did not fit" in out.stdout) == (cap is not None)
        with open(dst, "rb") as f:
            assert f.read() == want, (kind, h, w, c, q)

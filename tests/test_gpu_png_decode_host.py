"""GPU: cv2.imread's PNG frame from a host with no Python and no torch in the process -- examples/png_decode_host.cpp is built with
hipcc (only for hipMalloc / hipMemcpy) and run against the in-tree libnesr_hip.so: nesr_png_parse, nesr_png_decode, then
nesr_png_encode.  The file it writes decodes to the input's frame."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import png_cases, png_decode_cases as cases, png_decode_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_host_decodes_and_writes_the_frame_back(tmp_path, cuda_device):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "png_decode_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "png_decode_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    foreign = dict((c[0], c) for c in cases.foreign())
    files = [(png_cases.spec("runs", 33, 130, 4, 16)[0], png_cases.content("runs", 33, 130, 4, 16)),          # our own: 2 segments
             foreign["70x320x3x8-gradient-full"][1:], foreign["37x53x1x16-runs-full"][1:], foreign["37x53x4x8-impulses-l9"][1:]]
    src, dst = tmp_path / "in.png", tmp_path / "out.png"
    for data, frame in files:
        src.write_bytes(data)
        out = subprocess.run(["timeout", "-k", "10", "60", exe, lib, str(src), str(dst)], capture_output=True, text=True, timeout=90)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "contiguous" in out.stdout
        got = ref.decode(dst.read_bytes())
        assert got.dtype == frame.dtype and np.array_equal(got, frame)
    src.write_bytes(foreign["70x320x3x8-impulses-cut100"][1])                  # arbitrary IDAT cuts: refused with a message, no launch
    out = subprocess.run(["timeout", "-k", "10", "60", exe, lib, str(src), str(dst)], capture_output=True, text=True, timeout=90)
    assert out.returncode == 4 and "spans an IDAT boundary" in out.stderr
    src.write_bytes(cases.corrupt()[3][1])                                      # a wrong Adler-32: the status word
    out = subprocess.run(["timeout", "-k", "10", "60", exe, lib, str(src), str(dst)], capture_output=True, text=True, timeout=90)
    assert out.returncode == 4 and "status 0x80" in out.stderr

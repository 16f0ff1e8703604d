"""GPU: Swin2SR from a host with no Python and no torch in the process -- examples/swin2sr_host.cpp is built with hipcc (only for
hipMalloc / hipMemcpy) and run against the in-tree libnesr_hip.so: nesr_swin2sr_create with the `small_shift` configuration, the
weights from a flat file, nesr_swin2sr_upscale_u8 on one frame.  The frame it writes meets the u8 criterion of
tests/swin2sr_cases.py against the float64 route."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import swin2sr_cases as C
from tests import swin2sr_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_host_upscales_a_frame(tmp_path, cuda_device):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "swin2sr_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "swin2sr_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    case = C.by_name("small_shift")
    hw = (13, 18)
    frame, y64, tol = C.frame_reference(case.name, hw)
    np.concatenate([v.numpy().reshape(-1) for v in case.sd.values()]).astype(np.float32).tofile(tmp_path / "weights.f32")
    frame.tofile(tmp_path / "in.rgb")
    out = subprocess.run(["timeout", "-k", "10", "60", exe, lib, str(tmp_path / "weights.f32"), str(tmp_path / "in.rgb"), str(hw[0]), str(hw[1]),
                          str(tmp_path / "out.rgb")], capture_output=True, text=True, timeout=90)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    assert f"{len(case.sd)} tensors" in out.stdout and "13 x 18 -> 26 x 36 in 19 launches" in out.stdout
    got = np.fromfile(tmp_path / "out.rgb", np.uint8).reshape(26, 36, 3)
    excluded, wrong, n = R.u8_check(got, y64, tol)
    assert wrong == 0 and excluded <= C.MAX_THIN * n

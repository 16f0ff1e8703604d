"""GPU: Swin2SR's overlapped tiles from a host with no Python and no torch in the process -- examples/swin2sr_overlap_host.cpp is
built with hipcc (only for hipMalloc / hipMemcpy) and run against the in-tree libnesr_hip.so: the `small_shift` configuration, the
weights from a flat file, nesr_swin2sr_overlap_plan and nesr_swin2sr_upscale_overlapped_u8 on a 21 x 30 frame with tile 8,
tile_overlap 4.  The frame it writes meets the u8 criterion against the float64 composition of tests/swin2sr_overlap_ref.py; the
plan it prints has 35 windows."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import swin2sr_cases as C
from tests import swin2sr_overlap_ref as OR
from tests import swin2sr_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_host_upscales_a_frame_in_overlapped_tiles(tmp_path, cuda_device):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "swin2sr_overlap_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "swin2sr_overlap_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    name, (h, w), T, O, windows, _ = OR.OVERLAP_CASES[0]
    case = C.by_name(name)
    frame, y64, _, tol = OR.overlap_reference(0)
    np.concatenate([v.numpy().reshape(-1) for v in case.sd.values()]).astype(np.float32).tofile(tmp_path / "weights.f32")
    frame.tofile(tmp_path / "in.rgb")
    out = subprocess.run(["timeout", "-k", "10", "60", exe, lib, str(tmp_path / "weights.f32"), str(tmp_path / "in.rgb"), str(h), str(w), str(T), str(O),
                          str(tmp_path / "out.rgb"), "5"], capture_output=True, text=True, timeout=90)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    assert (name, h, w, T, O, windows) == ("small_shift", 21, 30, 8, 4, 35)
    assert f"{len(case.sd)} tensors" in out.stdout and "21 x 30 -> 42 x 60" in out.stdout
    assert "plan: 35 windows (5 x 7) of 8 x 8 in 24 x 32" in out.stdout and "7 batches, 141 launches" in out.stdout      # 7 x (19 + 1) + 1
    assert "last window: at (16, 24) -> (32, 48)" in out.stdout
    got = np.fromfile(tmp_path / "out.rgb", np.uint8).reshape(42, 60, 3)
    excluded, wrong, n = R.u8_check(got, y64, tol)
    assert wrong == 0 and excluded <= C.MAX_THIN * n

"""GPU: Swin2SR's tiled upscale from a host with no Python and no torch in the process -- examples/swin2sr_tiled_host.cpp is built
with hipcc (only for hipMalloc / hipMemcpy) and run against the in-tree libnesr_hip.so: the `small_shift` configuration, the weights
from a flat file, nesr_swin2sr_tile_plan and nesr_swin2sr_upscale_tiled_u8 on a 21 x 30 frame with tile 8, tile_pad 4.  The frame
it writes meets the u8 criterion against the float64 composition of tests/swin2sr_tiled_ref.py; the plan it prints has 12 tiles."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import swin2sr_cases as C
from tests import swin2sr_ref as R
from tests import swin2sr_tiled_ref as TR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_host_upscales_a_frame_in_tiles(tmp_path, cuda_device):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "swin2sr_tiled_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "swin2sr_tiled_host.cpp"), "-o", exe, "-ldl"], check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    name, (h, w), T, P, tiles = TR.tiled_case("small_shift")
    case = C.by_name(name)
    frame, y64, _, tol = TR.tiled_reference(name)
    np.concatenate([v.numpy().reshape(-1) for v in case.sd.values()]).astype(np.float32).tofile(tmp_path / "weights.f32")
    frame.tofile(tmp_path / "in.rgb")
    out = subprocess.run(["timeout", "-k", "10", "60", exe, lib, str(tmp_path / "weights.f32"), str(tmp_path / "in.rgb"), str(h), str(w), str(T), str(P),
                          str(tmp_path / "out.rgb"), "5"], capture_output=True, text=True, timeout=90)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    assert (h, w, T, P, tiles) == (21, 30, 8, 4, 12)
    assert f"{len(case.sd)} tensors" in out.stdout and "21 x 30 -> 42 x 60" in out.stdout
    assert "plan: 12 tiles (3 x 4), window 16 x 16" in out.stdout and "3 batches, 57 launches" in out.stdout      # 5 + 5 + 2 windows
    assert "last tile: window at (5, 14), crop (22, 20) 10 x 12 -> (32, 48)" in out.stdout
    got = np.fromfile(tmp_path / "out.rgb", np.uint8).reshape(42, 60, 3)
    excluded, wrong, n = R.u8_check(got, y64, tol)
    assert wrong == 0 and excluded <= C.MAX_THIN * n

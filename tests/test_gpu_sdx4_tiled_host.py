"""GPU: the x4 diffusion upscaler over windows from a host with no Python and no torch in the process -- examples/sdx4_tiled_host.cpp
is built with hipcc (only for hipMalloc / hipMemcpy) and run against the in-tree libnesr_hip.so: the three contexts of the crafted
configuration, the weights from one flat file, nesr_sdx4_tile_plan, nesr_sdx4_tiled_workspace_bytes and one
nesr_sdx4_upscale_tiled_u8 on the 24 x 40 frame with tile 16 and overlap 8.  The PPM it writes is the Python result, bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import sdx4_cases as C
from tests import sdx4_tiled_ref as T
from tests.test_gpu_sdx4_host import read_ppm
from tests.test_gpu_sdx4_tiled import call, pipe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_host_runs_the_tiled_pipeline(tmp_path, cuda_device):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "sdx4_tiled_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "sdx4_tiled_host.cpp"), "-o", exe, "-ldl"],
                   check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    m = C.models()
    np.concatenate([v.numpy().reshape(-1) for key in ("text", "unet", "vae") for v in m[key][0].values()]).astype(np.float32).tofile(tmp_path / "weights.f32")
    frame, noise, latents = T.crafted()
    with open(tmp_path / "frame.ppm", "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (T.W, T.H) + frame.numpy().tobytes())
    C.ids().numpy().astype(np.int32).tofile(tmp_path / "ids.i32")
    noise.numpy().tofile(tmp_path / "noise.f32")
    latents.numpy().tofile(tmp_path / "latents.f32")
    out = subprocess.run(["timeout", "-k", "10", "60", exe, lib, str(tmp_path / "weights.f32"), str(tmp_path / "frame.ppm"), str(tmp_path / "ids.i32"),
                          str(tmp_path / "noise.f32"), str(tmp_path / "latents.f32"), str(C.TOKENS), str(C.NOISE_LEVEL), str(T.STEPS), str(C.GUIDANCE),
                          str(tmp_path / "out.ppm"), str(T.TILE), str(T.OVERLAP), "crafted"], capture_output=True, text=True, timeout=90)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    want, _ = call(pipe())
    assert f"{T.H} x {T.W} -> {4 * T.H} x {4 * T.W}, 2 x 4 windows of 16 x 16 (last at 8, 24)" in out.stdout and f"in {pipe().last_launches()} launches" in out.stdout
    assert f"workspace {pipe().workspace_bytes(2, T.H, T.W, C.TOKENS, tile=T.TILE, tile_overlap=T.OVERLAP)} bytes" in out.stdout
    assert np.array_equal(read_ppm(tmp_path / "out.ppm"), want.cpu().numpy())

"""GPU: the x4 diffusion upscaler from a host with no Python and no torch in the process -- examples/sdx4_host.cpp is built with
hipcc (only for hipMalloc / hipMemcpy) and run against the in-tree libnesr_hip.so: the three contexts of the crafted configuration,
the weights from one flat file, one nesr_sdx4_upscale_u8.  The PPM it writes is the Python result, bit for bit.  A second run with
synthetic weights and the host's own generator for ids, noise and latents shows that route runs."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from neural_enhanced_super_resolution_amd import clip_text, unet
from tests import sdx4_cases as C
from tests.test_gpu_sdx4 import DEV, call, pipe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_ppm(path):
    data = open(path, "rb").read()
    magic, dims, maxval, rest = data.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    assert magic == b"P6" and maxval == b"255" and len(rest) == h * w * 3
    return np.frombuffer(rest, np.uint8).reshape(h, w, 3)


def test_cpp_host_runs_the_pipeline(tmp_path, cuda_device):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = str(tmp_path / "sdx4_host")
    subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "sdx4_host.cpp"), "-o", exe, "-ldl"],
                   check=True, timeout=300)
    lib = os.path.join(ROOT, "neural_enhanced_super_resolution_amd", "libnesr_hip.so")
    m = C.models()
    np.concatenate([v.numpy().reshape(-1) for key in ("text", "unet", "vae") for v in m[key][0].values()]).astype(np.float32).tofile(tmp_path / "weights.f32")
    frame = C.frame().numpy()
    with open(tmp_path / "frame.ppm", "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (C.W, C.H) + frame.tobytes())
    noise, latents = C.draws()
    C.ids().numpy().astype(np.int32).tofile(tmp_path / "ids.i32")
    noise.numpy().tofile(tmp_path / "noise.f32")
    latents.numpy().tofile(tmp_path / "latents.f32")
    out = subprocess.run(["timeout", "-k", "10", "60", exe, lib, str(tmp_path / "weights.f32"), str(tmp_path / "frame.ppm"), str(tmp_path / "ids.i32"),
                          str(tmp_path / "noise.f32"), str(tmp_path / "latents.f32"), str(C.TOKENS), str(C.NOISE_LEVEL), str(C.STEPS), str(C.GUIDANCE),
                          str(tmp_path / "out.ppm"), "crafted"], capture_output=True, text=True, timeout=90)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    tensors = " + ".join(str(len(m[key][0])) for key in ("text", "unet", "vae"))
    assert f"{tensors} tensors" in out.stdout and f"{C.H} x {C.W} -> {4 * C.H} x {4 * C.W}" in out.stdout and f"{C.STEPS} steps in " in out.stdout
    want, _ = call()
    launches = clip_text.launches_per_forward(**C.TEXT) + 1 + C.STEPS * (unet.launches_per_forward(**C.UNET) + 1)
    assert pipe().last_launches() > launches and f"in {pipe().last_launches()} launches" in out.stdout
    assert np.array_equal(read_ppm(tmp_path / "out.ppm"), want.cpu().numpy())
    own = subprocess.run(["timeout", "-k", "10", "60", exe, lib, "seed:5", str(tmp_path / "frame.ppm"), "-", "-", "-", "9", "3", "2", "1.0", str(tmp_path / "own.ppm"), "crafted"],
                         capture_output=True, text=True, timeout=90)
    assert own.returncode == 0, own.stdout + own.stderr
    img = read_ppm(tmp_path / "own.ppm")
    assert img.shape == (4 * C.H, 4 * C.W, 3) and "1 prompt(s) of 9 ids, 2 steps" in own.stdout and img.std() > 0
